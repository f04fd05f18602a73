// Host-side launch helpers: run-time values -> template arguments, and the per-device opt-in to
// more than 64 KiB of dynamic LDS.  Host code only; nothing here is seen by a kernel.
#pragma once

#include <type_traits>
#include <utility>

// ---- value -> template argument picks (plain C++17: tests/cabi/launch_pick_demo.cpp compiles this part alone) ----

template <int V>
using vsk_int = std::integral_constant<int, V>;

// f(vsk_int<V>{}) for the one V == v: true.  No V matches: nothing is called, false.
template <int... Vs, class F>
bool vsk_pick_int(int v, F &&f) {
    return ((v == Vs ? (f(vsk_int<Vs>{}), true) : false) || ...);
}

template <class F>
void vsk_pick_bool(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// ---- dynamic LDS above 64 KiB ----
#ifdef __HIP__
#include <hip/hip_runtime.h>

#include <atomic>

enum { VSK_MAX_DEVICES = 64 };

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute: set once per (kernel instantiation, device).
// One flag array per Kernel; a device index at or above VSK_MAX_DEVICES has no flag and sets the attribute every time.
// Returns 0 or the HIP error code.  `bytes` is the most the kernel is ever launched with, not this launch's share.
template <auto Kernel>
int vsk_raise_lds(size_t bytes) {
    static std::atomic<unsigned char> done[VSK_MAX_DEVICES];
    if (bytes <= 64 * 1024) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return (int)hipErrorInvalidDevice;
    const bool flagged = dev >= 0 && dev < VSK_MAX_DEVICES;
    if (flagged && done[dev].load(std::memory_order_acquire)) return 0;
    const int rc = (int)hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (rc == 0 && flagged) done[dev].store(1, std::memory_order_release);
    return rc;
}
#endif  // __HIP__
