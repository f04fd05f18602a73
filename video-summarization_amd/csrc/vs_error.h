// vs_error.h - the one error path of the C ABI files: the thread-local text behind vs_last_error()
// (vs_error.cpp), the printf-style setter and the macros that turn a HIP call's or a launcher's result into a return.
// Host code only.  The macros name hipError_t / hipGetErrorString: a file that uses them includes <hip/hip_runtime.h>.
#pragma once
#include <cstdarg>
#include <cstdio>

#include "vs_scorer.h"      // VS_OK, VS_ERR_*

int vs_fail_msg(int code, const char *msg);     // sets the calling thread's error text, returns `code`

inline int vs_failf(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return vs_fail_msg(code, buf);
}

#define VS_HIP(call)                                                                               \
    do {                                                                                           \
        const hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) return vs_failf(VS_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// a launcher's result: 0 done, > 0 a hipError_t, < 0 a shape the kernel group does not take
#define VS_LAUNCH(call)                                                                               \
    do {                                                                                              \
        const int e_ = (call);                                                                        \
        if (e_ > 0) return vs_failf(VS_ERR_HIP, "%s: %s", #call, hipGetErrorString((hipError_t)e_));  \
        if (e_ < 0) return vs_failf(VS_ERR_INVALID, "%s: unsupported shape", #call);                  \
    } while (0)

// ... of a launcher that has checked its shapes before (vs_cnn, vs_summary, vs_eval_device, vs_resize): any non-zero result is
// a hipError_t
#define VS_LAUNCH_HIP(call)                                                                           \
    do {                                                                                              \
        const int e_ = (call);                                                                        \
        if (e_ != 0) return vs_failf(VS_ERR_HIP, "%s: %s", #call, hipGetErrorString((hipError_t)e_)); \
    } while (0)
