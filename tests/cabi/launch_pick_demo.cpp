// The value -> template-argument picks of csrc/vs_launch.h alone, as plain C++17 (no HIP): tests/test_launch_pick_host.py
// builds this with the host compiler and -fsanitize=address,undefined.  Prints "OK" or the first failed check.
#include <cstdio>
#include <vector>

#include "vs_launch.h"

#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAILED line %d: %s\n", __LINE__, #__VA_ARGS__); return 1; } } while (0)

template <int V> struct Tag { static constexpr int value = V; };      // V must be usable as a template argument

int main() {
    for (int v : {32, 64, 128}) {               // a listed value: f exactly once, with that constant
        std::vector<int> seen;
        const bool found = vsk_pick_int<32, 64, 128>(v, [&](auto DH) { seen.push_back(Tag<DH()>::value); });
        CHECK(found && seen.size() == 1 && seen[0] == v);
    }
    for (int v : {0, -1, 33, 96, 256}) {        // an unlisted value: nothing called, false
        int calls = 0;
        CHECK(!vsk_pick_int<32, 64, 128>(v, [&](auto) { ++calls; }) && calls == 0);
    }
    int calls = 0;
    CHECK(!vsk_pick_int<>(1, [&](auto) { ++calls; }) && calls == 0);          // an empty list matches nothing
    for (bool b : {false, true}) {
        std::vector<int> seen;
        vsk_pick_bool(b, [&](auto B) { seen.push_back(Tag<B() ? 1 : 0>::value); });
        CHECK(seen.size() == 1 && seen[0] == (b ? 1 : 0));
    }
    int hits[3][2][2] = {};                      // nested picks reach every combination, each exactly once
    for (int dh : {32, 64, 128})
        for (int drop = 0; drop < 2; ++drop)
            for (int f16 = 0; f16 < 2; ++f16)
                CHECK(vsk_pick_int<32, 64, 128>(dh, [&](auto DH) {
                    vsk_pick_bool(drop != 0, [&](auto DROP) {
                        vsk_pick_int<0, 1>(f16, [&](auto F16) { ++hits[Tag<DH() / 64>::value][Tag<DROP()>::value][Tag<F16()>::value]; });
                    });
                }));
    for (auto &a : hits) for (auto &b : a) for (int h : b) CHECK(h == 1);
    std::printf("OK\n");
    return 0;
}
