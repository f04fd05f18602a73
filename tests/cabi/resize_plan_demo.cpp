// resize_plan_demo.cpp - csrc/vs_resize_plan.h alone, as a host program (built under AddressSanitizer and UBSan by
// tests/test_resize_host.py).
//   resize_plan_demo tables grid G [in out]...   prints the table of every (in, out) in 1..G x 1..G and of the listed pairs:
//                                                "axis in out ksize", then per output index "xmin n k[0] .. k[ksize-1]"
//   resize_plan_demo walk [n h w oh ow]...       runs resize_bilinear_u8's three stages on the host with the functions the kernel
//                                                calls, for every tile, at four byte alignments of both buffers and with and
//                                                without the R/B swap: every global, LDS and store address is asserted in
//                                                bounds, every wide access aligned, every output byte written exactly once, and
//                                                the result equal to the two passes run straight from the tables
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vs_resize_plan.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

static void print_axis(int in, int out) {
    const ResizeAxis A = resize_build_axis(in, out, false);      // in == out too: the filter itself, not the skipped pass
    std::printf("axis %d %d %d\n", in, out, A.ksize);
    for (int xx = 0; xx < out; ++xx) {
        std::printf("%d %d", A.bounds[2 * xx], A.bounds[2 * xx + 1]);
        for (int x = 0; x < A.ksize; ++x) std::printf(" %d", A.coef[(size_t)xx * A.ksize + x]);
        std::printf("\n");
    }
    CHECK(A.ksize == resize_ksize(in, out));
}

// the two passes straight from the tables, no tiles: what the walk must reproduce
static std::vector<uint8_t> direct(const ResizePlanHost &P, const uint8_t *src, int n, bool swap) {
    const ResizeGeom &g = P.g;
    std::vector<uint8_t> mid((size_t)n * g.H * g.OW * 3), out((size_t)n * g.OH * g.OW * 3);
    for (int f = 0; f < n; ++f)
        for (int r = 0; r < g.H; ++r)
            for (int oc = 0; oc < g.OW; ++oc)
                for (int ch = 0; ch < 3; ++ch) {
                    int32_t acc = 1 << (RESIZE_PRECISION_BITS - 1);
                    const int xmin = P.x.bounds[2 * oc], nx = P.x.bounds[2 * oc + 1];
                    for (int x = 0; x < nx; ++x)
                        acc += src[((size_t)f * g.H + r) * g.W * 3 + (size_t)(xmin + x) * 3 + (swap ? 2 - ch : ch)] * P.x.coef[(size_t)oc * g.kx + x];
                    mid[(((size_t)f * g.H + r) * g.OW + oc) * 3 + ch] = (uint8_t)resize_clip8(acc);
                }
    for (int f = 0; f < n; ++f)
        for (int oy = 0; oy < g.OH; ++oy)
            for (int b = 0; b < g.OW * 3; ++b) {
                int32_t acc = 1 << (RESIZE_PRECISION_BITS - 1);
                const int ymin = P.y.bounds[2 * oy], ny = P.y.bounds[2 * oy + 1];
                for (int y = 0; y < ny; ++y) acc += mid[((size_t)f * g.H + ymin + y) * g.OW * 3 + b] * P.y.coef[(size_t)oy * g.ky + y];
                out[((size_t)f * g.OH + oy) * g.OW * 3 + b] = (uint8_t)resize_clip8(acc);
            }
    return out;
}

static uint32_t lds_dword(const std::vector<uint8_t> &lds, size_t base, int64_t index, size_t region_bytes) {
    CHECK(index >= 0 && (size_t)index * 4 + 4 <= region_bytes);
    uint32_t v;
    std::memcpy(&v, lds.data() + base + (size_t)index * 4, 4);
    return v;
}

static void walk(int n, int h, int w, int oh, int ow) {
    const ResizePlanHost P = resize_make_plan(h, w, oh, ow);
    CHECK(P.ok);
    const ResizeGeom &g = P.g;
    std::printf("geom %d %d %d %d %d path %d tile %d %d tiles %d %d raw %d %d mid %d %d lds %d\n", n, h, w, oh, ow, g.path, g.tile_oh,
                g.tile_ow, g.tiles_y, g.tiles_x, g.raw_stride, g.raw_rows, g.mid_stride, g.mid_rows, g.lds_bytes);
    CHECK(g.mid_stride % 4 == 0 && g.raw_stride % 4 == 0 && g.raw_rows >= 1 && g.tile_ow == 1 << g.lane_shift);
    // the LDS regions follow each other, dword aligned, inside what a launch may ask for without opting in to more
    CHECK(g.raw_off == g.mid_rows * g.mid_stride && g.xk_off == g.raw_off + g.raw_rows * g.raw_stride);
    CHECK(g.yk_off == g.xk_off + g.tile_ow * g.kx * 4 && g.lds_bytes == g.yk_off + g.tile_oh * g.ky * 4 && g.lds_bytes <= RESIZE_LDS_BYTES);
    CHECK(g.raw_off % 4 == 0 && g.xk_off % 4 == 0 && g.yk_off % 4 == 0 && RESIZE_LDS_BYTES <= 65536);
    CHECK(resize_out_dwords(ResizeTile{0, 1, 0, g.tile_ow, 0, 1, 0, 1}) <= g.tile_ow);     // stage C: a lane per dword of the widest tile
    const int32_t *xb = P.x.bounds.data(), *yb = P.y.bounds.data();
    const size_t in_bytes = (size_t)n * (size_t)resize_frame_bytes(h, w), out_bytes = (size_t)n * (size_t)resize_frame_bytes(oh, ow);
    for (int align = 0; align < 4; ++align)
        for (int swap = 0; swap < 2; ++swap) {
            // exactly sized heap blocks behind an offset: a byte outside is the sanitizer's, the asserts below say which
            std::vector<uint8_t> in_block(in_bytes + 8), out_block(out_bytes + 8, 0);
            uint8_t *frames = in_block.data() + ((4 - ((uintptr_t)in_block.data() & 3)) & 3) + align;         // address % 4 == align
            uint8_t *out = out_block.data() + ((4 - ((uintptr_t)out_block.data() & 3)) & 3) + (3 - align);
            CHECK(((uintptr_t)frames & 3) == (uintptr_t)align && frames + in_bytes <= in_block.data() + in_block.size());
            CHECK(out + out_bytes <= out_block.data() + out_block.size());
            uint32_t seed = 12345u + (uint32_t)align;
            for (size_t i = 0; i < in_bytes; ++i) { seed = seed * 1664525u + 1013904223u; frames[i] = (uint8_t)(seed >> 24); }
            std::vector<int> written(out_bytes, 0);
            std::vector<uint8_t> lds((size_t)g.lds_bytes);                          // exactly what the launch asks for
            const size_t MID = 0, RAW = (size_t)g.raw_off;
            const size_t raw_bytes = (size_t)g.raw_rows * g.raw_stride, mid_bytes = (size_t)g.raw_off;
            for (int f = 0; f < n; ++f)
                for (int tile = 0; tile < g.tiles_y * g.tiles_x; ++tile) {
                    std::memset(lds.data(), 0xAA, lds.size());                      // what a block finds in LDS is anything
                    const ResizeTile t = resize_tile(g, xb, yb, tile);
                    CHECK(0 <= t.oy0 && t.oy0 < t.oy1 && t.oy1 <= oh && 0 <= t.ox0 && t.ox0 < t.ox1 && t.ox1 <= ow);
                    CHECK(0 <= t.r0 && t.r0 < t.r1 && t.r1 <= h && 0 <= t.c0 && t.c0 < t.c1 && t.c1 <= w);
                    CHECK(t.r1 - t.r0 <= g.mid_rows);
                    const int tw0 = t.ox1 - t.ox0, th0 = t.oy1 - t.oy0;
                    CHECK(tw0 * g.kx <= g.tile_ow * g.kx && th0 * g.ky <= g.tile_oh * g.ky);
                    for (int i = 0; i < tw0 * g.kx; ++i) {                           // the tile's coefficients -> LDS
                        CHECK((size_t)t.ox0 * g.kx + i < P.x.coef.size());
                        std::memcpy(lds.data() + g.xk_off + 4 * (size_t)i, &P.x.coef[(size_t)t.ox0 * g.kx + i], 4);
                    }
                    for (int i = 0; i < th0 * g.ky; ++i) {
                        CHECK((size_t)t.oy0 * g.ky + i < P.y.coef.size());
                        std::memcpy(lds.data() + g.yk_off + 4 * (size_t)i, &P.y.coef[(size_t)t.oy0 * g.ky + i], 4);
                    }
                    for (int oy = t.oy0; oy < t.oy1; ++oy) CHECK(yb[2 * oy] >= t.r0 && yb[2 * oy] + yb[2 * oy + 1] <= t.r1);
                    for (int oc = t.ox0; oc < t.ox1; ++oc) CHECK(xb[2 * oc] >= t.c0 && xb[2 * oc] + xb[2 * oc + 1] <= t.c1);
                    const uint8_t *src = frames + (size_t)f * (size_t)resize_frame_bytes(h, w);
                    uint8_t *dst = out + (size_t)f * (size_t)resize_frame_bytes(oh, ow);
                    const int seg = (t.c1 - t.c0) * 3, tw = t.ox1 - t.ox0, th = t.oy1 - t.oy0;
                    const int slots = g.raw_stride / 4 - 1;
                    CHECK(resize_raw_stride(seg) <= g.raw_stride);
                    for (int r = t.r0; r < t.r1; r += g.raw_rows) {
                        const int rows = t.r1 - r < g.raw_rows ? t.r1 - r : g.raw_rows;
                        for (int i = 0; i < rows * slots; ++i) {                    // stage A
                            const int rr = i / slots, j = i - rr * slots;
                            const uint8_t *row = src + resize_pixel_offset(w, r + rr, t.c0);
                            const int phase = (int)((uintptr_t)row & 3);
                            CHECK(slots >= resize_raw_slots(phase, seg));
                            const ResizeSlot s = resize_load_slot(phase, seg, j);
                            CHECK(s.count >= 0 && s.count <= 4);
                            const size_t at = (size_t)rr * g.raw_stride + s.lds_off;
                            if (s.count == 0) continue;
                            CHECK(at + 4 <= (size_t)rows * g.raw_stride && at + 4 <= raw_bytes && at % 4 == 0);
                            CHECK(row + s.seg_off + s.first >= frames && row + s.seg_off + s.first + s.count <= frames + in_bytes);
                            CHECK(s.seg_off + s.first >= 0 && s.seg_off + s.first + s.count <= seg);
                            if (s.count == 4) CHECK(((uintptr_t)(row + s.seg_off) & 3) == 0);
                            for (int b = s.first; b < s.first + s.count; ++b) lds[RAW + at + b] = row[s.seg_off + b];
                        }
                        for (int i = 0; i < rows * tw; ++i) {                       // stage B
                            const int rr = i / tw, oc = t.ox0 + (i - rr * tw);
                            const int phase = (int)((uintptr_t)(src + resize_pixel_offset(w, r + rr, t.c0)) & 3);
                            const int xmin = xb[2 * oc], nx = xb[2 * oc + 1];
                            int32_t a[3] = {1 << (RESIZE_PRECISION_BITS - 1), 1 << (RESIZE_PRECISION_BITS - 1), 1 << (RESIZE_PRECISION_BITS - 1)};
                            for (int x = 0; x < nx; ++x) {
                                const int byte = resize_raw_byte(phase, t.c0, xmin + x);
                                CHECK(byte >= 0 && (byte >> 2) * 4 + 8 <= g.raw_stride);
                                const int64_t word = ((int64_t)rr * g.raw_stride >> 2) + (byte >> 2);
                                const uint32_t lo = lds_dword(lds, RAW, word, (size_t)rows * g.raw_stride);
                                const uint32_t hi = lds_dword(lds, RAW, word + 1, (size_t)rows * g.raw_stride);
                                const uint32_t px = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (byte & 3)));
                                const uint32_t c = lds_dword(lds, (size_t)g.xk_off, (int64_t)(oc - t.ox0) * g.kx + x, (size_t)g.tile_ow * g.kx * 4);
                                a[0] += (int32_t)resize_mul(px & 255, c); a[1] += (int32_t)resize_mul((px >> 8) & 255, c); a[2] += (int32_t)resize_mul((px >> 16) & 255, c);
                            }
                            const int m = resize_mid_offset(g, t, r + rr, oc);
                            CHECK(m >= 0 && m + 3 <= (t.r1 - t.r0) * g.mid_stride && (size_t)m + 3 <= mid_bytes);
                            lds[MID + m] = (uint8_t)resize_clip8(swap ? a[2] : a[0]);
                            lds[MID + m + 1] = (uint8_t)resize_clip8(a[1]);
                            lds[MID + m + 2] = (uint8_t)resize_clip8(swap ? a[0] : a[2]);
                        }
                    }
                    const int nd = resize_out_dwords(t);
                    CHECK(nd * 4 <= g.mid_stride);
                    for (int i = 0; i < th * nd; ++i) {                             // stage C
                        const int oo = i / nd, j = i - oo * nd, oy = t.oy0 + oo;
                        const int ymin = yb[2 * oy], ny = yb[2 * oy + 1];
                        int32_t a[4];
                        for (int b = 0; b < 4; ++b) a[b] = 1 << (RESIZE_PRECISION_BITS - 1);
                        for (int y = 0; y < ny; ++y) {
                            const uint32_t v = lds_dword(lds, MID, resize_mid_dword(g, t, ymin + y, j), (size_t)(t.r1 - t.r0) * g.mid_stride);
                            const uint32_t c = lds_dword(lds, (size_t)g.yk_off, (int64_t)oo * g.ky + y, (size_t)g.tile_oh * g.ky * 4);
                            for (int b = 0; b < 4; ++b) a[b] += (int32_t)resize_mul((v >> (8 * b)) & 255, c);
                        }
                        uint8_t *p = dst + resize_pixel_offset(ow, oy, t.ox0) + 4 * j;
                        const int count = resize_store_count(t, j);
                        CHECK(count >= 1 && count <= 4);
                        CHECK(p >= out && p + count <= out + out_bytes);
                        for (int b = 0; b < count; ++b) { p[b] = (uint8_t)resize_clip8(a[b]); ++written[(size_t)(p + b - out)]; }
                    }
                }
            for (size_t i = 0; i < out_bytes; ++i) CHECK(written[i] == 1);
            const std::vector<uint8_t> want = direct(P, frames, n, swap != 0);
            CHECK(std::memcmp(want.data(), out, out_bytes) == 0);
        }
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::strcmp(argv[1], "tables") == 0) {
        int at = 2;
        if (argc >= 4 && std::strcmp(argv[2], "grid") == 0) {
            const int G = std::atoi(argv[3]);
            for (int in = 1; in <= G; ++in)
                for (int out = 1; out <= G; ++out) print_axis(in, out);
            at = 4;
        }
        for (; at + 1 < argc; at += 2) print_axis(std::atoi(argv[at]), std::atoi(argv[at + 1]));
    } else if (argc >= 2 && std::strcmp(argv[1], "walk") == 0) {
        for (int at = 2; at + 4 < argc; at += 5)
            walk(std::atoi(argv[at]), std::atoi(argv[at + 1]), std::atoi(argv[at + 2]), std::atoi(argv[at + 3]), std::atoi(argv[at + 4]));
    } else {
        std::printf("usage: resize_plan_demo tables [grid G] [in out]... | walk [n h w oh ow]...\n");
        return 2;
    }
    std::printf("OK\n");
    return 0;
}
