// vs_resize.hip - PIL's antialiased bilinear resize of 8-bit RGB frames on the device, bit for bit.
// One block owns a tile of output rows x output columns of one frame.  It stages the input rows its vertical taps need, a chunk
// at a time, as raw bytes in LDS (A), runs the horizontal pass on them into the rounded uint8 intermediate, also in LDS (B), and
// then runs the vertical pass out of that intermediate and stores the output bytes (C).  The intermediate never goes to memory.
// All arithmetic is integer multiply-add on PIL's 22-bit fixed-point coefficients, which the block keeps in LDS.  A skipped pass
// is a one-tap table of weight 1.  Every address comes from vs_resize_plan.h; global accesses wider than a byte happen only
// behind a test of the actual address.  Threads: column tid & (tile_ow - 1) of the tile, rows tid >> lane_shift and onwards -
// no division per item, and a thread's column window is read once.
#include <hip/hip_runtime.h>

#include "vs_device.h"
#include "vs_resize_kernels.h"

namespace {

__global__ __launch_bounds__(RESIZE_THREADS) void resize_bilinear_u8(const ResizeArgs A) {
    extern __shared__ uint32_t lds[];
    const ResizeGeom &g = A.g;
    uint32_t *mid32 = lds, *raw32 = lds + (g.raw_off >> 2);
    uint32_t *xk = lds + (g.xk_off >> 2), *yk = lds + (g.yk_off >> 2);
    uint8_t *mid = (uint8_t *)mid32, *raw = (uint8_t *)raw32;
    const int32_t tiles = g.tiles_y * g.tiles_x, tid = (int32_t)threadIdx.x;
    const int32_t frame = (int32_t)(blockIdx.x / (uint32_t)tiles), tile = (int32_t)(blockIdx.x - (uint32_t)frame * (uint32_t)tiles);
    const ResizeTile t = resize_tile(g, A.xb, A.yb, tile);
    const uint8_t *src = A.frames + (size_t)frame * (size_t)resize_frame_bytes(g.H, g.W);
    uint8_t *dst = A.out + (size_t)frame * (size_t)resize_frame_bytes(g.OH, g.OW);
    const int32_t seg = (t.c1 - t.c0) * 3, tw = t.ox1 - t.ox0, th = t.oy1 - t.oy0;
    const int32_t lane_x = tid & (g.tile_ow - 1), lane_y = tid >> g.lane_shift, lanes_y = RESIZE_THREADS >> g.lane_shift;
    const uint32_t half = 1u << (RESIZE_PRECISION_BITS - 1);

    // the tile's coefficients -> LDS (read after the first barrier below)
    for (int32_t i = tid; i < tw * g.kx; i += RESIZE_THREADS) xk[i] = (uint32_t)A.xk[(size_t)t.ox0 * g.kx + i];
    for (int32_t i = tid; i < th * g.ky; i += RESIZE_THREADS) yk[i] = (uint32_t)A.yk[(size_t)t.oy0 * g.ky + i];
    int32_t xmin = 0, nx = 0;
    if (lane_x < tw) { xmin = A.xb[2 * (t.ox0 + lane_x)]; nx = A.xb[2 * (t.ox0 + lane_x) + 1]; }

    for (int32_t r = t.r0; r < t.r1; r += g.raw_rows) {
        const int32_t rows = t.r1 - r < g.raw_rows ? t.r1 - r : g.raw_rows;
        // A: raw input bytes of rows [r, r + rows), columns [c0, c1) -> LDS, each row at the phase of its global address;
        // a wave per row, a lane per aligned dword
        for (int32_t rr = tid >> 6; rr < rows; rr += RESIZE_THREADS >> 6) {
            const uint8_t *row = src + resize_pixel_offset(g.W, r + rr, t.c0);
            const int32_t phase = (int32_t)((uintptr_t)row & 3), slots = resize_raw_slots(phase, seg);
            for (int32_t j = tid & 63; j < slots; j += 64) {
                const ResizeSlot s = resize_load_slot(phase, seg, j);
                if (s.count == 4) {
                    raw32[(rr * g.raw_stride + s.lds_off) >> 2] = *(const uint32_t *)(row + s.seg_off);     // aligned: (row - phase) is
                } else {
                    for (int32_t b = s.first; b < s.first + s.count; ++b) raw[rr * g.raw_stride + s.lds_off + b] = row[s.seg_off + b];
                }
            }
        }
        __syncthreads();
        // B: the horizontal pass of those rows, rounded to uint8 -> the intermediate
        if (lane_x < tw) {
            const uint32_t *k = xk + lane_x * g.kx;
            for (int32_t rr = lane_y; rr < rows; rr += lanes_y) {
                const int32_t phase = (int32_t)((uintptr_t)(src + resize_pixel_offset(g.W, r + rr, t.c0)) & 3);
                const uint32_t *line = raw32 + ((rr * g.raw_stride) >> 2);
                int32_t byte = resize_raw_byte(phase, t.c0, xmin);
                uint32_t a0 = half, a1 = half, a2 = half;
                for (int32_t x = 0; x < nx; ++x, byte += 3) {
                    const uint32_t lo = line[byte >> 2], hi = line[(byte >> 2) + 1];
                    const uint32_t px = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (byte & 3)));
                    const uint32_t c = k[x];
                    a0 += resize_mul(px & 255, c);
                    a1 += resize_mul((px >> 8) & 255, c);
                    a2 += resize_mul((px >> 16) & 255, c);
                }
                uint8_t *m = mid + resize_mid_offset(g, t, r + rr, t.ox0 + lane_x);
                m[0] = (uint8_t)resize_clip8((int32_t)(A.swap_rb ? a2 : a0));
                m[1] = (uint8_t)resize_clip8((int32_t)a1);
                m[2] = (uint8_t)resize_clip8((int32_t)(A.swap_rb ? a0 : a2));
            }
        }
        __syncthreads();
    }

    // C: the vertical pass, four consecutive bytes of an output row per item (channels are interleaved: it is bytewise)
    const int32_t nd = resize_out_dwords(t);
    if (lane_x < nd) {
        const int32_t j = lane_x, count = resize_store_count(t, j);
        for (int32_t oo = lane_y; oo < th; oo += lanes_y) {
            const int32_t oy = t.oy0 + oo;
            const int32_t ymin = A.yb[2 * oy], ny = A.yb[2 * oy + 1];
            const uint32_t *k = yk + oo * g.ky;
            uint32_t a0 = half, a1 = half, a2 = half, a3 = half;
            for (int32_t y = 0; y < ny; ++y) {
                const uint32_t v = mid32[resize_mid_dword(g, t, ymin + y, j)];
                const uint32_t c = k[y];
                a0 += resize_mul(v & 255, c);
                a1 += resize_mul((v >> 8) & 255, c);
                a2 += resize_mul((v >> 16) & 255, c);
                a3 += resize_mul(v >> 24, c);
            }
            const uint32_t b0 = (uint32_t)resize_clip8((int32_t)a0), b1 = (uint32_t)resize_clip8((int32_t)a1),
                           b2 = (uint32_t)resize_clip8((int32_t)a2), b3 = (uint32_t)resize_clip8((int32_t)a3);
            uint8_t *p = dst + resize_pixel_offset(g.OW, oy, t.ox0) + 4 * j;
            if (count == 4 && ((uintptr_t)p & 3) == 0) {
                *(uint32_t *)p = b0 | b1 << 8 | b2 << 16 | b3 << 24;
            } else if (count == 4 && ((uintptr_t)p & 1) == 0) {
                *(uint16_t *)p = (uint16_t)(b0 | b1 << 8);
                *(uint16_t *)(p + 2) = (uint16_t)(b2 | b3 << 8);
            } else {
                if (count > 0) p[0] = (uint8_t)b0;
                if (count > 1) p[1] = (uint8_t)b1;
                if (count > 2) p[2] = (uint8_t)b2;
                if (count > 3) p[3] = (uint8_t)b3;
            }
        }
    }
}

}  // namespace

int vsk_resize(const ResizeArgs &A, hipStream_t st) {
    const int64_t blocks = (int64_t)A.n * A.g.tiles_y * A.g.tiles_x;
    hipLaunchKernelGGL(resize_bilinear_u8, dim3((uint32_t)blocks), dim3(RESIZE_THREADS), (size_t)A.g.lds_bytes, st, A);
    VSK_CHECK_LAUNCH();
    return 0;
}
