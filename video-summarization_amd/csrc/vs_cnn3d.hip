// vs_cnn3d.hip - kernels of the R3D-18 video-level feature: 3-D conv + folded BatchNorm3d (+ residual)
// (+ ReLU) as an implicit GEMM on the fp32 matrix pipe, the fold-and-pack of one conv's weights, and the final mean, all on
// channels-last [N, T, H, W, C] activations.
//
// conv3d_igemm: rows = N*To*Ho*Wo output positions, columns = Cout, k = (kt, kh, kw, cin) ascending.  The tile, the thread-to-
// element maps and the LDS layout are conv_igemm's (vs_cnn.hip): a block of 4 waves owns a 64 x 64 tile, wave w its 32 x 32
// quarter in one accumulator; per k-step of 32 the block gathers its 64 x 32 slice of A (cnn3d_pos / cnn3d_tap / cnn3d_offset of
// vs_cnn3d_plan.h: padding taps in time or space, k >= K and rows >= M read as zero) and its 64 x 32 slice of the packed weights
// into LDS, the next step's loads in flight under this step's 16 MFMAs per wave.  LDS rows are 36 floats and each group of 8 k
// is stored as [k0 k2 k4 k6 | k1 k3 k5 k7], so that one 16-byte read per operand feeds 4 MFMAs whose k pairs are (0,1) (2,3)
// (4,5) (6,7): every output element is ONE chain of multiply-adds over k ascending, whatever tile or batch it lies in.
// Epilogue: + bias, + residual (read at the output's own offset) where the record has one, ReLU where the record asks for it.
#include "vs_cnn3d_kernels.h"
#include "vs_device.h"

namespace {

constexpr int NT = 256;
constexpr int LDS_ROW = CNN3D_TILE_K + 4;
static_assert(CNN3D_TILE_M == 64 && CNN3D_TILE_N == 64 && CNN3D_TILE_K == 32, "conv3d_igemm's thread-to-element maps are written for 64 x 64 x 32");

enum { GATHER_VEC4 = 0, GATHER_SCALAR = 1, GATHER_U8 = 2 };

// 4 consecutive k of one output position
template <int MODE>
__device__ __forceinline__ f32x4 gather4(const void *in, const Cnn3dConv &g, const Cnn3dPos &px, int k, const float *lut) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if constexpr (MODE == GATHER_VEC4) {           // Cin % 4 == 0: the 4 lie in one tap
        const int64_t off = cnn3d_offset(g, px, cnn3d_tap(g, k));
        if (off >= 0) v = *(const f32x4 *)((const float *)in + off);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const Cnn3dTap tp = cnn3d_tap(g, k + j);
            const int64_t off = cnn3d_offset(g, px, tp);
            if (off >= 0) {
                if constexpr (MODE == GATHER_U8) v[j] = lut[tp.c * 256 + ((const uint8_t *)in)[off]];
                else v[j] = ((const float *)in)[off];
            }
        }
    }
    return v;
}

__device__ __forceinline__ void lds_put(float *tile, int row, int kq, const f32x4 &v) {
    float *p = tile + row * LDS_ROW + 8 * (kq >> 1) + 2 * (kq & 1);
    *(f32x2 *)p = f32x2{v[0], v[2]};
    *(f32x2 *)(p + 4) = f32x2{v[1], v[3]};
}

template <int MODE>
__global__ __launch_bounds__(NT) void conv3d_igemm(const Cnn3dConvArgs A) {
    __shared__ __attribute__((aligned(16))) float As[CNN3D_TILE_M * LDS_ROW];
    __shared__ __attribute__((aligned(16))) float Bs[CNN3D_TILE_N * LDS_ROW];
    __shared__ float lut[MODE == GATHER_U8 ? 768 : 1];
    const Cnn3dConv &g = A.g;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, r = lane & 31, h = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * CNN3D_TILE_M;
    const int n0 = blockIdx.y * CNN3D_TILE_N;
    if constexpr (MODE == GATHER_U8) {             // ToTensor + Normalize in float, in torch's order of operations
        for (int i = t; i < 768; i += NT) lut[i] = ((float)(i & 255) / 255.0f - A.mean[i >> 8]) / A.std[i >> 8];
        __syncthreads();
    }
    // loads: thread t brings rows t/8 and t/8 + 32 of both operands, k = 4*(t%8) .. +3 of the step
    const int lr = t >> 3, kq = t & 7;
    const Cnn3dPos px0 = cnn3d_pos(g, m0 + lr), px1 = cnn3d_pos(g, m0 + lr + 32);
    const float *w0 = A.w + (int64_t)(n0 + lr) * g.Kp + 4 * kq, *w1 = w0 + (int64_t)32 * g.Kp;
    f32x4 a0, a1, b0, b1;
    auto fetch = [&](int kt) {
        const int k = kt * CNN3D_TILE_K + 4 * kq;
        a0 = gather4<MODE>(A.in, g, px0, k, lut);
        a1 = gather4<MODE>(A.in, g, px1, k, lut);
        b0 = *(const f32x4 *)(w0 + kt * CNN3D_TILE_K);
        b1 = *(const f32x4 *)(w1 + kt * CNN3D_TILE_K);
    };
    const int rm = 32 * (wv & 1), cn = 32 * (wv >> 1);
    const float *ap = As + (rm + r) * LDS_ROW + 4 * h, *bp = Bs + (cn + r) * LDS_ROW + 4 * h;
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int nk = g.Kp / CNN3D_TILE_K;
    fetch(0);
    for (int kt = 0; kt < nk; ++kt) {
        lds_put(As, lr, kq, a0); lds_put(As, lr + 32, kq, a1);
        lds_put(Bs, lr, kq, b0); lds_put(Bs, lr + 32, kq, b1);
        __syncthreads();
        if (kt + 1 < nk) fetch(kt + 1);
#pragma unroll
        for (int q = 0; q < CNN3D_TILE_K / 8; ++q) {
            const f32x4 av = *(const f32x4 *)(ap + 8 * q), bv = *(const f32x4 *)(bp + 8 * q);
            acc = MFMA32(av[0], bv[0], acc);
            acc = MFMA32(av[1], bv[1], acc);
            acc = MFMA32(av[2], bv[2], acc);
            acc = MFMA32(av[3], bv[3], acc);
        }
        __syncthreads();
    }
    // + bias, + residual, ReLU
    const int col = n0 + cn + r;
    const float bias = A.bias[col];                 // padded to the column tile
#pragma unroll
    for (int tt = 0; tt < 16; ++tt) {
        const int64_t off = cnn3d_store_offset(g, m0 + rm + acc_row(tt, h), col);
        if (off >= 0) {
            float v = acc[tt] + bias;
            if (A.residual) v += A.residual[off];
            A.out[off] = A.relu ? relu1(v) : v;
        }
    }
}

// one thread per element of the packed [Coutp][Kp] weights; the threads of k == 0 also write the bias
__global__ __launch_bounds__(NT) void cnn3d_pack_conv(const float *__restrict__ w, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                      const float *__restrict__ mean, const float *__restrict__ var, const Cnn3dConv g,
                                                      float *__restrict__ pw, float *__restrict__ pb) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= (int64_t)g.Coutp * g.Kp) return;
    const int co = (int)(i / g.Kp), k = (int)(i - (int64_t)co * g.Kp);
    float v = 0.f, b = 0.f;
    if (co < g.Cout) {
        const double scale = (double)gamma[co] / sqrt((double)var[co] + 1e-5);
        b = (float)((double)beta[co] - (double)mean[co] * scale);
        const Cnn3dTap tp = cnn3d_tap(g, k);
        if (tp.valid) v = (float)((double)w[((((int64_t)co * g.Cin + tp.c) * g.kt + tp.dt) * g.ks + tp.dh) * g.ks + tp.dw] * scale);
    }
    pw[i] = v;
    if (k == 0) pb[co] = b;
}

// one thread per (video, channel): the sum over the T'*H'*W' positions in memory order, then one division
__global__ __launch_bounds__(NT) void cnn3d_mean(const Cnn3dMeanArgs A) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= (int64_t)A.N * A.C) return;
    const int64_t n = i / A.C;
    const int c = (int)(i - n * A.C);
    const float *p = A.in + n * A.P * A.C + c;
    float s = 0.f;
    for (int64_t j = 0; j < A.P; ++j) s += p[j * A.C];
    A.out[i] = s / (float)A.P;
}

unsigned blocks_for(int64_t threads) { return (unsigned)((threads + NT - 1) / NT); }

}  // namespace

int vsk_cnn3d_pack_conv(const float *w, const float *gamma, const float *beta, const float *mean, const float *var, const Cnn3dConv &g,
                        float *packed_w, float *packed_b, hipStream_t st) {
    hipLaunchKernelGGL(cnn3d_pack_conv, dim3(blocks_for((int64_t)g.Coutp * g.Kp)), dim3(NT), 0, st, w, gamma, beta, mean, var, g, packed_w, packed_b);
    VSK_CHECK_LAUNCH();
    return 0;
}

int vsk_cnn3d_conv(const Cnn3dConvArgs &A, int input_kind, hipStream_t st) {
    const dim3 grid((unsigned)((A.g.M + CNN3D_TILE_M - 1) / CNN3D_TILE_M), (unsigned)(A.g.Coutp / CNN3D_TILE_N));
    const bool vec4 = input_kind == CNN3D_IN_F32_NDHWC && A.g.Cin % 4 == 0 && ((uintptr_t)A.in & 15) == 0;
    if (input_kind == CNN3D_IN_U8_NDHWC) hipLaunchKernelGGL(conv3d_igemm<GATHER_U8>, grid, dim3(NT), 0, st, A);
    else if (vec4) hipLaunchKernelGGL(conv3d_igemm<GATHER_VEC4>, grid, dim3(NT), 0, st, A);
    else hipLaunchKernelGGL(conv3d_igemm<GATHER_SCALAR>, grid, dim3(NT), 0, st, A);
    VSK_CHECK_LAUNCH();
    return 0;
}

int vsk_cnn3d_mean(const Cnn3dMeanArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(cnn3d_mean, dim3(blocks_for((int64_t)A.N * A.C)), dim3(NT), 0, st, A);
    VSK_CHECK_LAUNCH();
    return 0;
}
