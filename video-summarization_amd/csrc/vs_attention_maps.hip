// vs_attention_maps.hip — gfx950 kernels behind include/vs_inspect.h: the softmax weights P = softmax(q k^T * scale + keymask)
// of one attention layer (reference simnet.py:155-158, the tensor EncoderBlock.forward appends to attention_maps, :112-113),
// on request only.  The scoring kernels (vs_attention.hip) never form [T,T]; these read the same head-major q / k planes
// and produce
//   maps     [B,H,T,T]  the weights themselves (masked key columns exactly 0),
//   received [B,H,T]    (1/n_b) sum over the valid queries i of P[i, j]: the mean attention frame j receives,
//   entropy  [B,H,T]    -sum_j P log P per query, nats,
// the last two without ever storing [T,T].  Exact fp32 on v_mfma_f32_32x32x2_f32, head dim 32 / 64 / 128 / 256.
//
// Two passes, both built on ONE 32x32 score tile routine (tile_scores): a wave keeps 32 rows of one operand in registers
// ("fixed", the B operand: column r of the tile belongs to lane r / r + 32) and streams 32-row tiles of the other from
// global memory ("streamed", the A operand: accumulator register t holds streamed row acc_row(t, h)).  The q element is
// multiplied by scale * log2 e before the product in both passes, whichever side it is on, and the k-steps run in the
// same order, so both passes see the same bits of s.
//   probs_stats  (pass A) fixed = 32 QUERIES, streamed = keys: as in attn_fwd, the softmax statistics of a query are
//                lane-local plus one exchange with lane ^ 32.  Online softmax keeps m_i, l_i and w_i = sum_j e^(s-m)(s-m)
//                (the shifted form: every term <= 0, no large m_i cancels against a large sum), all in log2 units;
//                entropy_i = ln2 * (log2 l_i - w_i / l_i).  Stores c_i = m_i + log2 l_i, the log2 of the row's partition
//                sum, and (optionally) the entropy.
//   probs_apply  (pass B) fixed = 32 KEYS, streamed = queries: p = exp2(s - c_i).  With the keys on the lanes one
//                accumulator register is two 128-byte row segments of the map (rows acc_row(t, 0) and acc_row(t, 1), 32
//                consecutive keys each): the store shape MI355X_MICROARCH.md measures at full rate.  The stores are
//                per-lane dwords, so a row of any length T (65, 97, 130 ...) is written without touching its neighbours.
//                The wave owns its 32 keys for ALL queries, walked in order: the column sums need no atomics and no
//                cross-wave merge, two calls give the same bits and a video's result does not depend on its batch.
// No LDS, no barriers: the four waves of a block are independent (tile = 4 * block + wave).  The first fragment group of
// tile n + 1 is requested before the softmax / store epilogue of tile n.
#include "vs_device.h"
#include "vs_kernels.h"

namespace {

constexpr float LN2 = 0.69314718055994530942f;

// Fixed operand: row `row` (clamped by the caller) of a head-major [T, DH] plane, elements 8j + 4h .. + 3 for every j.
template <int DH>
__device__ __forceinline__ void load_fixed(const float *__restrict__ plane, int row, int h, float qmul, float (&f)[DH / 2]) {
    const float *p = plane + (size_t)row * DH + 4 * h;
#pragma unroll
    for (int j = 0; j < DH / 8; ++j) {
        const f32x4 v = *(const f32x4 *)(p + 8 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) f[4 * j + e] = v[e] * qmul;
    }
}

// First fragment group (<= 8 k-steps) of the streamed tile starting at row0 (rows beyond T re-read row T - 1; the caller
// masks them).  The loops below issue it for tile n + 1 before the epilogue of tile n.
template <int DH>
__device__ __forceinline__ const float *stream_ptr(const float *__restrict__ plane, int row0, int T, int r, int h) {
    int row = row0 + r; row = row < T ? row : T - 1;
    return plane + (size_t)row * DH + 4 * h;
}
template <int DH>
__device__ __forceinline__ void load_group0(const float *p, f32x4 (&a)[(DH / 8 < 8 ? DH / 8 : 8)]) {
    constexpr int NJ = DH / 8, NJH = NJ < 8 ? NJ : 8;
#pragma unroll
    for (int j = 0; j < NJH; ++j) a[j] = *(const f32x4 *)(p + 8 * j);
}

// s[t] = sum_d streamed[row acc_row(t, h)][d] * amul * fixed[col r][d]; a = the tile's first fragment group (load_group0),
// the later groups arrive one group ahead of their MFMAs.
template <int DH>
__device__ __forceinline__ f32x16 tile_scores(const float *p, f32x4 (&a)[(DH / 8 < 8 ? DH / 8 : 8)], float amul,
                                              const float (&fixed)[DH / 2]) {
    constexpr int NJ = DH / 8, NJH = NJ < 8 ? NJ : 8;
    f32x16 s;
#pragma unroll
    for (int t = 0; t < 16; ++t) s[t] = 0.f;
#pragma unroll
    for (int jh = 0; jh < NJ; jh += NJH) {
        f32x4 an[NJH];
        if (jh + NJH < NJ) {
#pragma unroll
            for (int j = 0; j < NJH; ++j) an[j] = *(const f32x4 *)(p + 8 * (jh + NJH + j));
        }
#pragma unroll
        for (int j = 0; j < NJH; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) s = MFMA32(a[j][e] * amul, fixed[4 * (jh + j) + e], s);
        if (jh + NJH < NJ) {
#pragma unroll
            for (int j = 0; j < NJH; ++j) a[j] = an[j];
        }
    }
    return s;
}

// ---- pass A: per-query softmax statistics (and entropy) ----
template <int DH>
__global__ __launch_bounds__(256) void probs_stats(
    const float *__restrict__ Q, const float *__restrict__ Kg, const uint8_t *__restrict__ mask, float *__restrict__ crow,
    float *__restrict__ entropy, int H, int T, float scale_log2e, int BH) {
    constexpr int NJH = DH / 8 < 8 ? DH / 8 : 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int nq = (T + 31) / 32;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= nq * BH) return;
    const int bh = tile / nq, q0 = (tile - bh * nq) * 32;
    const int b = bh / H;
    const size_t base = (size_t)bh * T * DH;
    const uint8_t *mk = mask ? mask + (size_t)b * T : nullptr;
    const float NEG_INF = -__builtin_inff();

    float qreg[DH / 2];
    {
        const int qr = q0 + r;
        load_fixed<DH>(Q + base, qr < T ? qr : T - 1, h, scale_log2e, qreg);
    }
    float m_run = NEG_INF, l_run = 0.f, w_run = 0.f;      // w = sum_j e^(s_j - m) (s_j - m), log2 units, <= 0
    f32x4 a[NJH];
    const float *kp = stream_ptr<DH>(Kg + base, 0, T, r, h);
    load_group0<DH>(kp, a);
    for (int k0 = 0; k0 < T; k0 += 32) {
        f32x16 s = tile_scores<DH>(kp, a, 1.0f, qreg);
        if (k0 + 32 < T) {
            kp = stream_ptr<DH>(Kg + base, k0 + 32, T, r, h);
            load_group0<DH>(kp, a);
        }
        if (mk != nullptr || k0 + 32 > T) {
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int key = k0 + acc_row(t, h);
                bool dead = key >= T;
                if (!dead && mk != nullptr) dead = mk[key] != 0;
                s[t] = dead ? NEG_INF : s[t];
            }
        }
        float mx = NEG_INF;
#pragma unroll
        for (int t = 0; t < 16; ++t) mx = fmaxf(mx, s[t]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = (m_new == NEG_INF) ? 0.f : m_new;      // nothing live yet: every p below is 0
        // sum e^(s - m_new)(s - m_new) over the old keys = alpha * (w + (m_run - m_new) * l); nothing when there were none
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
        const float shift = (m_run == NEG_INF) ? 0.f : (m_run - m_use) * l_run;
        float psum = 0.f, wsum = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const float ds = s[t] - m_use;
            const float p = __builtin_amdgcn_exp2f(ds);
            psum += p;
            wsum += (s[t] == NEG_INF) ? 0.f : p * ds;      // a masked key adds 0, not 0 * -inf
        }
        psum += __shfl_xor(psum, 32);
        wsum += __shfl_xor(wsum, 32);
        w_run = alpha * (w_run + shift) + wsum;
        l_run = alpha * l_run + psum;
        m_run = m_new;
    }
    const int q = q0 + r;
    if (q < T && h == 0) {
        const size_t o = (size_t)bh * T + q;
        const float lg = __log2f(l_run);
        crow[o] = m_run + lg;                                // log2 of the row's partition sum: p = exp2(s - c)
        if (entropy != nullptr) entropy[o] = LN2 * (lg - w_run / l_run);
    }
}

// ---- pass B: the weights themselves and / or their column means ----
template <int DH>
__global__ __launch_bounds__(256) void probs_apply(
    const float *__restrict__ Q, const float *__restrict__ Kg, const uint8_t *__restrict__ mask, const float *__restrict__ crow,
    float *__restrict__ maps, float *__restrict__ received, int H, int T, float scale_log2e, int BH) {
    constexpr int NJH = DH / 8 < 8 ? DH / 8 : 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int nk = (T + 31) / 32;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= nk * BH) return;
    const int bh = tile / nk, k0 = (tile - bh * nk) * 32;
    const int b = bh / H;
    const size_t base = (size_t)bh * T * DH, rbase = (size_t)bh * T;
    const uint8_t *mk = mask ? mask + (size_t)b * T : nullptr;

    const int key = k0 + r;
    const bool key_live = key < T && (mk == nullptr || mk[key] == 0);
    float kreg[DH / 2];
    load_fixed<DH>(Kg + base, key < T ? key : T - 1, h, 1.0f, kreg);

    float csum = 0.f;
    f32x4 a[NJH];
    const float *qp = stream_ptr<DH>(Q + base, 0, T, r, h);
    load_group0<DH>(qp, a);
    for (int q0 = 0; q0 < T; q0 += 32) {
        // lane r: the row constant of query q0 + r and whether that query counts in `received` (one coalesced load each;
        // register t then takes them from lane acc_row(t, h))
        const int ql = q0 + r, qlc = ql < T ? ql : T - 1;
        const float c_lane = crow[rbase + qlc];
        const float v_lane = (ql < T && (mk == nullptr || mk[qlc] == 0)) ? 1.f : 0.f;
        const f32x16 s = tile_scores<DH>(qp, a, scale_log2e, kreg);
        if (q0 + 32 < T) {
            qp = stream_ptr<DH>(Q + base, q0 + 32, T, r, h);
            load_group0<DH>(qp, a);
        }
        const bool all_count = mk == nullptr && q0 + 32 <= T;      // wave uniform
        float *mrow = maps != nullptr ? maps + (rbase + q0) * (size_t)T + key : nullptr;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int row = acc_row(t, h);
            const float c = __shfl(c_lane, row);
            const float p = key_live ? __builtin_amdgcn_exp2f(s[t] - c) : 0.f;
            if (mrow != nullptr && q0 + row < T && key < T) mrow[(size_t)row * T] = p;
            csum += all_count ? p : p * __shfl(v_lane, row);
        }
    }
    if (received != nullptr) {
        int n = 0;                                           // n_b: the video's valid queries
        for (int i0 = 0; i0 < T; i0 += 64) {
            const int i = i0 + lane;
            n += __popcll(__ballot(i < T && (mk == nullptr || mk[i] == 0)));
        }
        csum += __shfl_xor(csum, 32);
        if (h == 0 && key < T) received[rbase + key] = csum / (float)n;
    }
}

template <int DH>
int launch(const float *q, const float *k, const uint8_t *mask, float *maps, float *received, float *entropy, float *crow,
           int B, int H, int T, float scale, hipStream_t st) {
    const int BH = B * H;
    const long long tiles = (long long)BH * ((T + 31) / 32);
    if (tiles > (1ll << 30)) return -1;
    const unsigned grid = (unsigned)((tiles + 3) / 4);
    const float sl2 = vsk_attention_qscale(scale);
    hipLaunchKernelGGL(probs_stats<DH>, dim3(grid), dim3(256), 0, st, q, k, mask, crow, entropy, H, T, sl2, BH);
    VSK_CHECK_LAUNCH();
    if (maps != nullptr || received != nullptr) {
        hipLaunchKernelGGL(probs_apply<DH>, dim3(grid), dim3(256), 0, st, q, k, mask, (const float *)crow, maps, received,
                           H, T, sl2, BH);
        VSK_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace

size_t vsk_attention_probs_workspace_bytes(int B, int H, int T) {
    return ((size_t)B * H * T * sizeof(float) + 255) / 256 * 256;      // c = m + log2 l per (video, head, query)
}

int vsk_attention_probs(const float *q, const float *k, const uint8_t *mask, float *maps, float *received, float *entropy,
                        int B, int H, int T, int dh, float scale, void *workspace, hipStream_t st) {
    float *crow = (float *)workspace;
    switch (dh) {
    case 32: return launch<32>(q, k, mask, maps, received, entropy, crow, B, H, T, scale, st);
    case 64: return launch<64>(q, k, mask, maps, received, entropy, crow, B, H, T, scale, st);
    case 128: return launch<128>(q, k, mask, maps, received, entropy, crow, B, H, T, scale, st);
    case 256: return launch<256>(q, k, mask, maps, received, entropy, crow, B, H, T, scale, st);
    }
    return -1;
}
