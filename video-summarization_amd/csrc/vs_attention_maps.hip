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
//
// Both passes exist twice over ONE body each (stats_tile / apply_tile, which see a single (video, head)): the padded kernels
// find the video as plane bh of [B, H, T, dh], the packed ones (probs_stats_packed / probs_apply_packed) as rows cu[b] ..
// cu[b + 1] - 1 of the head-major [H, M, dh] planes of a packed ragged batch, from a device-built (video, tile) list.  The
// packed tile walk starts at the video's own first row, so a packed video gets the bits of the padded kernel on it alone.
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
// One wave, queries q0 .. q0 + 31 of ONE (video, head): Qv / Kv are that video's [T, DH] planes, crow_v / ent_v its T row
// constants / entropies, mk its key mask or nullptr.  Where the video lies - plane bh of a padded batch, or rows cu[b] ..
// of a packed plane - is the calling kernel's business: the arithmetic below never sees it.
template <int DH>
__device__ __forceinline__ void stats_tile(const float *__restrict__ Qv, const float *__restrict__ Kv, const uint8_t *__restrict__ mk,
                                           float *__restrict__ crow_v, float *__restrict__ ent_v, int T, int q0, float scale_log2e,
                                           int r, int h) {
    constexpr int NJH = DH / 8 < 8 ? DH / 8 : 8;
    const float NEG_INF = -__builtin_inff();

    float qreg[DH / 2];
    {
        const int qr = q0 + r;
        load_fixed<DH>(Qv, qr < T ? qr : T - 1, h, scale_log2e, qreg);
    }
    float m_run = NEG_INF, l_run = 0.f, w_run = 0.f;      // w = sum_j e^(s_j - m) (s_j - m), log2 units, <= 0
    f32x4 a[NJH];
    const float *kp = stream_ptr<DH>(Kv, 0, T, r, h);
    load_group0<DH>(kp, a);
    for (int k0 = 0; k0 < T; k0 += 32) {
        f32x16 s = tile_scores<DH>(kp, a, 1.0f, qreg);
        if (k0 + 32 < T) {
            kp = stream_ptr<DH>(Kv, k0 + 32, T, r, h);
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
        const float lg = __log2f(l_run);
        crow_v[q] = m_run + lg;                              // log2 of the row's partition sum: p = exp2(s - c)
        if (ent_v != nullptr) ent_v[q] = LN2 * (lg - w_run / l_run);
    }
}

template <int DH>
__global__ __launch_bounds__(256) void probs_stats(
    const float *__restrict__ Q, const float *__restrict__ Kg, const uint8_t *__restrict__ mask, float *__restrict__ crow,
    float *__restrict__ entropy, int H, int T, float scale_log2e, int BH) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nq = (T + 31) / 32;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= nq * BH) return;
    const int bh = tile / nq, q0 = (tile - bh * nq) * 32;
    const int b = bh / H;
    const size_t base = (size_t)bh * T * DH, rbase = (size_t)bh * T;
    stats_tile<DH>(Q + base, Kg + base, mask ? mask + (size_t)b * T : nullptr, crow + rbase, entropy ? entropy + rbase : nullptr,
                   T, q0, scale_log2e, lane & 31, lane >> 5);
}

// Packed ragged batch: Q / Kg head-major [H, M, DH], video b = rows cu[b] .. cu[b + 1] - 1 of every head's plane.  A wave's
// unit is (head, video, 32-query tile OF THAT VIDEO) from the device work list: the tile walk starts at the video's own first
// row, so the wave runs stats_tile exactly as the padded kernel runs it for that video alone (B = 1, T = T_v, no mask) - the
// same bits, whatever is packed before it.  Rows past the video's end re-read its own last row: no load passes row M - 1.
template <int DH>
__global__ __launch_bounds__(256) void probs_stats_packed(
    const float *__restrict__ Q, const float *__restrict__ Kg, const int *__restrict__ cu, const int *__restrict__ work,
    float *__restrict__ crow, float *__restrict__ entropy, int H, int M, int ntiles, float scale_log2e) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= ntiles * H) return;
    const int head = tile / ntiles, w = tile - head * ntiles;
    const int b = work[2 * w], q0 = work[2 * w + 1] * 32;
    if (b < 0) return;                                       // the device lengths gave fewer tiles than the host's
    const int row0 = cu[b], T = cu[b + 1] - row0;
    const size_t rbase = (size_t)head * M + row0, base = rbase * DH;
    stats_tile<DH>(Q + base, Kg + base, nullptr, crow + rbase, entropy ? entropy + rbase : nullptr, T, q0, scale_log2e,
                   lane & 31, lane >> 5);
}

// ---- pass B: the weights themselves and / or their column means ----
// One wave, keys k0 .. k0 + 31 of ONE (video, head) for all of its queries: Qv / Kv / mk / crow_v as in stats_tile, maps_v the
// video's [T, T] block of this head (or nullptr), recv_v its T column means (or nullptr).
template <int DH>
__device__ __forceinline__ void apply_tile(const float *__restrict__ Qv, const float *__restrict__ Kv, const uint8_t *__restrict__ mk,
                                           const float *__restrict__ crow_v, float *__restrict__ maps_v, float *__restrict__ recv_v,
                                           int T, int k0, float scale_log2e, int lane) {
    constexpr int NJH = DH / 8 < 8 ? DH / 8 : 8;
    const int r = lane & 31, h = lane >> 5;

    const int key = k0 + r;
    const bool key_live = key < T && (mk == nullptr || mk[key] == 0);
    float kreg[DH / 2];
    load_fixed<DH>(Kv, key < T ? key : T - 1, h, 1.0f, kreg);

    float csum = 0.f;
    f32x4 a[NJH];
    const float *qp = stream_ptr<DH>(Qv, 0, T, r, h);
    load_group0<DH>(qp, a);
    for (int q0 = 0; q0 < T; q0 += 32) {
        // lane r: the row constant of query q0 + r and whether that query counts in `received` (one coalesced load each;
        // register t then takes them from lane acc_row(t, h))
        const int ql = q0 + r, qlc = ql < T ? ql : T - 1;
        const float c_lane = crow_v[qlc];
        const float v_lane = (ql < T && (mk == nullptr || mk[qlc] == 0)) ? 1.f : 0.f;
        const f32x16 s = tile_scores<DH>(qp, a, scale_log2e, kreg);
        if (q0 + 32 < T) {
            qp = stream_ptr<DH>(Qv, q0 + 32, T, r, h);
            load_group0<DH>(qp, a);
        }
        const bool all_count = mk == nullptr && q0 + 32 <= T;      // wave uniform
        float *mrow = maps_v != nullptr ? maps_v + (size_t)q0 * T + key : nullptr;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int row = acc_row(t, h);
            const float c = __shfl(c_lane, row);
            const float p = key_live ? __builtin_amdgcn_exp2f(s[t] - c) : 0.f;
            if (mrow != nullptr && q0 + row < T && key < T) mrow[(size_t)row * T] = p;
            csum += all_count ? p : p * __shfl(v_lane, row);
        }
    }
    if (recv_v != nullptr) {
        int n = 0;                                           // n_b: the video's valid queries
        for (int i0 = 0; i0 < T; i0 += 64) {
            const int i = i0 + lane;
            n += __popcll(__ballot(i < T && (mk == nullptr || mk[i] == 0)));
        }
        csum += __shfl_xor(csum, 32);
        if (h == 0 && key < T) recv_v[key] = csum / (float)n;
    }
}

template <int DH>
__global__ __launch_bounds__(256) void probs_apply(
    const float *__restrict__ Q, const float *__restrict__ Kg, const uint8_t *__restrict__ mask, const float *__restrict__ crow,
    float *__restrict__ maps, float *__restrict__ received, int H, int T, float scale_log2e, int BH) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nk = (T + 31) / 32;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= nk * BH) return;
    const int bh = tile / nk, k0 = (tile - bh * nk) * 32;
    const int b = bh / H;
    const size_t base = (size_t)bh * T * DH, rbase = (size_t)bh * T;
    apply_tile<DH>(Q + base, Kg + base, mask ? mask + (size_t)b * T : nullptr, crow + rbase, maps ? maps + rbase * (size_t)T : nullptr,
                   received ? received + rbase : nullptr, T, k0, scale_log2e, lane);
}

// Packed: a wave owns 32 keys of ONE video for all of that video's queries (`received` divides by T_v: every query of a
// packed video is valid).  maps: the videos' [H, T_v, T_v] blocks one after the other; moff[b] = sum over u < b of T_u^2 as a
// 64-bit value (H * moff passes 2^31 floats for ordinary corpora).
template <int DH>
__global__ __launch_bounds__(256) void probs_apply_packed(
    const float *__restrict__ Q, const float *__restrict__ Kg, const int *__restrict__ cu, const int *__restrict__ work,
    const unsigned long long *__restrict__ moff, const float *__restrict__ crow, float *__restrict__ maps,
    float *__restrict__ received, int H, int M, int ntiles, float scale_log2e) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= ntiles * H) return;
    const int head = tile / ntiles, w = tile - head * ntiles;
    const int b = work[2 * w], k0 = work[2 * w + 1] * 32;
    if (b < 0) return;
    const int row0 = cu[b], T = cu[b + 1] - row0;
    const size_t rbase = (size_t)head * M + row0, base = rbase * DH;
    float *maps_v = maps ? maps + ((size_t)H * moff[b] + (size_t)head * T * T) : nullptr;
    apply_tile<DH>(Q + base, Kg + base, nullptr, crow + rbase, maps_v, received ? received + rbase : nullptr, T, k0, scale_log2e, lane);
}

// The packed kernels' device-resident plan, from the DEVICE lengths (one thread: a few hundred videos at most, stream-ordered
// before its consumers): row offsets cu[B + 1], 64-bit map offsets moff[B], the (video, 32-row tile) list.  The host sized
// `work` (cap pairs) and the grid from ITS copy of the lengths: pairs beyond cap are dropped, slots the device lengths leave
// unused say video -1.
__global__ void probs_plan_packed(const int *__restrict__ lengths, int B, int *__restrict__ cu, unsigned long long *__restrict__ moff,
                                  int *__restrict__ work, int cap) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int row = 0, n = 0;
    unsigned long long sq = 0;
    for (int b = 0; b < B; ++b) {
        const int t = lengths[b];
        cu[b] = row;
        moff[b] = sq;
        for (int q = 0; q < (t + 31) / 32; ++q, ++n)
            if (n < cap) { work[2 * n] = b; work[2 * n + 1] = q; }
        row += t;
        sq += (unsigned long long)t * (unsigned long long)t;
    }
    cu[B] = row;
    for (; n < cap; ++n) { work[2 * n] = -1; work[2 * n + 1] = 0; }
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

// Workspace of the packed form: the row constants [H, M], then the plan - moff[B] (64-bit), cu[B + 1], work[tiles][2].
struct PackedWs {
    float *crow;
    unsigned long long *moff;
    int *cu, *work;
};
size_t packed_crow_bytes(int H, int M) { return ((size_t)H * M * sizeof(float) + 255) / 256 * 256; }
PackedWs packed_ws(void *workspace, int B, int H, int M) {
    PackedWs p;
    p.crow = (float *)workspace;
    p.moff = (unsigned long long *)((char *)workspace + packed_crow_bytes(H, M));
    p.cu = (int *)(p.moff + B);
    p.work = p.cu + B + 1;
    return p;
}

template <int DH>
int launch_packed(const float *q, const float *k, const int *cu, const PackedWs &p, float *maps, float *received, float *entropy,
                  int H, int M, int tiles, float scale, hipStream_t st) {
    const unsigned grid = (unsigned)(((long long)tiles * H + 3) / 4);
    const float sl2 = vsk_attention_qscale(scale);
    hipLaunchKernelGGL(probs_stats_packed<DH>, dim3(grid), dim3(256), 0, st, q, k, cu, (const int *)p.work, p.crow, entropy, H, M, tiles,
                       sl2);
    VSK_CHECK_LAUNCH();
    if (maps != nullptr || received != nullptr) {
        hipLaunchKernelGGL(probs_apply_packed<DH>, dim3(grid), dim3(256), 0, st, q, k, cu, (const int *)p.work,
                           (const unsigned long long *)p.moff, (const float *)p.crow, maps, received, H, M, tiles, sl2);
        VSK_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace

size_t vsk_attention_probs_packed_workspace_bytes(int B, int H, int M, int tiles) {
    const size_t plan = (size_t)B * sizeof(unsigned long long) + ((size_t)B + 1 + 2 * (size_t)tiles) * sizeof(int);
    return packed_crow_bytes(H, M) + (plan + 255) / 256 * 256;
}

int vsk_attention_probs_packed_plan(const int *lengths_dev, int B, int H, int M, int tiles, void *workspace, hipStream_t st) {
    const PackedWs p = packed_ws(workspace, B, H, M);
    hipLaunchKernelGGL(probs_plan_packed, dim3(1), dim3(64), 0, st, lengths_dev, B, p.cu, p.moff, p.work, tiles);
    VSK_CHECK_LAUNCH();
    return 0;
}

int vsk_attention_probs_packed(const float *q, const float *k, const int *cu, float *maps, float *received, float *entropy, int B,
                               int H, int M, int tiles, int dh, float scale, void *workspace, hipStream_t st) {
    if ((long long)tiles * H > (1ll << 30)) return -1;
    const PackedWs p = packed_ws(workspace, B, H, M);
    if (cu == nullptr) cu = p.cu;
    switch (dh) {
    case 32: return launch_packed<32>(q, k, cu, p, maps, received, entropy, H, M, tiles, scale, st);
    case 64: return launch_packed<64>(q, k, cu, p, maps, received, entropy, H, M, tiles, scale, st);
    case 128: return launch_packed<128>(q, k, cu, p, maps, received, entropy, H, M, tiles, scale, st);
    }
    return -1;
}

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
