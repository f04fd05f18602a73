// vs_train_attention.hip — attention of the TRAINING path on gfx950: forward with dropout on the attention weights
// and a saved log-sum-exp, and the flash-style backward (reference simnet.py:155-161 under autograd).
//
// Exact fp32 on v_mfma_f32_32x32x2_f32 like the scoring path.  Conventions (vs_device.h): lane l, r = l & 31,
// h = l >> 5; A operand A[i = r][k = h], B operand B[k = h][j = r], accumulator register t holds
// D[row = acc_row(t, h)][col = r].  Two operand idioms are used throughout:
//   * "row fragment": a lane reads FOUR consecutive contraction indices kk = 8g + 4h + s of its row with one
//     ds_read_b128; MFMA step s contracts {8g + s, 8g + 4 + s}.  Both operands of a product use the same map.
//   * "accumulator as operand": a 32x32 result whose CONTRACTION index for the next product is its row index is used
//     register by register as that product's B operand (step t contracts rows acc_row(t,0), acc_row(t,1)); the other
//     operand is then read column-wise from a row-major LDS tile: ds_read_b32 at [acc_row(t,h)][c0 + r].
//
// Three kernels, all with 4 waves x 32 "owner" rows per block and the other sequence streamed through LDS in
// 32-row tiles (double-buffered, one barrier per tile):
//   attn_fwd_train   owner = queries.  S^T = K Q^T (lane = query), online softmax with the running maximum, dropout
//                    on the normalised-later weights, O^T += V^T P~^T; saves lse2 = log2 sum exp.
//   attn_bwd_dq      owner = queries.  S^T and dP^T = V dO^T recomputed, dS^T = P^T o (dP^T - delta), dQ^T += K^T dS^T.
//   attn_bwd_dkdv    owner = keys.     S = Q K^T and dP = dO V^T (lane = key), dV^T += dO^T P~, dK^T += Q^T dS.
// Recomputing S and dP in both backward kernels costs 7 products instead of 5 but needs no atomics and no
// cross-block hand-off: every output element is written once, by one wave, in a fixed order (bitwise reproducible).
// The dropout keep decisions come from vs_train_device.h's counter hash of (seed, site, (b*H + h)*T + query, key).
// DROP 1: every kernel evaluates the hash per element (13 vector instructions beside a 64-cycle MFMA: 20 % of the
// forward).  DROP 2 (round 3, the full training path): attn_dropout_bits evaluates it ONCE per layer into two bit-packed
// copies - one word per (query, 32 keys) for the kernels whose lanes own queries, one per (key, 32 queries) for the
// kernel whose lanes own keys - which the forward leaves in the activation record for the backward: a kernel reads one
// word per tile and lane and extracts a bit per element (3 instructions).  Same hash, same masks (GPU test: the two
// forms give bit-identical outputs).
//
// PACKED (packed ragged batches, vs_train_forward_packed): the videos' frames are concatenated, q / k / v are head-major over
// the packed rows ([H][Mtot][DH], what vsk_qkv writes for B = 1, T = Mtot), lse2 / delta are [H][Mtot] and out / dO / dqkv
// token-major over the packed rows.  A block takes (head, video, 128-row owner tile) from a work list built on the device
// (plan_packed_train) and streams only that video's rows cu[b] .. cu[b+1]: the difference to the padded form is confined to
// owner_tile() (vs_train_attention_owner.h) - where the block's rows, its keep words and its dropout row keys live - so a video's tile loops, LDS layout
// and summation order are those of the same video run alone.  No key mask: a packed batch has no padded rows.
#include "vs_launch.h"
#include "vs_train_attention_owner.h"
#include "vs_train_device.h"
#include "vs_train_kernels.h"

namespace {

constexpr float NEG_INF = -__builtin_inff();

template <int DH>
struct TileLds {                       // one staged 32-row tile pair + its per-row side data
    static constexpr int LD = DH + 4;  // 16 distinct rows x b128 then cover all 64 banks
    float a[32][LD];                   // K  (fwd, dq)  |  Q * scale * log2e (dkdv)
    float b[32][LD];                   // V  (fwd, dq)  |  dO               (dkdv)
    float s0[32];                      // key bias (0 / -inf)  |  lse2 (+inf on rows >= T)
    float s1[32];                      //                      |  delta
    unsigned rk[32];                   //                      |  dropout row keys
};

// global -> registers -> LDS staging of a 32 x DH tile pair by 256 threads (DH / 32 float4 per thread and matrix)
template <int DH>
struct Stager {
    static constexpr int NV = DH / 32;          // float4 per thread per matrix
    f32x4 va[NV], vb[NV];
    __device__ __forceinline__ void load(const float *pa, size_t lda, const float *pb, size_t ldb, int row0, int nrows,
                                         float mul_a) {
        const int tid = threadIdx.x;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + 256 * i, row = idx / (DH / 4), c4 = (idx % (DH / 4)) * 4;
            const bool ok = row0 + row < nrows;
            va[i] = ok ? *(const f32x4 *)(pa + (size_t)(row0 + row) * lda + c4) * mul_a : f32x4{0.f, 0.f, 0.f, 0.f};
            vb[i] = ok ? *(const f32x4 *)(pb + (size_t)(row0 + row) * ldb + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    __device__ __forceinline__ void store(TileLds<DH> &t) const {
        const int tid = threadIdx.x;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + 256 * i, row = idx / (DH / 4), c4 = (idx % (DH / 4)) * 4;
            *(f32x4 *)&t.a[row][c4] = va[i];
            *(f32x4 *)&t.b[row][c4] = vb[i];
        }
    }
};

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int t = 0; t < 16; ++t) z[t] = 0.f;
    return z;
}

// S^T tile (lane = query): sum_c K[key][c] * Qs[query][c] + key bias; keys in rows
template <int DH>
__device__ __forceinline__ f32x16 st_tile(const TileLds<DH> &t, const f32x4 (&qf)[DH / 8], int r, int h) {
    f32x16 s = zero16();
#pragma unroll
    for (int g = 0; g < DH / 8; ++g) {
        const f32x4 kf = *(const f32x4 *)&t.a[r][8 * g + 4 * h];
#pragma unroll
        for (int e = 0; e < 4; ++e) s = MFMA32(kf[e], qf[g][e], s);
    }
#pragma unroll
    for (int tg = 0; tg < 4; ++tg) {
        const f32x4 bv = *(const f32x4 *)&t.s0[8 * tg + 4 * h];
#pragma unroll
        for (int e = 0; e < 4; ++e) s[4 * tg + e] += bv[e];
    }
    return s;
}

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
template <int DH, int DROP, bool PACKED>        // DROP 0: none, 1: hash per element, 2: bit-packed keep masks (dbits)
__global__ __launch_bounds__(256) void attn_fwd_train(
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
    const uint8_t *__restrict__ mask, float *__restrict__ out, float *__restrict__ lse2, int H, int T_all, float scale,
    unsigned long long seed, unsigned site, float p, const unsigned *__restrict__ dbits, const VstPackedPlan pk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];      // 2 x TileLds<DH>: 68 KB at head dim 128
    TileLds<DH> *lds = reinterpret_cast<TileLds<DH> *>(lds_raw);
    const Owner own = owner_tile<PACKED>(H, T_all, pk);
    if (PACKED && own.T <= 0) return;
    const int T = own.T, qt = own.tile, hd = own.hd;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int qi = qt * 128 + wave * 32 + r, qc = qi < T ? qi : T - 1;
    const float sl2 = scale * 1.4426950408889634f;
    const float *qb = q + own.plane * DH, *kb = k + own.plane * DH, *vb = v + own.plane * DH;
    const DropSite ds = drop_site(seed, site, p);
    const unsigned rkq = drop_rowkey(ds, (unsigned)(own.plane + qc));

    f32x4 qf[DH / 8];
#pragma unroll
    for (int g = 0; g < DH / 8; ++g) qf[g] = *(const f32x4 *)(qb + (size_t)qc * DH + 8 * g + 4 * h) * sl2;
    f32x16 o[DH / 32];
#pragma unroll
    for (int cb = 0; cb < DH / 32; ++cb) o[cb] = zero16();
    float m_run = NEG_INF, l_run = 0.f;

    Stager<DH> sg;
    auto side = [&](TileLds<DH> &t, int key0) __attribute__((always_inline)) {
        if (tid < 32) {
            const int key = key0 + tid;
            t.s0[tid] = (key >= T || (!PACKED && mask != nullptr && mask[own.tok + key])) ? NEG_INF : 0.f;
        }
    };
    const int nkt = (T + 31) / 32;
    const unsigned *bq = DROP == 2 ? dbits + own.wbase + (size_t)qc * nkt : nullptr;      // this query's keep words
    unsigned kw = DROP == 2 ? bq[0] : 0u;
    sg.load(kb, DH, vb, DH, 0, T, 1.0f);
    sg.store(lds[0]);
    side(lds[0], 0);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const TileLds<DH> &t = lds[kt & 1];
        if (kt + 1 < nkt) sg.load(kb, DH, vb, DH, 32 * (kt + 1), T, 1.0f);
        const unsigned kw_cur = kw;
        if (DROP == 2 && kt + 1 < nkt) kw = bq[kt + 1];
        f32x16 s = st_tile<DH>(t, qf, r, h);
        float mx = s[0];
#pragma unroll
        for (int e = 1; e < 16; ++e) mx = fmaxf(mx, s[e]);
        mx = pair_max(mx);
        const float m_new = fmaxf(m_run, mx);
        const float m_use = m_new == NEG_INF ? 0.f : m_new;       // a row with no valid key so far: keep p = 0, not NaN
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
        float ls = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) { s[e] = __builtin_amdgcn_exp2f(s[e] - m_use); ls += s[e]; }
        l_run = l_run * alpha + ls;
        m_run = m_new;
        if (DROP == 1) {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                s[e] = drop_keep(ds, rkq, (unsigned)(32 * kt + acc_row(e, h))) ? s[e] * ds.scale : 0.f;
        }
        if (DROP == 2) {
            const unsigned kwh = kw_cur >> (4 * h);                  // bit acc_row(e, h) = (e & 3) + 8 (e >> 2) + 4 h
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = (kwh >> ((e & 3) + 8 * (e >> 2)) & 1u) ? s[e] * ds.scale : 0.f;
        }
#pragma unroll
        for (int cb = 0; cb < DH / 32; ++cb)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[cb][e] *= alpha;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
#pragma unroll
            for (int cb = 0; cb < DH / 32; ++cb) {
                const float vf = t.b[acc_row(e, h)][32 * cb + r];
                o[cb] = MFMA32(vf, s[e], o[cb]);
            }
        }
        if (kt + 1 < nkt) { sg.store(lds[(kt + 1) & 1]); side(lds[(kt + 1) & 1], 32 * (kt + 1)); }
        __syncthreads();
    }
    const float l_tot = pair_sum(l_run);
    const float inv = 1.0f / l_tot;         // l_tot == 0 (every key masked): NaN rows, like softmax of all -inf
    if (qi < T) {
        float *op = out + (own.tok + qi) * (H * DH) + hd * DH;
#pragma unroll
        for (int cb = 0; cb < DH / 32; ++cb)
#pragma unroll
            for (int tg = 0; tg < 4; ++tg) {
                f32x4 w;
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = o[cb][4 * tg + e] * inv;
                *(f32x4 *)(op + 32 * cb + 8 * tg + 4 * h) = w;
            }
        if (h == 0) lse2[own.plane + qi] = m_run + log2f(l_tot);
    }
}

// ------------------------------------------------------------------------------------------
// backward, queries own: dQ
// ------------------------------------------------------------------------------------------
template <int DH, int DROP, bool PACKED>
__global__ __launch_bounds__(256) void attn_bwd_dq(
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
    const uint8_t *__restrict__ mask, const float *__restrict__ dO, const float *__restrict__ lse2,
    const float *__restrict__ delta, float *__restrict__ dqkv, int H, int T_all, float scale, unsigned long long seed,
    unsigned site, float p, const unsigned *__restrict__ dbits, const VstPackedPlan pk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];      // 2 x TileLds<DH>: 68 KB at head dim 128
    TileLds<DH> *lds = reinterpret_cast<TileLds<DH> *>(lds_raw);
    const Owner own = owner_tile<PACKED>(H, T_all, pk);
    if (PACKED && own.T <= 0) return;
    const int T = own.T, qt = own.tile, hd = own.hd, d = H * DH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int qi = qt * 128 + wave * 32 + r, qc = qi < T ? qi : T - 1;
    const float sl2 = scale * 1.4426950408889634f;
    const float *qb = q + own.plane * DH, *kb = k + own.plane * DH, *vb = v + own.plane * DH;
    const DropSite ds = drop_site(seed, site, p);
    const unsigned rkq = drop_rowkey(ds, (unsigned)(own.plane + qc));

    f32x4 qf[DH / 8], dof[DH / 8];
#pragma unroll
    for (int g = 0; g < DH / 8; ++g) {
        qf[g] = *(const f32x4 *)(qb + (size_t)qc * DH + 8 * g + 4 * h) * sl2;
        dof[g] = *(const f32x4 *)(dO + (own.tok + qc) * d + hd * DH + 8 * g + 4 * h);
    }
    const float lq = lse2[own.plane + qc], dq_delta = delta[own.plane + qc];
    f32x16 acc[DH / 32];
#pragma unroll
    for (int cb = 0; cb < DH / 32; ++cb) acc[cb] = zero16();

    Stager<DH> sg;
    auto side = [&](TileLds<DH> &t, int key0) __attribute__((always_inline)) {
        if (tid < 32) {
            const int key = key0 + tid;
            t.s0[tid] = (key >= T || (!PACKED && mask != nullptr && mask[own.tok + key])) ? NEG_INF : 0.f;
        }
    };
    const int nkt = (T + 31) / 32;
    const unsigned *bq = DROP == 2 ? dbits + own.wbase + (size_t)qc * nkt : nullptr;
    unsigned kw = DROP == 2 ? bq[0] : 0u;
    sg.load(kb, DH, vb, DH, 0, T, 1.0f);
    sg.store(lds[0]);
    side(lds[0], 0);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const TileLds<DH> &t = lds[kt & 1];
        if (kt + 1 < nkt) sg.load(kb, DH, vb, DH, 32 * (kt + 1), T, 1.0f);
        const unsigned kwh = kw >> (4 * h);
        if (DROP == 2 && kt + 1 < nkt) kw = bq[kt + 1];
        f32x16 s = st_tile<DH>(t, qf, r, h);
        f32x16 dp = zero16();
#pragma unroll
        for (int g = 0; g < DH / 8; ++g) {
            const f32x4 vf = *(const f32x4 *)&t.b[r][8 * g + 4 * h];
#pragma unroll
            for (int e = 0; e < 4; ++e) dp = MFMA32(vf[e], dof[g][e], dp);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float pe = __builtin_amdgcn_exp2f(s[e] - lq);
            float g = dp[e];
            if (DROP == 1) g = drop_keep(ds, rkq, (unsigned)(32 * kt + acc_row(e, h))) ? g * ds.scale : 0.f;
            if (DROP == 2) g = (kwh >> ((e & 3) + 8 * (e >> 2)) & 1u) ? g * ds.scale : 0.f;
            s[e] = pe * (g - dq_delta);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
#pragma unroll
            for (int cb = 0; cb < DH / 32; ++cb) {
                const float kf = t.a[acc_row(e, h)][32 * cb + r];
                acc[cb] = MFMA32(kf, s[e], acc[cb]);
            }
        }
        if (kt + 1 < nkt) { sg.store(lds[(kt + 1) & 1]); side(lds[(kt + 1) & 1], 32 * (kt + 1)); }
        __syncthreads();
    }
    if (qi < T) {
        float *op = dqkv + (own.tok + qi) * (3 * d) + hd * DH;
#pragma unroll
        for (int cb = 0; cb < DH / 32; ++cb)
#pragma unroll
            for (int tg = 0; tg < 4; ++tg) {
                f32x4 w;
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = acc[cb][4 * tg + e] * scale;
                *(f32x4 *)(op + 32 * cb + 8 * tg + 4 * h) = w;
            }
    }
}

// ------------------------------------------------------------------------------------------
// backward, keys own: dK and dV
// ------------------------------------------------------------------------------------------
template <int DH, int DROP, bool PACKED>
__global__ __launch_bounds__(256) void attn_bwd_dkdv(
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
    const uint8_t *__restrict__ mask, const float *__restrict__ dO, const float *__restrict__ lse2,
    const float *__restrict__ delta, float *__restrict__ dqkv, int H, int T_all, float scale, unsigned long long seed,
    unsigned site, float p, const unsigned *__restrict__ dbits, const VstPackedPlan pk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];      // 2 x TileLds<DH>: 68 KB at head dim 128
    TileLds<DH> *lds = reinterpret_cast<TileLds<DH> *>(lds_raw);
    const Owner own = owner_tile<PACKED>(H, T_all, pk);
    if (PACKED && own.T <= 0) return;
    const int T = own.T, ktile = own.tile, hd = own.hd, d = H * DH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int ki = ktile * 128 + wave * 32 + r, kc = ki < T ? ki : T - 1;
    const float sl2 = scale * 1.4426950408889634f;
    const float *qb = q + own.plane * DH, *kb = k + own.plane * DH, *vb = v + own.plane * DH;
    const float *dob = dO + own.tok * d + hd * DH;          // row stride d
    const DropSite ds = drop_site(seed, site, p);

    f32x4 kf[DH / 8], vf[DH / 8];
#pragma unroll
    for (int g = 0; g < DH / 8; ++g) {
        kf[g] = *(const f32x4 *)(kb + (size_t)kc * DH + 8 * g + 4 * h);
        vf[g] = *(const f32x4 *)(vb + (size_t)kc * DH + 8 * g + 4 * h);
    }
    const float kbias = (ki >= T || (!PACKED && mask != nullptr && mask[own.tok + kc])) ? NEG_INF : 0.f;
    f32x16 dk[DH / 32], dv[DH / 32];
#pragma unroll
    for (int cb = 0; cb < DH / 32; ++cb) { dk[cb] = zero16(); dv[cb] = zero16(); }

    Stager<DH> sg;
    auto side = [&](TileLds<DH> &t, int q0) __attribute__((always_inline)) {
        if (tid < 32) {
            const int qi = q0 + tid;
            const bool ok = qi < T;
            t.s0[tid] = ok ? lse2[own.plane + qi] : __builtin_inff();      // p = exp2(s - inf) = 0 on rows >= T
            t.s1[tid] = ok ? delta[own.plane + qi] : 0.f;
            if (DROP == 1) t.rk[tid] = drop_rowkey(ds, (unsigned)(own.plane + (ok ? qi : 0)));
        }
    };
    const int nqt = (T + 31) / 32;
    // DROP 2: the key-major copy (second half of dbits): one word per (key, 32 queries)
    const unsigned *bk = DROP == 2 ? dbits + own.wall + own.wbase + (size_t)kc * nqt : nullptr;
    unsigned kw = DROP == 2 ? bk[0] : 0u;
    sg.load(qb, DH, dob, d, 0, T, sl2);
    sg.store(lds[0]);
    side(lds[0], 0);
    __syncthreads();
    for (int it = 0; it < nqt; ++it) {
        const TileLds<DH> &t = lds[it & 1];
        if (it + 1 < nqt) sg.load(qb, DH, dob, d, 32 * (it + 1), T, sl2);
        const unsigned kwh = kw >> (4 * h);
        if (DROP == 2 && it + 1 < nqt) kw = bk[it + 1];
        // S[query][key] - lse2[query]: the row constant is the accumulator's initial value
        f32x16 s, dp = zero16();
#pragma unroll
        for (int tg = 0; tg < 4; ++tg) {
            const f32x4 lv = *(const f32x4 *)&t.s0[8 * tg + 4 * h];
#pragma unroll
            for (int e = 0; e < 4; ++e) s[4 * tg + e] = -lv[e];
        }
#pragma unroll
        for (int g = 0; g < DH / 8; ++g) {
            const f32x4 qv = *(const f32x4 *)&t.a[r][8 * g + 4 * h];
            const f32x4 dov = *(const f32x4 *)&t.b[r][8 * g + 4 * h];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s = MFMA32(qv[e], kf[g][e], s);
                dp = MFMA32(dov[e], vf[g][e], dp);
            }
        }
        f32x16 pd;          // dropped-out probabilities (the B operand of dV)
#pragma unroll
        for (int tg = 0; tg < 4; ++tg) {
            const f32x4 dl = *(const f32x4 *)&t.s1[8 * tg + 4 * h];
            u32x4 rk4 = {0u, 0u, 0u, 0u};
            if (DROP == 1) rk4 = *(const u32x4 *)&t.rk[8 * tg + 4 * h];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 4 * tg + e;
                const float pe = __builtin_amdgcn_exp2f(s[i] + kbias);
                float g = dp[i], pk = pe;
                if (DROP != 0) {
                    const bool keep = DROP == 1 ? drop_keep(ds, rk4[e], (unsigned)ki) : (kwh >> (e + 8 * tg) & 1u) != 0u;
                    g = keep ? g * ds.scale : 0.f;
                    pk = keep ? pe * ds.scale : 0.f;
                }
                pd[i] = pk;
                s[i] = pe * (g - dl[e]);          // dS
            }
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
#pragma unroll
            for (int cb = 0; cb < DH / 32; ++cb) {
                const float dof = t.b[acc_row(e, h)][32 * cb + r];
                const float qf = t.a[acc_row(e, h)][32 * cb + r];
                dv[cb] = MFMA32(dof, pd[e], dv[cb]);
                dk[cb] = MFMA32(qf, s[e], dk[cb]);
            }
        }
        if (it + 1 < nqt) { sg.store(lds[(it + 1) & 1]); side(lds[(it + 1) & 1], 32 * (it + 1)); }
        __syncthreads();
    }
    if (ki < T) {
        float *op = dqkv + (own.tok + ki) * (3 * d) + hd * DH;
        const float ln2 = 0.6931471805599453f;       // dK = scale * dS^T Q = (dS^T Qs) / log2(e)
#pragma unroll
        for (int cb = 0; cb < DH / 32; ++cb)
#pragma unroll
            for (int tg = 0; tg < 4; ++tg) {
                f32x4 wk, wv;
#pragma unroll
                for (int e = 0; e < 4; ++e) { wk[e] = dk[cb][4 * tg + e] * ln2; wv[e] = dv[cb][4 * tg + e]; }
                *(f32x4 *)(op + d + 32 * cb + 8 * tg + 4 * h) = wk;
                *(f32x4 *)(op + 2 * d + 32 * cb + 8 * tg + 4 * h) = wv;
            }
    }
}

// The keep decisions of one layer's attention dropout, bit-packed twice: words [BH][T queries][W] with bit j of word w =
// keep(query, key 32 w + j), then words [BH][T keys][W] with bit j of word w = keep(query 32 w + j, key); W = ceil(T / 32).
// A wave owns 32 queries x 64 keys: lane l hashes query (l & 31) against the 32 keys of word (l >> 5); the transposed
// words come from 32 ballots (bit j of every lane's word = the column of key j).  Bits beyond T are 0.
// PACKED: blockIdx.y = video; BH = heads, rows / words of video b at (head * Mtot + cu[b]) / (head * words + bo[b]).
template <bool PACKED>
__global__ __launch_bounds__(256) void attn_dropout_bits(unsigned *__restrict__ bits, int BH, int T_all, unsigned long long seed,
                                                         unsigned site, float p, const VstPackedPlan pk) {
    const int r0 = PACKED ? pk.cu[blockIdx.y] : 0;
    const int T = PACKED ? pk.cu[blockIdx.y + 1] - r0 : T_all;
    const int W = (T + 31) / 32, W2 = (W + 1) / 2;
    const DropSite ds = drop_site(seed, site, p);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, g = lane >> 5;
    const size_t ntile = (size_t)BH * W * W2;
    unsigned *bitsK = bits + (PACKED ? (size_t)BH * pk.words : (size_t)BH * T * W);
    for (size_t tile = (size_t)blockIdx.x * 4 + wave; tile < ntile; tile += (size_t)gridDim.x * 4) {
        const int t2 = (int)(tile % W2), qt = (int)((tile / W2) % W), bh = (int)(tile / ((size_t)W2 * W));
        const size_t plane = PACKED ? (size_t)bh * pk.Mtot + r0 : (size_t)bh * T;               // dropout row key of query 0
        const size_t wbase = PACKED ? (size_t)bh * pk.words + pk.bo[blockIdx.y] : (size_t)bh * T * W;
        const int q = 32 * qt + r, kw = 2 * t2 + g;
        unsigned word = 0u;
        if (q < T && kw < W) {
            const unsigned rk = drop_rowkey(ds, (unsigned)(plane + q));
#pragma unroll 8
            for (int j = 0; j < 32; ++j) {
                const int key = 32 * kw + j;
                word |= (key < T && drop_keep(ds, rk, (unsigned)key)) ? (1u << j) : 0u;
            }
            bits[wbase + (size_t)q * W + kw] = word;
        }
        unsigned mine = 0u;
#pragma unroll 8
        for (int j = 0; j < 32; ++j) {
            const unsigned long long bal = __ballot((word >> j) & 1u);
            if (r == j) mine = g == 0 ? (unsigned)bal : (unsigned)(bal >> 32);
        }
        const int key = 64 * t2 + 32 * g + r;       // lane (r, g) holds the queries-of-this-tile word of key 64 t2 + 32 g + r
        if (key < T) bitsK[wbase + (size_t)key * W + qt] = mine;
    }
}

// cu [B+1] row offsets, bo [B+1] keep-word offsets (T_b * ceil(T_b / 32) words per video and head) and the (video, 128-row
// owner tile) work list of a packed batch, from DEVICE lengths (one thread: B is a few hundred at most).  The list is
// ordered longest video first (by its number of owner tiles): a block's time grows with the rows it streams, and the grid is
// a few waves of blocks deep, so the long blocks must not start last.  The host sized the launches from its copy of the
// lengths: a length is cut at the host's longest video tmax (the positional gather and the keep-word launch are sized by
// it) and rows beyond Mtot are cut, a video whose keep words would not fit in the words_cap words the host sized per head
// and copy gets length 0 (every consumer skips it: no tile in the list, cu[b + 1] == cu[b]), pairs beyond work_cap are
// dropped, and the unused tail of the list is marked (video -1: the block returns).  So cu, bo and the list are all bounded
// by what the host allocated, whatever the device lengths say.
__global__ void plan_packed_train(const int *__restrict__ lengths, int B, int Mtot, int tmax, unsigned words_cap,
                                  int *__restrict__ cu, int *__restrict__ bo, int *__restrict__ work, int work_cap) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int row = 0, words = 0, most = 0;
    for (int b = 0; b < B; ++b) {
        cu[b] = row;
        bo[b] = words;
        int t = lengths[b];
        t = t > tmax ? tmax : t;
        t = t < 0 ? 0 : (t > Mtot - row ? Mtot - row : t);
        if ((unsigned long long)words + (unsigned long long)t * ((t + 31) / 32) > words_cap) t = 0;
        most = (t + 127) / 128 > most ? (t + 127) / 128 : most;
        row += t;
        words += t * ((t + 31) / 32);
    }
    cu[B] = row;
    bo[B] = words;
    int n = 0;
    for (int nt = most; nt >= 1; --nt)
        for (int b = 0; b < B; ++b) {
            if ((cu[b + 1] - cu[b] + 127) / 128 != nt) continue;
            for (int q = 0; q < nt; ++q) {
                if (n < work_cap) { work[2 * n] = b; work[2 * n + 1] = q; }
                ++n;
            }
        }
    for (; n < work_cap; ++n) { work[2 * n] = -1; work[2 * n + 1] = 0; }
}

// keep[h][query][key] (bytes) of ONE video of a packed batch: T frames from packed row row0
__global__ __launch_bounds__(256) void attn_dropout_mask_video(uint8_t *__restrict__ keep, int H, int T, int Mtot, int row0,
                                                               unsigned long long seed, unsigned site, float p) {
    const DropSite ds = drop_site(seed, site, p);
    const size_t total = (size_t)H * T * T;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const unsigned j = (unsigned)(i % T), qh = (unsigned)(i / T), query = qh % (unsigned)T, hd = qh / (unsigned)T;
        keep[i] = drop_keep(ds, drop_rowkey(ds, hd * (unsigned)Mtot + (unsigned)row0 + query), j) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void attn_dropout_mask(uint8_t *__restrict__ keep, int BH, int T, unsigned long long seed,
                                                         unsigned site, float p) {
    const DropSite ds = drop_site(seed, site, p);
    const size_t total = (size_t)BH * T * T;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const unsigned j = (unsigned)(i % T), row = (unsigned)(i / T);       // row = bh * T + query
        keep[i] = drop_keep(ds, drop_rowkey(ds, row), j) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void rows_dropout_mask(uint8_t *__restrict__ keep, int M, int cols, unsigned long long seed,
                                                         unsigned site, float p) {
    const DropSite ds = drop_site(seed, site, p);
    const size_t total = (size_t)M * cols;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const unsigned c = (unsigned)(i % cols), row = (unsigned)(i / cols);
        keep[i] = drop_keep(ds, drop_rowkey(ds, row), c) ? 1 : 0;
    }
}

}  // namespace

// One launch of a kernel of this file: two staged tiles of dynamic LDS; above 64 KiB (head dim 128 up) the kernel's
// per-device limit is raised first (vs_launch.h).  Returns that raise's code, 0 once launched.
template <int DH, auto Kernel, class... Args>
static int launch_tiles(dim3 grid, hipStream_t st, Args... args) {
    constexpr size_t lds_bytes = 2 * sizeof(TileLds<DH>);
    if (const int rc = vsk_raise_lds<Kernel>(lds_bytes)) return rc;
    hipLaunchKernelGGL(Kernel, grid, dim3(256), lds_bytes, st, args...);
    return 0;
}
// rc = f(DH, DROP) with both as constants; DROP 0: p == 0, 2: bit-packed keep words given, 1: hashed per element.
// -1: no kernel for this head dim.
template <class F>
static int pick_dh_drop(int dh, float p, const unsigned *dbits, F &&f) {
    const int drop = !(p > 0.f) ? 0 : dbits != nullptr ? 2 : 1;
    int rc = 0;
    // head dim 256, round 4: correctness first (1 wave / SIMD, spills)
    const bool found = vsk_pick_int<32, 64, 128, 256>(dh, [&](auto DH) { vsk_pick_int<0, 1, 2>(drop, [&](auto DROP) { rc = f(DH, DROP); }); });
    return found ? rc : -1;
}

size_t vst_attention_dropout_bits_words(int B, int H, int T) { return 2 * (size_t)B * H * T * ((T + 31) / 32); }

// dbits (vst_attention_dropout_bits_words(B, H, T) words) <- both bit-packed copies of this layer's keep decisions
int vst_attention_dropout_bits(unsigned *dbits, int B, int H, int T, unsigned long long seed, unsigned site, float p,
                               hipStream_t st) {
    const int W = (T + 31) / 32;
    const size_t ntile = (size_t)B * H * W * ((W + 1) / 2);
    const int blocks = (int)((ntile + 3) / 4 < 16384 ? (ntile + 3) / 4 : 16384);
    hipLaunchKernelGGL(attn_dropout_bits<false>, dim3(blocks < 1 ? 1 : blocks), dim3(256), 0, st, dbits, B * H, T, seed, site, p,
                       VstPackedPlan{});
    VSK_CHECK_LAUNCH();
    return 0;
}

// ---- packed ragged batches ----
size_t vst_packed_plan_ints(int B, int work_cap) { return 2 * (size_t)(B + 1) + 2 * (size_t)work_cap; }

// plan (vst_packed_plan_ints(B, work_cap) ints) <- cu | bo | work from the device lengths; the VstPackedPlan of the kernels
int vst_plan_packed(const int *lengths_dev, int B, int Mtot, int tmax, size_t words, int *plan, int work_cap, hipStream_t st,
                    VstPackedPlan *pk) {
    int *cu = plan, *bo = plan + (B + 1), *work = plan + 2 * (B + 1);
    hipLaunchKernelGGL(plan_packed_train, dim3(1), dim3(64), 0, st, lengths_dev, B, Mtot, tmax, (unsigned)words, cu, bo, work,
                       work_cap);
    VSK_CHECK_LAUNCH();
    *pk = VstPackedPlan{cu, bo, work, work_cap, Mtot, (unsigned)words};
    return 0;
}

// dbits (2 * H * pk.words words) <- both bit-packed copies of the keep decisions of every video; tmax: the longest video
int vst_attention_dropout_bits_packed(unsigned *dbits, int B, int H, int tmax, unsigned long long seed, unsigned site, float p,
                                      hipStream_t st, const VstPackedPlan &pk) {
    const int W = (tmax + 31) / 32;
    const size_t ntile = (size_t)H * W * ((W + 1) / 2);
    const int blocks = (int)((ntile + 3) / 4 < 1024 ? (ntile + 3) / 4 : 1024);
    hipLaunchKernelGGL(attn_dropout_bits<true>, dim3(blocks < 1 ? 1 : blocks, B), dim3(256), 0, st, dbits, H, 0, seed, site, p, pk);
    VSK_CHECK_LAUNCH();
    return 0;
}

int vst_attention_fwd_packed(const float *q, const float *k, const float *v, float *out, float *lse2, int H, int dh, float scale,
                             unsigned long long seed, unsigned site, float p, hipStream_t st, const unsigned *dbits,
                             const VstPackedPlan &pk) {
    if (p < 0.f || p >= 1.f || pk.nwork <= 0) return -1;
    const dim3 grid(H * pk.nwork);
    const uint8_t *mask = nullptr;
    if (const int rc = pick_dh_drop(dh, p, dbits, [&](auto DH, auto DROP) {
            return launch_tiles<DH(), attn_fwd_train<DH(), DROP(), true>>(grid, st, q, k, v, mask, out, lse2, H, 0, scale, seed, site, p, dbits, pk);
        }))
        return rc;
    VSK_CHECK_LAUNCH();
    return 0;
}

int vst_attention_bwd_packed(const float *q, const float *k, const float *v, const float *dO, const float *lse2,
                             const float *delta, float *dqkv, int H, int dh, float scale, unsigned long long seed, unsigned site,
                             float p, hipStream_t st, const unsigned *dbits, const VstPackedPlan &pk) {
    if (p < 0.f || p >= 1.f || pk.nwork <= 0) return -1;
    const dim3 grid(H * pk.nwork);
    const uint8_t *mask = nullptr;
    if (const int rc = pick_dh_drop(dh, p, dbits, [&](auto DH, auto DROP) {
            return launch_tiles<DH(), attn_bwd_dkdv<DH(), DROP(), true>>(grid, st, q, k, v, mask, dO, lse2, delta, dqkv, H, 0, scale, seed, site, p, dbits, pk);
        }))
        return rc;
    VSK_CHECK_LAUNCH();
    if (const int rc = pick_dh_drop(dh, p, dbits, [&](auto DH, auto DROP) {
            return launch_tiles<DH(), attn_bwd_dq<DH(), DROP(), true>>(grid, st, q, k, v, mask, dO, lse2, delta, dqkv, H, 0, scale, seed, site, p, dbits, pk);
        }))
        return rc;
    VSK_CHECK_LAUNCH();
    return 0;
}

// test hook: keep (H * T * T bytes) of one video of a packed batch (T frames from packed row row0 of Mtot)
int vst_attention_dropout_mask_video(uint8_t *keep, int H, int T, int Mtot, int row0, unsigned long long seed, unsigned site,
                                     float p, hipStream_t st) {
    const size_t total = (size_t)H * T * T;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(attn_dropout_mask_video, dim3(blocks < 1 ? 1 : blocks), dim3(256), 0, st, keep, H, T, Mtot, row0, seed, site, p);
    VSK_CHECK_LAUNCH();
    return 0;
}

// dbits: the bit-packed keep masks (vst_attention_dropout_bits) or nullptr (the kernels then hash per element: same masks)
int vst_attention_fwd(const float *q, const float *k, const float *v, const uint8_t *mask, float *out, float *lse2,
                      int B, int H, int T, int dh, float scale, unsigned long long seed, unsigned site, float p,
                      hipStream_t st, const unsigned *dbits) {
    if (p < 0.f || p >= 1.f) return -1;
    const dim3 grid(B * H * ((T + 127) / 128));
    if (const int rc = pick_dh_drop(dh, p, dbits, [&](auto DH, auto DROP) {
            return launch_tiles<DH(), attn_fwd_train<DH(), DROP(), false>>(grid, st, q, k, v, mask, out, lse2, H, T, scale, seed, site, p, dbits, VstPackedPlan{});
        }))
        return rc;
    VSK_CHECK_LAUNCH();
    return 0;
}

int vst_attention_bwd(const float *q, const float *k, const float *v, const uint8_t *mask, const float *dO,
                      const float *lse2, const float *delta, float *dqkv, int B, int H, int T, int dh, float scale,
                      unsigned long long seed, unsigned site, float p, hipStream_t st, const unsigned *dbits) {
    if (p < 0.f || p >= 1.f) return -1;
    const dim3 grid(B * H * ((T + 127) / 128));
    if (const int rc = pick_dh_drop(dh, p, dbits, [&](auto DH, auto DROP) {
            return launch_tiles<DH(), attn_bwd_dkdv<DH(), DROP(), false>>(grid, st, q, k, v, mask, dO, lse2, delta, dqkv, H, T, scale, seed, site, p, dbits, VstPackedPlan{});
        }))
        return rc;
    VSK_CHECK_LAUNCH();
    if (const int rc = pick_dh_drop(dh, p, dbits, [&](auto DH, auto DROP) {
            return launch_tiles<DH(), attn_bwd_dq<DH(), DROP(), false>>(grid, st, q, k, v, mask, dO, lse2, delta, dqkv, H, T, scale, seed, site, p, dbits, VstPackedPlan{});
        }))
        return rc;
    VSK_CHECK_LAUNCH();
    return 0;
}

int vst_attention_dropout_mask(uint8_t *keep, int B, int H, int T, unsigned long long seed, unsigned site, float p,
                               hipStream_t st) {
    const size_t total = (size_t)B * H * T * T;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(attn_dropout_mask, dim3(blocks < 1 ? 1 : blocks), dim3(256), 0, st, keep, B * H, T, seed, site, p);
    VSK_CHECK_LAUNCH();
    return 0;
}

int vst_rows_dropout_mask(uint8_t *keep, int M, int cols, unsigned long long seed, unsigned site, float p, hipStream_t st) {
    const size_t total = (size_t)M * cols;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(rows_dropout_mask, dim3(blocks < 1 ? 1 : blocks), dim3(256), 0, st, keep, M, cols, seed, site, p);
    VSK_CHECK_LAUNCH();
    return 0;
}
