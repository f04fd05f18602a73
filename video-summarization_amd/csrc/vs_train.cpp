// vs_train.cpp — the C ABI of include/vs_train.h: the train-mode forward of the scorer with its activation record,
// and the backward pass.  Launch sequences only; the kernels are in vs_kernels.hip (NT GEMMs, reused for every
// forward Linear and — against transposed weights — for every dgrad), vs_train_kernels.hip and
// vs_train_attention.hip.  Which form the record has and which mode word each launch gets is decided once per call, in
// vs_train_plan.h; forward_impl / backward_impl only read that plan.  The transposed weights of the
// backward are image families of the handle like the scoring side's: vsw_ensure (vs_weights.cpp) builds them.
#include "vs_train.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <string>

#include "vs_error.h"
#include "vs_train_device_sites.h"
#include "vs_train_kernels.h"
#include "vs_weights_impl.h"

namespace {

size_t align_floats(size_t n) { return (n + 63) / 64 * 64; }      // 256-byte granules

thread_local uint32_t g_last_format = 0;      // VsTrainPlan::format of this thread's last forward (vs_train_last_format)

// A packed ragged batch (vs_train_forward_packed) as the host sees it: every row-wise kernel runs it as ONE "video" of Mtot
// rows (B = 1, T = Mtot below); the positional rows, the attention, its keep words and the loss know the boundaries.
struct PackedCtx {
    int B = 0, Mtot = 0, tmax = 0, nwork = 0;      // nwork: (video, 128-row owner tile) pairs
    size_t words = 0;                              // keep words per head and orientation: sum T_b * ceil(T_b / 32)
    const int *lengths_dev = nullptr;
};

int packed_ctx(const vs_model_desc &D, const int32_t *lengths, int32_t B, PackedCtx &pc) {
    if (!lengths || B <= 0) return vs_failf(VS_ERR_INVALID, "lengths is NULL or B=%d", B);
    pc = PackedCtx{};
    pc.B = B;
    long long rows = 0, words = 0, nwork = 0;
    for (int b = 0; b < B; ++b) {
        const int t = lengths[b];
        if (t <= 0) return vs_failf(VS_ERR_INVALID, "lengths[%d]=%d", b, t);
        if (D.max_len > 0 && t > D.max_len)
            return vs_failf(VS_ERR_INVALID, "lengths[%d]=%d exceeds the positional table (max_len=%d)", b, t, D.max_len);
        rows += t; words += (long long)t * ((t + 31) / 32); nwork += (t + 127) / 128;
        pc.tmax = t > pc.tmax ? t : pc.tmax;
    }
    if (rows > (1ll << 28) || words >= (1ll << 31)) return vs_failf(VS_ERR_INVALID, "too many frames (%lld rows, %lld keep words per head)", rows, words);
    pc.Mtot = (int)rows; pc.words = (size_t)words; pc.nwork = (int)nwork;
    return VS_OK;
}

// ... of a call that has no model: any length fits
int packed_lengths(const int32_t *lengths, int32_t B, PackedCtx &pc) { return packed_ctx(vs_model_desc{}, lengths, B, pc); }

// ---- activation record (floats) ----
struct LayerSaved { size_t qkv, att, lse, z1, st1, y1, ffn, z2, st2, y2, dbits; };
struct SavedLayout {
    size_t h0 = 0, total = 0;
    std::vector<LayerSaved> layers;
};
SavedLayout saved_layout(const vs_model_desc &D, int B, int T, const PackedCtx *pc = nullptr) {
    SavedLayout S;
    const size_t M = (size_t)B * T, d = D.d_model;
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += align_floats(n); return o; };
    S.h0 = take(M * d);
    S.layers.resize(D.num_layers);
    for (auto &L : S.layers) {
        L.qkv = take(3 * M * d); L.att = take(M * d); L.lse = take((size_t)B * D.num_heads * T);
        L.z1 = take(M * d); L.st1 = take(2 * M); L.y1 = take(M * d);
        L.ffn = take(4 * M * d);
        L.z2 = take(M * d); L.st2 = take(2 * M); L.y2 = take(M * d);
        // the layer's attention keep masks, bit-packed (packed batches: per video, T_b * ceil(T_b / 32) words, not Mtot^2 / 32)
        L.dbits = take(pc ? 2 * (size_t)D.num_heads * pc->words : vst_attention_dropout_bits_words(B, D.num_heads, T));
    }
    S.total = off;
    return S;
}

// ---- scratch (floats): the forward uses `a` only ----
struct WorkLayout { size_t a, g0, g1, dz, dbr, gf, dy1, datt, dqkv, delta, part, wg, pe, plan, total; };
WorkLayout work_layout(const vs_model_desc &D, int B, int T, const PackedCtx *pc = nullptr) {
    WorkLayout W{};
    const size_t M = (size_t)B * T, d = D.d_model, din = D.in_features;
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += align_floats(n); return o; };
    W.a = take(M * d);
    W.g0 = take(M * d); W.g1 = take(M * d);
    W.dz = take(M * d); W.dbr = take(M * d);
    W.gf = take(4 * M * d);
    W.dy1 = take(M * d); W.datt = take(M * d);
    W.dqkv = take(3 * M * d);
    W.delta = take((size_t)B * D.num_heads * T);
    const size_t nblk = (size_t)vst_ln_bwd_blocks((int)M);
    W.part = take(nblk * (2 * d + 2));
    size_t wg = 0;                      // the largest split-partial area of the five weight shapes [N, K]
    const size_t shapes[5][2] = {{d, 4 * d}, {4 * d, d}, {d, d}, {3 * d, d}, {d, din}};
    for (auto &s : shapes) {
        const size_t f = vst_wgrad_workspace_floats((int)M, (int)s[0], (int)s[1]);
        wg = f > wg ? f : wg;
    }
    W.wg = take(wg);
    // packed batches: the positional rows gathered per frame (forward) and the device plan (cu | bo | work list)
    W.pe = take(pc && D.max_len > 0 ? M * d : 0);
    W.plan = take(pc ? vst_packed_plan_ints(pc->B, pc->nwork) : 0);
    W.total = off;
    return W;
}

// Where field `field` of layer `layer` lies in the record (test / inspection hook); field 4, the log-sum-exp rows, is laid out
// per head over the packed rows and exists for packed batches only
int saved_field(const vs_weights *w, int B, int T, const PackedCtx *pc, int layer, int field, size_t *offset_bytes, size_t *count) {
    const LayerSaved A = saved_layout(w->desc, B, T, pc).layers[layer];
    const size_t M = (size_t)B * T, Md = M * w->desc.d_model;
    size_t off, n;
    switch (field) {
        case 0: off = A.ffn; n = 4 * Md; break;
        case 1: off = A.att; n = Md; break;
        case 2: off = A.y1; n = Md; break;
        case 3: off = A.y2; n = Md; break;
        case 4: if (pc) { off = A.lse; n = M * w->desc.num_heads; break; }
            [[fallthrough]];
        default: return vs_failf(VS_ERR_INVALID, "saved_field: unknown field %d", field);
    }
    *offset_bytes = off * sizeof(float);
    *count = n;
    return VS_OK;
}

// The checks of both directions that need no buffer, in their order: w / x, the plan's own (B, T, the positional table, the
// dropout probabilities - and, in the backward, a handed-back record form), x's alignment, the device.  No device work yet.
int plan_call(const vs_weights *w, const float *x, int B, int T, const vs_dropout_cfg *drop, bool packed, bool backward,
              VsTrainPlan *plan) {
    if (!w || !x) return vs_failf(VS_ERR_INVALID, "weights/x is NULL");
    const VsTrainIn in{w->desc.d_model, w->desc.num_heads, w->desc.max_len, w->has_pe, B, T, packed, drop ? drop->flags : 0u,
                       drop ? drop->p : 0.f, drop ? drop->p_embed : 0.f, drop ? drop->reserved : 0u, backward};
    std::string err;
    if (int rc = vs_train_plan(in, vsk_options(), plan, &err)) return vs_fail_msg(rc, err.c_str());
    if ((uintptr_t)x & 15) return vs_failf(VS_ERR_INVALID, "x must be 16-byte aligned");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != w->device)
        return vs_failf(VS_ERR_INVALID, "called on device %d, the weights handle lives on device %d", dev, w->device);
    return VS_OK;
}

// size and alignment of the record and the scratch; `hidden`: the forward's optional output
int check_buffers(const SavedLayout &S, const WorkLayout &W, const void *saved, size_t saved_bytes, const void *workspace,
                  size_t workspace_bytes, bool forward, const void *hidden) {
    if (saved_bytes < S.total * sizeof(float))
        return vs_failf(VS_ERR_WORKSPACE, "saved %zu bytes < %zu needed", saved_bytes, S.total * sizeof(float));
    if (workspace_bytes < W.total * sizeof(float))
        return vs_failf(VS_ERR_WORKSPACE, "workspace %zu bytes < %zu needed", workspace_bytes, W.total * sizeof(float));
    if (((uintptr_t)saved & 255) || ((uintptr_t)workspace & 255) || (hidden && ((uintptr_t)hidden & 15)))
        return vs_fail_msg(VS_ERR_INVALID, forward ? "saved/workspace must be 256-byte, hidden 16-byte aligned" : "saved/workspace must be 256-byte aligned");
    return VS_OK;
}

}  // namespace

extern "C" {

int vs_train_prepare(vs_weights *w, void *stream) {
    if (!w) return vs_failf(VS_ERR_INVALID, "weights is NULL");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != w->device)
        return vs_failf(VS_ERR_INVALID, "called on device %d, the weights handle lives on device %d", dev, w->device);
    return vsw_ensure(w, VSW_TRANSPOSED, stream);       // allocates the second blob: a caller can do that outside its backward pass
}

size_t vs_train_saved_bytes(const vs_weights *w, int32_t B, int32_t T) {
    if (!w || B <= 0 || T <= 0) return 0;
    return saved_layout(w->desc, B, T).total * sizeof(float);
}

size_t vs_train_workspace_bytes(const vs_weights *w, int32_t B, int32_t T) {
    if (!w || B <= 0 || T <= 0) return 0;
    return work_layout(w->desc, B, T).total * sizeof(float);
}

int vs_train_saved_field(const vs_weights *w, int32_t B, int32_t T, int32_t layer, int32_t field, size_t *offset_bytes,
                         size_t *count) {
    if (!w || !offset_bytes || !count || B <= 0 || T <= 0 || layer < 0 || layer >= w->desc.num_layers)
        return vs_failf(VS_ERR_INVALID, "saved_field: bad arguments");
    return saved_field(w, B, T, nullptr, layer, field, offset_bytes, count);
}

uint32_t vs_train_last_format(void) { return g_last_format; }

uint32_t vs_train_dropout_site(int32_t layer, int32_t which) { return layer < 0 ? VS_SITE_EMBED : VS_SITE_LAYER(layer, which); }

// pc != nullptr: a packed ragged batch, B = 1 and T = Mtot (no key mask)
// One layer's attention, forward and backward, on the kernel the plan names.  q / k / v: planes `kv_stride` floats apart;
// dbits: the layer's bit-packed keep words (p > 0) - the 16-bit kernels have no hash-per-element form, the exact ones take either
static int attention_forward(const VsTrainPlan &plan, const float *qkv, const uint8_t *key_pad_mask, float *out, float *lse, int B,
                             int H, int T, int dh, float scale, unsigned long long seed, unsigned site, float p,
                             const unsigned *dbits, const VstPackedPlan &pk, hipStream_t st) {
    const float *q = qkv, *k = qkv + plan.kv_stride, *v = qkv + 2 * plan.kv_stride;
    switch (plan.attention) {
        case VST_ATT_PACKED16: VS_LAUNCH(vst_attention_fwd_bf16_packed(q, k, v, out, lse, H, dh, scale, p, dbits, st, plan.form.f16, pk)); break;
        case VST_ATT_PACKED_EXACT: VS_LAUNCH(vst_attention_fwd_packed(q, k, v, out, lse, H, dh, scale, seed, site, p, st, dbits, pk)); break;
        case VST_ATT_PADDED16:
            VS_LAUNCH(vst_attention_fwd_bf16(q, k, v, key_pad_mask, out, lse, B, H, T, dh, scale, p, dbits, st, plan.mode_attention));
            break;
        case VST_ATT_PADDED_EXACT: VS_LAUNCH(vst_attention_fwd(q, k, v, key_pad_mask, out, lse, B, H, T, dh, scale, seed, site, p, st, dbits)); break;   // :155-161
    }
    return VS_OK;
}

static int attention_backward(const VsTrainPlan &plan, const float *qkv, const uint8_t *key_pad_mask, const float *datt, const float *lse,
                              const float *delta, float *dqkv, int B, int H, int T, int dh, float scale, unsigned long long seed,
                              unsigned site, float p, const unsigned *dbits, const VstPackedPlan &pk, hipStream_t st) {
    const float *q = qkv, *k = qkv + plan.kv_stride, *v = qkv + 2 * plan.kv_stride;
    switch (plan.attention) {
        case VST_ATT_PACKED16:
            VS_LAUNCH(vst_attention_bwd_bf16_packed(q, k, v, datt, lse, delta, dqkv, H, dh, scale, p, dbits, st, plan.form.f16, pk));
            break;
        case VST_ATT_PACKED_EXACT:
            VS_LAUNCH(vst_attention_bwd_packed(q, k, v, datt, lse, delta, dqkv, H, dh, scale, seed, site, p, st, dbits, pk));
            break;
        case VST_ATT_PADDED16:
            VS_LAUNCH(vst_attention_bwd_bf16(q, k, v, key_pad_mask, datt, lse, delta, dqkv, B, H, T, dh, scale, p, dbits, st,
                                              plan.mode_attention, plan.attention_out16));
            break;
        case VST_ATT_PADDED_EXACT:
            VS_LAUNCH(vst_attention_bwd(q, k, v, key_pad_mask, datt, lse, delta, dqkv, B, H, T, dh, scale, seed, site, p, st, dbits));
            break;
    }
    return VS_OK;
}

// pc != nullptr: a packed ragged batch, B = 1 and T = Mtot (no key mask)
static int forward_impl(const vs_weights *w, const float *x, const uint8_t *key_pad_mask, int32_t B, int32_t T,
                        const vs_dropout_cfg *drop, float *scores, float *hidden, void *saved, size_t saved_bytes,
                        void *workspace, size_t workspace_bytes, void *stream, const PackedCtx *pc) {
    VsTrainPlan plan;
    if (int rc = plan_call(w, x, B, T, drop, pc != nullptr, false, &plan)) return rc;
    if (!scores || !saved || !workspace) return vs_failf(VS_ERR_INVALID, "scores/saved/workspace is NULL");
    const vs_model_desc &D = w->desc;
    const SavedLayout S = saved_layout(D, B, T, pc);
    const WorkLayout W = work_layout(D, B, T, pc);
    if (int rc = check_buffers(S, W, saved, saved_bytes, workspace, workspace_bytes, true, hidden)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int d = D.d_model, H = D.num_heads, L = D.num_layers, M = B * T;
    const float p = drop ? drop->p : 0.f;
    // the embedding dropout lives INSIDE PositionalEncoding (simnet.py:224,237): a use_pos=False model has none
    const float p_embed = (drop && w->has_pe) ? drop->p_embed : 0.f;
    g_last_format = plan.format;
    const unsigned long long seed = drop ? drop->seed : 0ull;
    const int dn = w->dn();                                   // LayerNorm width / attention-scale d_model (== d unless embedded)
    const float scale = 1.0f / sqrtf((float)dn);             // simnet.py:126: d_model ** -0.5
    float *sv = (float *)saved, *ws = (float *)workspace;
    float *a = ws + W.a;

    vsw_order(w, stream);
    if (plan.families) if (int rc = vsw_ensure(w, plan.families, stream)) return rc;
    // packed: the device builds cu / bo / the work list from the device lengths (no host memory is read after return), and
    // the positional rows are gathered per video - the embedding then adds row m of them to frame m
    VstPackedPlan pk{};
    const float *pe = w->has_pe ? w->p(w->pe) : nullptr;
    if (pc) {
        VS_LAUNCH(vst_plan_packed(pc->lengths_dev, pc->B, M, pc->tmax, pc->words, (int *)(ws + W.plan), pc->nwork, st, &pk));
        if (w->has_pe) {
            VS_LAUNCH(vsk_gather_rows(w->p(w->pe), pk.cu, pc->B, pc->tmax, d, ws + W.pe, st));
            pe = ws + W.pe;
        }
    }
    // Embedding + positional table + dropout(sparsity)   simnet.py:211, 237-238
    float *h0 = sv + S.h0;
    VS_LAUNCH(vsk_linear(x, w->p(w->embed_w), w->p(w->f_embed_w), w->p(w->embed_b), h0, M, d, D.in_features, 0,
                          pe, T, plan.mode_linear, st));
    if (p_embed > 0.f) VS_LAUNCH(vst_dropout_rows(h0, M, d, seed, VS_SITE_EMBED, p_embed, st));
    const float *h_in = h0;
    for (int l = 0; l < L; ++l) {
        const LayerOff &P = w->layers[l];
        const LayerSaved &A = S.layers[l];
        const bool last = l == L - 1;
        float *qkv = sv + A.qkv;
        // (16-bit q / k / v: q arrives times scale * log2 e, the scoring path's form)
        if (plan.qkv_rows16)       // A-stationary form (bit-identical to the tiled one)
            VS_LAUNCH(vst_gemm_rows16(h_in, w->p(P.r_wqkv), w->p(P.bqkv), qkv, nullptr, M, 3 * d, d, 3, vsk_attention_qscale(scale), 0ull, 0u,
                                       0.f, st, T, H, d / H));
        else
            VS_LAUNCH(vsk_qkv(h_in, w->p(P.wqkv), w->p(P.f_wqkv), w->p(P.bqkv), qkv, B, T, d, H, plan.mode_qkv, st,
                               plan.form.qkv16 ? vsk_attention_qscale(scale) : 1.0f));         // :148-153
        unsigned *dbits = p > 0.f ? (unsigned *)(sv + A.dbits) : nullptr;
        if (dbits && pc) VS_LAUNCH(vst_attention_dropout_bits_packed(dbits, pc->B, H, pc->tmax, seed, VS_SITE_LAYER(l, VS_SITE_ATTN), p, st, pk));
        else if (dbits) VS_LAUNCH(vst_attention_dropout_bits(dbits, B, H, T, seed, VS_SITE_LAYER(l, VS_SITE_ATTN), p, st));
        if (int rc = attention_forward(plan, qkv, key_pad_mask, sv + A.att, sv + A.lse, B, H, T, d / H, scale, seed,
                                       VS_SITE_LAYER(l, VS_SITE_ATTN), p, dbits, pk, st)) return rc;
        VS_LAUNCH(vsk_linear(sv + A.att, w->p(P.wo), w->p(P.f_wo), w->p(P.bo), a, M, d, d, 0, nullptr, 1, plan.mode_linear, st));      // :163
        VS_LAUNCH(vst_rows_fwd(a, h_in, w->p(P.ln1g), w->p(P.ln1b), sv + A.z1, sv + A.y1, nullptr, sv + A.st1, M, d,
                                seed, VS_SITE_LAYER(l, VS_SITE_DROP1), p, nullptr, nullptr, 0, nullptr, st, dn));              // :107
        // fc1 (+ ReLU + mlp.dropout in the GEMM epilogue, :181) writes the MLP hidden tensor, fc2 reads it
        if (plan.form.rows16)         // the A-stationary form (vs_train_gemm_rows.hip), bit-identical to the tiled one
            VS_LAUNCH(vst_gemm_rows16(sv + A.y1, w->p(P.r_w1), w->p(P.b1), sv + A.ffn, nullptr, M, 4 * d, d, p > 0.f ? 0 : 2, 0.f, seed,
                                       VS_SITE_LAYER(l, VS_SITE_MLP), p, st));
        else if (p > 0.f)
            VS_LAUNCH(vsk_linear_relu_dropout(sv + A.y1, w->p(P.w1), w->p(P.f_w1), w->p(P.b1), sv + A.ffn, M, 4 * d, d, seed,
                                               VS_SITE_LAYER(l, VS_SITE_MLP), p, st, plan.mode_fc1));
        else
            VS_LAUNCH(vsk_linear(sv + A.y1, w->p(P.w1), w->p(P.f_w1), w->p(P.b1), sv + A.ffn, M, 4 * d, d, 1, nullptr, 1, plan.mode_fc1, st));
        VS_LAUNCH(vsk_linear(sv + A.ffn, w->p(P.w2), w->p(P.f_w2), w->p(P.b2), a, M, d, 4 * d, 0, nullptr, 1, plan.mode_fc2, st));  // :182
        VS_LAUNCH(vst_rows_fwd(a, sv + A.y1, w->p(P.ln2g), w->p(P.ln2b), sv + A.z2, sv + A.y2, last ? hidden : nullptr,
                                sv + A.st2, M, d, seed, VS_SITE_LAYER(l, VS_SITE_DROP2), p,
                                last ? w->p(w->final_w) : nullptr, last ? w->p(w->final_b) : nullptr, D.num_classes,
                                last ? scores : nullptr, st, dn));                                                              // :110, :42
        h_in = sv + A.y2;
    }
    return VS_OK;
}

static int backward_impl(vs_weights *w, const float *x, const uint8_t *key_pad_mask, int32_t B, int32_t T,
                         const vs_dropout_cfg *drop, const float *d_scores, const float *d_hidden, const void *saved,
                         size_t saved_bytes, const vs_model_grads *grads, float *dx, void *workspace,
                         size_t workspace_bytes, void *stream, const PackedCtx *pc) {
    VsTrainPlan plan;       // the form the record was written in: handed back in drop->reserved, else derived again
    if (int rc = plan_call(w, x, B, T, drop, pc != nullptr, true, &plan)) return rc;
    if (!saved || !workspace || !grads || !grads->layers || !grads->embed_w || !grads->embed_b || !grads->final_w ||
        !grads->final_b)
        return vs_failf(VS_ERR_INVALID, "saved/workspace/grads is NULL");
    const vs_model_desc &D = w->desc;
    const SavedLayout S = saved_layout(D, B, T, pc);
    const WorkLayout W = work_layout(D, B, T, pc);
    if (int rc = check_buffers(S, W, saved, saved_bytes, workspace, workspace_bytes, false, nullptr)) return rc;
    hipStream_t st = (hipStream_t)stream;
    // W^T for the dgrad GEMMs, and the copies of it only some kernels read (the second blob is allocated by the first such call)
    if (int rc = vsw_ensure(w, VSW_TRANSPOSED | (plan.transposed_fragments ? (unsigned)VSW_TRANSPOSED_FRAGMENTS : 0u) |
                                   (plan.t16 ? (unsigned)VSW_TRANSPOSED_W2_16 : 0u), stream)) return rc;
    const int d = D.d_model, H = D.num_heads, L = D.num_layers, M = B * T, nc = D.num_classes;
    const float p = drop ? drop->p : 0.f;
    // the embedding dropout lives INSIDE PositionalEncoding (simnet.py:224,237): a use_pos=False model has none
    const float p_embed = (drop && w->has_pe) ? drop->p_embed : 0.f;
    const unsigned long long seed = drop ? drop->seed : 0ull;
    const int dn = w->dn();
    const float scale = 1.0f / sqrtf((float)dn);
    const float *sv = (const float *)saved;
    float *ws = (float *)workspace;
    float *g[2] = {ws + W.g0, ws + W.g1};
    float *dz = ws + W.dz, *dbr = ws + W.dbr, *gf = ws + W.gf, *dy1 = ws + W.dy1, *datt = ws + W.datt;
    float *dqkv = ws + W.dqkv, *delta = ws + W.delta, *part = ws + W.part, *wg = ws + W.wg;
    const float *zeros = w->tp(w->zeros);
    const int nblk = vst_ln_bwd_blocks(M);
    VstPackedPlan pk{};       // packed: the plan is rebuilt from the device lengths (one small launch), not kept in the record
    if (pc) VS_LAUNCH(vst_plan_packed(pc->lengths_dev, pc->B, M, pc->tmax, pc->words, (int *)(ws + W.plan), pc->nwork, st, &pk));

    // final_layer (simnet.py:42): d_W = d_scores^T hidden, d_b = column sums of d_scores
    {
        const float *y_last = sv + S.layers[L - 1].y2;
        if (d_scores) {
            for (int c = 0; c < nc; ++c) {
                VS_LAUNCH(vst_weighted_colsum(d_scores + c, nc, y_last, part, M, d, st));
                VS_LAUNCH(vst_reduce_rows(part, nblk, 1, d, grads->final_w + (size_t)c * d, nullptr, nullptr, 1, st));
                VS_LAUNCH(vst_reduce_rows(part + (size_t)nblk * d, nblk, 1, 1, grads->final_b + c, nullptr, nullptr, 1, st));
            }
        } else {
            VS_HIP(hipMemsetAsync(grads->final_w, 0, (size_t)nc * d * sizeof(float), st));
            VS_HIP(hipMemsetAsync(grads->final_b, 0, (size_t)nc * sizeof(float), st));
        }
    }

    int cur = 0;
    for (int l = L - 1; l >= 0; --l) {
        const LayerOff &P = w->layers[l];
        const LayerOffT &Q = w->tlayers[l];
        const LayerSaved &A = S.layers[l];
        const vs_layer_grads &G = grads->layers[l];
        const bool last = l == L - 1;
        const float *h_in = l == 0 ? sv + S.h0 : sv + S.layers[l - 1].y2;
        // norm2 (+ the score head's pull on the last layer); d(fc2 output) = dropout2 mask on dz2
        VS_LAUNCH(vst_ln_bwd(last ? d_hidden : g[cur], last ? d_scores : nullptr, w->p(w->final_w), nc, sv + A.z2, sv + A.st2,
                              w->p(P.ln2g), dz, p > 0.f ? dbr : nullptr, part, M, d, seed, VS_SITE_LAYER(l, VS_SITE_DROP2), p, st, dn));
        VS_LAUNCH(vst_reduce_rows(part, nblk, 2, d, G.ln2_g, G.ln2_b, nullptr, 1, st));
        const float *dm = p > 0.f ? dbr : dz;
        // mlp.fc2: weight/bias gradient, then the gradient of its input
        VS_LAUNCH(vst_wgrad(dm, d, sv + A.ffn, 4 * d, M, d, 4 * d, G.w2, nullptr, nullptr, G.b2, nullptr, nullptr, d, wg, st, plan.mode_wgrad_w2));
        // ... through mlp.dropout + ReLU in the GEMM's epilogue: the saved activation is > 0 exactly where both let
        // the value through (the gated gradient gf is stored the way the activation is: plan.mode_gate)
        const float gate_scale = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
        if (plan.form.rows16)
            VS_LAUNCH(vst_gemm_rows16(dm, w->tp(Q.t16_w2), zeros, gf, sv + A.ffn, M, 4 * d, d, 1, gate_scale, 0ull, 0u, 0.f, st));
        else
            VS_LAUNCH(vsk_linear_gate(dm, w->tp(Q.t_w2), w->tp(Q.tf_w2), zeros, sv + A.ffn, gate_scale, gf, M, 4 * d, d, st, plan.mode_gate));
        VS_LAUNCH(vst_wgrad(gf, 4 * d, sv + A.y1, d, M, 4 * d, d, G.w1, nullptr, nullptr, G.b1, nullptr, nullptr, 4 * d, wg, st, plan.mode_wgrad_w1));
        // d y1 = dz2 (residual) + d(fc1 input): the residual rides in the GEMM epilogue
        VS_LAUNCH(vsk_linear(gf, w->tp(Q.t_w1), w->tp(Q.tf_w1), zeros, dy1, M, d, 4 * d, 0, dz, M, plan.mode_dgrad_fc1, st));
        // norm1; d(feature_projection output) = dropout1 mask on dz1
        VS_LAUNCH(vst_ln_bwd(dy1, nullptr, nullptr, 0, sv + A.z1, sv + A.st1, w->p(P.ln1g), dz, p > 0.f ? dbr : nullptr, part,
                              M, d, seed, VS_SITE_LAYER(l, VS_SITE_DROP1), p, st, dn));
        VS_LAUNCH(vst_reduce_rows(part, nblk, 2, d, G.ln1_g, G.ln1_b, nullptr, 1, st));
        const float *da = p > 0.f ? dbr : dz;
        VS_LAUNCH(vst_wgrad(da, d, sv + A.att, d, M, d, d, G.wo, nullptr, nullptr, G.bo, nullptr, nullptr, d, wg, st, plan.mode_linear));
        // d(attention output), then delta = its row dot with the saved output, then the attention itself
        VS_LAUNCH(vsk_linear(da, w->tp(Q.t_wo), w->tp(Q.tf_wo), zeros, datt, M, d, d, 0, nullptr, 1, plan.mode_datt, st));
        VS_LAUNCH(vst_head_rowdot(datt, sv + A.att, delta, M, T, H, d / H, st, plan.mode_rowdot));
        if (int rc = attention_backward(plan, sv + A.qkv, key_pad_mask, datt, sv + A.lse, delta, dqkv, B, H, T, d / H, scale, seed,
                                        VS_SITE_LAYER(l, VS_SITE_ATTN), p, p > 0.f ? (const unsigned *)(sv + A.dbits) : nullptr, pk, st))
            return rc;
        // q / k / v projections: one [3d, d] weight gradient dealt to the three parameters
        VS_LAUNCH(vst_wgrad(dqkv, 3 * d, h_in, d, M, 3 * d, d, G.wq, G.wk, G.wv, G.bq, G.bk, G.bv, d, wg, st, plan.mode_wgrad_qkv));
        // gradient of the layer input = dz1 (residual) + dqkv Wqkv
        VS_LAUNCH(vsk_linear(dqkv, w->tp(Q.t_wqkv), w->tp(Q.tf_wqkv), zeros, g[cur ^ 1], M, d, 3 * d, 0, dz, M, plan.mode_dgrad_qkv, st));
        cur ^= 1;
    }
    // Embedding (simnet.py:211, 237-238): dropout(sparsity) mask, then the Linear
    float *gh0 = g[cur];
    if (p_embed > 0.f) VS_LAUNCH(vst_dropout_rows(gh0, M, d, seed, VS_SITE_EMBED, p_embed, st));
    VS_LAUNCH(vst_wgrad(gh0, d, x, D.in_features, M, d, D.in_features, grads->embed_w, nullptr, nullptr, grads->embed_b,
                         nullptr, nullptr, d, wg, st, plan.mode_linear));
    if (dx) VS_LAUNCH(vsk_linear(gh0, w->tp(w->t_embed_w), w->tp(w->tf_embed_w), zeros, dx, M, D.in_features, d, 0, nullptr, 1, plan.mode_linear, st));
    return VS_OK;
}

int vs_train_forward(const vs_weights *w, const float *x, const uint8_t *key_pad_mask, int32_t B, int32_t T,
                     const vs_dropout_cfg *drop, float *scores, float *hidden, void *saved, size_t saved_bytes,
                     void *workspace, size_t workspace_bytes, void *stream) {
    return forward_impl(w, x, key_pad_mask, B, T, drop, scores, hidden, saved, saved_bytes, workspace, workspace_bytes, stream, nullptr);
}

int vs_train_backward(vs_weights *w, const float *x, const uint8_t *key_pad_mask, int32_t B, int32_t T,
                      const vs_dropout_cfg *drop, const float *d_scores, const float *d_hidden, const void *saved,
                      size_t saved_bytes, const vs_model_grads *grads, float *dx, void *workspace,
                      size_t workspace_bytes, void *stream) {
    return backward_impl(w, x, key_pad_mask, B, T, drop, d_scores, d_hidden, saved, saved_bytes, grads, dx, workspace,
                         workspace_bytes, stream, nullptr);
}

// ---- packed ragged batches ----
int vs_train_check_packed(const vs_model_desc *desc, const int32_t *lengths, int32_t B) {
    if (!desc) return vs_failf(VS_ERR_INVALID, "desc is NULL");
    PackedCtx pc;
    return packed_ctx(*desc, lengths, B, pc);
}

size_t vs_train_saved_bytes_desc(const vs_model_desc *desc, const int32_t *lengths, int32_t B, int32_t T) {
    if (!desc || desc->d_model <= 0 || desc->num_heads <= 0 || desc->num_layers <= 0 || B <= 0) return 0;
    if (!lengths) return T > 0 ? saved_layout(*desc, B, T).total * sizeof(float) : 0;
    PackedCtx pc;
    if (packed_ctx(*desc, lengths, B, pc) != VS_OK) return 0;
    return saved_layout(*desc, 1, pc.Mtot, &pc).total * sizeof(float);
}

size_t vs_train_saved_bytes_packed(const vs_weights *w, const int32_t *lengths, int32_t B) {
    return (w && lengths) ? vs_train_saved_bytes_desc(&w->desc, lengths, B, 0) : 0;
}

size_t vs_train_workspace_bytes_packed(const vs_weights *w, const int32_t *lengths, int32_t B) {
    PackedCtx pc;
    if (!w || !lengths || packed_ctx(w->desc, lengths, B, pc) != VS_OK) return 0;
    return work_layout(w->desc, 1, pc.Mtot, &pc).total * sizeof(float);
}

int vs_train_saved_field_packed(const vs_weights *w, const int32_t *lengths, int32_t B, int32_t layer, int32_t field,
                                size_t *offset_bytes, size_t *count) {
    PackedCtx pc;
    if (!w || !offset_bytes || !count || layer < 0 || layer >= w->desc.num_layers)
        return vs_failf(VS_ERR_INVALID, "saved_field: bad arguments");
    if (int rc = packed_ctx(w->desc, lengths, B, pc)) return rc;
    return saved_field(w, 1, pc.Mtot, &pc, layer, field, offset_bytes, count);
}

int vs_train_forward_packed(const vs_weights *w, const float *x, const int32_t *lengths, const int32_t *lengths_dev, int32_t B,
                            const vs_dropout_cfg *drop, float *scores, float *hidden, void *saved, size_t saved_bytes,
                            void *workspace, size_t workspace_bytes, void *stream) {
    if (!w) return vs_failf(VS_ERR_INVALID, "weights is NULL");
    if (!lengths_dev) return vs_failf(VS_ERR_INVALID, "lengths_dev is NULL");
    PackedCtx pc;
    if (int rc = packed_ctx(w->desc, lengths, B, pc)) return rc;
    pc.lengths_dev = lengths_dev;
    return forward_impl(w, x, nullptr, 1, pc.Mtot, drop, scores, hidden, saved, saved_bytes, workspace, workspace_bytes, stream, &pc);
}

int vs_train_backward_packed(vs_weights *w, const float *x, const int32_t *lengths, const int32_t *lengths_dev, int32_t B,
                             const vs_dropout_cfg *drop, const float *d_scores, const float *d_hidden, const void *saved,
                             size_t saved_bytes, const vs_model_grads *grads, float *dx, void *workspace,
                             size_t workspace_bytes, void *stream) {
    if (!w) return vs_failf(VS_ERR_INVALID, "weights is NULL");
    if (!lengths_dev) return vs_failf(VS_ERR_INVALID, "lengths_dev is NULL");
    PackedCtx pc;
    if (int rc = packed_ctx(w->desc, lengths, B, pc)) return rc;
    pc.lengths_dev = lengths_dev;
    return backward_impl(w, x, nullptr, 1, pc.Mtot, drop, d_scores, d_hidden, saved, saved_bytes, grads, dx, workspace,
                         workspace_bytes, stream, &pc);
}

int vs_mse_packed_loss_forward(const float *output, const float *target, int32_t n, double denom, float *scratch, float *loss,
                               void *stream) {
    if (!output || !target || !scratch || !loss || n <= 0 || !(denom > 0.0)) return vs_failf(VS_ERR_INVALID, "mse_packed_loss: bad arguments");
    VS_LAUNCH(vst_mse_scaled_fwd(output, target, n, (float)(1.0 / denom), scratch, loss, (hipStream_t)stream));
    return VS_OK;
}

int vs_mse_packed_loss_backward(const float *output, const float *target, const float *d_loss, int32_t n, double denom,
                                float *d_output, void *stream) {
    if (!output || !target || !d_loss || !d_output || n <= 0 || !(denom > 0.0)) return vs_failf(VS_ERR_INVALID, "mse_packed_loss: bad arguments");
    VS_LAUNCH(vst_mse_scaled_bwd(output, target, d_loss, n, (float)(1.0 / denom), d_output, (hipStream_t)stream));
    return VS_OK;
}

// scratch of the two per-kernel entry points below: the device plan, then delta [H][Mtot]
static size_t attention_packed_plan_floats(const PackedCtx &pc) { return align_floats(vst_packed_plan_ints(pc.B, pc.nwork)); }

size_t vs_train_attention_packed_scratch_bytes(const int32_t *lengths, int32_t B, int32_t H) {
    PackedCtx pc;
    if (H <= 0 || packed_lengths(lengths, B, pc) != VS_OK) return 0;
    return (attention_packed_plan_floats(pc) + align_floats((size_t)H * pc.Mtot)) * sizeof(float);
}

int vs_train_attention_forward_packed(const float *q, const float *k, const float *v, float *out, float *lse2,
                                      const int32_t *lengths, const int32_t *lengths_dev, int32_t B, int32_t H, int32_t dh,
                                      float scale, uint64_t seed, uint32_t site, float p, void *scratch, size_t scratch_bytes,
                                      void *stream) {
    if (!q || !k || !v || !out || !lse2 || !lengths_dev || !scratch) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    PackedCtx pc;
    if (H <= 0) return vs_failf(VS_ERR_INVALID, "H=%d", H);
    if (int rc = packed_lengths(lengths, B, pc)) return rc;
    if (scratch_bytes < vs_train_attention_packed_scratch_bytes(lengths, B, H) || ((uintptr_t)scratch & 255))
        return vs_failf(VS_ERR_WORKSPACE, "scratch %zu bytes < %zu needed (256-byte aligned)", scratch_bytes, vs_train_attention_packed_scratch_bytes(lengths, B, H));
    hipStream_t st = (hipStream_t)stream;
    VstPackedPlan pk{};
    VS_LAUNCH(vst_plan_packed(lengths_dev, B, pc.Mtot, pc.tmax, pc.words, (int *)scratch, pc.nwork, st, &pk));
    VS_LAUNCH(vst_attention_fwd_packed(q, k, v, out, lse2, H, dh, scale, seed, site, p, st, nullptr, pk));
    return VS_OK;
}

int vs_train_attention_backward_packed(const float *q, const float *k, const float *v, const float *out, const float *d_out,
                                       const float *lse2, float *dqkv, const int32_t *lengths, const int32_t *lengths_dev,
                                       int32_t B, int32_t H, int32_t dh, float scale, uint64_t seed, uint32_t site, float p,
                                       void *scratch, size_t scratch_bytes, void *stream) {
    if (!q || !k || !v || !out || !d_out || !lse2 || !dqkv || !lengths_dev || !scratch) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    PackedCtx pc;
    if (H <= 0) return vs_failf(VS_ERR_INVALID, "H=%d", H);
    if (int rc = packed_lengths(lengths, B, pc)) return rc;
    if (scratch_bytes < vs_train_attention_packed_scratch_bytes(lengths, B, H) || ((uintptr_t)scratch & 255))
        return vs_failf(VS_ERR_WORKSPACE, "scratch %zu bytes < %zu needed (256-byte aligned)", scratch_bytes, vs_train_attention_packed_scratch_bytes(lengths, B, H));
    hipStream_t st = (hipStream_t)stream;
    float *delta = (float *)scratch + attention_packed_plan_floats(pc);
    VstPackedPlan pk{};
    VS_LAUNCH(vst_plan_packed(lengths_dev, B, pc.Mtot, pc.tmax, pc.words, (int *)scratch, pc.nwork, st, &pk));
    VS_LAUNCH(vst_head_rowdot(d_out, out, delta, pc.Mtot, pc.Mtot, H, dh, st));
    VS_LAUNCH(vst_attention_bwd_packed(q, k, v, d_out, lse2, delta, dqkv, H, dh, scale, seed, site, p, st, nullptr, pk));
    return VS_OK;
}

// ... and of the two 16-bit entry points: the device plan | delta [H][Mtot] | both bit-packed copies of the keep words
namespace {
struct PackedLpScratch { size_t delta, dbits, total; };      // floats
PackedLpScratch packed_lp_scratch(const PackedCtx &pc, int H) {
    PackedLpScratch S{};
    S.delta = attention_packed_plan_floats(pc);
    S.dbits = S.delta + align_floats((size_t)H * pc.Mtot);
    S.total = S.dbits + align_floats(2 * (size_t)H * pc.words);
    return S;
}
// the argument checks of the two entry points (before any device access); pc out
int packed_lp_check(const int32_t *lengths, int32_t B, int32_t H, int32_t dh, float p, const void *scratch, size_t scratch_bytes,
                    PackedCtx &pc) {
    if (H <= 0) return vs_failf(VS_ERR_INVALID, "H=%d", H);
    if (!vst_attention_bf16_supported(dh)) return vs_failf(VS_ERR_INVALID, "head dim %d: the 16-bit attention kernels take 32 / 64 / 128", dh);
    if (!(p >= 0.f && p < 1.f)) return vs_failf(VS_ERR_INVALID, "dropout probability must be in [0, 1): p=%g", p);
    if (int rc = packed_lengths(lengths, B, pc)) return rc;
    const size_t need = packed_lp_scratch(pc, H).total * sizeof(float);
    if (scratch_bytes < need || ((uintptr_t)scratch & 255))
        return vs_failf(VS_ERR_WORKSPACE, "scratch %zu bytes < %zu needed (256-byte aligned)", scratch_bytes, need);
    return VS_OK;
}
}  // namespace

size_t vs_train_attention_packed_lp_scratch_bytes(const int32_t *lengths, int32_t B, int32_t H) {
    PackedCtx pc;
    if (H <= 0 || packed_lengths(lengths, B, pc) != VS_OK) return 0;
    return packed_lp_scratch(pc, H).total * sizeof(float);
}

int vs_train_attention_forward_packed_lp(const float *q, const float *k, const float *v, float *out, float *lse2,
                                         const int32_t *lengths, const int32_t *lengths_dev, int32_t B, int32_t H, int32_t dh,
                                         float scale, uint64_t seed, uint32_t site, float p, int32_t f16, void *scratch,
                                         size_t scratch_bytes, void *stream) {
    if (!q || !k || !v || !out || !lse2 || !lengths_dev || !scratch) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    PackedCtx pc;
    if (int rc = packed_lp_check(lengths, B, H, dh, p, scratch, scratch_bytes, pc)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const PackedLpScratch S = packed_lp_scratch(pc, H);
    unsigned *dbits = p > 0.f ? (unsigned *)((float *)scratch + S.dbits) : nullptr;
    VstPackedPlan pk{};
    VS_LAUNCH(vst_plan_packed(lengths_dev, B, pc.Mtot, pc.tmax, pc.words, (int *)scratch, pc.nwork, st, &pk));
    if (dbits) VS_LAUNCH(vst_attention_dropout_bits_packed(dbits, B, H, pc.tmax, seed, site, p, st, pk));
    VS_LAUNCH(vst_attention_fwd_bf16_packed(q, k, v, out, lse2, H, dh, scale, p, dbits, st, f16 != 0, pk));
    return VS_OK;
}

int vs_train_attention_backward_packed_lp(const float *q, const float *k, const float *v, const float *out, const float *d_out,
                                          const float *lse2, float *dqkv, const int32_t *lengths, const int32_t *lengths_dev,
                                          int32_t B, int32_t H, int32_t dh, float scale, uint64_t seed, uint32_t site, float p,
                                          int32_t f16, void *scratch, size_t scratch_bytes, void *stream) {
    if (!q || !k || !v || !out || !d_out || !lse2 || !dqkv || !lengths_dev || !scratch) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    PackedCtx pc;
    if (int rc = packed_lp_check(lengths, B, H, dh, p, scratch, scratch_bytes, pc)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const PackedLpScratch S = packed_lp_scratch(pc, H);
    float *delta = (float *)scratch + S.delta;
    unsigned *dbits = p > 0.f ? (unsigned *)((float *)scratch + S.dbits) : nullptr;
    VstPackedPlan pk{};
    VS_LAUNCH(vst_plan_packed(lengths_dev, B, pc.Mtot, pc.tmax, pc.words, (int *)scratch, pc.nwork, st, &pk));
    if (dbits) VS_LAUNCH(vst_attention_dropout_bits_packed(dbits, B, H, pc.tmax, seed, site, p, st, pk));
    VS_LAUNCH(vst_head_rowdot(d_out, out, delta, pc.Mtot, pc.Mtot, H, dh, st, 2 | (f16 ? VSK_F16 : 0)));      // dO enters delta as the kernels see it: rounded
    VS_LAUNCH(vst_attention_bwd_bf16_packed(q, k, v, d_out, lse2, delta, dqkv, H, dh, scale, p, dbits, st, f16 != 0, pk));
    return VS_OK;
}

int vs_train_dropout_mask_attention_packed(uint8_t *keep, const int32_t *lengths, int32_t B, int32_t H, uint64_t seed,
                                           uint32_t site, float p, void *stream) {
    PackedCtx pc;
    if (!keep || H <= 0) return vs_failf(VS_ERR_INVALID, "bad arguments");
    if (int rc = packed_lengths(lengths, B, pc)) return rc;
    size_t off = 0;
    int row0 = 0;
    for (int b = 0; b < B; ++b) {
        VS_LAUNCH(vst_attention_dropout_mask_video(keep + off, H, lengths[b], pc.Mtot, row0, seed, site, p, (hipStream_t)stream));
        off += (size_t)H * lengths[b] * lengths[b];
        row0 += lengths[b];
    }
    return VS_OK;
}

int vs_mse_mask_loss_forward(const float *output, const float *target, const uint8_t *mask, int32_t n, int32_t mean,
                             float *scratch, float *loss, void *stream) {
    if (!output || !target || !scratch || !loss || n <= 0) return vs_failf(VS_ERR_INVALID, "mse_mask_loss: bad arguments");
    VS_LAUNCH(vst_mse_mask_fwd(output, target, mask, n, mean, scratch, loss, (hipStream_t)stream));
    return VS_OK;
}

int vs_mse_mask_loss_backward(const float *output, const float *target, const uint8_t *mask, const float *d_loss,
                              int32_t n, int32_t mean, float *d_output, void *stream) {
    if (!output || !target || !d_loss || !d_output || n <= 0) return vs_failf(VS_ERR_INVALID, "mse_mask_loss: bad arguments");
    VS_LAUNCH(vst_mse_mask_bwd(output, target, mask, d_loss, n, mean, d_output, (hipStream_t)stream));
    return VS_OK;
}

size_t vs_pretrain_head_state_bytes(int32_t B, int32_t T, int32_t F) {
    if (B <= 0 || T <= 0 || F <= 0) return 0;
    return align_floats(vsp_head_scratch_floats(B, T, F)) * sizeof(float);
}

namespace {
struct HeadWork { size_t dfeats, wt, zeros, wg, total; };
HeadWork head_work(int B, int T, int d, int F) {
    HeadWork W{};
    const size_t M = (size_t)B * T;
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += align_floats(n); return o; };
    W.dfeats = take(M * F);
    W.wt = take((size_t)d * F);
    W.zeros = take((size_t)(d > F ? d : F));
    W.wg = take(vst_wgrad_workspace_floats((int)M, F, d));
    W.total = off;
    return W;
}
// video_transform behind the head's own backward (d_feats in ws + W.dfeats), padded and packed: weight / bias gradient, then the
// gradient of the hidden state (NT GEMM against W^T)
int head_backward_tail(const float *hidden, const float *vt_w, int M, int d, int F, float *d_hidden, float *d_vt_w, float *d_vt_b,
                       float *ws, const HeadWork &W, hipStream_t st) {
    VS_LAUNCH(vst_wgrad(ws + W.dfeats, F, hidden, d, M, F, d, d_vt_w, nullptr, nullptr, d_vt_b, nullptr, nullptr, F, ws + W.wg, st));
    VS_LAUNCH(vst_transpose(vt_w, ws + W.wt, F, d, st));                                     // [F,d] -> [d,F]
    VS_HIP(hipMemsetAsync(ws + W.zeros, 0, (size_t)(d > F ? d : F) * sizeof(float), st));
    VS_LAUNCH(vsk_linear(ws + W.dfeats, ws + W.wt, nullptr, ws + W.zeros, d_hidden, M, d, F, 0, nullptr, 1, 0, st));
    return VS_OK;
}
}  // namespace

size_t vs_pretrain_head_workspace_bytes(int32_t B, int32_t T, int32_t d, int32_t F) {
    if (B <= 0 || T <= 0 || d <= 0 || F <= 0) return 0;
    return head_work(B, T, d, F).total * sizeof(float);
}

int vs_pretrain_head_forward(const float *hidden, const float *logits, const uint8_t *key_pad_mask, const float *vid,
                             const float *vt_w, const float *vt_b, int32_t B, int32_t T, int32_t d, int32_t F,
                             float temp, int32_t entropy_penalty, float *feats, void *head_state, float *losses,
                             void *stream) {
    if (!hidden || !logits || !vid || !vt_w || !vt_b || !feats || !head_state || !losses)
        return vs_failf(VS_ERR_INVALID, "pretrain head: NULL pointer");
    if (B <= 0 || T <= 0 || d <= 0 || d % 32 || (F != 256 && F != 512 && F != 768 && F != 1024) || !(temp > 0.f))
        return vs_failf(VS_ERR_INVALID, "pretrain head: B=%d T=%d d=%d F=%d temp=%g unsupported (d %% 32 == 0, F in {256,512,768,1024})", B, T, d, F, temp);
    hipStream_t st = (hipStream_t)stream;
    VS_LAUNCH(vsk_linear(hidden, vt_w, nullptr, vt_b, feats, B * T, F, d, 0, nullptr, 1, 0, st));           // :79
    VS_LAUNCH(vsp_head_forward(feats, logits, key_pad_mask, vid, B, T, F, 1.0f / temp, entropy_penalty,
                                (float *)head_state, losses, st));
    return VS_OK;
}

int vs_pretrain_head_backward(const float *hidden, const float *logits, const uint8_t *key_pad_mask, const float *vid,
                              const float *vt_w, const float *feats, void *head_state, const float *d_losses,
                              int32_t B, int32_t T, int32_t d, int32_t F, float temp, int32_t entropy_penalty,
                              float *d_hidden, float *d_logits, float *d_vt_w, float *d_vt_b, void *workspace,
                              size_t workspace_bytes, void *stream) {
    if (!hidden || !logits || !vid || !vt_w || !feats || !head_state || !d_losses || !d_hidden || !d_logits || !d_vt_w ||
        !d_vt_b || !workspace)
        return vs_failf(VS_ERR_INVALID, "pretrain head: NULL pointer");
    if (B <= 0 || T <= 0 || d <= 0 || d % 32 || (F != 256 && F != 512 && F != 768 && F != 1024) || !(temp > 0.f))
        return vs_failf(VS_ERR_INVALID, "pretrain head: B=%d T=%d d=%d F=%d temp=%g unsupported", B, T, d, F, temp);
    const HeadWork W = head_work(B, T, d, F);
    if (workspace_bytes < W.total * sizeof(float) || ((uintptr_t)workspace & 255))
        return vs_failf(VS_ERR_WORKSPACE, "pretrain head: workspace %zu bytes < %zu needed (256-byte aligned)", workspace_bytes, W.total * sizeof(float));
    hipStream_t st = (hipStream_t)stream;
    float *ws = (float *)workspace;
    const int M = B * T;
    VS_LAUNCH(vsp_head_backward(feats, logits, key_pad_mask, vid, B, T, F, 1.0f / temp, entropy_penalty,
                                 (const float *)head_state, d_losses, ws + W.dfeats, d_logits, st));
    return head_backward_tail(hidden, vt_w, M, d, F, d_hidden, d_vt_w, d_vt_b, ws, W, st);
}

// ---- the head on a packed ragged batch ----
namespace {
struct HeadPacked { int Mtot = 0, tmax = 0, NC = 0; };      // NC: (video, 64-frame chunk) pairs
bool head_width_ok(int F) { return F == 256 || F == 512 || F == 768 || F == 1024; }
bool head_shape_ok(int d, int F) { return d > 0 && d % 32 == 0 && head_width_ok(F); }
int head_packed_ctx(const int32_t *lengths, int32_t B, HeadPacked &hp) {
    PackedCtx pc;
    if (int rc = packed_lengths(lengths, B, pc)) return rc;
    hp.Mtot = pc.Mtot; hp.tmax = pc.tmax; hp.NC = 0;
    for (int b = 0; b < B; ++b) hp.NC += (lengths[b] + 63) / 64;
    return VS_OK;
}
}  // namespace

size_t vs_pretrain_head_state_bytes_packed(const int32_t *lengths, int32_t B, int32_t F) {
    HeadPacked hp;
    if (!head_width_ok(F) || head_packed_ctx(lengths, B, hp) != VS_OK) return 0;
    return align_floats(vsp_head_scratch_floats_packed(B, hp.Mtot, hp.NC, F)) * sizeof(float);
}

size_t vs_pretrain_head_workspace_bytes_packed(const int32_t *lengths, int32_t B, int32_t d, int32_t F) {
    HeadPacked hp;
    if (!head_shape_ok(d, F) || head_packed_ctx(lengths, B, hp) != VS_OK) return 0;
    return head_work(1, hp.Mtot, d, F).total * sizeof(float);
}

static int head_packed_check(const int32_t *lengths, int32_t B, int32_t ref_len, int32_t d, int32_t F, float temp, HeadPacked &hp) {
    if (int rc = head_packed_ctx(lengths, B, hp)) return rc;
    if (ref_len < hp.tmax) return vs_failf(VS_ERR_INVALID, "pretrain head: ref_len=%d is below max(lengths)=%d", ref_len, hp.tmax);
    if (ref_len > (1 << 24)) return vs_failf(VS_ERR_INVALID, "pretrain head: ref_len=%d too large", ref_len);
    if (!head_shape_ok(d, F) || !(temp > 0.f))
        return vs_failf(VS_ERR_INVALID, "pretrain head: d=%d F=%d temp=%g unsupported (d %% 32 == 0, F in {256,512,768,1024}, temp > 0)", d, F, temp);
    return VS_OK;
}

int vs_pretrain_head_forward_packed(const float *hidden, const float *logits, const int32_t *lengths, const int32_t *lengths_dev,
                                    int32_t B, int32_t ref_len, const float *vid, const float *vt_w, const float *vt_b,
                                    int32_t d, int32_t F, float temp, int32_t entropy_penalty, float *feats, void *head_state,
                                    float *losses, void *stream) {
    if (!hidden || !logits || !lengths || !lengths_dev || !vid || !vt_w || !vt_b || !feats || !head_state || !losses)
        return vs_failf(VS_ERR_INVALID, "pretrain head: NULL pointer");
    HeadPacked hp;
    if (int rc = head_packed_check(lengths, B, ref_len, d, F, temp, hp)) return rc;
    hipStream_t st = (hipStream_t)stream;
    VS_LAUNCH(vsk_linear(hidden, vt_w, nullptr, vt_b, feats, hp.Mtot, F, d, 0, nullptr, 1, 0, st));
    VS_LAUNCH(vsp_head_forward_packed(feats, logits, lengths_dev, vid, B, hp.Mtot, hp.tmax, hp.NC, ref_len, F, 1.0f / temp,
                                       entropy_penalty, (float *)head_state, losses, st));
    return VS_OK;
}

int vs_pretrain_head_backward_packed(const float *hidden, const float *logits, const int32_t *lengths, const int32_t *lengths_dev,
                                     int32_t B, int32_t ref_len, const float *vid, const float *vt_w, const float *feats,
                                     void *head_state, const float *d_losses, int32_t d, int32_t F, float temp,
                                     int32_t entropy_penalty, float *d_hidden, float *d_logits, float *d_vt_w, float *d_vt_b,
                                     void *workspace, size_t workspace_bytes, void *stream) {
    if (!hidden || !logits || !lengths || !lengths_dev || !vid || !vt_w || !feats || !head_state || !d_losses || !d_hidden ||
        !d_logits || !d_vt_w || !d_vt_b || !workspace)
        return vs_failf(VS_ERR_INVALID, "pretrain head: NULL pointer");
    HeadPacked hp;
    if (int rc = head_packed_check(lengths, B, ref_len, d, F, temp, hp)) return rc;
    const HeadWork W = head_work(1, hp.Mtot, d, F);
    if (workspace_bytes < W.total * sizeof(float) || ((uintptr_t)workspace & 255))
        return vs_failf(VS_ERR_WORKSPACE, "pretrain head: workspace %zu bytes < %zu needed (256-byte aligned)", workspace_bytes, W.total * sizeof(float));
    hipStream_t st = (hipStream_t)stream;
    float *ws = (float *)workspace;
    const int M = hp.Mtot;
    VS_LAUNCH(vsp_head_backward_packed(feats, logits, lengths_dev, B, M, hp.tmax, hp.NC, ref_len, F, 1.0f / temp, entropy_penalty,
                                        (float *)head_state, d_losses, ws + W.dfeats, d_logits, st));
    return head_backward_tail(hidden, vt_w, M, d, F, d_hidden, d_vt_w, d_vt_b, ws, W, st);      // M = the Mtot packed rows
}

int vs_train_attention_forward(const float *q, const float *k, const float *v, const uint8_t *key_pad_mask, float *out,
                               float *lse2, int32_t B, int32_t H, int32_t T, int32_t dh, float scale, uint64_t seed,
                               uint32_t site, float p, void *stream) {
    if (!q || !k || !v || !out || !lse2) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (B <= 0 || H <= 0 || T <= 0) return vs_failf(VS_ERR_INVALID, "B=%d H=%d T=%d", B, H, T);
    VS_LAUNCH(vst_attention_fwd(q, k, v, key_pad_mask, out, lse2, B, H, T, dh, scale, seed, site, p, (hipStream_t)stream));
    return VS_OK;
}

int vs_train_attention_backward(const float *q, const float *k, const float *v, const uint8_t *key_pad_mask,
                                const float *out, const float *d_out, const float *lse2, float *dqkv, float *scratch,
                                int32_t B, int32_t H, int32_t T, int32_t dh, float scale, uint64_t seed, uint32_t site,
                                float p, void *stream) {
    if (!q || !k || !v || !out || !d_out || !lse2 || !dqkv || !scratch) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (B <= 0 || H <= 0 || T <= 0) return vs_failf(VS_ERR_INVALID, "B=%d H=%d T=%d", B, H, T);
    hipStream_t st = (hipStream_t)stream;
    VS_LAUNCH(vst_head_rowdot(d_out, out, scratch, B * T, T, H, dh, st));
    VS_LAUNCH(vst_attention_bwd(q, k, v, key_pad_mask, d_out, lse2, scratch, dqkv, B, H, T, dh, scale, seed, site, p, st));
    return VS_OK;
}

size_t vs_train_attention_dropout_bits_bytes(int32_t B, int32_t H, int32_t T) {
    if (B <= 0 || H <= 0 || T <= 0) return 0;
    return vst_attention_dropout_bits_words(B, H, T) * sizeof(unsigned);
}

int vs_train_attention_dropout_bits(void *dbits, int32_t B, int32_t H, int32_t T, uint64_t seed, uint32_t site, float p,
                                    void *stream) {
    if (!dbits || B <= 0 || H <= 0 || T <= 0) return vs_failf(VS_ERR_INVALID, "dropout_bits: bad arguments");
    VS_LAUNCH(vst_attention_dropout_bits((unsigned *)dbits, B, H, T, seed, site, p, (hipStream_t)stream));
    return VS_OK;
}

int vs_train_attention_forward_bf16(const float *q, const float *k, const float *v, const uint8_t *key_pad_mask, float *out,
                                    float *lse2, int32_t B, int32_t H, int32_t T, int32_t dh, float scale, float p,
                                    const void *dbits, int32_t in16, void *stream) {
    if (!q || !k || !v || !out || !lse2) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (B <= 0 || H <= 0 || T <= 0) return vs_failf(VS_ERR_INVALID, "B=%d H=%d T=%d", B, H, T);
    VS_LAUNCH(vst_attention_fwd_bf16(q, k, v, key_pad_mask, out, lse2, B, H, T, dh, scale, p, (const unsigned *)dbits,
                                      (hipStream_t)stream, ((in16 & ~VSK_F16) ? 1 : 0) | (in16 & VSK_F16)));
    return VS_OK;
}

int vs_train_attention_backward_bf16(const float *q, const float *k, const float *v, const uint8_t *key_pad_mask,
                                     const float *out, const float *d_out, const float *lse2, float *dqkv, float *scratch,
                                     int32_t B, int32_t H, int32_t T, int32_t dh, float scale, float p, const void *dbits,
                                     int32_t in16, void *stream) {
    if (!q || !k || !v || !out || !d_out || !lse2 || !dqkv || !scratch) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (B <= 0 || H <= 0 || T <= 0) return vs_failf(VS_ERR_INVALID, "B=%d H=%d T=%d", B, H, T);
    hipStream_t st = (hipStream_t)stream;
    VS_LAUNCH(vst_head_rowdot(d_out, out, scratch, B * T, T, H, dh, st, 2 | (in16 & VSK_F16)));       // dO enters delta as the kernels see it: bf16 / f16
    VS_LAUNCH(vst_attention_bwd_bf16(q, k, v, key_pad_mask, d_out, lse2, scratch, dqkv, B, H, T, dh, scale, p,
                                      (const unsigned *)dbits, st, ((in16 & ~VSK_F16) ? 1 : 0) | (in16 & VSK_F16)));
    return VS_OK;
}

size_t vs_train_wgrad_scratch_floats(int32_t M, int32_t N, int32_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return vst_wgrad_workspace_floats(M, N, K);
}

int vs_train_wgrad(const float *dY, const float *X, int32_t M, int32_t N, int32_t K, float *dW, float *db,
                   float *scratch, void *stream) {
    if (!dY || !X || !dW || !scratch) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (M <= 0 || N <= 0 || K <= 0 || N % 4 || K % 4) return vs_failf(VS_ERR_INVALID, "M=%d N=%d K=%d unsupported (N, K multiples of 4)", M, N, K);
    VS_LAUNCH(vst_wgrad(dY, N, X, K, M, N, K, dW, nullptr, nullptr, db, nullptr, nullptr, N, scratch, (hipStream_t)stream));
    return VS_OK;
}

int vs_train_wgrad_bf16(const float *dY, const float *X, int32_t M, int32_t N, int32_t K, float *dW, float *db,
                        float *scratch, void *stream) {
    if (!dY || !X || !dW || !scratch) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (M <= 0 || N <= 0 || K <= 0 || N % 4 || K % 4) return vs_failf(VS_ERR_INVALID, "M=%d N=%d K=%d unsupported (N, K multiples of 4)", M, N, K);
    VS_LAUNCH(vst_wgrad(dY, N, X, K, M, N, K, dW, nullptr, nullptr, db, nullptr, nullptr, N, scratch, (hipStream_t)stream, 1));
    return VS_OK;
}

int vs_train_dropout_mask_attention(uint8_t *keep, int32_t B, int32_t H, int32_t T, uint64_t seed, uint32_t site,
                                    float p, void *stream) {
    if (!keep || B <= 0 || H <= 0 || T <= 0) return vs_failf(VS_ERR_INVALID, "bad arguments");
    VS_LAUNCH(vst_attention_dropout_mask(keep, B, H, T, seed, site, p, (hipStream_t)stream));
    return VS_OK;
}

int vs_train_dropout_mask_rows(uint8_t *keep, int32_t M, int32_t cols, uint64_t seed, uint32_t site, float p,
                               void *stream) {
    if (!keep || M <= 0 || cols <= 0) return vs_failf(VS_ERR_INVALID, "bad arguments");
    VS_LAUNCH(vst_rows_dropout_mask(keep, M, cols, seed, site, p, (hipStream_t)stream));
    return VS_OK;
}

}  // extern "C"
