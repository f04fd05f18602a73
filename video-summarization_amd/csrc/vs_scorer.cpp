// vs_scorer.cpp — the C ABI of include/vs_scorer.h: argument checks, workspace carving and the per-layer launch
// sequence of the scorer's eval forward.  The weights handle it reads is vs_weights.cpp's, the error text vs_error.cpp's.
#include "vs_scorer.h"
#include "vs_inspect.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "vs_error.h"
#include "vs_kernels.h"
#include "vs_train_kernels.h"      // vst_attention_fwd: the head-dim-256 attention of the scoring path
#include "vs_weights_impl.h"

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- optional per-stage HIP-event timing (bench.py's roofline leg) ----
// Events come from a pool that vs_profile_collect refills, so a profiled forward creates none after the first.
const char *const kStageNames[VS_NUM_STAGES] = {"embed_pe", "qkv_proj", "attention", "outproj_ln", "fc1_relu", "fc2_ln_score"};
struct StageRec { int stage; hipEvent_t a, b; };
std::mutex g_prof_mu;
std::atomic<bool> g_prof_on{false};
std::vector<StageRec> g_prof;
std::vector<hipEvent_t> g_event_pool;

hipEvent_t take_event() {
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        if (!g_event_pool.empty()) { hipEvent_t e = g_event_pool.back(); g_event_pool.pop_back(); return e; }
    }
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
}

struct StageScope {
    hipStream_t st; int stage; hipEvent_t a = nullptr, b = nullptr; bool on;
    StageScope(int stage_, hipStream_t st_) : st(st_), stage(stage_), on(g_prof_on.load(std::memory_order_relaxed)) {
        if (!on) return;
        a = take_event(); b = take_event();
        if (!a || !b) { on = false; return; }
        (void)hipEventRecord(a, st);
    }
    ~StageScope() {
        if (!on) return;
        (void)hipEventRecord(b, st);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof.push_back({stage, a, b});
    }
};

}  // namespace

// ---- A/B switches: environment read once, then only vs_set_option() ----
namespace {
struct OptionName { const char *name; int VskOptions::*field; int dflt; };
const OptionName kOptions[] = {
    {"VS_SKINNY_ROWS", &VskOptions::skinny_rows, 16384}, {"VS_LP_MIN_ROWS", &VskOptions::lp_min_rows, 8192},
    {"VS_MLP_ABL", &VskOptions::mlp_abl, 0},             {"VS_EXACT_UNFUSED", &VskOptions::exact_unfused, 0},
    {"VS_LP_STORE32", &VskOptions::lp_store32, 0},
    {"VS_LP_MLP_UNFUSED", &VskOptions::lp_mlp_unfused, 0}, {"VS_LP_TAIL_UNFUSED", &VskOptions::lp_tail_unfused, 0},
    {"VS_LP_QKV_UNFUSED", &VskOptions::lp_qkv_unfused, 0}, {"VS_LP_EMBED_UNFUSED", &VskOptions::lp_embed_unfused, 0},
    {"VS_LP_MIN_ROWS_FUSED", &VskOptions::lp_min_rows_fused, 256}, {"VS_LP_TILE256", &VskOptions::lp_tile256, 0},
    {"VS_ATTN_W64_CHECKED", &VskOptions::attn_w64_checked, 0}, {"VS_TRAIN_LP_MIN_ROWS", &VskOptions::train_lp_min_rows, 1024},
    {"VS_ATTN_W64", &VskOptions::attn_w64, 1},           {"VS_ATTN_W64_ABL", &VskOptions::attn_w64_abl, 0},
    {"VS_LAYER_TAIL_MIN_ROWS", &VskOptions::layer_tail_min_rows, 1024},
};
int option_from_env(const OptionName &o) {
    const char *e = getenv(o.name);
    if (!e) return o.dflt;
    return *e ? atoi(e) : 1;      // "VAR=" (set but empty) counts as on, like the old `getenv != nullptr` switches
}
}  // namespace

VskOptions &vsk_options() {
    static VskOptions opts = [] {
        VskOptions o{};
        for (const auto &k : kOptions) o.*(k.field) = option_from_env(k);
        return o;
    }();
    return opts;
}

int vsk_device_cus() {
    static std::atomic<int> cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (dev >= 0 && dev < 64) { const int c = cus[dev].load(std::memory_order_relaxed); if (c > 0) return c; }
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return -1;
    if (dev >= 0 && dev < 64) cus[dev].store(n, std::memory_order_relaxed);
    return n;
}

extern "C" {

int vs_abi_version(void) { return VS_ABI_VERSION; }

size_t vs_scorer_workspace_bytes(const vs_weights *w, int32_t B, int32_t T) {
    if (!w || B <= 0 || T <= 0) return 0;
    const size_t md = align_up((size_t)B * T * w->desc.d_model * sizeof(float), 256);
    return 10 * md;     // h0, h1, q, k, v, att, ffn(4)
}

}  // extern "C"

namespace {
// packed ragged batch (vs_scorer_forward_packed): the frames of all videos concatenated as ONE "video" of Mtot rows
// for every row-wise kernel; only the positional rows and the attention know about the video boundaries
struct PackedInfo {
    const float *pe_rows;    // [Mtot, d] positional rows gathered per frame (or nullptr without a positional table)
    const int *cu;           // device [B+1] row offsets
    const int *work;         // device [nwork][2] (video, query tile)
    int nwork, nw;           // query tile = 32*nw rows
};

// vs_inspect_forward: after the QKV stage of every selected layer the attention-map kernels READ that layer's q / k planes
// (exact path: fp32, head-major) - nothing the forward computes depends on it
struct InspectHook {
    const int32_t *layers;   // host, ascending
    int n_layers;
    float *maps, *received, *entropy;      // [n_layers, B, H, N, N] / [n_layers, B, H, N] / [n_layers, B, H, N], any nullptr
    void *workspace;         // vsk_attention_probs_workspace_bytes(B, H, N)
    // packed (pk != nullptr): received / entropy [n_layers, H, M], maps [n_layers] x the videos' [H, T_b, T_b] blocks;
    // workspace: vsk_attention_probs_packed_workspace_bytes, its plan already built (vsk_attention_probs_packed_plan)
    int videos = 0, tiles = 0;             // B and sum ceil(T_b / 32) of the packed batch
    size_t map_stride = 0;                 // H * sum T_b^2: floats of one layer's maps
};

// cls != nullptr (use_cls=True, reference simnet.py:205-206, 214-216, 47-51): x has T frames per video, a class token
// [d_model] is prepended AFTER the positional encoding, so the encoder sees T + 1 positions (the token is never
// padding) and scores / hidden have T + 1 rows per video.
int forward_core(const vs_weights *w, const float *x, const uint8_t *key_pad_mask, int32_t B,
                 int32_t T, uint32_t flags, float *scores, float *hidden, void *workspace,
                 size_t workspace_bytes, void *stream, const PackedInfo *pk, const float *cls = nullptr,
                 const InspectHook *ins = nullptr) {
    if (!w || !x || !scores) return vs_failf(VS_ERR_INVALID, "weights/x/scores is NULL");
    if (B <= 0 || T <= 0) return vs_failf(VS_ERR_INVALID, "B=%d T=%d", B, T);
    const vs_model_desc &D = w->desc;
    const int Tf = T;                   // frames per video (rows of x, positional rows)
    const int sig = (flags & VS_FLAG_SIGMOID) ? 1 : 0;
    // which kernels run: decided once, in vs_forward_plan.h; everything below only reads `plan`
    const VsForwardIn in{D.d_model, D.num_heads, D.num_layers, D.in_features, D.max_len, w->dn(), w->has_pe, w->has_b_embed,
                         B, Tf, flags, cls != nullptr, pk != nullptr};
    VsForwardPlan plan;
    std::string err;
    if (int rc = vs_forward_plan(in, vsk_options(), &plan, &err)) return vs_fail_msg(rc, err.c_str());
    T = plan.T;                         // sequence length the encoder sees
    const size_t need_core = vs_scorer_workspace_bytes(w, B, T);
    const size_t need = need_core + (cls ? align_up((size_t)B * T, 256) : 0);       // + the [B, T+1] key mask
    if (!workspace || workspace_bytes < need)
        return vs_failf(VS_ERR_WORKSPACE, "workspace %zu bytes < %zu needed", workspace_bytes, need);
    if (((uintptr_t)workspace & 255) || ((uintptr_t)x & 15) || (hidden && ((uintptr_t)hidden & 15)) || (cls && ((uintptr_t)cls & 15)))
        return vs_failf(VS_ERR_INVALID, "workspace must be 256-byte, x/hidden/cls_token 16-byte aligned");
    // kernel-layout weight images this forward reads, (re)built only if the parameters changed since their last use
    vsw_order(w, stream);       // parameters written on another stream (vs_weights_update): ordered on the device
    if (plan.families) if (int rc = vsw_ensure(w, plan.families, stream)) return rc;

    hipStream_t st = (hipStream_t)stream;
    const int d = D.d_model, H = D.num_heads, L = D.num_layers, M = plan.M;
    const size_t md = align_up((size_t)M * d * sizeof(float), 256) / sizeof(float);
    float *ws = (float *)workspace;
    float *h0 = ws, *h1 = ws + md, *qkv = ws + 2 * md, *att = ws + 5 * md, *ffn = ws + 6 * md;
    void *h16 = ffn + 2 * md;               // [M, d] bf16 copy of the current LayerNorm output (the upper half of ffn: the
                                            // bf16 hidden tensor needs the lower half only)
    const size_t kv = plan.kv_stride;       // floats between the q, k and v planes
    const int dn = w->dn();                             // LayerNorm width / the d_model of the attention scale (== d unless embedded)
    const float scale = 1.0f / sqrtf((float)dn);       // reference simnet.py:126: d_model ** -0.5
    const float qs = vsk_attention_qscale(scale);
    const bool f16x3 = plan.linear == VS_ARITH_F16X3;
    auto frag = [&](size_t f, size_t h) { return w->p(f16x3 ? h : f); };      // a weight's fragment-major image in this arithmetic
    const float *pe_rows = pk ? pk->pe_rows : (w->has_pe ? w->p(w->pe) : nullptr);
    {   // Embedding + positional table (simnet.py:211, 237-238)
        StageScope ps(VS_STAGE_EMBED, st);
        switch (plan.embed) {
        case VS_EMBED_CLS: {
            // frames through the embedding GEMM into a free region (h1), then token row + frames -> h0, mask -> mask'
            VS_LAUNCH(vsk_linear(x, w->p(w->embed_w), frag(w->f_embed_w, w->h_embed_w), w->p(w->embed_b), h1, B * Tf, d,
                                 D.in_features, 0, pe_rows, Tf, plan.mode_linear, st));
            uint8_t *mask1 = key_pad_mask ? (uint8_t *)workspace + need_core : nullptr;
            VS_LAUNCH(vsk_insert_cls(h1, cls, key_pad_mask, h0, mask1, B, Tf, d, st));
            key_pad_mask = mask1;
        } break;
        case VS_EMBED_BF16_QKV: {
            const LayerOff &N = w->layers[0];
            const VskNextQkv nq{w->p(N.b_qkv), w->p(N.bqkv), qkv, T, H, qs};
            VS_LAUNCH(vsk_embed_bf16(x, w->p(w->b_embed), w->p(w->embed_b), pe_rows, T, h0, M, d, D.in_features, &nq, st));
        } break;
        case VS_EMBED_SPLITK:
            // K = in_features split 8 ways; the partials (8 x [M, d]: the q .. ffn regions, all free here) + bias + positional rows -> h0
            VS_LAUNCH(vsk_linear_parts(x, frag(w->f_embed_w, w->h_embed_w), qkv, M, d, D.in_features, 8, st, f16x3));
            VS_LAUNCH(vsk_sum_parts_pe(qkv, 8, w->p(w->embed_b), pe_rows, T, h0, M, d, st));
            break;
        case VS_EMBED_GEMM:
            VS_LAUNCH(vsk_linear(x, w->p(w->embed_w), frag(w->f_embed_w, w->h_embed_w), w->p(w->embed_b), h0, M, d, D.in_features, 0,
                                 pe_rows, T, plan.mode_linear, st));
            break;
        }
    }
    if (plan.layer == VS_LAYER_RING) VS_LAUNCH(vsk_to_bf16(h0, h16, (size_t)M * d, st));
    for (int l = 0; l < L; ++l) {
        const LayerOff &P = w->layers[l];
        const bool last = l == L - 1;
        float *dst = (last && hidden) ? hidden : h0;
        // the score head rides on the last layer's closing kernel
        const float *head_w = last ? w->p(w->final_w) : nullptr, *head_b = last ? w->p(w->final_b) : nullptr;
        float *head_out = last ? scores : nullptr;
        VskNextQkv nq{}, *next = nullptr;
        if (plan.next_qkv && !last) {
            const LayerOff &N = w->layers[l + 1];
            nq = VskNextQkv{w->p(N.b_qkv), w->p(N.bqkv), qkv, T, H, qs};
            next = &nq;
        }
        if (plan.layer == VS_LAYER_RING) {
            StageScope ps(VS_STAGE_QKV, st);
            VS_LAUNCH(vsk_gemm16(h16, w->p(P.r_wqkv), w->p(P.bqkv), qkv, M, 3 * d, d, 3, 1, T, H, d / H, qs, st));
        } else if (l == 0 ? plan.embed != VS_EMBED_BF16_QKV : !plan.tail_writes_qkv()) {      // else: written by the kernel before this layer
            StageScope ps(VS_STAGE_QKV, st);
            VS_LAUNCH(vsk_qkv(h0, w->p(P.wqkv), frag(P.f_wqkv, P.h_wqkv), w->p(P.bqkv), qkv, B, T, d, H, plan.mode_qkv, st,
                              plan.qkv16 ? qs : 1.0f));
        }
        if (ins) {
            for (int i = 0; i < ins->n_layers; ++i) {
                if (ins->layers[i] != l) continue;
                const size_t rows = (size_t)B * H * T;
                if (pk) {       // B = 1, T = M: at flags 0 the q / k planes are the head-major [H, M, dh] planes of the packed kernels
                    VS_LAUNCH(vsk_attention_probs_packed(qkv, qkv + kv, pk->cu, ins->maps ? ins->maps + i * ins->map_stride : nullptr,
                                                         ins->received ? ins->received + i * rows : nullptr,
                                                         ins->entropy ? ins->entropy + i * rows : nullptr, ins->videos, H, M, ins->tiles,
                                                         d / H, scale, ins->workspace, st));
                    continue;
                }
                VS_LAUNCH(vsk_attention_probs(qkv, qkv + kv, key_pad_mask, ins->maps ? ins->maps + i * rows * T : nullptr,
                                              ins->received ? ins->received + i * rows : nullptr,
                                              ins->entropy ? ins->entropy + i * rows : nullptr, B, H, T, d / H, scale, ins->workspace, st));
            }
        }
        {
            StageScope ps(VS_STAGE_ATTENTION, st);
            switch (plan.attention) {
            case VS_ATT_PACKED:
                VS_LAUNCH(vsk_attention_packed(qkv, qkv + kv, qkv + 2 * kv, att, H, M, d / H, scale, pk->cu, pk->work, pk->nwork, pk->nw,
                                               plan.mode_attention, st));
                break;
            case VS_ATT_DH256:      // its log-sum-exp output lands in the MLP hidden region, which is free here
                VS_LAUNCH(vst_attention_fwd(qkv, qkv + kv, qkv + 2 * kv, key_pad_mask, att, ffn, B, H, T, 256, scale, 0ull, 0u, 0.f, st, nullptr));
                break;
            case VS_ATT_SPLITKV:
                VS_LAUNCH(vsk_attention_splitkv(qkv, qkv + kv, qkv + 2 * kv, key_pad_mask, att, B, H, T, d / H, scale, st));
                break;
            case VS_ATT_LOWPREC:
                VS_LAUNCH(vsk_attention_bf16(qkv, qkv + kv, qkv + 2 * kv, key_pad_mask, att, B, H, T, d / H, scale, plan.mode_attention, st));
                break;
            case VS_ATT_EXACT:
                VS_LAUNCH(vsk_attention(qkv, qkv + kv, qkv + 2 * kv, key_pad_mask, att, B, H, T, d / H, scale, st));
                break;
            }
        }
        if (plan.ln1 != VS_LN_NONE) {       // out-projection + norm1 -> h1 as a stage of its own (the GEMM's output goes to the q
                                            // region, free after the attention)
            StageScope ps(VS_STAGE_OUTPROJ_LN, st);
            switch (plan.ln1) {
            case VS_LN_SPLITK_ROWS:     // K = d in two slices (q / k regions)
                VS_LAUNCH(vsk_linear_parts(att, frag(P.f_wo, P.h_wo), qkv, M, d, d, 2, st, f16x3));
                VS_LAUNCH(vsk_rows_res_ln(qkv, h0, w->p(P.ln1g), w->p(P.ln1b), h1, M, d, nullptr, nullptr, 0, 0, nullptr, st, nullptr, dn,
                                          2, w->p(P.bo)));
                break;
            case VS_LN_GEMM_ROWS:
                VS_LAUNCH(vsk_linear(att, w->p(P.wo), frag(P.f_wo, P.h_wo), w->p(P.bo), qkv, M, d, d, 0, nullptr, 1, plan.mode_linear, st));
                VS_LAUNCH(vsk_rows_res_ln(qkv, h0, w->p(P.ln1g), w->p(P.ln1b), h1, M, d, nullptr, nullptr, 0, 0, nullptr, st, nullptr, dn));
                break;
            default:
                VS_LAUNCH(vsk_linear_res_ln(att, w->p(P.wo), frag(P.f_wo, P.h_wo), w->p(P.bo), h0, w->p(P.ln1g), w->p(P.ln1b), h1, M, d, d,
                                            nullptr, nullptr, 0, 0, nullptr, plan.mode_qkv, st));
            }
        }
        switch (plan.layer) {
        case VS_LAYER_RING: {
            {   // out-projection (bf16 attention output in, fp32 out into the q region, free by now) + norm1 -> h1 (+ bf16 copy)
                StageScope ps(VS_STAGE_OUTPROJ_LN, st);
                VS_LAUNCH(vsk_gemm16(att, w->p(P.r_wo), w->p(P.bo), qkv, M, d, d, 0, 0, 1, 0, 0, 1.0f, st));
                VS_LAUNCH(vsk_rows_res_ln(qkv, h0, w->p(P.ln1g), w->p(P.ln1b), h1, M, d, nullptr, nullptr, 0, 0, nullptr, st, h16, dn));
            }
            {
                StageScope ps(VS_STAGE_FC1, st);
                VS_LAUNCH(vsk_gemm16(h16, w->p(P.r_w1), w->p(P.b1), ffn, M, 4 * d, d, 1, 1, 1, 0, 0, 1.0f, st));
            }
            // fc2 (fp32 out into the att region) + norm2 (+ score head) -> h0 / hidden (+ bf16 copy for the next layer)
            StageScope ps(VS_STAGE_FC2_LN, st);
            VS_LAUNCH(vsk_gemm16(ffn, w->p(P.r_w2), w->p(P.b2), att, M, d, 4 * d, 0, 0, 1, 0, 0, 1.0f, st));
            VS_LAUNCH(vsk_rows_res_ln(att, h1, w->p(P.ln2g), w->p(P.ln2b), dst, M, d, head_w, head_b, D.num_classes, sig, head_out, st,
                                      last ? nullptr : h16, dn));
        } break;
        case VS_LAYER_BF16_TAIL: {      // h1 never exists in HBM
            StageScope ps(VS_STAGE_FC2_LN, st);
            VS_LAUNCH(vsk_mlp_bf16(h0, att, w->p(P.bo), w->p(P.ln1g), w->p(P.ln1b), w->p(P.b_mlp), w->p(P.b1), w->p(P.b2),
                                   w->p(P.ln2g), w->p(P.ln2b), dst, M, d, head_w, head_b, D.num_classes, sig, head_out, next, st));
        } break;
        case VS_LAYER_BF16_MLP: {       // the whole MLP block as one kernel (hidden activations in registers)
            StageScope ps(VS_STAGE_FC2_LN, st);
            VS_LAUNCH(vsk_mlp_bf16(h1, nullptr, nullptr, nullptr, nullptr, w->p(P.b_mlp), w->p(P.b1), w->p(P.b2), w->p(P.ln2g), w->p(P.ln2b), dst, M, d,
                                   head_w, head_b, D.num_classes, sig, head_out, next, st));
        } break;
        case VS_LAYER_EXACT_PAIR: {
            if (M >= vsk_options().layer_tail_min_rows) {
                // one launch instead of the pair (a launcher fact, like cu and work: the plan says EXACT_PAIR either way); h1 stays
                // in registers.  Recorded under fc2 alone: bench.py folds the out-projection, fc1 and QKV shares into that row
                // when fc1 has no launches, as for the bf16 tail.
                StageScope ps(VS_STAGE_FC2_LN, st);
                const LayerOff *N = last ? nullptr : &w->layers[l + 1];
                VS_LAUNCH(vsk_layer_tail(att, w->p(P.wo), w->p(P.bo), h0, w->p(P.ln1g), w->p(P.ln1b), w->p(P.w1), w->p(P.b1), ffn, w->p(P.w2),
                                         w->p(P.b2), w->p(P.ln2g), w->p(P.ln2b), dst, N ? w->p(N->wqkv) : nullptr, N ? w->p(N->bqkv) : nullptr,
                                         qkv, head_w, head_b, D.num_classes, sig, head_out, B, T, d, H, st));
                break;
            }
            {   // recorded under fc1 / fc2: the stage table has no out-projection row then, and these two rows' FLOPs omit the
                // out-projection and QKV shares (their TFLOP/s are understated, never overstated)
                StageScope ps(VS_STAGE_FC1, st);
                VS_LAUNCH(vsk_outproj_ln_fc1(att, w->p(P.wo), w->p(P.bo), h0, w->p(P.ln1g), w->p(P.ln1b), h1, w->p(P.w1), w->p(P.b1), ffn, M, d, st));
            }
            StageScope ps(VS_STAGE_FC2_LN, st);
            if (last) {
                VS_LAUNCH(vsk_linear_res_ln(ffn, w->p(P.w2), w->p(P.f_w2), w->p(P.b2), h1, w->p(P.ln2g), w->p(P.ln2b), dst, M, d, 4 * d,
                                            head_w, head_b, D.num_classes, sig, head_out, 0, st));
            } else {
                const LayerOff &N = w->layers[l + 1];
                VS_LAUNCH(vsk_fc2_ln_qkv(ffn, w->p(P.w2), w->p(P.b2), h1, w->p(P.ln2g), w->p(P.ln2b), dst, w->p(N.wqkv), w->p(N.bqkv), qkv,
                                         B, T, d, H, st));
            }
        } break;
        case VS_LAYER_STAGES: {
            {
                StageScope ps(VS_STAGE_FC1, st);
                VS_LAUNCH(vsk_linear(h1, w->p(P.w1), frag(P.f_w1, P.h_w1), w->p(P.b1), ffn, M, 4 * d, d, 1, nullptr, 1, plan.mode_ffn, st));
            }
            StageScope ps(VS_STAGE_FC2_LN, st);
            switch (plan.ln2) {
            case VS_LN_SPLITK_ROWS:     // K = 4 d split four ways (partials in the q / k / v / att regions, free by now), LayerNorm (+ score head) as a row pass
                VS_LAUNCH(vsk_linear_parts(ffn, frag(P.f_w2, P.h_w2), qkv, M, d, 4 * d, 4, st, f16x3));
                VS_LAUNCH(vsk_rows_res_ln(qkv, h1, w->p(P.ln2g), w->p(P.ln2b), dst, M, d, head_w, head_b, D.num_classes, sig, head_out, st, nullptr, dn,
                                          4, w->p(P.b2)));
                break;
            case VS_LN_GEMM_ROWS:       // (the GEMM's output goes to the att region, free after fc1)
                VS_LAUNCH(vsk_linear(ffn, w->p(P.w2), frag(P.f_w2, P.h_w2), w->p(P.b2), att, M, d, 4 * d, 0, nullptr, 1, plan.mode_linear, st));
                VS_LAUNCH(vsk_rows_res_ln(att, h1, w->p(P.ln2g), w->p(P.ln2b), dst, M, d, head_w, head_b, D.num_classes, sig, head_out, st, nullptr, dn));
                break;
            default:
                VS_LAUNCH(vsk_linear_res_ln(ffn, w->p(P.w2), frag(P.f_w2, P.h_w2), w->p(P.b2), h1, w->p(P.ln2g), w->p(P.ln2b), dst, M, d,
                                            4 * d, head_w, head_b, D.num_classes, sig, head_out, plan.mode_ffn, st));
            }
        } break;
        }
    }
    return VS_OK;
}
}  // namespace

extern "C" {

int vs_scorer_forward(const vs_weights *w, const float *x, const uint8_t *key_pad_mask, int32_t B,
                      int32_t T, uint32_t flags, float *scores, float *hidden, void *workspace,
                      size_t workspace_bytes, void *stream) {
    return forward_core(w, x, key_pad_mask, B, T, flags, scores, hidden, workspace, workspace_bytes, stream, nullptr);
}

size_t vs_scorer_workspace_bytes_cls(const vs_weights *w, int32_t B, int32_t T) {
    if (!w || B <= 0 || T <= 0) return 0;
    return vs_scorer_workspace_bytes(w, B, T + 1) + align_up((size_t)B * (T + 1), 256);
}

int vs_scorer_forward_cls(const vs_weights *w, const float *x, const uint8_t *key_pad_mask, const float *cls_token,
                          int32_t B, int32_t T, uint32_t flags, float *scores, float *hidden, void *workspace,
                          size_t workspace_bytes, void *stream) {
    if (!cls_token) return vs_failf(VS_ERR_INVALID, "cls_token is NULL");
    return forward_core(w, x, key_pad_mask, B, T, flags, scores, hidden, workspace, workspace_bytes, stream, nullptr, cls_token);
}

// ---- attention maps (include/vs_inspect.h) ----
size_t vs_inspect_workspace_bytes(const vs_weights *w, int32_t B, int32_t T, int32_t with_cls) {
    if (!w || B <= 0 || T <= 0) return 0;
    const size_t core = with_cls ? vs_scorer_workspace_bytes_cls(w, B, T) : vs_scorer_workspace_bytes(w, B, T);
    return align_up(core, 256) + vsk_attention_probs_workspace_bytes(B, w->desc.num_heads, T + (with_cls ? 1 : 0));
}

int vs_inspect_forward(const vs_weights *w, const float *x, const uint8_t *key_pad_mask, const float *cls_token,
                       int32_t B, int32_t T, const int32_t *layers, int32_t n_layers,
                       float *scores, float *hidden, float *maps, float *received, float *entropy,
                       void *workspace, size_t workspace_bytes, void *stream) {
    if (!w) return vs_failf(VS_ERR_INVALID, "weights is NULL");
    if (!layers || n_layers <= 0) return vs_failf(VS_ERR_INVALID, "layers is NULL or n_layers=%d", n_layers);
    for (int i = 0; i < n_layers; ++i) {
        if (layers[i] < 0 || layers[i] >= w->desc.num_layers)
            return vs_failf(VS_ERR_INVALID, "layers[%d]=%d out of range (num_layers=%d)", i, layers[i], w->desc.num_layers);
        if (i && layers[i] <= layers[i - 1]) return vs_failf(VS_ERR_INVALID, "layers must be strictly ascending (layers[%d]=%d after %d)", i, layers[i], layers[i - 1]);
    }
    if (!maps && !received && !entropy) return vs_failf(VS_ERR_INVALID, "maps, received and entropy are all NULL");
    if (((uintptr_t)maps | (uintptr_t)received | (uintptr_t)entropy) & 15)
        return vs_failf(VS_ERR_INVALID, "maps / received / entropy must be 16-byte aligned");
    if (B <= 0 || T <= 0) return vs_failf(VS_ERR_INVALID, "B=%d T=%d", B, T);
    const size_t core = align_up(cls_token ? vs_scorer_workspace_bytes_cls(w, B, T) : vs_scorer_workspace_bytes(w, B, T), 256);
    const size_t need = vs_inspect_workspace_bytes(w, B, T, cls_token != nullptr);
    if (!workspace || workspace_bytes < need)
        return vs_failf(VS_ERR_WORKSPACE, "workspace %zu bytes < %zu needed", workspace_bytes, need);
    const InspectHook ins{layers, n_layers, maps, received, entropy, (char *)workspace + core};
    return forward_core(w, x, key_pad_mask, B, T, 0u, scores, hidden, workspace, core, stream, nullptr, cls_token, &ins);
}

size_t vs_attention_probs_workspace_bytes(int32_t B, int32_t H, int32_t T) {
    if (B <= 0 || H <= 0 || T <= 0) return 0;
    return vsk_attention_probs_workspace_bytes(B, H, T);
}

int vs_attention_probs_f32(const float *q, const float *k, const uint8_t *key_pad_mask, float *maps, float *received,
                           float *entropy, int32_t B, int32_t H, int32_t T, int32_t dh, float scale, void *workspace,
                           size_t workspace_bytes, void *stream) {
    if (!q || !k) return vs_failf(VS_ERR_INVALID, "q / k is NULL");
    if (!maps && !received && !entropy) return vs_failf(VS_ERR_INVALID, "maps, received and entropy are all NULL");
    if (B <= 0 || H <= 0 || T <= 0) return vs_failf(VS_ERR_INVALID, "B=%d H=%d T=%d", B, H, T);
    if (dh != 32 && dh != 64 && dh != 128 && dh != 256) return vs_failf(VS_ERR_INVALID, "head_dim=%d unsupported (32, 64, 128 or 256)", dh);
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)maps | (uintptr_t)received | (uintptr_t)entropy) & 15)
        return vs_failf(VS_ERR_INVALID, "q / k / maps / received / entropy must be 16-byte aligned");
    const size_t need = vsk_attention_probs_workspace_bytes(B, H, T);
    if (!workspace || workspace_bytes < need)
        return vs_failf(VS_ERR_WORKSPACE, "workspace %zu bytes < %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 255) return vs_failf(VS_ERR_INVALID, "workspace must be 256-byte aligned");
    VS_LAUNCH(vsk_attention_probs(q, k, key_pad_mask, maps, received, entropy, B, H, T, dh, scale, workspace, (hipStream_t)stream));
    return VS_OK;
}

// ---- packed ragged batches ----
static int packed_plan(const vs_weights *w, const int32_t *lengths, int32_t B, std::vector<int> &cu,
                       std::vector<int> &work, int &nw, int aprec = 0) {
    if (!w || !lengths || B <= 0) return vs_failf(VS_ERR_INVALID, "weights/lengths is NULL or B=%d", B);
    const vs_model_desc &D = w->desc;
    const int dh = D.d_model / D.num_heads;
    if (dh != 32 && dh != 64 && dh != 128) return vs_failf(VS_ERR_INVALID, "packed batches need head_dim 32, 64 or 128 (got %d)", dh);
    cu.assign(B + 1, 0);
    long long r8 = 0, r4 = 0;
    for (int b = 0; b < B; ++b) {
        const int t = lengths[b];
        if (t <= 0) return vs_failf(VS_ERR_INVALID, "lengths[%d]=%d", b, t);
        if (w->has_pe && t > D.max_len)
            return vs_failf(VS_ERR_INVALID, "T=%d exceeds the positional table (max_len=%d)", t, D.max_len);
        if ((long long)cu[b] + t > (1ll << 30)) return vs_failf(VS_ERR_INVALID, "too many frames");
        cu[b + 1] = cu[b] + t;
        r8 += (t + 255) / 256 * 256;
        r4 += (t + 127) / 128 * 128;
    }
    nw = vs_packed_waves(dh, aprec, r8, r4);
    const int qb = 32 * nw;
    work.clear();
    for (int b = 0; b < B; ++b)
        for (int q = 0; q < (lengths[b] + qb - 1) / qb; ++q) { work.push_back(b); work.push_back(q); }
    return VS_OK;
}

// (video, tile) pairs the plan area is sized for: ALWAYS the 128-row tiling, the longer of the two lists, so the
// size does not depend on which tiling the forward picks for the flags it is given
static size_t packed_plan_capacity(const int32_t *lengths, int32_t B) {
    size_t n = 0;
    for (int b = 0; b < B; ++b) n += (size_t)(lengths[b] + 127) / 128;
    return n;
}

size_t vs_scorer_workspace_bytes_packed(const vs_weights *w, const int32_t *lengths, int32_t B) {
    std::vector<int> cu, work;
    int nw = 0;
    if (packed_plan(w, lengths, B, cu, work, nw) != VS_OK) return 0;
    const size_t md = align_up((size_t)cu[B] * w->desc.d_model * sizeof(float), 256);
    // + gathered positional rows, plan (row offsets + work list)
    return 11 * md + align_up((cu.size() + 2 * packed_plan_capacity(lengths, B)) * sizeof(int), 256);
}

// vs_scorer_forward_packed, and vs_inspect_forward_packed (ins != nullptr: its hook, workspace_bytes = the forward's share)
static int forward_packed(const vs_weights *w, const float *x, const int32_t *lengths, const int32_t *lengths_dev,
                          int32_t B, uint32_t flags, float *scores, float *hidden, void *workspace,
                          size_t workspace_bytes, void *stream, const InspectHook *ins) {
    if (!lengths_dev) return vs_failf(VS_ERR_INVALID, "lengths_dev is NULL");
    if (!w) return vs_failf(VS_ERR_INVALID, "weights is NULL");
    if ((flags & VS_FLAG_BF16_ATTENTION) && (flags & VS_FLAG_F16X3_ATTENTION))
        return vs_failf(VS_ERR_INVALID, "VS_FLAG_BF16_ATTENTION and VS_FLAG_F16X3_ATTENTION are exclusive");
    const int aprec = vs_attention_prec(flags);
    std::vector<int> cu, work;
    int nw = 0;
    if (aprec == 2 && w->desc.d_model / w->desc.num_heads == 128)
        return vs_failf(VS_ERR_INVALID, "VS_FLAG_F16X3_ATTENTION needs head_dim 32 or 64 (got 128)");
    if (int rc = packed_plan(w, lengths, B, cu, work, nw, aprec)) return rc;
    const size_t need = vs_scorer_workspace_bytes_packed(w, lengths, B);
    if (!workspace || workspace_bytes < need)
        return vs_failf(VS_ERR_WORKSPACE, "workspace %zu bytes < %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 255) return vs_failf(VS_ERR_INVALID, "workspace must be 256-byte aligned");
    const int M = cu[B], d = w->desc.d_model;
    const size_t md = align_up((size_t)M * d * sizeof(float), 256);
    hipStream_t st = (hipStream_t)stream;
    float *pe_rows = (float *)((char *)workspace + 10 * md);
    int *plan = (int *)((char *)workspace + 11 * md);
    // the device builds its own copy of the plan from the device lengths (no host memory is read after return,
    // no synchronisation); the host copy above only sized the launch
    const size_t cap = packed_plan_capacity(lengths, B);
    if (work.size() / 2 > cap) return vs_failf(VS_ERR_INVALID, "internal: packed plan %zu > capacity %zu", work.size() / 2, cap);
    VS_LAUNCH(vsk_plan_packed(lengths_dev, B, 32 * nw, plan, plan + cu.size(), (int)cap, st));
    PackedInfo pk{nullptr, plan, plan + cu.size(), (int)(work.size() / 2), nw};
    if (w->has_pe) {
        int tmax = 0;
        for (int b = 0; b < B; ++b) tmax = lengths[b] > tmax ? lengths[b] : tmax;
        VS_LAUNCH(vsk_gather_rows(w->p(w->pe), pk.cu, B, tmax, d, pe_rows, st));
        pk.pe_rows = pe_rows;
    }
    return forward_core(w, x, nullptr, 1, M, flags, scores, hidden, workspace, 10 * md, stream, &pk, nullptr, ins);
}

int vs_scorer_forward_packed(const vs_weights *w, const float *x, const int32_t *lengths, const int32_t *lengths_dev,
                             int32_t B, uint32_t flags, float *scores, float *hidden, void *workspace,
                             size_t workspace_bytes, void *stream) {
    return forward_packed(w, x, lengths, lengths_dev, B, flags, scores, hidden, workspace, workspace_bytes, stream, nullptr);
}

// ---- attention maps on packed ragged batches (include/vs_inspect.h) ----
// M = sum of the lengths, tiles = sum ceil(T_b / 32) (the capacity rule of the size function AND of the launch), sumsq = sum T_b^2
static int probs_packed_sizes(const int32_t *lengths, int32_t B, int &M, int &tiles, size_t &sumsq) {
    if (!lengths || B <= 0) return vs_failf(VS_ERR_INVALID, "lengths is NULL or B=%d", B);
    long long m = 0, n = 0;
    sumsq = 0;
    for (int b = 0; b < B; ++b) {
        const int t = lengths[b];
        if (t <= 0) return vs_failf(VS_ERR_INVALID, "lengths[%d]=%d", b, t);
        m += t;
        n += (t + 31) / 32;
        sumsq += (size_t)t * (size_t)t;
        if (m > (1ll << 30)) return vs_failf(VS_ERR_INVALID, "too many frames");
    }
    M = (int)m;
    tiles = (int)n;
    return VS_OK;
}

size_t vs_attention_probs_packed_workspace_bytes(const int32_t *lengths, int32_t B, int32_t H) {
    int M = 0, tiles = 0;
    size_t sumsq = 0;
    if (H <= 0 || probs_packed_sizes(lengths, B, M, tiles, sumsq) != VS_OK) return 0;
    return vsk_attention_probs_packed_workspace_bytes(B, H, M, tiles);
}

int vs_attention_probs_packed_f32(const float *q, const float *k, const int32_t *lengths, const int32_t *lengths_dev, int32_t B,
                                  int32_t H, int32_t dh, float scale, float *maps, float *received, float *entropy,
                                  void *workspace, size_t workspace_bytes, void *stream) {
    if (!q || !k) return vs_failf(VS_ERR_INVALID, "q / k is NULL");
    if (!lengths_dev) return vs_failf(VS_ERR_INVALID, "lengths_dev is NULL");
    if (!maps && !received && !entropy) return vs_failf(VS_ERR_INVALID, "maps, received and entropy are all NULL");
    if (H <= 0) return vs_failf(VS_ERR_INVALID, "H=%d", H);
    int M = 0, tiles = 0;
    size_t sumsq = 0;
    if (int rc = probs_packed_sizes(lengths, B, M, tiles, sumsq)) return rc;
    if (dh != 32 && dh != 64 && dh != 128) return vs_failf(VS_ERR_INVALID, "head_dim=%d unsupported on packed batches (32, 64 or 128)", dh);
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)maps | (uintptr_t)received | (uintptr_t)entropy) & 15)
        return vs_failf(VS_ERR_INVALID, "q / k / maps / received / entropy must be 16-byte aligned");
    const size_t need = vsk_attention_probs_packed_workspace_bytes(B, H, M, tiles);
    if (!workspace || workspace_bytes < need)
        return vs_failf(VS_ERR_WORKSPACE, "workspace %zu bytes < %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 255) return vs_failf(VS_ERR_INVALID, "workspace must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    VS_LAUNCH(vsk_attention_probs_packed_plan(lengths_dev, B, H, M, tiles, workspace, st));
    VS_LAUNCH(vsk_attention_probs_packed(q, k, nullptr, maps, received, entropy, B, H, M, tiles, dh, scale, workspace, st));
    return VS_OK;
}

size_t vs_inspect_workspace_bytes_packed(const vs_weights *w, const int32_t *lengths, int32_t B) {
    const size_t core = vs_scorer_workspace_bytes_packed(w, lengths, B);      // 0: invalid (checks w, lengths, the head dim)
    if (core == 0) return 0;
    return align_up(core, 256) + vs_attention_probs_packed_workspace_bytes(lengths, B, w->desc.num_heads);
}

int vs_inspect_forward_packed(const vs_weights *w, const float *x, const int32_t *lengths, const int32_t *lengths_dev, int32_t B,
                              const int32_t *layers, int32_t n_layers, float *scores, float *hidden, float *maps, float *received,
                              float *entropy, void *workspace, size_t workspace_bytes, void *stream) {
    if (!w) return vs_failf(VS_ERR_INVALID, "weights is NULL");
    if (!lengths_dev) return vs_failf(VS_ERR_INVALID, "lengths_dev is NULL");
    if (!layers || n_layers <= 0) return vs_failf(VS_ERR_INVALID, "layers is NULL or n_layers=%d", n_layers);
    for (int i = 0; i < n_layers; ++i) {
        if (layers[i] < 0 || layers[i] >= w->desc.num_layers)
            return vs_failf(VS_ERR_INVALID, "layers[%d]=%d out of range (num_layers=%d)", i, layers[i], w->desc.num_layers);
        if (i && layers[i] <= layers[i - 1]) return vs_failf(VS_ERR_INVALID, "layers must be strictly ascending (layers[%d]=%d after %d)", i, layers[i], layers[i - 1]);
    }
    if (!x || !scores) return vs_failf(VS_ERR_INVALID, "weights/x/scores is NULL");
    if (!maps && !received && !entropy) return vs_failf(VS_ERR_INVALID, "maps, received and entropy are all NULL");
    if (((uintptr_t)maps | (uintptr_t)received | (uintptr_t)entropy | (uintptr_t)x | (uintptr_t)hidden) & 15)
        return vs_failf(VS_ERR_INVALID, "x / hidden / maps / received / entropy must be 16-byte aligned");
    std::vector<int> cu, work;
    int nw = 0;
    if (int rc = packed_plan(w, lengths, B, cu, work, nw)) return rc;      // B, the lengths, the positional table, the head dim
    int M = 0, tiles = 0;
    size_t sumsq = 0;
    if (int rc = probs_packed_sizes(lengths, B, M, tiles, sumsq)) return rc;
    const size_t core = align_up(vs_scorer_workspace_bytes_packed(w, lengths, B), 256);
    const size_t need = core + vsk_attention_probs_packed_workspace_bytes(B, w->desc.num_heads, M, tiles);
    if (!workspace || workspace_bytes < need)
        return vs_failf(VS_ERR_WORKSPACE, "workspace %zu bytes < %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 255) return vs_failf(VS_ERR_INVALID, "workspace must be 256-byte aligned");
    InspectHook ins{layers, n_layers, maps, received, entropy, (char *)workspace + core};
    ins.videos = B;
    ins.tiles = tiles;
    ins.map_stride = (size_t)w->desc.num_heads * sumsq;
    VS_LAUNCH(vsk_attention_probs_packed_plan(lengths_dev, B, w->desc.num_heads, M, tiles, ins.workspace, (hipStream_t)stream));
    return forward_packed(w, x, lengths, lengths_dev, B, 0u, scores, hidden, workspace, core, stream, &ins);
}

int vs_profile_enable(int32_t on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto &r : g_prof) { g_event_pool.push_back(r.a); g_event_pool.push_back(r.b); }
    g_prof.clear();
    if (!on) {      // profiling off: give the events back to the runtime
        for (hipEvent_t e : g_event_pool) (void)hipEventDestroy(e);
        g_event_pool.clear();
    }
    g_prof_on.store(on != 0);
    return VS_OK;
}

int vs_set_option(const char *name, int32_t value) {
    if (!name) return vs_failf(VS_ERR_INVALID, "option name is NULL");
    for (const auto &k : kOptions)
        if (strcmp(k.name, name) == 0) {
            vsk_options().*(k.field) = value < 0 ? option_from_env(k) : value;
            return VS_OK;
        }
    return vs_failf(VS_ERR_INVALID, "unknown option %s", name);
}

int vs_profile_collect(double *ms_sum, int64_t *launches) {
    if (!ms_sum || !launches) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (int i = 0; i < VS_NUM_STAGES; ++i) { ms_sum[i] = 0.0; launches[i] = 0; }
    for (auto &r : g_prof) {
        VS_HIP(hipEventSynchronize(r.b));
        float ms = 0.f;
        VS_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        ms_sum[r.stage] += ms;
        launches[r.stage] += 1;
        g_event_pool.push_back(r.a);
        g_event_pool.push_back(r.b);
    }
    g_prof.clear();
    return VS_OK;
}

const char *vs_stage_name(int32_t stage) {
    return (stage >= 0 && stage < VS_NUM_STAGES) ? kStageNames[stage] : "";
}

#ifdef VS_WITH_DIAG
// Diagnostic entry (not part of include/vs_scorer.h): fc1-shaped GEMM with s_memtime phase stamps.
// diag = [grid*4 waves][8] u64: issue, mfma, epilogue, stage, barrier, total cycles, k-tiles, t_begin.
int vs_diag_gemm(const float *A, const float *W, const float *bias, float *C, int32_t M, int32_t N, int32_t K,
                 int32_t grid, unsigned long long *diag, void *stream) {
    VS_LAUNCH(vsk_diag_gemm(A, W, bias, C, M, N, K, grid, diag, (hipStream_t)stream));
    return VS_OK;
}
// Diagnostic entry: exact head-dim-64 attention with per-phase s_memtime stamps; returns the number of blocks (> 0) or
// -status.  diag: [blocks * 8 waves][16] u64 (layout: vs_attention.hip, attn_fwd_pipe DIAG).
int vs_diag_attention(const float *q, const float *k, const float *v, float *out, int32_t B, int32_t H, int32_t T,
                      float scale, unsigned long long *diag, void *stream) {
    const int blocks = vsk_diag_attention(q, k, v, out, B, H, T, scale, diag, (hipStream_t)stream);
    return blocks;
}
int vs_diag_attention_lp(const float *q, const float *k, const float *v, float *out, int32_t B, int32_t H, int32_t T,
                         float scale, int32_t prec, unsigned long long *diag, void *stream) {
    return vsk_diag_attention_lp(q, k, v, out, B, H, T, scale, prec, diag, (hipStream_t)stream);
}
#endif  // VS_WITH_DIAG

static int linear_entry(const float *A, const float *W, const float *bias, float *C, int32_t M, int32_t N,
                        int32_t K, int32_t relu, const float *pe, int32_t T, int bf16, void *stream) {
    if (!A || !W || !bias || !C) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (M <= 0 || N <= 0 || N % 32 || K <= 0 || K % 32)
        return vs_failf(VS_ERR_INVALID, "M=%d N=%d K=%d unsupported (N, K multiples of 32)", M, N, K);
    if (pe && (T <= 0 || relu)) return vs_failf(VS_ERR_INVALID, "pe needs T > 0 and relu == 0");
    VS_LAUNCH(vsk_linear(A, W, nullptr, bias, C, M, N, K, relu, pe, T > 0 ? T : 1, bf16, (hipStream_t)stream));
    return VS_OK;
}

int vs_linear_bf16_operands(const void *A16, const void *W16, const float *bias, void *C, int32_t M, int32_t N, int32_t K,
                            int32_t relu, int32_t c16, void *stream) {
    if (!A16 || !W16 || !bias || !C) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (!vsk_gemm16_supported(M, N, K)) return vs_failf(VS_ERR_INVALID, "M=%d N=%d K=%d unsupported (N, K multiples of 32)", M, N, K);
    if (((uintptr_t)A16 | (uintptr_t)W16 | (uintptr_t)C | (uintptr_t)bias) & 15) return vs_failf(VS_ERR_INVALID, "operands must be 16-byte aligned");
    VS_LAUNCH(vsk_gemm16(A16, W16, bias, C, M, N, K, relu ? 1 : 0, c16 ? 1 : 0, 1, 0, 0, 1.0f, (hipStream_t)stream));
    return VS_OK;
}

int vs_qkv_proj_bf16_operands(const void *h16, const void *Wqkv16, const float *bqkv, void *qkv, int32_t B, int32_t T,
                              int32_t d, int32_t H, int32_t c16, void *stream) {
    if (!h16 || !Wqkv16 || !bqkv || !qkv) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (B <= 0 || T <= 0 || d <= 0 || d % 32 || H <= 0 || d % H || (d / H) % 32)
        return vs_failf(VS_ERR_INVALID, "B=%d T=%d d=%d H=%d unsupported", B, T, d, H);
    VS_LAUNCH(vsk_gemm16(h16, Wqkv16, bqkv, qkv, B * T, 3 * d, d, 3, c16 ? 1 : 0, T, H, d / H,
                         vsk_attention_qscale(1.0f / sqrtf((float)d)), (hipStream_t)stream));
    return VS_OK;
}

int vs_to_bf16(const float *src, void *dst16, size_t n, void *stream) {
    if (!src || !dst16 || n % 8 || (((uintptr_t)src | (uintptr_t)dst16) & 15)) return vs_failf(VS_ERR_INVALID, "vs_to_bf16: n %% 8 == 0, 16-byte aligned pointers");
    VS_LAUNCH(vsk_to_bf16(src, dst16, n, (hipStream_t)stream));
    return VS_OK;
}

int vs_linear_bf16_a16(const void *A16, const float *W, const float *bias, float *C, int32_t M, int32_t N, int32_t K,
                       const float *pe, void *stream) {
    if (!A16 || !W || !bias || !C) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (M <= 0 || N <= 0 || N % 32 || K <= 0 || K % 32)
        return vs_failf(VS_ERR_INVALID, "M=%d N=%d K=%d unsupported (N, K multiples of 32)", M, N, K);
    VS_LAUNCH(vsk_linear((const float *)A16, W, nullptr, bias, C, M, N, K, 0, pe, M, 1 | VSK_A16, (hipStream_t)stream));
    return VS_OK;
}

int vs_linear_f32(const float *A, const float *W, const float *bias, float *C, int32_t M, int32_t N,
                  int32_t K, int32_t relu, const float *pe, int32_t T, void *stream) {
    return linear_entry(A, W, bias, C, M, N, K, relu, pe, T, 0, stream);
}

int vs_linear_bf16(const float *A, const float *W, const float *bias, float *C, int32_t M, int32_t N,
                   int32_t K, int32_t relu, const float *pe, int32_t T, void *stream) {
    return linear_entry(A, W, bias, C, M, N, K, relu, pe, T, 1, stream);
}

int vs_mlp_block_bf16(const vs_weights *w, int32_t layer, const float *h, float *out, int32_t M, int32_t with_head,
                      int32_t sigmoid, float *scores, void *stream) {
    if (!w || !h || !out) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (layer < 0 || layer >= w->desc.num_layers || M <= 0) return vs_failf(VS_ERR_INVALID, "layer=%d M=%d", layer, M);
    if (!vsk_mlp_bf16_supported(w->desc.d_model))
        return vs_failf(VS_ERR_INVALID, "the fused bf16 MLP kernel needs d_model == 256 (got %d)", w->desc.d_model);
    if (with_head && !scores) return vs_failf(VS_ERR_INVALID, "scores is NULL");
    if (((uintptr_t)h & 15) || ((uintptr_t)out & 15)) return vs_failf(VS_ERR_INVALID, "h/out must be 16-byte aligned");
    const LayerOff &P = w->layers[layer];
    if (int rc = vsw_ensure(w, VSW_BF16, stream)) return rc;
    VS_LAUNCH(vsk_mlp_bf16(h, nullptr, nullptr, nullptr, nullptr, w->p(P.b_mlp), w->p(P.b1), w->p(P.b2), w->p(P.ln2g), w->p(P.ln2b), out, M,
                           w->desc.d_model, with_head ? w->p(w->final_w) : nullptr, with_head ? w->p(w->final_b) : nullptr,
                           w->desc.num_classes, sigmoid, with_head ? scores : nullptr, nullptr, (hipStream_t)stream));
    return VS_OK;
}

int vs_linear_f16x3(const float *A, const float *W, const float *bias, float *C, int32_t M, int32_t N,
                    int32_t K, int32_t relu, const float *pe, int32_t T, void *stream) {
    return linear_entry(A, W, bias, C, M, N, K, relu, pe, T, 2, stream);
}

int vs_qkv_proj_f32(const float *h, const float *Wqkv, const float *bqkv, float *qkv, int32_t B,
                    int32_t T, int32_t d, int32_t H, void *stream) {
    if (!h || !Wqkv || !bqkv || !qkv) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (B <= 0 || T <= 0 || d <= 0 || d % 32 || H <= 0 || d % H || (d / H) % 32)
        return vs_failf(VS_ERR_INVALID, "B=%d T=%d d=%d H=%d unsupported", B, T, d, H);
    VS_LAUNCH(vsk_qkv(h, Wqkv, nullptr, bqkv, qkv, B, T, d, H, 0, (hipStream_t)stream));
    return VS_OK;
}

int vs_attention_f32(const float *q, const float *k, const float *v, const uint8_t *key_pad_mask,
                     float *out, int32_t B, int32_t H, int32_t T, int32_t dh, float scale, void *stream) {
    if (!q || !k || !v || !out) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (B <= 0 || H <= 0 || T <= 0) return vs_failf(VS_ERR_INVALID, "B=%d H=%d T=%d", B, H, T);
    if (dh != 32 && dh != 64 && dh != 128) return vs_failf(VS_ERR_INVALID, "head_dim=%d unsupported", dh);
    VS_LAUNCH(vsk_attention(q, k, v, key_pad_mask, out, B, H, T, dh, scale, (hipStream_t)stream));
    return VS_OK;
}

static int attention_lp_entry(const float *q, const float *k, const float *v, const uint8_t *key_pad_mask,
                              float *out, int32_t B, int32_t H, int32_t T, int32_t dh, float scale, int prec, void *stream) {
    if (!q || !k || !v || !out) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (B <= 0 || H <= 0 || T <= 0) return vs_failf(VS_ERR_INVALID, "B=%d H=%d T=%d", B, H, T);
    if (dh != 32 && dh != 64 && !(dh == 128 && prec == 1))
        return vs_failf(VS_ERR_INVALID, "head_dim=%d unsupported on the %s path", dh, prec == 1 ? "bf16" : "f16x3");
    VS_LAUNCH(vsk_attention_bf16(q, k, v, key_pad_mask, out, B, H, T, dh, scale, prec, (hipStream_t)stream));
    return VS_OK;
}

int vs_attention_bf16(const float *q, const float *k, const float *v, const uint8_t *key_pad_mask,
                      float *out, int32_t B, int32_t H, int32_t T, int32_t dh, float scale, void *stream) {
    return attention_lp_entry(q, k, v, key_pad_mask, out, B, H, T, dh, scale, 1, stream);
}

int vs_attention_bf16_stored(const void *q16, const void *k16, const void *v16, const uint8_t *key_pad_mask,
                             void *out16, int32_t B, int32_t H, int32_t T, int32_t dh, void *stream) {
    if (!q16 || !k16 || !v16 || !out16) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (B <= 0 || H <= 0 || T <= 0) return vs_failf(VS_ERR_INVALID, "B=%d H=%d T=%d", B, H, T);
    if (dh != 32 && dh != 64 && dh != 128) return vs_failf(VS_ERR_INVALID, "head_dim=%d unsupported on the bf16 path", dh);
    if ((((uintptr_t)q16 | (uintptr_t)k16 | (uintptr_t)v16 | (uintptr_t)out16) & 15) != 0)
        return vs_failf(VS_ERR_INVALID, "q16 / k16 / v16 / out16 must be 16-byte aligned");
    VS_LAUNCH(vsk_attention_bf16((const float *)q16, (const float *)k16, (const float *)v16, key_pad_mask, (float *)out16, B, H, T, dh,
                                 1.0f, 1 | VSK_STORE16, (hipStream_t)stream));
    return VS_OK;
}

float vs_attention_qscale(float scale) { return vsk_attention_qscale(scale); }

int vs_attention_f16x3(const float *q, const float *k, const float *v, const uint8_t *key_pad_mask,
                       float *out, int32_t B, int32_t H, int32_t T, int32_t dh, float scale, void *stream) {
    return attention_lp_entry(q, k, v, key_pad_mask, out, B, H, T, dh, scale, 2, stream);
}

static int linear_ln_entry(const float *A, const float *W, const float *bias,
                           const float *residual, const float *gamma, const float *beta,
                           float *out, int32_t M, int32_t N, int32_t K, const float *score_w,
                           const float *score_b, int32_t num_classes, int32_t sigmoid,
                           float *scores, int bf16, void *stream) {
    if (!A || !W || !bias || !residual || !gamma || !beta || !out) return vs_failf(VS_ERR_INVALID, "NULL pointer");
    if (M <= 0 || N <= 0 || N % 64 || N > 512 || K <= 0 || K % 16)
        return vs_failf(VS_ERR_INVALID, "M=%d N=%d K=%d unsupported (N multiple of 64 <= 512, K multiple of 16)", M, N, K);
    if (score_w && (!score_b || !scores || num_classes <= 0))
        return vs_failf(VS_ERR_INVALID, "score head needs score_b, scores and num_classes > 0");
    if (bf16 && N > 256) return vs_failf(VS_ERR_INVALID, "N=%d unsupported on the bf16 path (N <= 256)", N);
    VS_LAUNCH(vsk_linear_res_ln(A, W, nullptr, bias, residual, gamma, beta, out, M, N, K, score_w, score_b, num_classes,
                                sigmoid, scores, bf16, (hipStream_t)stream));
    return VS_OK;
}

int vs_linear_residual_layernorm_f32(const float *A, const float *W, const float *bias,
                                     const float *residual, const float *gamma, const float *beta,
                                     float *out, int32_t M, int32_t N, int32_t K, const float *score_w,
                                     const float *score_b, int32_t num_classes, int32_t sigmoid,
                                     float *scores, void *stream) {
    return linear_ln_entry(A, W, bias, residual, gamma, beta, out, M, N, K, score_w, score_b, num_classes, sigmoid,
                           scores, 0, stream);
}

int vs_linear_residual_layernorm_bf16(const float *A, const float *W, const float *bias,
                                      const float *residual, const float *gamma, const float *beta,
                                      float *out, int32_t M, int32_t N, int32_t K, const float *score_w,
                                      const float *score_b, int32_t num_classes, int32_t sigmoid,
                                      float *scores, void *stream) {
    return linear_ln_entry(A, W, bias, residual, gamma, beta, out, M, N, K, score_w, score_b, num_classes, sigmoid,
                           scores, 1, stream);
}

int vs_linear_residual_layernorm_f16x3(const float *A, const float *W, const float *bias,
                                       const float *residual, const float *gamma, const float *beta,
                                       float *out, int32_t M, int32_t N, int32_t K, const float *score_w,
                                       const float *score_b, int32_t num_classes, int32_t sigmoid,
                                       float *scores, void *stream) {
    return linear_ln_entry(A, W, bias, residual, gamma, beta, out, M, N, K, score_w, score_b, num_classes, sigmoid,
                           scores, 2, stream);
}

}  // extern "C"
