// vs_weights_layout.h - where everything lies in the two device allocations of a packed-parameter handle (DESIGN.md section
// 42): a pure function of the model's shape and of the three image sizes only the kernels know.  vs_weights (vs_weights_impl.h)
// IS this layout plus its pointers and version stamps; the launch sequences read the named fields, vs_weights.cpp and the
// optimizer walk the two tables.
// Host code, plain C++17, no HIP and no globals: tests/cabi/weights_layout_demo.cpp compiles this header alone.
#pragma once
#include <stddef.h>

#include <vector>

#include "vs_scorer.h"      // vs_model_desc

struct LayerOff {
    size_t wqkv, bqkv, wo, bo, ln1g, ln1b, w1, b1, w2, b2, ln2g, ln2b;
    size_t f_wqkv, f_wo, f_w1, f_w2;        // fragment-major copies for the latency kernels
    size_t h_wqkv, h_wo, h_w1, h_w2;        // their fp16x3 counterparts (hi|lo f16 halves, same size)
    size_t b_mlp;                           // Wo, W1, W2 as the LDS images of the fused bf16 layer-tail kernel (vsk_pack_mlp_bf16)
    size_t b_qkv;                           // Wqkv as the LDS images of that kernel's QKV epilogue (vsk_pack_qkv_bf16)
    size_t r_wqkv, r_wo, r_w1, r_w2;        // plain row-major bf16 copies (family VSW_ROWS16): the bf16-operand GEMM of d_model > 256
                                            // (vs_gemm_ring.hip) and the training path's A-stationary GEMM (vs_train_gemm_rows.hip)
};

// transposed weights for the dgrad GEMMs of the training backward (dX = dY W is an NT GEMM against W^T), in the second blob
struct LayerOffT {
    size_t t_wqkv, t_wo, t_w1, t_w2;          // W^T, row-major
    size_t t16_w2;                            // W2^T as bf16 (the A-stationary fc2 input-gradient GEMM of the bf16 training mode)
    size_t tf_wqkv, tf_wo, tf_w1, tf_w2;      // the same in fragment-major order (latency kernels at small batch)
};

// one parameter tensor as the caller hands it over (vs_model_params order): floats into the first blob
struct VsTensorAt { size_t off, n; };

// one weight matrix W [N, K] and its image in every per-matrix family; VSW_NONE: the family has no image of this matrix
constexpr size_t VSW_NONE = ~(size_t)0;
struct VsMatrixAt {
    size_t src;                     // first blob
    int N, K;
    size_t frag, f16x3, rows16;     // first blob: N K floats, N K floats, N K bf16
    size_t t, tfrag, t16;           // second blob: W^T [K, N] row-major, fragment-major, as bf16
};

struct VsWeightsLayout {
    // ---- first blob: the parameters and the scoring side's images ----
    size_t embed_w = 0, embed_b = 0, pe = 0, final_w = 0, final_b = 0, f_embed_w = 0, h_embed_w = 0;
    size_t b_embed = 0;           // W_embed as the LDS images of the bf16 embedding kernel (vsk_pack_embed_bf16), if supported
    bool has_b_embed = false;
    bool has_pe = false;
    std::vector<LayerOff> layers;
    size_t blob_floats = 0;
    // ---- second blob: transposed weights + a zero vector ----
    size_t t_embed_w = 0, tf_embed_w = 0, zeros = 0, zeros_floats = 0;
    std::vector<LayerOffT> tlayers;
    size_t tblob_floats = 0;
    // ---- the same offsets as tables ----
    std::vector<VsTensorAt> tensors;      // 4 + 16 L: embedding, 16 per layer (q / k / v are slices of wqkv / bqkv), score head
    std::vector<VsMatrixAt> matrices;     // 1 + 4 L: embed_w, then per layer wqkv, wo, w1, w2
};

// mlp_image_bytes / qkv_image_bytes / embed_image_bytes: vsk_mlp_bf16_image_bytes(d), vsk_qkv_bf16_image_bytes(d),
// vsk_embed_bf16_image_bytes(d, in_features); 0 = the kernel does not take this shape (no image is laid out)
inline VsWeightsLayout vs_weights_layout(const vs_model_desc &D, bool has_pe, size_t mlp_image_bytes, size_t qkv_image_bytes,
                                         size_t embed_image_bytes) {
    VsWeightsLayout W;
    const size_t d = D.d_model, din = D.in_features, nc = D.num_classes;
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += (n + 63) / 64 * 64; return o; };      // 256-byte granules
    W.embed_w = take(d * din);
    W.embed_b = take(d);
    W.has_pe = has_pe;
    if (has_pe) W.pe = take((size_t)D.max_len * d);
    W.layers.resize(D.num_layers);
    for (auto &L : W.layers) {
        L.wqkv = take(3 * d * d); L.bqkv = take(3 * d);
        L.wo = take(d * d);       L.bo = take(d);
        L.ln1g = take(d);         L.ln1b = take(d);
        L.w1 = take(4 * d * d);   L.b1 = take(4 * d);
        L.w2 = take(4 * d * d);   L.b2 = take(d);
        L.ln2g = take(d);         L.ln2b = take(d);
    }
    W.final_w = take(nc * d);
    W.final_b = take(nc);
    // (the fragment and f16x3 families are laid out for every shape, also those whose forward never reads them)
    W.f_embed_w = take(d * din);
    for (auto &L : W.layers) { L.f_wqkv = take(3 * d * d); L.f_wo = take(d * d); L.f_w1 = take(4 * d * d); L.f_w2 = take(4 * d * d); }
    W.h_embed_w = take(d * din);
    for (auto &L : W.layers) { L.h_wqkv = take(3 * d * d); L.h_wo = take(d * d); L.h_w1 = take(4 * d * d); L.h_w2 = take(4 * d * d); }
    if (mlp_image_bytes)
        for (auto &L : W.layers) { L.b_mlp = take(mlp_image_bytes / sizeof(float)); L.b_qkv = take(qkv_image_bytes / sizeof(float)); }
    for (auto &L : W.layers) { L.r_wqkv = take(3 * d * d / 2); L.r_wo = take(d * d / 2); L.r_w1 = take(4 * d * d / 2); L.r_w2 = take(4 * d * d / 2); }
    W.has_b_embed = embed_image_bytes != 0;
    if (W.has_b_embed) W.b_embed = take(embed_image_bytes / sizeof(float));
    W.blob_floats = off;

    off = 0;
    W.t_embed_w = take(d * din);
    W.tf_embed_w = take(d * din);
    W.tlayers.resize(D.num_layers);
    for (auto &L : W.tlayers) {
        L.t_wqkv = take(3 * d * d); L.t_wo = take(d * d); L.t_w1 = take(4 * d * d); L.t_w2 = take(4 * d * d);
        L.t16_w2 = take(4 * d * d / 2);
        L.tf_wqkv = take(3 * d * d); L.tf_wo = take(d * d); L.tf_w1 = take(4 * d * d); L.tf_w2 = take(4 * d * d);
    }
    W.zeros_floats = 4 * d > din ? 4 * d : din;
    W.zeros = take(W.zeros_floats);
    W.tblob_floats = off;

    W.tensors.reserve(4 + 16 * W.layers.size());
    W.matrices.reserve(1 + 4 * W.layers.size());
    W.tensors.push_back({W.embed_w, d * din});
    W.tensors.push_back({W.embed_b, d});
    W.matrices.push_back({W.embed_w, (int)d, (int)din, W.f_embed_w, W.h_embed_w, VSW_NONE, W.t_embed_w, W.tf_embed_w, VSW_NONE});
    for (size_t l = 0; l < W.layers.size(); ++l) {
        const LayerOff &P = W.layers[l];
        const LayerOffT &Q = W.tlayers[l];
        for (size_t s = 0; s < 3; ++s) {      // wq, bq, wk, bk, wv, bv
            W.tensors.push_back({P.wqkv + s * d * d, d * d});
            W.tensors.push_back({P.bqkv + s * d, d});
        }
        W.tensors.push_back({P.wo, d * d});       W.tensors.push_back({P.bo, d});
        W.tensors.push_back({P.ln1g, d});         W.tensors.push_back({P.ln1b, d});
        W.tensors.push_back({P.w1, 4 * d * d});   W.tensors.push_back({P.b1, 4 * d});
        W.tensors.push_back({P.w2, 4 * d * d});   W.tensors.push_back({P.b2, d});
        W.tensors.push_back({P.ln2g, d});         W.tensors.push_back({P.ln2b, d});
        W.matrices.push_back({P.wqkv, (int)(3 * d), (int)d, P.f_wqkv, P.h_wqkv, P.r_wqkv, Q.t_wqkv, Q.tf_wqkv, VSW_NONE});
        W.matrices.push_back({P.wo, (int)d, (int)d, P.f_wo, P.h_wo, P.r_wo, Q.t_wo, Q.tf_wo, VSW_NONE});
        W.matrices.push_back({P.w1, (int)(4 * d), (int)d, P.f_w1, P.h_w1, P.r_w1, Q.t_w1, Q.tf_w1, VSW_NONE});
        W.matrices.push_back({P.w2, (int)d, (int)(4 * d), P.f_w2, P.h_w2, P.r_w2, Q.t_w2, Q.tf_w2, Q.t16_w2});
    }
    W.tensors.push_back({W.final_w, nc * d});
    W.tensors.push_back({W.final_b, nc});
    return W;
}
