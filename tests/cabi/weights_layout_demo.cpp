// csrc/vs_weights_layout.h alone, as plain C++17 (no HIP): tests/test_weights_layout_host.py builds this with the host compiler
// and -fsanitize=address,undefined.  The oracle is the layout code the header replaced, restated here as straight-line code: the
// `take` sequence of vs_weights_pack, the one of the allocation branch of ensure_transposed, and the optimizer's handle_tensor
// switch.  Over a grid of model shapes: every offset of both blobs and both totals equal the oracle's, the tensor table equals
// handle_tensor entry by entry, the matrix table has the five shapes, and every range lies inside its blob and overlaps no other.
// Prints "OK" or the first failed check.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "vs_weights_layout.h"

#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAILED line %d: %s  (d=%d L=%d in=%d classes=%d max_len=%d)\n", __LINE__, #__VA_ARGS__, \
                                                         D.d_model, D.num_layers, D.in_features, D.num_classes, D.max_len); return 1; } } while (0)

namespace {

// the image sizes the kernels of vs_mlp_fused.hip report: 40 960-byte LDS images, 4 + 32 of them for Wo | W1 | W2, 12 for Wqkv, one
// per 64 input features for the embedding; d_model 256 only
const size_t IMG = 40960;
size_t mlp_bytes(int d) { return d == 256 ? 36 * IMG : 0; }
size_t qkv_bytes(int d) { return d == 256 ? 12 * IMG : 0; }
size_t embed_bytes(int d, int K) { return d == 256 && K > 0 && K % 64 == 0 ? (size_t)(K / 64) * IMG : 0; }

struct Old {
    size_t embed_w = 0, embed_b = 0, pe = 0, final_w = 0, final_b = 0, f_embed_w = 0, h_embed_w = 0, b_embed = 0, blob_floats = 0;
    bool has_pe = false, has_b_embed = false;
    std::vector<LayerOff> layers;
    size_t t_embed_w = 0, tf_embed_w = 0, zeros = 0, nz = 0, tblob_floats = 0;
    std::vector<LayerOffT> tlayers;
};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
size_t align_floats(size_t n) { return (n + 63) / 64 * 64; }

// vs_weights_pack before the layout header
void old_pack(const vs_model_desc *desc, bool pos_embedding, Old *w) {
    const size_t d = desc->d_model, din = desc->in_features, nc = desc->num_classes;
    const bool mlp_supported = d == 256;
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += align_up(n, 64); return o; };   // 256-B aligned
    w->embed_w = take(d * din);
    w->embed_b = take(d);
    w->has_pe = pos_embedding;
    if (w->has_pe) w->pe = take((size_t)desc->max_len * d);
    w->layers.resize(desc->num_layers);
    for (auto &L : w->layers) {
        L.wqkv = take(3 * d * d); L.bqkv = take(3 * d);
        L.wo = take(d * d);       L.bo = take(d);
        L.ln1g = take(d);         L.ln1b = take(d);
        L.w1 = take(4 * d * d);   L.b1 = take(4 * d);
        L.w2 = take(4 * d * d);   L.b2 = take(d);
        L.ln2g = take(d);         L.ln2b = take(d);
    }
    w->final_w = take(nc * d);
    w->final_b = take(nc);
    w->f_embed_w = take(d * din);
    for (auto &L : w->layers) {
        L.f_wqkv = take(3 * d * d); L.f_wo = take(d * d); L.f_w1 = take(4 * d * d); L.f_w2 = take(4 * d * d);
    }
    w->h_embed_w = take(d * din);
    for (auto &L : w->layers) {
        L.h_wqkv = take(3 * d * d); L.h_wo = take(d * d); L.h_w1 = take(4 * d * d); L.h_w2 = take(4 * d * d);
    }
    if (mlp_supported)
        for (auto &L : w->layers) {
            L.b_mlp = take(mlp_bytes((int)d) / sizeof(float));
            L.b_qkv = take(qkv_bytes((int)d) / sizeof(float));
        }
    for (auto &L : w->layers) {
        L.r_wqkv = take(3 * d * d / 2); L.r_wo = take(d * d / 2); L.r_w1 = take(4 * d * d / 2); L.r_w2 = take(4 * d * d / 2);
    }
    w->has_b_embed = embed_bytes((int)d, (int)din) != 0;
    if (w->has_b_embed) w->b_embed = take(embed_bytes((int)d, (int)din) / sizeof(float));
    w->blob_floats = off;
}

// the allocation branch of ensure_transposed before the layout header
void old_transposed(const vs_model_desc *desc, Old *w) {
    const size_t d = desc->d_model, din = desc->in_features;
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += align_floats(n); return o; };
    w->t_embed_w = take(d * din);
    w->tf_embed_w = take(d * din);
    w->tlayers.resize(desc->num_layers);
    for (auto &L : w->tlayers) {
        L.t_wqkv = take(3 * d * d); L.t_wo = take(d * d); L.t_w1 = take(4 * d * d); L.t_w2 = take(4 * d * d);
        L.t16_w2 = take(4 * d * d / 2);
        L.tf_wqkv = take(3 * d * d); L.tf_wo = take(d * d); L.tf_w1 = take(4 * d * d); L.tf_w2 = take(4 * d * d);
    }
    const size_t nz = 4 * d > din ? 4 * d : din;
    w->zeros = take(nz);
    w->nz = nz;
    w->tblob_floats = off;
}

// the optimizer's handle_tensor before the tensor table: tensor `i` in vs_model_params order
VsTensorAt old_handle_tensor(const vs_model_desc &desc, const Old *w, int i) {
    const size_t d = desc.d_model, din = desc.in_features, nc = desc.num_classes;
    const int L = desc.num_layers;
    if (i == 0) return {w->embed_w, d * din};
    if (i == 1) return {w->embed_b, d};
    if (i == 2 + 16 * L) return {w->final_w, nc * d};
    if (i == 3 + 16 * L) return {w->final_b, nc};
    const LayerOff &o = w->layers[(i - 2) / 16];
    switch ((i - 2) % 16) {
        case 0: return {o.wqkv, d * d};
        case 1: return {o.bqkv, d};
        case 2: return {o.wqkv + d * d, d * d};
        case 3: return {o.bqkv + d, d};
        case 4: return {o.wqkv + 2 * d * d, d * d};
        case 5: return {o.bqkv + 2 * d, d};
        case 6: return {o.wo, d * d};
        case 7: return {o.bo, d};
        case 8: return {o.ln1g, d};
        case 9: return {o.ln1b, d};
        case 10: return {o.w1, 4 * d * d};
        case 11: return {o.b1, 4 * d};
        case 12: return {o.w2, 4 * d * d};
        case 13: return {o.b2, d};
        case 14: return {o.ln2g, d};
        default: return {o.ln2b, d};
    }
}

struct Range { size_t off, n; };
// every range inside [0, total) and disjoint from every other
bool disjoint_inside(std::vector<Range> r, size_t total) {
    std::sort(r.begin(), r.end(), [](const Range &a, const Range &b) { return a.off < b.off; });
    size_t end = 0;
    for (const Range &x : r) {
        if (x.n == 0 || x.off < end || x.off % 64) return false;
        end = x.off + x.n;
    }
    return end <= total;
}

int check(const vs_model_desc &D, bool pos) {
    const int d = D.d_model, din = D.in_features, Ln = D.num_layers;
    const size_t sd = d, sin = din;
    Old O;
    old_pack(&D, pos, &O);
    old_transposed(&D, &O);
    const VsWeightsLayout W = vs_weights_layout(D, pos, mlp_bytes(d), qkv_bytes(d), embed_bytes(d, din));

    // ---- first blob ----
    CHECK(W.embed_w == O.embed_w && W.embed_b == O.embed_b && W.has_pe == O.has_pe && W.pe == O.pe);
    CHECK(W.final_w == O.final_w && W.final_b == O.final_b && W.f_embed_w == O.f_embed_w && W.h_embed_w == O.h_embed_w);
    CHECK(W.has_b_embed == O.has_b_embed && W.b_embed == O.b_embed && W.blob_floats == O.blob_floats);
    CHECK((int)W.layers.size() == Ln && (int)W.tlayers.size() == Ln);
    for (int l = 0; l < Ln; ++l) {
        const LayerOff &a = W.layers[l], &b = O.layers[l];
        CHECK(a.wqkv == b.wqkv && a.bqkv == b.bqkv && a.wo == b.wo && a.bo == b.bo && a.ln1g == b.ln1g && a.ln1b == b.ln1b);
        CHECK(a.w1 == b.w1 && a.b1 == b.b1 && a.w2 == b.w2 && a.b2 == b.b2 && a.ln2g == b.ln2g && a.ln2b == b.ln2b);
        CHECK(a.f_wqkv == b.f_wqkv && a.f_wo == b.f_wo && a.f_w1 == b.f_w1 && a.f_w2 == b.f_w2);
        CHECK(a.h_wqkv == b.h_wqkv && a.h_wo == b.h_wo && a.h_w1 == b.h_w1 && a.h_w2 == b.h_w2);
        CHECK(a.b_mlp == b.b_mlp && a.b_qkv == b.b_qkv);
        CHECK(a.r_wqkv == b.r_wqkv && a.r_wo == b.r_wo && a.r_w1 == b.r_w1 && a.r_w2 == b.r_w2);
    }
    // ---- second blob ----
    CHECK(W.t_embed_w == O.t_embed_w && W.tf_embed_w == O.tf_embed_w && W.zeros == O.zeros && W.zeros_floats == O.nz);
    CHECK(W.tblob_floats == O.tblob_floats);
    for (int l = 0; l < Ln; ++l) {
        const LayerOffT &a = W.tlayers[l], &b = O.tlayers[l];
        CHECK(a.t_wqkv == b.t_wqkv && a.t_wo == b.t_wo && a.t_w1 == b.t_w1 && a.t_w2 == b.t_w2 && a.t16_w2 == b.t16_w2);
        CHECK(a.tf_wqkv == b.tf_wqkv && a.tf_wo == b.tf_wo && a.tf_w1 == b.tf_w1 && a.tf_w2 == b.tf_w2);
    }

    // ---- the tensor table: handle_tensor, entry by entry ----
    CHECK((int)W.tensors.size() == 4 + 16 * Ln);
    for (int i = 0; i < 4 + 16 * Ln; ++i) {
        const VsTensorAt want = old_handle_tensor(D, &O, i);
        CHECK(W.tensors[i].off == want.off && W.tensors[i].n == want.n);
    }

    // ---- the matrix table: [d, in_features], then [3d, d], [d, d], [4d, d], [d, 4d] per layer, each with the old named offsets ----
    CHECK((int)W.matrices.size() == 1 + 4 * Ln);
    const VsMatrixAt &E = W.matrices[0];
    CHECK(E.src == O.embed_w && E.N == d && E.K == din && E.frag == O.f_embed_w && E.f16x3 == O.h_embed_w && E.rows16 == VSW_NONE);
    CHECK(E.t == O.t_embed_w && E.tfrag == O.tf_embed_w && E.t16 == VSW_NONE);
    for (int l = 0; l < Ln; ++l) {
        const LayerOff &P = O.layers[l];
        const LayerOffT &Q = O.tlayers[l];
        const VsMatrixAt *m = &W.matrices[1 + 4 * l];
        CHECK(m[0].N == 3 * d && m[0].K == d && m[1].N == d && m[1].K == d && m[2].N == 4 * d && m[2].K == d && m[3].N == d && m[3].K == 4 * d);
        CHECK(m[0].src == P.wqkv && m[0].frag == P.f_wqkv && m[0].f16x3 == P.h_wqkv && m[0].rows16 == P.r_wqkv);
        CHECK(m[1].src == P.wo && m[1].frag == P.f_wo && m[1].f16x3 == P.h_wo && m[1].rows16 == P.r_wo);
        CHECK(m[2].src == P.w1 && m[2].frag == P.f_w1 && m[2].f16x3 == P.h_w1 && m[2].rows16 == P.r_w1);
        CHECK(m[3].src == P.w2 && m[3].frag == P.f_w2 && m[3].f16x3 == P.h_w2 && m[3].rows16 == P.r_w2);
        CHECK(m[0].t == Q.t_wqkv && m[0].tfrag == Q.tf_wqkv && m[0].t16 == VSW_NONE);
        CHECK(m[1].t == Q.t_wo && m[1].tfrag == Q.tf_wo && m[1].t16 == VSW_NONE);
        CHECK(m[2].t == Q.t_w1 && m[2].tfrag == Q.tf_w1 && m[2].t16 == VSW_NONE);
        CHECK(m[3].t == Q.t_w2 && m[3].tfrag == Q.tf_w2 && m[3].t16 == Q.t16_w2);
    }

    // ---- every range inside its blob, none overlapping another ----
    std::vector<Range> r0, r1;
    r0.push_back({W.embed_w, sd * sin});
    r0.push_back({W.embed_b, sd});
    if (W.has_pe) r0.push_back({W.pe, (size_t)D.max_len * sd});
    for (const LayerOff &L : W.layers) {
        r0.push_back({L.wqkv, 3 * sd * sd}); r0.push_back({L.bqkv, 3 * sd});
        r0.push_back({L.wo, sd * sd});       r0.push_back({L.bo, sd});
        r0.push_back({L.ln1g, sd});          r0.push_back({L.ln1b, sd});
        r0.push_back({L.w1, 4 * sd * sd});   r0.push_back({L.b1, 4 * sd});
        r0.push_back({L.w2, 4 * sd * sd});   r0.push_back({L.b2, sd});
        r0.push_back({L.ln2g, sd});          r0.push_back({L.ln2b, sd});
        if (mlp_bytes(d)) { r0.push_back({L.b_mlp, mlp_bytes(d) / 4}); r0.push_back({L.b_qkv, qkv_bytes(d) / 4}); }
    }
    r0.push_back({W.final_w, (size_t)D.num_classes * sd});
    r0.push_back({W.final_b, (size_t)D.num_classes});
    if (W.has_b_embed) r0.push_back({W.b_embed, embed_bytes(d, din) / 4});
    for (const VsMatrixAt &m : W.matrices) {
        const size_t nk = (size_t)m.N * m.K;
        r0.push_back({m.frag, nk});
        r0.push_back({m.f16x3, nk});
        if (m.rows16 != VSW_NONE) r0.push_back({m.rows16, nk / 2});
        r1.push_back({m.t, nk});
        r1.push_back({m.tfrag, nk});
        if (m.t16 != VSW_NONE) r1.push_back({m.t16, nk / 2});
    }
    r1.push_back({W.zeros, W.zeros_floats});
    CHECK(disjoint_inside(r0, W.blob_floats));
    CHECK(disjoint_inside(r1, W.tblob_floats));
    // (the tensor table's q / k / v slices: each inside its wqkv / bqkv, which the ranges above cover)
    for (int l = 0; l < Ln; ++l)
        for (int s = 0; s < 3; ++s) {
            CHECK(W.tensors[2 + 16 * l + 2 * s].off == W.layers[l].wqkv + s * sd * sd);
            CHECK(W.tensors[2 + 16 * l + 2 * s + 1].off == W.layers[l].bqkv + s * sd);
        }
    return 0;
}

}  // namespace

int main() {
    int cases = 0;
    for (int d : {64, 128, 256, 320, 512, 1024})
        for (int layers : {1, 2, 4})
            for (int in_features : {32, 1024})
                for (int classes : {1, 3})
                    for (int max_len : {0, 100}) {
                        const vs_model_desc D{d, d / 64, layers, in_features, max_len, classes};
                        if (check(D, max_len > 0)) return 1;
                        ++cases;
                    }
    if (cases != 6 * 3 * 2 * 2 * 2) { std::printf("FAILED: %d cases\n", cases); return 1; }
    std::printf("OK\n");
    return 0;
}
