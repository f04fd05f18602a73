// vs_weights.cpp — the packed-parameter handle `vs_weights` (vs_weights_impl.h): pack / update / free,
// the copy of the caller's tensors into the blob, the stream ordering of the handle, and vsw_ensure, the one place that
// (re)builds a kernel-layout image family when a call that reads it finds it older than the parameters.  Where everything
// lies is decided once per handle, by vs_weights_layout.h; this file only walks that layout's two tables.
#include <hip/hip_runtime.h>

#include <mutex>

#include "vs_kernels.h"
#include "vs_train_kernels.h"      // vst_transpose_batch
#include "vs_weights_impl.h"

static_assert(sizeof(vs_layer_params) == 16 * sizeof(void *), "vs_layer_params: 16 pointers in declaration order");

namespace {

std::mutex g_wmu;       // the image families, the second blob and the ordering fields of every handle

int check_desc(const vs_model_desc *d) {
    if (!d) return vs_failf(VS_ERR_INVALID, "desc is NULL");
    if (d->d_model <= 0 || d->d_model % 64 || d->d_model > 1024)
        return vs_failf(VS_ERR_INVALID, "d_model=%d unsupported (multiple of 64, <= 1024)", d->d_model);
    if (d->num_heads <= 0 || d->d_model % d->num_heads)
        return vs_failf(VS_ERR_INVALID, "d_model=%d not divisible by num_heads=%d", d->d_model, d->num_heads);
    const int dh = d->d_model / d->num_heads;
    if (dh != 32 && dh != 64 && dh != 128 && dh != 256)
        return vs_failf(VS_ERR_INVALID, "head_dim=%d unsupported (32, 64, 128 or 256)", dh);
    if (d->num_layers < 1) return vs_failf(VS_ERR_INVALID, "num_layers=%d unsupported (>= 1)", d->num_layers);
    if (d->in_features <= 0 || d->in_features % 32)
        return vs_failf(VS_ERR_INVALID, "in_features=%d unsupported (multiple of 32)", d->in_features);
    if (d->num_classes <= 0) return vs_failf(VS_ERR_INVALID, "num_classes=%d", d->num_classes);
    if (d->max_len < 0) return vs_failf(VS_ERR_INVALID, "max_len=%d", d->max_len);
    return VS_OK;
}

// copies the parameters into w->blob (stream-ordered on `st`): one batched copy kernel for the embedding / head and
// one per encoder layer instead of 16 hipMemcpyAsync per layer (an optimizer step re-packs on every iteration).
// params->pos_embedding == NULL on an UPDATE keeps the table already packed (it is a buffer: an optimizer never writes it).
int fill_weights(vs_weights *w, const vs_model_params *params, hipStream_t st, bool update) {
    const vs_model_desc *desc = &w->desc;
    if (!params->embed_w || !params->embed_b || !params->final_w || !params->final_b ||
        (desc->num_layers > 0 && !params->layers))
        return vs_failf(VS_ERR_INVALID, "a required parameter pointer is NULL");
    if ((params->pos_embedding != nullptr) != (desc->max_len > 0) && !(update && !params->pos_embedding))
        return vs_failf(VS_ERR_INVALID, "pos_embedding / max_len mismatch");
    VskCopySegs segs{};
    bool ok = true;
    auto add = [&](size_t tensor, const float *src) {
        if (!src || segs.count >= VSK_COPY_MAX_SEGS) { ok = false; return; }
        const VsTensorAt &t = w->tensors[tensor];
        segs.src[segs.count] = src; segs.dst[segs.count] = w->blob + t.off; segs.n[segs.count] = (unsigned)t.n; ++segs.count;
    };
    auto flush = [&]() { if (ok && segs.count) ok = vsk_copy_segments(segs, st) == 0; segs.count = 0; };
    const size_t head = w->tensors.size() - 2;
    add(0, params->embed_w);
    add(1, params->embed_b);
    add(head, params->final_w);
    add(head + 1, params->final_b);
    flush();
    if (w->has_pe && params->pos_embedding)
        ok &= hipMemcpyAsync(w->blob + w->pe, params->pos_embedding, (size_t)desc->max_len * desc->d_model * sizeof(float),
                             hipMemcpyDeviceToDevice, st) == hipSuccess;
    for (int l = 0; l < desc->num_layers && ok; ++l) {
        const float *const *P = &params->layers[l].wq;      // the layer's 16 tensors, in the table's order
        for (int j = 0; j < 16; ++j) add(2 + 16 * (size_t)l + j, P[j]);
        flush();
    }
    if (!ok)
        return vs_failf(VS_ERR_HIP, "parameter copy failed (NULL pointer or launch error: %s)",
                        hipGetErrorString(hipGetLastError()));
    return VS_OK;
}

// ---- how each family is built: walks of the matrix table.  `stale`: the families this vsw_ensure rebuilds ----
int packed(bool ok) {
    return ok ? VS_OK : vs_failf(VS_ERR_HIP, "weight image packing failed: %s", hipGetErrorString(hipGetLastError()));
}

// one launch for all matrices (a reference-sized training step rebuilds this family after every optimizer step)
int build_fragments(const vs_weights *w, unsigned, hipStream_t st) {
    bool ok = true;
    VskMatJobs fj{};
    for (const VsMatrixAt &m : w->matrices) {
        if (fj.n == VskMatJobs::MAX) { ok &= vsk_pack_fragments_batch(fj, st) == 0; fj.n = 0; }
        fj.in[fj.n] = w->blob + m.src; fj.out[fj.n] = w->blob + m.frag; fj.rows[fj.n] = m.N; fj.cols[fj.n] = m.K; ++fj.n;
    }
    ok &= vsk_pack_fragments_batch(fj, st) == 0;
    return packed(ok);
}

int build_f16x3(const vs_weights *w, unsigned, hipStream_t st) {
    bool ok = true;
    for (const VsMatrixAt &m : w->matrices) ok &= vsk_pack_fragments_f16x3(w->blob + m.src, w->blob + m.f16x3, m.N, m.K, st) == 0;
    return packed(ok);
}

// the LDS images of the fused bf16 kernels hold several matrices each: per layer, not per matrix
int build_lds_images(const vs_weights *w, unsigned, hipStream_t st) {
    bool ok = true;
    float *blob = w->blob;
    const int d = w->desc.d_model;
    if (w->has_b_embed) ok &= vsk_pack_embed_bf16(blob + w->embed_w, blob + w->b_embed, d, w->desc.in_features, st) == 0;
    if (vsk_mlp_bf16_supported(d))
        for (const LayerOff &L : w->layers) {
            ok &= vsk_pack_mlp_bf16(blob + L.wo, blob + L.w1, blob + L.w2, blob + L.b_mlp, d, st) == 0;
            ok &= vsk_pack_qkv_bf16(blob + L.wqkv, blob + L.b_qkv, d, st) == 0;
        }
    return packed(ok);
}

int build_rows16(const vs_weights *w, unsigned, hipStream_t st) {
    bool ok = true;
    for (const VsMatrixAt &m : w->matrices)
        if (m.rows16 != VSW_NONE) ok &= vsk_to_bf16(w->blob + m.src, w->blob + m.rows16, (size_t)m.N * m.K, st) == 0;
    return packed(ok);
}

// W [N, K] -> W^T [K, N] row-major and / or its fragment-major copy, whichever is stale: one launch per family and group of
// matrices, the two families of a group behind each other (the pack reads what the transpose wrote)
int build_transposes(const vs_weights *w, unsigned stale, hipStream_t st) {
    const bool do_t = stale & VSW_TRANSPOSED, do_f = stale & VSW_TRANSPOSED_FRAGMENTS;
    VskMatJobs tj{}, fj{};
    auto flush = [&]() -> int {
        if (tj.n == 0) return 0;
        if (do_t) if (int rc = vst_transpose_batch(tj, st)) return rc;
        if (do_f) if (int rc = vsk_pack_fragments_batch(fj, st)) return rc;
        tj.n = fj.n = 0;
        return 0;
    };
    for (size_t i = 0; i < w->matrices.size(); ++i) {
        const VsMatrixAt &m = w->matrices[i];
        if (i % 4 == 1 && tj.n + 4 > VskMatJobs::MAX) VS_LAUNCH(flush());     // a layer's four matrices stay in one launch
        tj.in[tj.n] = w->blob + m.src; tj.out[tj.n] = w->tblob + m.t; tj.rows[tj.n] = m.N; tj.cols[tj.n] = m.K; ++tj.n;
        fj.in[fj.n] = w->tblob + m.t; fj.out[fj.n] = w->tblob + m.tfrag; fj.rows[fj.n] = m.K; fj.cols[fj.n] = m.N; ++fj.n;      // W^T is [K, N]
    }
    VS_LAUNCH(flush());
    return VS_OK;
}

// bf16 copy of every W2^T (vst_gemm_rows16's weight operand in the backward of the bf16 training mode): reads the transposes
int build_transposed_w2_16(const vs_weights *w, unsigned, hipStream_t st) {
    const size_t d = w->desc.d_model;
    for (const LayerOffT &Q : w->tlayers) VS_LAUNCH(vsk_to_bf16(w->tblob + Q.t_w2, w->tblob + Q.t16_w2, 4 * d * d, st));
    return VS_OK;
}

// row i: family 1 << i, stamped in vs_weights::built[i].  Rows with the same builder are adjacent and built by one call of it.
struct Family { unsigned bit; int blob; int (*build)(const vs_weights *, unsigned stale, hipStream_t); };
const Family kFamilies[VSW_NUM_FAMILIES] = {
    {VSW_FRAGMENTS, 0, build_fragments},
    {VSW_F16X3, 0, build_f16x3},
    {VSW_BF16, 0, build_lds_images},
    {VSW_ROWS16, 0, build_rows16},
    {VSW_TRANSPOSED, 1, build_transposes},
    {VSW_TRANSPOSED_FRAGMENTS, 1, build_transposes},
    {VSW_TRANSPOSED_W2_16, 1, build_transposed_w2_16},
};

}  // namespace

void vsw_mark(const vs_weights *w, void *stream) {
    if (!w->order_event) {
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return; }
        w->order_event = (void *)ev;
    }
    if (hipEventRecord((hipEvent_t)w->order_event, (hipStream_t)stream) == hipSuccess) {
        w->order_stream = stream;
        w->order_recorded = true;
    } else {
        (void)hipGetLastError();
    }
}

void vsw_order(const vs_weights *w, void *stream) {
    if (w->order_recorded && w->order_stream != stream)
        if (hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)w->order_event, 0) != hipSuccess) (void)hipGetLastError();
}

int vsw_ensure(const vs_weights *w, unsigned families, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(g_wmu);
    unsigned stale = 0, blobs = 0;
    for (int i = 0; i < VSW_NUM_FAMILIES; ++i)
        if (families & kFamilies[i].bit) {
            blobs |= 1u << kFamilies[i].blob;
            if (w->built[i] != w->version) stale |= kFamilies[i].bit;
        }
    if ((blobs & 2u) && !w->tblob) {      // the second blob: allocated by the first call that needs one of its families
        const size_t off = w->tblob_floats, nz = w->zeros_floats;
        VS_HIP(hipMalloc((void **)&w->tblob, off * sizeof(float)));
        VS_HIP(hipMemsetAsync(w->tblob + w->zeros, 0, nz * sizeof(float), st));
    }
    vsw_order(w, stream);       // parameters written / images built on another stream: wait for them on the device
    if (!stale) return VS_OK;
    // what is (re)built below is ordered behind `stream` when this scope ends
    struct Mark { const vs_weights *w; void *s; ~Mark() { vsw_mark(w, s); } } mark{w, stream};
    int (*done)(const vs_weights *, unsigned, hipStream_t) = nullptr;
    for (int i = 0; i < VSW_NUM_FAMILIES; ++i) {
        const Family &F = kFamilies[i];
        if (!(stale & F.bit)) continue;
        if (F.build != done) {
            if (int rc = F.build(w, stale, st)) return rc;
            done = F.build;
        }
        w->built[i] = w->version;       // a stamp is set only behind launches that were enqueued without error
    }
    return VS_OK;
}

extern "C" {

int vs_weights_pack(const vs_model_desc *desc, const vs_model_params *params, void *stream,
                    vs_weights **out) {
    if (int rc = check_desc(desc)) return rc;
    if (!params || !out) return vs_failf(VS_ERR_INVALID, "params/out is NULL");
    const int d = desc->d_model;
    vs_weights *w = new vs_weights();
    static_cast<VsWeightsLayout &>(*w) =
        vs_weights_layout(*desc, params->pos_embedding != nullptr, vsk_mlp_bf16_supported(d) ? vsk_mlp_bf16_image_bytes(d) : 0,
                          vsk_mlp_bf16_supported(d) ? vsk_qkv_bf16_image_bytes(d) : 0, vsk_embed_bf16_image_bytes(d, desc->in_features));
    w->desc = *desc;
    if (hipGetDevice(&w->device) != hipSuccess) { delete w; return vs_failf(VS_ERR_HIP, "hipGetDevice failed"); }
    const size_t bytes = w->blob_floats * sizeof(float);
    hipError_t e = hipMalloc((void **)&w->blob, bytes);
    if (e != hipSuccess) { delete w; return vs_failf(VS_ERR_HIP, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); }
    if (int rc = fill_weights(w, params, (hipStream_t)stream, false)) {
        (void)hipFree(w->blob);
        delete w;
        return rc;
    }
    w->version = 1;
    vsw_mark(w, stream);
    *out = w;
    return VS_OK;
}

int vs_weights_update(vs_weights *w, const vs_model_params *params, void *stream) {
    if (!w || !params) return vs_failf(VS_ERR_INVALID, "weights/params is NULL");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != w->device)
        return vs_failf(VS_ERR_INVALID, "vs_weights_update on device %d, handle was packed on device %d", dev, w->device);
    ++w->version;        // every image family (and the training side's transposes) is rebuilt on its next use
    vsw_order(w, stream);   // (images still being read / built on another stream)
    const int rc = fill_weights(w, params, (hipStream_t)stream, true);
    vsw_mark(w, stream);
    return rc;
}

int vs_weights_set_norm_width(vs_weights *w, int32_t norm_width) {
    if (!w) return vs_failf(VS_ERR_INVALID, "weights is NULL");
    if (norm_width <= 0 || norm_width % 4 || norm_width > w->desc.d_model)
        return vs_failf(VS_ERR_INVALID, "norm_width=%d unsupported (multiple of 4, 0 < norm_width <= d_model = %d)", norm_width, w->desc.d_model);
    w->norm_width = norm_width;
    return VS_OK;
}

void vs_weights_free(vs_weights *w) {
    if (!w) return;
    if (w->blob) (void)hipFree(w->blob);
    if (w->tblob) (void)hipFree(w->tblob);
    if (w->order_event) (void)hipEventDestroy((hipEvent_t)w->order_event);
    delete w;
}

}  // extern "C"
