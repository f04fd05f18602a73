// vs_cnn.cpp — host side of the GoogLeNet pool5 front end (include/features/vs_features.h): the argument checks (no GPU needed),
// the packed model, and the forward, which only walks the plan of vs_cnn_plan.h - one launch per record.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <new>

#include "features/vs_features.h"
#include "vs_cnn_kernels.h"
#include "vs_cnn_plan.h"
#include "vs_error.h"
#include "vs_scorer.h"

static_assert(VS_CNN_NUM_CONVS == CNN_NUM_CONVS && VS_CNN_FEATURES == CNN_FEATURES, "vs_features.h and vs_cnn_plan.h disagree");
static_assert(VS_CNN_INPUT_F32_NCHW == CNN_IN_F32_NCHW && VS_CNN_INPUT_U8_NHWC == CNN_IN_U8_NHWC && VS_CNN_INPUT_F32_NHWC == CNN_IN_F32_NHWC,
              "vs_features.h and vs_cnn_plan.h disagree");

struct vs_cnn_weights {
    float *blob = nullptr;      // every conv's packed weights and bias, at the plan's w_off / b_off
    int64_t floats = 0;
};

namespace {

int check_conv_shape(const char *who, int32_t cout, int32_t cin, int32_t k) {
    if (cout < 1 || cin < 1 || k < 1 || cout > 65536 || cin > 65536 || k > 15)
        return vs_failf(VS_ERR_INVALID, "%s: cout=%d cin=%d k=%d outside [1, 65536] x [1, 65536] x [1, 15]", who, cout, cin, k);
    return VS_OK;
}

}  // namespace

extern "C" {

int32_t vs_cnn_min_side(void) { return cnn_min_side(); }

size_t vs_cnn_workspace_bytes(int32_t n, int32_t h, int32_t w) {
    const CnnPlan P = cnn_make_plan(n, h, w, CNN_IN_F32_NCHW);
    if (!P.ok) {
        vs_failf(VS_ERR_INVALID, "cnn: n=%d h=%d w=%d: %s (smallest h, w: %d)", n, h, w, P.why, cnn_min_side());
        return 0;
    }
    return (size_t)P.workspace_bytes;
}

int vs_cnn_pack(const vs_cnn_params *params, void *stream, vs_cnn_weights **out) {
    if (!params || !out) return vs_failf(VS_ERR_INVALID, "cnn_pack: params / out is NULL");
    *out = nullptr;
    for (int i = 0; i < CNN_NUM_CONVS; ++i) {
        const vs_cnn_conv_params &c = params->conv[i];
        if (!c.weight || !c.gamma || !c.beta || !c.running_mean || !c.running_var)
            return vs_failf(VS_ERR_INVALID, "cnn_pack: conv %d has a NULL tensor", i);
    }
    const CnnPlan P = cnn_make_plan(1, cnn_min_side(), cnn_min_side(), CNN_IN_F32_NCHW);     // the blob's layout depends on no shape
    vs_cnn_weights *W = new (std::nothrow) vs_cnn_weights;
    if (!W) return vs_failf(VS_ERR_INVALID, "cnn_pack: out of host memory");
    W->floats = P.blob_floats;
    if (const hipError_t e = hipMalloc((void **)&W->blob, (size_t)P.blob_floats * 4)) {
        delete W;
        return vs_failf(VS_ERR_HIP, "cnn_pack: hipMalloc of %lld bytes: %s", (long long)P.blob_floats * 4, hipGetErrorString(e));
    }
    for (int i = 0; i < CNN_NUM_CONVS; ++i) {
        const vs_cnn_conv_params &c = params->conv[i];
        const CnnConvRec &R = P.conv[i];
        if (const int e = vsk_cnn_pack_conv(c.weight, c.gamma, c.beta, c.running_mean, c.running_var, R.g, W->blob + R.w_off, W->blob + R.b_off,
                                            (hipStream_t)stream)) {
            vs_cnn_free(W);
            return vs_failf(VS_ERR_HIP, "cnn_pack: conv %d: %s", i, hipGetErrorString((hipError_t)e));
        }
    }
    *out = W;
    return VS_OK;
}

void vs_cnn_free(vs_cnn_weights *W) {
    if (!W) return;
    if (W->blob) (void)hipFree(W->blob);
    delete W;
}

int vs_cnn_forward(const vs_cnn_weights *W, const void *input, int32_t input_kind, int32_t n, int32_t h, int32_t w, float *out,
                   void *workspace, size_t workspace_bytes, void *stream) {
    if (!W || !input || !out || !workspace) return vs_failf(VS_ERR_INVALID, "cnn_forward: weights / input / out / workspace is NULL");
    if (input_kind != VS_CNN_INPUT_F32_NCHW && input_kind != VS_CNN_INPUT_U8_NHWC)
        return vs_failf(VS_ERR_INVALID, "cnn_forward: input_kind=%d is neither F32_NCHW nor U8_NHWC", input_kind);
    const CnnPlan P = cnn_make_plan(n, h, w, input_kind);
    if (!P.ok) return vs_failf(VS_ERR_INVALID, "cnn_forward: n=%d h=%d w=%d: %s (smallest h, w: %d)", n, h, w, P.why, cnn_min_side());
    if (workspace_bytes < (size_t)P.workspace_bytes)
        return vs_failf(VS_ERR_INVALID, "cnn_forward: workspace %zu bytes < %lld needed", workspace_bytes, (long long)P.workspace_bytes);
    if (((uintptr_t)workspace & 255) != 0) return vs_failf(VS_ERR_INVALID, "cnn_forward: workspace is not 256-byte aligned");
    if (P.blob_floats != W->floats) return vs_failf(VS_ERR_INVALID, "cnn_forward: the packed model does not match this library");
    hipStream_t st = (hipStream_t)stream;
    float *ws = (float *)workspace;
    auto buf = [&](int b) { return ws + P.buf_off[b]; };
    for (int s = 0; s < CNN_NUM_STEPS; ++s) {
        if (!P.step[s].pool) {
            const CnnConvRec &R = P.conv[P.step[s].index];
            CnnConvArgs A{};
            A.g = R.g;
            A.in = R.in_buf == CNN_BUF_INPUT ? input : (const void *)buf(R.in_buf);
            A.w = W->blob + R.w_off; A.bias = W->blob + R.b_off;
            A.out = buf(R.out_buf); A.c0 = R.c0; A.ldc = R.ldc;
            VS_LAUNCH_HIP(vsk_cnn_conv(A, R.in_buf == CNN_BUF_INPUT ? input_kind : CNN_IN_F32_NHWC, st));
        } else {
            const CnnPoolRec &R = P.pool[P.step[s].index];
            const CnnPoolArgs A{buf(R.in_buf), R.out_buf == CNN_BUF_OUTPUT ? out : buf(R.out_buf), R.N, R.H, R.W, R.C, R.k, R.s, R.p, R.Ho, R.Wo};
            if (R.avg) VS_LAUNCH_HIP(vsk_cnn_avgpool(A, st));
            else VS_LAUNCH_HIP(vsk_cnn_maxpool(A, st));
        }
    }
    return VS_OK;
}

size_t vs_cnn_packed_floats(int32_t cout, int32_t cin, int32_t k) {
    if (check_conv_shape("cnn_packed_floats", cout, cin, k)) return 0;
    const CnnConv g = cnn_conv_geometry(1, k, k, cin, cout, k, 1, 0, CNN_IN_F32_NHWC);
    return (size_t)(cnn_packed_weight_floats(g) + g.Coutp);
}

int vs_cnn_pack_conv(const vs_cnn_conv_params *c, int32_t cout, int32_t cin, int32_t k, float *packed, void *stream) {
    if (!c || !packed || !c->weight || !c->gamma || !c->beta || !c->running_mean || !c->running_var)
        return vs_failf(VS_ERR_INVALID, "cnn_pack_conv: conv / packed / a tensor is NULL");
    if (int rc = check_conv_shape("cnn_pack_conv", cout, cin, k)) return rc;
    const CnnConv g = cnn_conv_geometry(1, k, k, cin, cout, k, 1, 0, CNN_IN_F32_NHWC);
    VS_LAUNCH_HIP(vsk_cnn_pack_conv(c->weight, c->gamma, c->beta, c->running_mean, c->running_var, g, packed, packed + cnn_packed_weight_floats(g),
                                 (hipStream_t)stream));
    return VS_OK;
}

int vs_cnn_conv(const void *input, int32_t input_kind, int32_t n, int32_t h, int32_t w, int32_t cin, const float *packed, int32_t cout,
                int32_t k, int32_t stride, int32_t pad, float *out, int32_t c0, int32_t ldc, void *stream) {
    if (!input || !packed || !out) return vs_failf(VS_ERR_INVALID, "cnn_conv: input / packed / out is NULL");
    if (input_kind < VS_CNN_INPUT_F32_NCHW || input_kind > VS_CNN_INPUT_F32_NHWC) return vs_failf(VS_ERR_INVALID, "cnn_conv: input_kind=%d unknown", input_kind);
    if (int rc = check_conv_shape("cnn_conv", cout, cin, k)) return rc;
    if (input_kind == VS_CNN_INPUT_U8_NHWC && cin != 3) return vs_failf(VS_ERR_INVALID, "cnn_conv: uint8 frames have 3 channels, not %d", cin);
    if (n < 1 || h < 1 || w < 1 || stride < 1 || pad < 0 || pad >= k)
        return vs_failf(VS_ERR_INVALID, "cnn_conv: n=%d h=%d w=%d stride=%d pad=%d (pad < k=%d)", n, h, w, stride, pad, k);
    if (c0 < 0 || ldc < 1 || (int64_t)c0 + cout > ldc) return vs_failf(VS_ERR_INVALID, "cnn_conv: channels [%d, %d + %d) outside a row of %d", c0, c0, cout, ldc);
    const CnnConv g = cnn_conv_geometry(n, h, w, cin, cout, k, stride, pad, input_kind);
    if (g.Ho < 1 || g.Wo < 1 || g.M > (int64_t)1 << 30) return vs_failf(VS_ERR_INVALID, "cnn_conv: no output pixel, or more than 2^30 of them");
    CnnConvArgs A{};
    A.g = g; A.in = input; A.w = packed; A.bias = packed + cnn_packed_weight_floats(g); A.out = out; A.c0 = c0; A.ldc = ldc;
    VS_LAUNCH_HIP(vsk_cnn_conv(A, input_kind, (hipStream_t)stream));
    return VS_OK;
}

int vs_cnn_maxpool(const float *input, int32_t n, int32_t h, int32_t w, int32_t c, int32_t k, int32_t stride, int32_t pad, int32_t ceil_mode,
                   float *out, void *stream) {
    if (!input || !out) return vs_failf(VS_ERR_INVALID, "cnn_maxpool: input / out is NULL");
    if (n < 1 || h < 1 || w < 1 || c < 4 || c % 4 != 0 || k < 1 || stride < 1 || pad < 0 || 2 * pad > k)
        return vs_failf(VS_ERR_INVALID, "cnn_maxpool: n=%d h=%d w=%d c=%d (a multiple of 4) k=%d stride=%d pad=%d (at most k / 2)", n, h, w, c, k, stride, pad);
    if ((((uintptr_t)input | (uintptr_t)out) & 15) != 0) return vs_failf(VS_ERR_INVALID, "cnn_maxpool: input / out is not 16-byte aligned");
    const int32_t ho = cnn_pool_out(h, k, stride, pad, ceil_mode), wo = cnn_pool_out(w, k, stride, pad, ceil_mode);
    if (ho < 1 || wo < 1 || (int64_t)n * ho * wo * c > (int64_t)1 << 40) return vs_failf(VS_ERR_INVALID, "cnn_maxpool: no output pixel, or too many");
    const CnnPoolArgs A{input, out, n, h, w, c, k, stride, pad, ho, wo};
    VS_LAUNCH_HIP(vsk_cnn_maxpool(A, (hipStream_t)stream));
    return VS_OK;
}

}  // extern "C"
