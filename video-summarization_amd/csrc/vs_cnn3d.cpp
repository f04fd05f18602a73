// vs_cnn3d.cpp — host side of the R3D-18 video-level feature (include/features/vs_video_features.h): the argument checks (no GPU
// needed), the packed model, and the forward, which only walks the plan of vs_cnn3d_plan.h - one launch per record, then the mean.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <new>

#include "features/vs_video_features.h"
#include "vs_cnn3d_kernels.h"
#include "vs_cnn3d_plan.h"
#include "vs_error.h"
#include "vs_scorer.h"

static_assert(VS_R3D_NUM_CONVS == CNN3D_NUM_CONVS && VS_R3D_FEATURES == CNN3D_FEATURES, "vs_video_features.h and vs_cnn3d_plan.h disagree");
static_assert(VS_CNN3D_INPUT_F32_NCDHW == CNN3D_IN_F32_NCDHW && VS_CNN3D_INPUT_U8_NDHWC == CNN3D_IN_U8_NDHWC &&
                  VS_CNN3D_INPUT_F32_NDHWC == CNN3D_IN_F32_NDHWC,
              "vs_video_features.h and vs_cnn3d_plan.h disagree");

struct vs_r3d_weights {
    float *blob = nullptr;      // every conv's packed weights and bias, at the plan's w_off / b_off
    int64_t floats = 0;
};

namespace {

int check_conv_shape(const char *who, int32_t cout, int32_t cin, int32_t kt, int32_t ks) {
    if (cout < 1 || cin < 1 || kt < 1 || ks < 1 || cout > 65536 || cin > 65536 || kt > 15 || ks > 15)
        return vs_failf(VS_ERR_INVALID, "%s: cout=%d cin=%d kt=%d ks=%d outside [1, 65536]^2 x [1, 15]^2", who, cout, cin, kt, ks);
    return VS_OK;
}

void set_normalisation(Cnn3dConvArgs &A) {
    A.mean[0] = VS_R3D_MEAN_R; A.mean[1] = VS_R3D_MEAN_G; A.mean[2] = VS_R3D_MEAN_B;
    A.std[0] = VS_R3D_STD_R; A.std[1] = VS_R3D_STD_G; A.std[2] = VS_R3D_STD_B;
}

}  // namespace

extern "C" {

size_t vs_r3d_workspace_bytes(int32_t n, int32_t t, int32_t h, int32_t w) {
    const Cnn3dPlan P = cnn3d_make_plan(n, t, h, w, CNN3D_IN_F32_NCDHW);
    if (!P.ok) {
        vs_failf(VS_ERR_INVALID, "r3d: n=%d t=%d h=%d w=%d: %s", n, t, h, w, P.why);
        return 0;
    }
    return (size_t)P.workspace_bytes;
}

double vs_r3d_flops(int32_t n, int32_t t, int32_t h, int32_t w) {
    const Cnn3dPlan P = cnn3d_make_plan(n, t, h, w, CNN3D_IN_F32_NCDHW);
    if (!P.ok) {
        vs_failf(VS_ERR_INVALID, "r3d: n=%d t=%d h=%d w=%d: %s", n, t, h, w, P.why);
        return 0.0;
    }
    return (double)P.flops;
}

int vs_r3d_normalisation(float *mean_std) {
    if (!mean_std) return vs_failf(VS_ERR_INVALID, "r3d_normalisation: mean_std is NULL");
    Cnn3dConvArgs A{};
    set_normalisation(A);
    for (int c = 0; c < 3; ++c) { mean_std[c] = A.mean[c]; mean_std[3 + c] = A.std[c]; }
    return VS_OK;
}

int vs_r3d_pack(const vs_r3d_params *params, void *stream, vs_r3d_weights **out) {
    if (!params || !out) return vs_failf(VS_ERR_INVALID, "r3d_pack: params / out is NULL");
    *out = nullptr;
    for (int i = 0; i < CNN3D_NUM_CONVS; ++i) {
        const vs_cnn3d_conv_params &c = params->conv[i];
        if (!c.weight || !c.gamma || !c.beta || !c.running_mean || !c.running_var)
            return vs_failf(VS_ERR_INVALID, "r3d_pack: conv %d has a NULL tensor", i);
    }
    const Cnn3dPlan P = cnn3d_make_plan(1, 1, 1, 1, CNN3D_IN_F32_NCDHW);       // the blob's layout depends on no shape
    vs_r3d_weights *W = new (std::nothrow) vs_r3d_weights;
    if (!W) return vs_failf(VS_ERR_INVALID, "r3d_pack: out of host memory");
    W->floats = P.blob_floats;
    if (const hipError_t e = hipMalloc((void **)&W->blob, (size_t)P.blob_floats * 4)) {
        delete W;
        return vs_failf(VS_ERR_HIP, "r3d_pack: hipMalloc of %lld bytes: %s", (long long)P.blob_floats * 4, hipGetErrorString(e));
    }
    for (int i = 0; i < CNN3D_NUM_CONVS; ++i) {
        const vs_cnn3d_conv_params &c = params->conv[i];
        const Cnn3dConvRec &R = P.conv[i];
        if (const int e = vsk_cnn3d_pack_conv(c.weight, c.gamma, c.beta, c.running_mean, c.running_var, R.g, W->blob + R.w_off, W->blob + R.b_off,
                                              (hipStream_t)stream)) {
            vs_r3d_free(W);
            return vs_failf(VS_ERR_HIP, "r3d_pack: conv %d: %s", i, hipGetErrorString((hipError_t)e));
        }
    }
    *out = W;
    return VS_OK;
}

void vs_r3d_free(vs_r3d_weights *W) {
    if (!W) return;
    if (W->blob) (void)hipFree(W->blob);
    delete W;
}

int vs_r3d_forward(const vs_r3d_weights *W, const void *input, int32_t input_kind, int32_t n, int32_t t, int32_t h, int32_t w, float *out,
                   void *workspace, size_t workspace_bytes, void *stream) {
    if (!W || !input || !out || !workspace) return vs_failf(VS_ERR_INVALID, "r3d_forward: weights / input / out / workspace is NULL");
    if (input_kind != VS_CNN3D_INPUT_F32_NCDHW && input_kind != VS_CNN3D_INPUT_U8_NDHWC)
        return vs_failf(VS_ERR_INVALID, "r3d_forward: input_kind=%d is neither F32_NCDHW nor U8_NDHWC", input_kind);
    const Cnn3dPlan P = cnn3d_make_plan(n, t, h, w, input_kind);
    if (!P.ok) return vs_failf(VS_ERR_INVALID, "r3d_forward: n=%d t=%d h=%d w=%d: %s", n, t, h, w, P.why);
    if (workspace_bytes < (size_t)P.workspace_bytes)
        return vs_failf(VS_ERR_INVALID, "r3d_forward: workspace %zu bytes < %lld needed", workspace_bytes, (long long)P.workspace_bytes);
    if (((uintptr_t)workspace & 255) != 0) return vs_failf(VS_ERR_INVALID, "r3d_forward: workspace is not 256-byte aligned");
    if (P.blob_floats != W->floats) return vs_failf(VS_ERR_INVALID, "r3d_forward: the packed model does not match this library");
    hipStream_t st = (hipStream_t)stream;
    float *ws = (float *)workspace;
    auto buf = [&](int b) { return ws + P.buf_off[b]; };
    for (int i = 0; i < CNN3D_NUM_CONVS; ++i) {
        const Cnn3dConvRec &R = P.conv[i];
        Cnn3dConvArgs A{};
        A.g = R.g;
        A.in = R.in_buf == CNN3D_BUF_INPUT ? input : (const void *)buf(R.in_buf);
        A.w = W->blob + R.w_off; A.bias = W->blob + R.b_off;
        A.residual = R.res_buf == CNN3D_BUF_NONE ? nullptr : buf(R.res_buf);
        A.out = buf(R.out_buf); A.relu = R.relu;
        set_normalisation(A);
        VS_LAUNCH_HIP(vsk_cnn3d_conv(A, R.in_buf == CNN3D_BUF_INPUT ? input_kind : CNN3D_IN_F32_NDHWC, st));
    }
    const Cnn3dMeanArgs Mn{buf(P.pool_buf), out, P.pool_positions, n, CNN3D_FEATURES};
    VS_LAUNCH_HIP(vsk_cnn3d_mean(Mn, st));
    return VS_OK;
}

size_t vs_cnn3d_packed_floats(int32_t cout, int32_t cin, int32_t kt, int32_t ks) {
    if (check_conv_shape("cnn3d_packed_floats", cout, cin, kt, ks)) return 0;
    const Cnn3dConv g = cnn3d_conv_geometry(1, kt, ks, ks, cin, cout, kt, ks, 1, 1, 0, 0, CNN3D_IN_F32_NDHWC);
    return (size_t)(cnn3d_packed_weight_floats(g) + g.Coutp);
}

int vs_cnn3d_pack_conv(const vs_cnn3d_conv_params *c, int32_t cout, int32_t cin, int32_t kt, int32_t ks, float *packed, void *stream) {
    if (!c || !packed || !c->weight || !c->gamma || !c->beta || !c->running_mean || !c->running_var)
        return vs_failf(VS_ERR_INVALID, "cnn3d_pack_conv: conv / packed / a tensor is NULL");
    if (int rc = check_conv_shape("cnn3d_pack_conv", cout, cin, kt, ks)) return rc;
    const Cnn3dConv g = cnn3d_conv_geometry(1, kt, ks, ks, cin, cout, kt, ks, 1, 1, 0, 0, CNN3D_IN_F32_NDHWC);
    VS_LAUNCH_HIP(vsk_cnn3d_pack_conv(c->weight, c->gamma, c->beta, c->running_mean, c->running_var, g, packed, packed + cnn3d_packed_weight_floats(g),
                                   (hipStream_t)stream));
    return VS_OK;
}

int vs_cnn3d_conv(const void *input, int32_t input_kind, int32_t n, int32_t t, int32_t h, int32_t w, int32_t cin, const float *packed, int32_t cout,
                  int32_t kt, int32_t ks, int32_t stride_t, int32_t stride_s, int32_t pad_t, int32_t pad_s, const float *residual, int32_t relu,
                  float *out, void *stream) {
    if (!input || !packed || !out) return vs_failf(VS_ERR_INVALID, "cnn3d_conv: input / packed / out is NULL");
    if (input_kind < VS_CNN3D_INPUT_F32_NCDHW || input_kind > VS_CNN3D_INPUT_F32_NDHWC)
        return vs_failf(VS_ERR_INVALID, "cnn3d_conv: input_kind=%d unknown", input_kind);
    if (int rc = check_conv_shape("cnn3d_conv", cout, cin, kt, ks)) return rc;
    if (input_kind == VS_CNN3D_INPUT_U8_NDHWC && cin != 3) return vs_failf(VS_ERR_INVALID, "cnn3d_conv: uint8 frames have 3 channels, not %d", cin);
    if (n < 1 || t < 1 || h < 1 || w < 1 || stride_t < 1 || stride_s < 1 || pad_t < 0 || pad_s < 0 || pad_t >= kt || pad_s >= ks)
        return vs_failf(VS_ERR_INVALID, "cnn3d_conv: n=%d t=%d h=%d w=%d stride=(%d, %d) pad=(%d, %d) (pad < k=(%d, %d))", n, t, h, w, stride_t,
                        stride_s, pad_t, pad_s, kt, ks);
    if ((int64_t)n * t * h * w > (int64_t)1 << 30) return vs_failf(VS_ERR_INVALID, "cnn3d_conv: more than 2^30 input positions");
    const Cnn3dConv g = cnn3d_conv_geometry(n, t, h, w, cin, cout, kt, ks, stride_t, stride_s, pad_t, pad_s, input_kind);
    if (g.To < 1 || g.Ho < 1 || g.Wo < 1 || g.M > (int64_t)1 << 30) return vs_failf(VS_ERR_INVALID, "cnn3d_conv: no output position, or more than 2^30 of them");
    Cnn3dConvArgs A{};
    A.g = g; A.in = input; A.w = packed; A.bias = packed + cnn3d_packed_weight_floats(g); A.residual = residual; A.out = out; A.relu = relu != 0;
    set_normalisation(A);
    VS_LAUNCH_HIP(vsk_cnn3d_conv(A, input_kind, (hipStream_t)stream));
    return VS_OK;
}

}  // extern "C"
