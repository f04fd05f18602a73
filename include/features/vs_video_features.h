/*
 * vs_video_features.h — C ABI of the R3D-18 video-level feature on the device: the decoded frames of a video in, float
 * [N, 512] out, the target that pretraining distils against.  Reference: src/data/preprocess/feature_extraction.py:45-76
 * (get_video_feature) over src/data/preprocess/models.py:40-66 (R3D18 = torchvision's r3d_18 without its fc).
 *
 * The network: stem Conv3d(3, 64, k (3,7,7), stride (1,2,2), pad (1,3,3)) + BatchNorm3d + ReLU; layer1..layer4 of two
 * BasicBlocks each, planes 64 / 128 / 256 / 512, the first block's stride 1 / 2 / 2 / 2 in all three dimensions.  A block
 * is conv1 (3x3x3, stride s, pad 1) + BN + ReLU, conv2 (3x3x3, stride 1, pad 1) + BN, out = ReLU(conv2 + identity); the
 * first block of layer2..4 takes its identity through downsample = Conv3d(1x1x1, stride 2) + BN.  Then the mean over
 * T' x H' x W'.  No conv has a bias.  20 convs in all.  Every T, H, W >= 1 is accepted: no layer is ever empty.
 *
 * BatchNorm always uses the RUNNING statistics (eps 1e-5).  The reference never calls .eval(), so it would normalise each
 * channel by this one video's own statistics: a defect that is not reproduced (as for vs_features.h).  It is folded into
 * the conv at pack time: scale = gamma / sqrt(var + 1e-5) and bias = beta - mean * scale in double, w * scale rounded to
 * float once.
 *
 * No pretrained weights are fetched or shipped: the caller passes every tensor.
 *
 * Arithmetic: exact fp32 on the matrix pipe; every output element is one chain of multiply-adds over k = (kt, kh, kw, cin)
 * ascending, so a video's feature does not depend on the batch it is computed in (bit for bit).  Activations between the
 * layers are channels-last, float [N, T, H, W, C].
 *
 * Every int function returns 0 or a VS_ERR_* status (vs_scorer.h) and sets vs_last_error().  The argument checks need no GPU.
 */
#ifndef VS_VIDEO_FEATURES_H
#define VS_VIDEO_FEATURES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VS_R3D_NUM_CONVS 20
#define VS_R3D_FEATURES 512

/* what `input` holds */
#define VS_CNN3D_INPUT_F32_NCDHW 0 /* float [N, 3, T, H, W], already normalised: what the reference's model(video) receives */
#define VS_CNN3D_INPUT_U8_NDHWC 1  /* uint8 [N, T, H, W, 3] RGB, the decoded frame stack: x / 255, - mean, / std happen in the stem's gather */
#define VS_CNN3D_INPUT_F32_NDHWC 2 /* float [N, T, H, W, C]: the activations between layers (vs_cnn3d_conv only) */

/* The reference's Normalize for this network (the Kinetics statistics), written once: vs_r3d_forward and vs_cnn3d_conv hand
 * them to the kernel, which builds its table of ((float)u / 255 - mean) / std from them. */
#define VS_R3D_MEAN_R 0.43216f
#define VS_R3D_MEAN_G 0.394666f
#define VS_R3D_MEAN_B 0.37645f
#define VS_R3D_STD_R 0.22803f
#define VS_R3D_STD_G 0.22145f
#define VS_R3D_STD_B 0.216989f

/* One conv + BatchNorm3d, DEVICE pointers: weight float [Cout, Cin, kt, ks, ks] (torch's layout), the rest float [Cout]. */
typedef struct vs_cnn3d_conv_params {
    const float *weight, *gamma, *beta, *running_mean, *running_var;
} vs_cnn3d_conv_params;

/* The 20 convs in execution order: stem, then for each block of layer1.0 layer1.1 layer2.0 ... layer4.1:
 * conv1, downsample (layer2.0, layer3.0 and layer4.0 only), conv2. */
typedef struct vs_r3d_params {
    vs_cnn3d_conv_params conv[VS_R3D_NUM_CONVS];
} vs_r3d_params;

typedef struct vs_r3d_weights vs_r3d_weights; /* the packed model: folded weights [Cout][kt][kh][kw][Cin] and biases, on the device */

/* Folds and packs the model on `stream` (one small launch per conv; the sources may be released once the stream has
 * passed them). */
int vs_r3d_pack(const vs_r3d_params *params, void *stream, vs_r3d_weights **out);
void vs_r3d_free(vs_r3d_weights *weights);

/* Bytes of device workspace a forward of n videos of t frames of h x w needs; 0 on invalid arguments. */
size_t vs_r3d_workspace_bytes(int32_t n, int32_t t, int32_t h, int32_t w);

/* Multiply-adds times two of the 20 convs of such a forward, from the plan's records (padding taps counted); 0 on invalid
 * arguments. */
double vs_r3d_flops(int32_t n, int32_t t, int32_t h, int32_t w);

/* mean_std: HOST float [6], receives mean R G B then std R G B as the kernel gets them. */
int vs_r3d_normalisation(float *mean_std);

/* out float [n, 512] (DEVICE).  input_kind: VS_CNN3D_INPUT_F32_NCDHW or VS_CNN3D_INPUT_U8_NDHWC.  workspace: DEVICE,
 * 256-byte aligned, at least vs_r3d_workspace_bytes(n, t, h, w).  Asynchronous on `stream`. */
int vs_r3d_forward(const vs_r3d_weights *weights, const void *input, int32_t input_kind, int32_t n, int32_t t, int32_t h,
                   int32_t w, float *out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the layer kernels with explicit geometry (tests, other networks) ---- */

/* Floats of one conv's packed form: weights [Coutp][Kp] (Cout padded to 64 rows, kt*ks*ks*Cin padded to 32) followed by
 * the bias [Coutp]; 0 on invalid arguments. */
size_t vs_cnn3d_packed_floats(int32_t cout, int32_t cin, int32_t kt, int32_t ks);
/* Folds one conv + BatchNorm3d into `packed` (DEVICE, vs_cnn3d_packed_floats floats). */
int vs_cnn3d_pack_conv(const vs_cnn3d_conv_params *conv, int32_t cout, int32_t cin, int32_t kt, int32_t ks, float *packed,
                       void *stream);

/* conv kt x ks x ks with temporal / spatial stride and padding + folded BatchNorm3d, then + residual (nullable; float
 * [n, To, Ho, Wo, cout], the output's shape), then ReLU where relu != 0.  input: n videos of t frames of h x w with cin
 * channels in the layout of input_kind (U8_NDHWC: cin == 3, normalised in the gather; a padding tap is 0 after
 * normalisation, in time as in space).  out: float [n, To, Ho, Wo, cout].  16-byte loads along cin need F32_NDHWC with
 * cin % 4 == 0 and a 16-byte aligned input. */
int vs_cnn3d_conv(const void *input, int32_t input_kind, int32_t n, int32_t t, int32_t h, int32_t w, int32_t cin,
                  const float *packed, int32_t cout, int32_t kt, int32_t ks, int32_t stride_t, int32_t stride_s, int32_t pad_t,
                  int32_t pad_s, const float *residual, int32_t relu, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VS_VIDEO_FEATURES_H */
