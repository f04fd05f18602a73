/*
 * vs_features.h — C ABI of the GoogLeNet pool5 frame features on the device: decoded frames in, float [N, 1024] out, the
 * tensor the scorer (vs_scorer.h) takes as its input.  Reference: src/data/preprocess/feature_extraction.py:10-42
 * (get_google_net_features) over src/data/preprocess/models.py:10-37 (GoogleNet = torchvision's googlenet without its
 * dropout and fc, transform_input never applied).
 *
 * The network: conv1 7x7/2, maxpool 3x3/2, conv2 1x1, conv3 3x3, maxpool 3x3/2, inception 3a 3b, maxpool 3x3/2,
 * inception 4a..4e, maxpool 2x2/2, inception 5a 5b, the mean over H x W.  Every max pool has ceil_mode; every conv is
 * conv (no bias) + BatchNorm (eps 0.001) + ReLU; an Inception block is four branches - 1x1; 1x1 then 3x3; 1x1 then 3x3
 * (torchvision's "5x5" branch is 3x3); maxpool 3x3/1 pad 1 then 1x1 - concatenated on channels.  57 convs in all.
 *
 * BatchNorm always uses the RUNNING statistics (the reference never calls .eval(), so it would normalise each batch by
 * its own statistics: a defect that is not reproduced - every published google_pool5 feature set is eval-mode).  It is
 * folded into the conv at pack time: scale = gamma / sqrt(var + 0.001) and bias = beta - mean * scale in double,
 * w * scale rounded to float once.
 *
 * Arithmetic: exact fp32 on the matrix pipe; every output element is one chain of multiply-adds over k = (kh, kw, cin)
 * ascending, so a frame's features do not depend on the batch it is computed in (bit for bit).
 *
 * Every function returns 0 or a VS_ERR_* status (vs_scorer.h) and sets vs_last_error().  The argument checks need no GPU.
 */
#ifndef VS_FEATURES_H
#define VS_FEATURES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VS_CNN_NUM_CONVS 57
#define VS_CNN_FEATURES 1024

/* what `input` holds */
#define VS_CNN_INPUT_F32_NCHW 0 /* float [N, 3, H, W], already normalised: what the reference's model.forward receives */
#define VS_CNN_INPUT_U8_NHWC 1  /* uint8 [N, H, W, 3] RGB, the decoded frames: x / 255, - mean, / std happen in conv1's gather */
#define VS_CNN_INPUT_F32_NHWC 2 /* float [N, H, W, C]: the activations between layers (vs_cnn_conv only) */

/* One conv + BatchNorm, DEVICE pointers: weight float [Cout, Cin, k, k] (torch's layout), the rest float [Cout]. */
typedef struct vs_cnn_conv_params {
    const float *weight, *gamma, *beta, *running_mean, *running_var;
} vs_cnn_conv_params;

/* The 57 convs in this order: conv1, conv2, conv3, then for each of inception3a 3b 4a 4b 4c 4d 4e 5a 5b:
 * branch1, branch2.0, branch2.1, branch3.0, branch3.1, branch4.1. */
typedef struct vs_cnn_params {
    vs_cnn_conv_params conv[VS_CNN_NUM_CONVS];
} vs_cnn_params;

typedef struct vs_cnn_weights vs_cnn_weights; /* the packed model: folded weights [Cout][kh][kw][Cin] and biases, on the device */

/* Folds and packs the model on `stream` (one small launch per conv; the sources may be released once the stream has
 * passed them). */
int vs_cnn_pack(const vs_cnn_params *params, void *stream, vs_cnn_weights **out);
void vs_cnn_free(vs_cnn_weights *weights);

/* Smallest H and W the network accepts (15: below it a pooling layer would have no output, as in torch). */
int32_t vs_cnn_min_side(void);

/* Bytes of device workspace a forward of n frames of h x w needs; 0 on invalid arguments. */
size_t vs_cnn_workspace_bytes(int32_t n, int32_t h, int32_t w);

/* out float [n, 1024] (DEVICE).  input_kind: VS_CNN_INPUT_F32_NCHW or VS_CNN_INPUT_U8_NHWC.  workspace: DEVICE, 256-byte
 * aligned, at least vs_cnn_workspace_bytes(n, h, w).  Asynchronous on `stream`. */
int vs_cnn_forward(const vs_cnn_weights *weights, const void *input, int32_t input_kind, int32_t n, int32_t h, int32_t w,
                   float *out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the layer kernels with explicit geometry (tests, other networks) ---- */

/* Floats of one conv's packed form: weights [Coutp][Kp] (Cout padded to 64 rows, k*k*Cin padded to 32) followed by the
 * bias [Coutp]; 0 on invalid arguments. */
size_t vs_cnn_packed_floats(int32_t cout, int32_t cin, int32_t k);
/* Folds one conv + BatchNorm into `packed` (DEVICE, vs_cnn_packed_floats floats). */
int vs_cnn_pack_conv(const vs_cnn_conv_params *conv, int32_t cout, int32_t cin, int32_t k, float *packed, void *stream);

/* conv k x k, stride, pad + folded BatchNorm + ReLU.  input: n frames of h x w with cin channels in the layout of
 * input_kind (U8_NHWC: cin == 3, normalised in the gather; a padding tap is 0 after normalisation).  out: float, pixel
 * (n, ho, wo) channel j at out[((n * Ho + ho) * Wo + wo) * ldc + c0 + j]; the other channels of a wider destination are
 * not touched.  16-byte loads along cin need F32_NHWC with cin % 4 == 0 and a 16-byte aligned input. */
int vs_cnn_conv(const void *input, int32_t input_kind, int32_t n, int32_t h, int32_t w, int32_t cin, const float *packed,
                int32_t cout, int32_t k, int32_t stride, int32_t pad, float *out, int32_t c0, int32_t ldc, void *stream);

/* max pool on float NHWC, c % 4 == 0; padding and ceil_mode overhang are -inf; bit-equal to torch's max_pool2d.
 * out: float [n, Ho, Wo, c] with torch's output size. */
int vs_cnn_maxpool(const float *input, int32_t n, int32_t h, int32_t w, int32_t c, int32_t k, int32_t stride, int32_t pad,
                   int32_t ceil_mode, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VS_FEATURES_H */
