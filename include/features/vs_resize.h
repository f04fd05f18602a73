/*
 * vs_resize.h — C ABI of the frame resize on the device: decoded uint8 [N, H, W, 3] frames in, uint8 [N, oh, ow, 3] out, the
 * frames vs_cnn_forward (vs_features.h) takes as VS_CNN_INPUT_U8_NHWC.  Reference: transforms.Resize(size) in
 * src/data/preprocess/feature_extraction.py:108-113, which for the PIL images it is given is
 * PIL.Image.resize((ow, oh), Image.BILINEAR) frame by frame.  The result here is the same bytes.
 *
 * The algorithm (PIL's antialiased bilinear for 8-bit images): per axis, scale = (double)(float)in / out, the triangle filter
 * widened by max(scale, 1), each output's window clamped to the image and its weights normalised in double, then rounded to
 * 22-bit fixed point.  A sample is (2^21 + sum pixel * k) >> 22 in int32, clamped to [0, 255].  The horizontal pass runs
 * first and its output is ROUNDED TO UINT8 before the vertical pass reads it; a pass whose sizes are equal is skipped.  The
 * coefficient tables are built on the host at plan creation (the only floating point in the path) and uploaded once.
 *
 * A frame's bytes do not depend on the batch it is resized in.  Frames and outputs may start at any byte address.
 *
 * Every function returns 0 or a VS_ERR_* status (vs_scorer.h) and sets vs_last_error().  The argument checks need no GPU.
 */
#ifndef VS_RESIZE_H
#define VS_RESIZE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VS_RESIZE_SWAP_RB 1u /* read B, G, R and write R, G, B (decoded OpenCV frames); with equal sizes: a swapping copy */

/* which form of the kernel a plan chose, once, at creation */
#define VS_RESIZE_PATH_FUSED 0      /* the default tile of 32 output rows x 64 output columns */
#define VS_RESIZE_PATH_SMALL_TILE 1 /* a smaller tile: the default one's input rows or columns would not fit the LDS staging */

typedef struct vs_resize_plan vs_resize_plan; /* one geometry: its coefficient tables on the device and its tile */

/* torchvision's rule for an int size: the shorter side becomes `size`, the longer int(size * long / short); w <= h counts
 * as "w is shorter".  Sides are 1 .. 65536. */
int vs_resize_output_size(int32_t h, int32_t w, int32_t size, int32_t *oh, int32_t *ow);

/* Builds the tables for h x w -> oh x ow on the host and uploads them on `stream` (the one host-to-device copy of the
 * path; it has completed when the call returns).  VS_ERR_INVALID for a reduction so large (several thousand to one) that
 * one output pixel's window does not fit the staging. */
int vs_resize_plan_create(int32_t h, int32_t w, int32_t oh, int32_t ow, void *stream, vs_resize_plan **out);
void vs_resize_plan_free(vs_resize_plan *plan);

/* The plan's path (VS_RESIZE_PATH_*) and its tile of output rows x output columns. */
int vs_resize_plan_describe(const vs_resize_plan *plan, int32_t *path, int32_t *tile_oh, int32_t *tile_ow);

/* Bytes of device workspace a run of n frames needs.  Both paths keep the intermediate in LDS: 0 today. */
size_t vs_resize_workspace_bytes(const vs_resize_plan *plan, int32_t n);

/* frames uint8 [n, h, w, 3] -> out uint8 [n, oh, ow, 3], both DEVICE, any alignment, not overlapping.  flags: 0 or
 * VS_RESIZE_SWAP_RB.  workspace: DEVICE, at least vs_resize_workspace_bytes(plan, n) (NULL where that is 0).  One launch,
 * asynchronous on `stream`: no host-to-device copy and no synchronisation. */
int vs_resize_run(const vs_resize_plan *plan, const uint8_t *frames, int32_t n, uint32_t flags, uint8_t *out, void *workspace,
                  size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VS_RESIZE_H */
