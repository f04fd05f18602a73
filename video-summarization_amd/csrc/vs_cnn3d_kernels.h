// vs_cnn3d_kernels.h - launchers of vs_cnn3d.hip as vs_cnn3d.cpp sees them.  Each returns 0 or the HIP error code of its launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vs_cnn3d_plan.h"

struct Cnn3dConvArgs {
    Cnn3dConv g;
    const void *in;             // float or uint8, in the layout of g's strides
    const float *w, *bias;      // packed [Coutp][Kp] and [Coutp]
    const float *residual;      // NULL, or channels-last [M][Cout]: added after the bias, before the ReLU
    float *out;                 // channels-last [M][Cout]
    int32_t relu;
    float mean[3], std[3];      // uint8 frames only: ((float)u / 255 - mean) / std per channel, built into the LDS table
};

struct Cnn3dMeanArgs {
    const float *in;            // [N][P][C]
    float *out;                 // [N][C]
    int64_t P;
    int32_t N, C;
};

// torch's weight [Cout][Cin][kt][ks][ks] + BatchNorm3d (eps 1e-5) -> packed [Coutp][Kp] (k order kt, kh, kw, cin; zero rows and
// zero k padding) and bias
int vsk_cnn3d_pack_conv(const float *w, const float *gamma, const float *beta, const float *mean, const float *var, const Cnn3dConv &g,
                        float *packed_w, float *packed_b, hipStream_t st);
int vsk_cnn3d_conv(const Cnn3dConvArgs &A, int input_kind, hipStream_t st);
int vsk_cnn3d_mean(const Cnn3dMeanArgs &A, hipStream_t st);
