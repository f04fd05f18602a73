// vs_cnn_kernels.h - launchers of vs_cnn.hip as vs_cnn.cpp sees them.  Each returns 0 or the HIP error code of its launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vs_cnn_plan.h"

struct CnnConvArgs {
    CnnConv g;
    const void *in;             // float or uint8, in the layout of g's strides
    const float *w, *bias;      // packed [Coutp][Kp] and [Coutp]
    float *out;
    int32_t c0, ldc;
};

struct CnnPoolArgs {
    const float *in;
    float *out;
    int32_t N, H, W, C, k, s, p, Ho, Wo;
};

// torch's weight [Cout][Cin][k][k] + BatchNorm -> packed [Coutp][Kp] (k order kh, kw, cin; zero rows and zero k padding) and bias
int vsk_cnn_pack_conv(const float *w, const float *gamma, const float *beta, const float *mean, const float *var, const CnnConv &g,
                      float *packed_w, float *packed_b, hipStream_t st);
int vsk_cnn_conv(const CnnConvArgs &A, int input_kind, hipStream_t st);
int vsk_cnn_maxpool(const CnnPoolArgs &A, hipStream_t st);
int vsk_cnn_avgpool(const CnnPoolArgs &A, hipStream_t st);
