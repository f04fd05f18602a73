// vs_resize_kernels.h - the launcher of vs_resize.hip as vs_resize.cpp sees it.  Returns 0 or the HIP error code of its launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vs_resize_plan.h"

struct ResizeArgs {
    ResizeGeom g;
    const uint8_t *frames;              // uint8 [n, H, W, 3], any byte alignment
    uint8_t *out;                       // uint8 [n, OH, OW, 3], any byte alignment
    const int32_t *xb, *xk, *yb, *yk;   // DEVICE: bounds [OW][2], coefficients [OW][kx], bounds [OH][2], coefficients [OH][ky]
    int32_t n, swap_rb;
};

int vsk_resize(const ResizeArgs &A, hipStream_t st);
