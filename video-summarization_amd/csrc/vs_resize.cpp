// vs_resize.cpp — host side of the frame resize (include/features/vs_resize.h): the argument checks (no GPU needed), the plan
// (tables built by vs_resize_plan.h and uploaded once, the tile chosen once) and the run, which is one launch.
// This translation unit computes the coefficient tables: it is built with -ffp-contract=off (_lib.EXTRA_FLAGS).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <new>
#include <vector>

#include "features/vs_resize.h"
#include "vs_error.h"
#include "vs_resize_kernels.h"
#include "vs_resize_plan.h"
#include "vs_scorer.h"

static_assert(VS_RESIZE_PATH_FUSED == RESIZE_PATH_FUSED && VS_RESIZE_PATH_SMALL_TILE == RESIZE_PATH_SMALL_TILE,
              "vs_resize.h and vs_resize_plan.h disagree");

struct vs_resize_plan {
    ResizeGeom g{};
    int32_t *tables = nullptr;      // DEVICE: x bounds, x coefficients, y bounds, y coefficients
    const int32_t *xb = nullptr, *xk = nullptr, *yb = nullptr, *yk = nullptr;
};

extern "C" {

int vs_resize_output_size(int32_t h, int32_t w, int32_t size, int32_t *oh, int32_t *ow) {
    if (!oh || !ow) return vs_failf(VS_ERR_INVALID, "resize_output_size: oh / ow is NULL");
    if (!resize_output_size(h, w, size, oh, ow))
        return vs_failf(VS_ERR_INVALID, "resize_output_size: h=%d w=%d size=%d: every side, the result's too, must be in [1, %d]", h, w, size,
                    (int)RESIZE_MAX_SIDE);
    return VS_OK;
}

int vs_resize_plan_create(int32_t h, int32_t w, int32_t oh, int32_t ow, void *stream, vs_resize_plan **out) {
    if (!out) return vs_failf(VS_ERR_INVALID, "resize_plan_create: out is NULL");
    *out = nullptr;
    if (h < 1 || w < 1 || oh < 1 || ow < 1)
        return vs_failf(VS_ERR_INVALID, "resize_plan_create: h=%d w=%d oh=%d ow=%d: a size is below 1", h, w, oh, ow);
    const ResizePlanHost P = resize_make_plan(h, w, oh, ow);
    if (!P.ok) return vs_failf(VS_ERR_INVALID, "resize_plan_create: h=%d w=%d oh=%d ow=%d: %s", h, w, oh, ow, P.why);
    std::vector<int32_t> host;
    host.reserve(P.x.bounds.size() + P.x.coef.size() + P.y.bounds.size() + P.y.coef.size());
    const size_t at_xb = 0, at_xk = P.x.bounds.size(), at_yb = at_xk + P.x.coef.size(), at_yk = at_yb + P.y.bounds.size();
    host.insert(host.end(), P.x.bounds.begin(), P.x.bounds.end());
    host.insert(host.end(), P.x.coef.begin(), P.x.coef.end());
    host.insert(host.end(), P.y.bounds.begin(), P.y.bounds.end());
    host.insert(host.end(), P.y.coef.begin(), P.y.coef.end());
    vs_resize_plan *R = new (std::nothrow) vs_resize_plan;
    if (!R) return vs_failf(VS_ERR_INVALID, "resize_plan_create: out of host memory");
    R->g = P.g;
    hipError_t e = hipMalloc((void **)&R->tables, host.size() * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(R->tables, host.data(), host.size() * 4, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);     // `host` goes away with this call
    if (e != hipSuccess) {
        vs_resize_plan_free(R);
        return vs_failf(VS_ERR_HIP, "resize_plan_create: uploading %zu table bytes: %s", host.size() * 4, hipGetErrorString(e));
    }
    R->xb = R->tables + at_xb; R->xk = R->tables + at_xk; R->yb = R->tables + at_yb; R->yk = R->tables + at_yk;
    *out = R;
    return VS_OK;
}

void vs_resize_plan_free(vs_resize_plan *plan) {
    if (!plan) return;
    if (plan->tables) (void)hipFree(plan->tables);
    delete plan;
}

int vs_resize_plan_describe(const vs_resize_plan *plan, int32_t *path, int32_t *tile_oh, int32_t *tile_ow) {
    if (!plan || !path || !tile_oh || !tile_ow) return vs_failf(VS_ERR_INVALID, "resize_plan_describe: plan / path / tile_oh / tile_ow is NULL");
    *path = plan->g.path; *tile_oh = plan->g.tile_oh; *tile_ow = plan->g.tile_ow;
    return VS_OK;
}

size_t vs_resize_workspace_bytes(const vs_resize_plan *plan, int32_t n) {
    if (!plan || n < 1) {
        vs_failf(VS_ERR_INVALID, "resize_workspace_bytes: plan is NULL or n=%d is below 1", n);
        return 0;
    }
    return 0;       // both paths keep the rounded intermediate in LDS
}

int vs_resize_run(const vs_resize_plan *plan, const uint8_t *frames, int32_t n, uint32_t flags, uint8_t *out, void *workspace,
                  size_t workspace_bytes, void *stream) {
    if (!plan || !frames || !out) return vs_failf(VS_ERR_INVALID, "resize_run: plan / frames / out is NULL");
    if (n < 1) return vs_failf(VS_ERR_INVALID, "resize_run: n=%d is below 1", n);
    if (flags & ~VS_RESIZE_SWAP_RB) return vs_failf(VS_ERR_INVALID, "resize_run: unknown flags 0x%x", flags);
    const size_t need = 0;          // = vs_resize_workspace_bytes(plan, n)
    if (workspace_bytes < need || (need > 0 && !workspace))
        return vs_failf(VS_ERR_INVALID, "resize_run: workspace %zu bytes < %zu needed", workspace_bytes, need);
    const ResizeGeom &g = plan->g;
    if ((int64_t)n * g.tiles_y * g.tiles_x >= (int64_t)1 << 31)
        return vs_failf(VS_ERR_INVALID, "resize_run: n=%d frames of %d x %d tiles are more than 2^31 blocks", n, g.tiles_y, g.tiles_x);
    ResizeArgs A{};
    A.g = g; A.frames = frames; A.out = out; A.xb = plan->xb; A.xk = plan->xk; A.yb = plan->yb; A.yk = plan->yk;
    A.n = n; A.swap_rb = (flags & VS_RESIZE_SWAP_RB) ? 1 : 0;
    if (const int e = vsk_resize(A, (hipStream_t)stream)) return vs_failf(VS_ERR_HIP, "resize_run: launch: %s", hipGetErrorString((hipError_t)e));
    return VS_OK;
}

}  // extern "C"
