// Device-side helper shared by the training attention kernels (vs_train_attention.hip: exact fp32; vs_train_attention_bf16.hip:
// the 16-bit matrix pipe): where a block works - on a padded batch or on a packed ragged one.
#pragma once
#include "vs_train_kernels.h"

namespace {

// Where a block works.  Padded batches: (video * H + head, owner tile) from blockIdx, T the common length.  Packed ragged
// batches: (head, video, owner tile) from the work list, T = that video's length.  plane: first row of the (video, head) in
// the head-major planes (and in lse2 / delta; + query = the dropout row key); tok: first row of the video in the
// token-major tensors; wbase: first word of the (video, head) in one bit-packed copy of the keep decisions, wall: words of
// one copy (the key-major copy follows the query-major one).
struct Owner { int T, b, hd, tile; size_t plane, tok, wbase, wall; };
template <bool PACKED>
__device__ __forceinline__ Owner owner_tile(int H, int T, const VstPackedPlan &pk) {
    Owner o;
    if constexpr (PACKED) {
        const int wi = blockIdx.x / H, hd = blockIdx.x - wi * H;      // the heads of a tile side by side: the list's order is the grid's
        const int b = pk.work[2 * wi];
        o.hd = hd; o.b = b; o.tile = pk.work[2 * wi + 1];
        if (b < 0) { o.T = 0; o.plane = o.tok = o.wbase = o.wall = 0; return o; }      // (device lengths gave fewer tiles than the host's)
        const int r0 = pk.cu[b];
        o.T = pk.cu[b + 1] - r0;
        o.plane = (size_t)hd * pk.Mtot + r0;
        o.tok = (size_t)r0;
        o.wbase = (size_t)hd * pk.words + pk.bo[b];
        o.wall = (size_t)H * pk.words;
    } else {
        const int nt = (T + 127) / 128, W = (T + 31) / 32;
        const int bh = blockIdx.x / nt;
        o.T = T; o.tile = blockIdx.x - bh * nt; o.b = bh / H; o.hd = bh - o.b * H;
        o.plane = (size_t)bh * T;
        o.tok = (size_t)o.b * T;
        o.wbase = (size_t)bh * T * W;
        o.wall = (size_t)gridDim.x / nt * T * W;
    }
    return o;
}

}  // namespace
