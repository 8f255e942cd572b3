// rt_batch_order.hpp -- the candidate order of a batch of frames (DESIGN.md 4.2 "Frame batching"): which local tile an iteration of the batch's primary stage handles, and
// where a wave's candidates go inside the workgroup's stretch of the candidate list.  Plain integer arithmetic, evaluated on the device by k_primary_interleaved and on the
// host by rt_debug_batch_order (tests/test_gpu_batch_interleave.py checks it against an enumeration, without a GPU).
//
// A batch of K frames holds K nearly identical copies of every pixel's work (the frames differ in uFrameIndex and a sub-pixel jitter).  The slots are
// frame-major -- lt' = k * nLocalTiles + lt, rt_frame.hpp -- and stay so; the ORDER of the candidate list, from which every later list and queue inherits which
// rays share a wave, is pixel-major: the K copies of a pixel stand side by side, in adjacent lanes of every launch that follows.
#pragma once
#include "rt_frame.hpp"

namespace rtd {

// Virtual tile v of k_primary_interleaved's grid, v < nLocalTiles * batch, frame-minor: the `batch` frames of spatial tile lt = v / batch follow each other.
// Returns the local tile index lt' of rt_frame.hpp (the slot numbering does not change).
RT_HOST_DEV int batch_tile_of_virtual(int v, int batch, int nLocalTiles) {
    const int lt = v / batch;
    return (v - lt * batch) * nLocalTiles + lt;
}

// A wave notes one ballot per iteration, m[k * stride] for k < n (n <= 32): bit `lane` = the lane has an item in iteration k.  The wave's items are laid out
// lane by lane, and a lane's items by iteration.  First position of `lane`'s items, relative to the wave's first item:
RT_HOST_DEV uint32_t interleaved_lane_start(const unsigned long long *m, int stride, int n, uint32_t lane) {
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t r = 0;
    for (int k = 0; k < n; ++k) r += (uint32_t)__builtin_popcountll(m[k * stride] & below);
    return r;
}
// ... and the position of its item of iteration i, given the lane's own bits (bit k = m[k * stride] >> lane & 1)
RT_HOST_DEV uint32_t interleaved_index(uint32_t laneStart, uint32_t laneBits, int i) { return laneStart + (uint32_t)__builtin_popcount(laneBits & ((1u << i) - 1u)); }
RT_HOST_DEV uint32_t interleaved_lane_bits(const unsigned long long *m, int stride, int n, uint32_t lane) {
    uint32_t b = 0;
    for (int k = 0; k < n; ++k) b |= (uint32_t)((m[k * stride] >> lane) & 1ull) << k;
    return b;
}

}  // namespace rtd
