// rt_mesh_morph.hip -- morph-target blending of the dynamic mesh: dst := base + the weighted deltas of the entries that name each
// vertex, written where the skin (the rest array) or rebuild, refit and the bound raster draws (the positions) read it.  A translation unit of its
// own for the reason rt_mesh_skin.hip is one: the code objects of the other mesh files stay the machine code they were.  rt_mesh.hip owns the arrays.
//
// One thread per vertex, 256 per block, so a wave is one slice of the packed form (rt_morph_pack.hpp): its row range comes from two scalar loads of
// the slice table and the walk over the rows has a wave-uniform trip count.  A row is one 16-byte record per lane, 64 consecutive records per wave
// (one contiguous KiB per load instruction), and one gather from the weight table, 256 KiB at the target limit and resident in cache.  A pad record
// reads weight 0 of a table that always has one and is dropped by a select; so is an entry whose weight is +-0.  The sums form a chain in input
// order, but no load depends on them: four rows' records and weights are loaded before the first of them is used.  No LDS, no atomics, no scratch.
//
// The arithmetic is rt_morph_positions' (rt_morph_pack.cpp), operation for operation: a rounded product, a rounded sum, nothing fused, and a vertex
// without an unskipped entry keeps its base position's bits.
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/rt_mi355.h"
#include "rt_mesh.hpp"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kPad = 0xFFFFFFFFu;   // rtl::kMorphPadTarget

struct Acc { float x, y, z; };

__device__ __forceinline__ uint32_t weight_slot(uint4 r) { return r.w == kPad ? 0u : r.w; }
// one entry: skipped when it is a pad record or its weight is +-0
__device__ __forceinline__ void blend(Acc &a, uint4 r, float wt) {
    const float w = r.w == kPad ? 0.0f : wt;
    const bool use = w != 0.0f;
    const float tx = w * __uint_as_float(r.x), ty = w * __uint_as_float(r.y), tz = w * __uint_as_float(r.z);
    const float sx = a.x + tx, sy = a.y + ty, sz = a.z + tz;
    a.x = use ? sx : a.x; a.y = use ? sy : a.y; a.z = use ? sz : a.z;
}

__global__ __launch_bounds__(256) void k_mesh_morph(const float *__restrict__ base, const uint32_t *__restrict__ sliceFirst, const uint4 *__restrict__ entries,
                                                    const float *__restrict__ weights, int nVerts, int nSlices, float *__restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int slice = __builtin_amdgcn_readfirstlane(i >> 6);   // a wave is a slice
    if (slice >= nSlices) return;                               // a whole wave behind the last slice
    const bool live = i < nVerts;                               // a lane behind the last vertex walks pad records and stores nothing
    const uint32_t r0 = sliceFirst[slice], r1 = sliceFirst[slice + 1];
    Acc a = {0.0f, 0.0f, 0.0f};
    if (live) { const float *p = base + (size_t)i * 3; a.x = p[0]; a.y = p[1]; a.z = p[2]; }
    const uint4 *e = entries + (size_t)r0 * 64 + (threadIdx.x & 63);
    uint32_t k = r0;
    for (; k + 4 <= r1; k += 4, e += 4 * 64) {
        const uint4 q0 = e[0], q1 = e[64], q2 = e[128], q3 = e[192];
        const float w0 = weights[weight_slot(q0)], w1 = weights[weight_slot(q1)], w2 = weights[weight_slot(q2)], w3 = weights[weight_slot(q3)];
        blend(a, q0, w0); blend(a, q1, w1); blend(a, q2, w2); blend(a, q3, w3);
    }
    for (; k < r1; ++k, e += 64) {
        const uint4 q = e[0];
        blend(a, q, weights[weight_slot(q)]);
    }
    if (live) { float *o = dst + (size_t)i * 3; o[0] = a.x; o[1] = a.y; o[2] = a.z; }
}

}  // namespace

namespace rtl {

void morph_launch(hipStream_t st, const float *base, const uint32_t *sliceFirst, const void *entries, const float *weights, int nVerts, float *dst) {
    const int nSlices = (nVerts + 63) / 64;
    const unsigned blocks = (unsigned)std::max<size_t>(1, ((size_t)nVerts + 255) / 256);
    hipLaunchKernelGGL(k_mesh_morph, dim3(blocks), dim3(256), 0, st, base, sliceFirst, reinterpret_cast<const uint4 *>(entries), weights, nVerts, nSlices, dst);
}

}  // namespace rtl
