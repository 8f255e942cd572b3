// rt_mesh_colors.hip -- per-vertex colours of the dynamic mesh: kept per vertex and, row for row beside the triangle array, per
// corner, and the query that blends them at a hit.  A translation unit of its own for the reason rt_mesh_skin.hip is one: the code objects of the other
// mesh files stay the machine code they were.  rt_mesh.hip owns the arrays.
//   k_color_fill  one thread per vertex: one 16-byte store of (0.85, 0.85, 0.85, 0), when colours are enabled;
//   k_color_rows  one thread per row: order[row], three indices, three 16-byte vertex colours, three 16-byte stores to colRows;
//   k_hit_colors  one thread per hit: the 16-byte RtHit and the row's three corner colours as three 16-byte loads, 12 bytes stored.
// No LDS, no atomics, no scratch.  The arithmetic is rt_mesh_colors.hpp's, operation for operation.
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/rt_mi355.h"
#include "rt_mesh.hpp"
#include "rt_mesh_colors.hpp"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void k_color_fill(float4 *__restrict__ vertCol, int nVerts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nVerts) vertCol[i] = make_float4(rtcolor::kGrey, rtcolor::kGrey, rtcolor::kGrey, 0.0f);
}

__global__ __launch_bounds__(256) void k_color_rows(const int *__restrict__ order, const uint32_t *__restrict__ idx, const float4 *__restrict__ vertCol, int nTris,
                                                    int nVerts, float4 *__restrict__ colRows) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nTris) return;
    const int k = order[r];
    float4 c0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c1 = c0, c2 = c0;
    if (k >= 0 && k < nTris) {
        const uint32_t *ix = idx + (size_t)k * 3;
        const uint32_t i0 = ix[0], i1 = ix[1], i2 = ix[2];
        if (i0 < (uint32_t)nVerts && i1 < (uint32_t)nVerts && i2 < (uint32_t)nVerts) { c0 = vertCol[i0]; c1 = vertCol[i1]; c2 = vertCol[i2]; }   // (validated on upload)
    }
    float4 *o = colRows + (size_t)r * 3;
    o[0] = make_float4(c0.x, c0.y, c0.z, 0.0f); o[1] = make_float4(c1.x, c1.y, c1.z, 0.0f); o[2] = make_float4(c2.x, c2.y, c2.z, 0.0f);
}

// A prim outside [0, nTris) -- a miss, an analytic hit, a stale record -- reads nothing and answers zeros.
__global__ __launch_bounds__(256) void k_hit_colors(const float4 *__restrict__ hits, int n, const float4 *__restrict__ colRows, int nTris, float *__restrict__ colors) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 h = hits[i];
    const int prim = __float_as_int(h.y);
    float out[3] = {0.0f, 0.0f, 0.0f};
    if (prim >= 0 && prim < nTris) {
        const float4 *R = colRows + (size_t)prim * 3;
        const float4 r0 = R[0], r1 = R[1], r2 = R[2];
        const float c0[3] = {r0.x, r0.y, r0.z}, c1[3] = {r1.x, r1.y, r1.z}, c2[3] = {r2.x, r2.y, r2.z};
        rtcolor::blend_colors(c0, c1, c2, h.z, h.w, out);
    }
    float *o = colors + (size_t)i * 3;
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
}

inline unsigned blocks_for(size_t n) { return (unsigned)std::max<size_t>(1, (n + 255) / 256); }

}  // namespace

namespace rtl {

void colors_launch_fill(hipStream_t st, float4 *vertCol, int nVerts) {
    hipLaunchKernelGGL(k_color_fill, dim3(blocks_for((size_t)nVerts)), dim3(256), 0, st, vertCol, nVerts);
}

void colors_launch_rows(hipStream_t st, const int *order, const uint32_t *idx, const float4 *vertCol, int nTris, int nVerts, float4 *colRows) {
    hipLaunchKernelGGL(k_color_rows, dim3(blocks_for((size_t)nTris)), dim3(256), 0, st, order, idx, vertCol, nTris, nVerts, colRows);
}

void colors_launch_hit_colors(hipStream_t st, const void *hits, int n, const float4 *colRows, int nTris, float *colors) {
    hipLaunchKernelGGL(k_hit_colors, dim3(blocks_for((size_t)n)), dim3(256), 0, st, static_cast<const float4 *>(hits), n, colRows, nTris, colors);
}

}  // namespace rtl
