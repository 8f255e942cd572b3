// rt_mesh_uvs.hip -- vertex UVs and the albedo texture of the dynamic mesh: the UVs kept per vertex and, row for row beside the
// triangle array, per corner, and the two queries that blend them at a hit and sample the texture there.  A translation unit of its own for the reason
// rt_mesh_colors.hip is one: the code objects of the other mesh files stay the machine code they were.  rt_mesh.hip owns the arrays.
//   k_uv_rows     one thread per row: order[row], three indices, three 8-byte vertex UVs, two 16-byte stores to uvRows;
//   k_hit_uvs     one thread per hit: the 16-byte RtHit and the row as two 16-byte loads, 8 bytes stored;
//   k_hit_texels  one thread per hit: the same, then up to four 4-byte texel loads and the decode table, 12 bytes stored.
// No LDS, no atomics.  Every index is checked against its array before use.  The arithmetic is rt_mesh_uvs.hpp's, operation for operation.
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/rt_mi355.h"
#include "rt_mesh.hpp"
#include "rt_mesh_uvs.hpp"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void k_uv_rows(const int *__restrict__ order, const uint32_t *__restrict__ idx, const float2 *__restrict__ vertUv, int nTris, int nVerts,
                                                 float4 *__restrict__ uvRows) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nTris) return;
    const int k = order[r];
    float2 c0 = make_float2(0.0f, 0.0f), c1 = c0, c2 = c0;
    if (k >= 0 && k < nTris) {
        const uint32_t *ix = idx + (size_t)k * 3;
        const uint32_t i0 = ix[0], i1 = ix[1], i2 = ix[2];
        if (i0 < (uint32_t)nVerts && i1 < (uint32_t)nVerts && i2 < (uint32_t)nVerts) { c0 = vertUv[i0]; c1 = vertUv[i1]; c2 = vertUv[i2]; }   // (validated on upload)
    }
    float4 *o = uvRows + (size_t)r * 2;
    o[0] = make_float4(c0.x, c0.y, c1.x, c1.y); o[1] = make_float4(c2.x, c2.y, 0.0f, 0.0f);
}

// the UV of hit record h on its row; false (and zeros) for a prim outside [0, nTris) -- a miss, an analytic hit, a stale record -- with nothing read
__device__ inline bool hit_uv(const float4 h, const float4 *__restrict__ uvRows, int nTris, float *uv) {
    const int prim = __float_as_int(h.y);
    uv[0] = 0.0f; uv[1] = 0.0f;
    if (prim < 0 || prim >= nTris) return false;
    const float4 *R = uvRows + (size_t)prim * 2;
    const float4 r0 = R[0], r1 = R[1];
    const float c0[2] = {r0.x, r0.y}, c1[2] = {r0.z, r0.w}, c2[2] = {r1.x, r1.y};
    rtuv::blend_uvs(c0, c1, c2, h.z, h.w, uv);
    return true;
}

__global__ __launch_bounds__(256) void k_hit_uvs(const float4 *__restrict__ hits, int n, const float4 *__restrict__ uvRows, int nTris, float *__restrict__ uvs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float uv[2];
    (void)hit_uv(hits[i], uvRows, nTris, uv);
    float *o = uvs + (size_t)i * 2;
    o[0] = uv[0]; o[1] = uv[1];
}

__global__ __launch_bounds__(256) void k_hit_texels(const float4 *__restrict__ hits, int n, const float4 *__restrict__ uvRows, int nTris, rtuv::Texture tex,
                                                    float *__restrict__ texels) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float uv[2], out[3] = {0.0f, 0.0f, 0.0f};
    if (hit_uv(hits[i], uvRows, nTris, uv)) rtuv::sample(tex, uv[0], uv[1], out);   // (sample keeps every texel index inside W x H)
    float *o = texels + (size_t)i * 3;
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
}

inline unsigned blocks_for(size_t n) { return (unsigned)std::max<size_t>(1, (n + 255) / 256); }

}  // namespace

namespace rtl {

void uvs_launch_rows(hipStream_t st, const int *order, const uint32_t *idx, const float2 *vertUv, int nTris, int nVerts, float4 *uvRows) {
    hipLaunchKernelGGL(k_uv_rows, dim3(blocks_for((size_t)nTris)), dim3(256), 0, st, order, idx, vertUv, nTris, nVerts, uvRows);
}

void uvs_launch_hit_uvs(hipStream_t st, const void *hits, int n, const float4 *uvRows, int nTris, float *uvs) {
    hipLaunchKernelGGL(k_hit_uvs, dim3(blocks_for((size_t)n)), dim3(256), 0, st, static_cast<const float4 *>(hits), n, uvRows, nTris, uvs);
}

void uvs_launch_hit_texels(hipStream_t st, const void *hits, int n, const float4 *uvRows, int nTris, const rtuv::Texture &tex, float *texels) {
    hipLaunchKernelGGL(k_hit_texels, dim3(blocks_for((size_t)n)), dim3(256), 0, st, static_cast<const float4 *>(hits), n, uvRows, nTris, tex, texels);
}

}  // namespace rtl
