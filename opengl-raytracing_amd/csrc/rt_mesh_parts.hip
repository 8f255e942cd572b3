// rt_mesh_parts.hip -- the part-aware kernels of the dynamic mesh: the gather of a rebuild and of a refit with one model matrix per
// part, read from the device table, and the map from a hit's prim to (part, triangle of the part).  A translation unit of its own for the reason
// rt_mesh_refit.hip is one: the code objects of rt_mesh.hip and rt_mesh_refit.hip stay the machine code they were.  rt_mesh.hip owns the tables.
//
// Part lookup: partOf[input triangle], 16 bits per triangle, written once by rt_mesh_upload_parts.  A thread pays one 2-byte load -- coalesced in the
// gather, where thread i owns triangle i; beside the perm[i] gather it already does in the refit -- and no search, no LDS and no barrier.  The matrix
// is one 64-byte entry of the table, 64-byte aligned, read as four 16-byte loads of which the xyz lanes are used (12 of the 16 floats).  Neighbouring
// triangles almost always share a part, so a wave's matrix loads fall on one or two cache lines; in the refit they need not, and the table (256 KiB at
// 4096 parts) then sits in L2 beside the positions it is gathered with.
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/rt_mi355.h"
#include "rt_mesh.hpp"

#pragma clang fp contract(off)

namespace {

// one vertex under the matrix whose columns are c0 .. c3: k_mesh_gather's expression, glm's mat4 * vec4 order
__device__ __forceinline__ void world(const float4 &c0, const float4 &c1, const float4 &c2, const float4 &c3, const float *__restrict__ p, float *v) {
    const float x = p[0], y = p[1], z = p[2];
    v[0] = (c0.x * x + c1.x * y) + (c2.x * z + c3.x * 1.0f);
    v[1] = (c0.y * x + c1.y * y) + (c2.y * z + c3.y * 1.0f);
    v[2] = (c0.z * x + c1.z * y) + (c2.z * z + c3.z * 1.0f);
}

// the three corners of input triangle `tri` under its part's matrix
__device__ __forceinline__ void corners(const float *__restrict__ pos, const uint32_t *__restrict__ idx, const uint16_t *__restrict__ partOf,
                                        const float4 *__restrict__ mats, int tri, float v[3][3]) {
    const float4 *M = mats + (size_t)partOf[tri] * 4;
    const float4 c0 = M[0], c1 = M[1], c2 = M[2], c3 = M[3];
    for (int c = 0; c < 3; ++c) world(c0, c1, c2, c3, pos + (size_t)idx[(size_t)tri * 3 + c] * 3, v[c]);
}

// k_mesh_gather with the matrix of the triangle's part: nine floats (v0, e1 = b - a, e2 = c - a) per input triangle, in input order
__global__ void k_parts_gather(const float *__restrict__ pos, const uint32_t *__restrict__ idx, const uint16_t *__restrict__ partOf,
                               const float4 *__restrict__ mats, int nTris, float *__restrict__ t9) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nTris) return;
    float v[3][3];
    corners(pos, idx, partOf, mats, i, v);
    float *o = t9 + (size_t)i * 9;
    for (int j = 0; j < 3; ++j) { o[j] = v[0][j]; o[3 + j] = v[1][j] - v[0][j]; o[6 + j] = v[2][j] - v[0][j]; }
}

// k_refit_tris with the matrix of the triangle's part: input triangle perm[i] into the row it had, three 16-byte stores
__global__ void k_parts_refit_tris(const float *__restrict__ pos, const uint32_t *__restrict__ idx, const int *__restrict__ perm,
                                   const int *__restrict__ outOfPos, const uint16_t *__restrict__ partOf, const float4 *__restrict__ mats, int nTris,
                                   float4 *__restrict__ t12) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nTris) return;
    float v[3][3];
    corners(pos, idx, partOf, mats, perm[i], v);
    float4 *o = t12 + (size_t)outOfPos[i] * 3;
    o[0] = make_float4(v[0][0], v[0][1], v[0][2], 0.0f);
    o[1] = make_float4(v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2], 0.0f);
    o[2] = make_float4(v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2], 0.0f);
}

// hit -> (part, triangle of the part): prim is a row of the triangle array, order[prim] the input triangle.  A prim outside [0, nTris) -- a miss, an
// analytic hit, a stale record -- reads neither table.
__global__ void k_hit_parts(const RtHit *__restrict__ hits, int n, const int *__restrict__ order, int nTris, const uint16_t *__restrict__ partOf,
                            const int32_t *__restrict__ partFirst, int32_t *__restrict__ parts, int32_t *__restrict__ tris) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int prim = hits[i].prim;
    int part = -1, tri = -1;
    if (prim >= 0 && prim < nTris) {
        const int t = order[prim];
        part = (int)partOf[t];
        tri = t - partFirst[part];
    }
    if (parts) parts[i] = part;
    if (tris) tris[i] = tri;
}

inline unsigned blocks_for(size_t n) { return (unsigned)std::max<size_t>(1, (n + 255) / 256); }

}  // namespace

namespace rtl {

void parts_launch_gather(hipStream_t st, const float *pos, const uint32_t *idx, const uint16_t *partOf, const float *mats, int nTris, float *t9) {
    hipLaunchKernelGGL(k_parts_gather, dim3(blocks_for((size_t)nTris)), dim3(256), 0, st, pos, idx, partOf, reinterpret_cast<const float4 *>(mats), nTris, t9);
}

void parts_launch_refit_tris(hipStream_t st, const float *pos, const uint32_t *idx, const int *perm, const int *outOfPos, const uint16_t *partOf, const float *mats,
                             int nTris, float4 *t12) {
    hipLaunchKernelGGL(k_parts_refit_tris, dim3(blocks_for((size_t)nTris)), dim3(256), 0, st, pos, idx, perm, outOfPos, partOf,
                       reinterpret_cast<const float4 *>(mats), nTris, t12);
}

void parts_launch_hit_parts(hipStream_t st, const void *hits, int n, const int *order, int nTris, const uint16_t *partOf, const int32_t *partFirst, int32_t *parts,
                            int32_t *tris) {
    hipLaunchKernelGGL(k_hit_parts, dim3(blocks_for((size_t)n)), dim3(256), 0, st, static_cast<const RtHit *>(hits), n, order, nTris, partOf, partFirst, parts, tris);
}

}  // namespace rtl
