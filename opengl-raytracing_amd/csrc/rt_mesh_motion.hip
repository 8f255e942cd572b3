// rt_mesh_motion.hip -- the previous pose of the dynamic mesh: the rows of the triangle array as they were before the most recent
// update, kept row for row beside the current ones, and the query that moves a hit point back into that pose.  A translation unit of its own for the
// reason rt_mesh_skin.hip is one: the code objects of the other mesh files stay the machine code they were.  rt_mesh.hip owns the arrays.
//
// Rows are 48 bytes, [v0 -][e1 -][e2 -], and are only ever copied: a thread moves one row as three 16-byte loads and three 16-byte stores, so a wave
// moves 3 KiB of whole cache lines whichever way it is indexed.  A refit keeps every input triangle in its row and the update is a plain device copy.
// A rebuild reorders the rows, so it is bracketed by two kernels over build positions i (perm[i] = the input triangle at position i of the sorted
// order, outOfPos[i] = the row that position lands in -- the two tables k_mesh_order composes):
//   before the sorts reuse the permutation:  byInput[perm_old[i]] = tris[outOfPos[i]]       (k_prev_scatter; the read is the gathered side)
//   after the new rows are written:          prev[outOfPos[i]]    = byInput[perm_new[i]]    (k_prev_gather;  the read is the gathered side)
// Both permutations are bijections of [0, nTris), so every row of byInput and of prev is written exactly once.  No LDS, no atomics, no arithmetic.
//
// k_hit_prev_points: one thread per hit -- the 16-byte RtHit, 12 bytes of hit point, the two rows as three 16-byte loads each (issued together,
// before the first use), 12 bytes stored.  The arithmetic is rt_hit_motion's (rt_mesh_motion.hpp), operation for operation.
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/rt_mi355.h"
#include "rt_mesh.hpp"
#include "rt_mesh_motion.hpp"

#pragma clang fp contract(off)

namespace {

__global__ void k_prev_scatter(const float4 *__restrict__ tris, const int *__restrict__ perm, const int *__restrict__ outOfPos, int nTris,
                               float4 *__restrict__ byInput) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nTris) return;
    const float4 *s = tris + (size_t)outOfPos[i] * 3;
    const float4 a = s[0], b = s[1], c = s[2];
    float4 *o = byInput + (size_t)perm[i] * 3;
    o[0] = a; o[1] = b; o[2] = c;
}

__global__ void k_prev_gather(const float4 *__restrict__ byInput, const int *__restrict__ perm, const int *__restrict__ outOfPos, int nTris,
                              float4 *__restrict__ prev) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nTris) return;
    const float4 *s = byInput + (size_t)perm[i] * 3;
    const float4 a = s[0], b = s[1], c = s[2];
    float4 *o = prev + (size_t)outOfPos[i] * 3;
    o[0] = a; o[1] = b; o[2] = c;
}

// A prim outside [0, nTris) -- a miss, an analytic hit, a stale record -- reads neither array and answers zeros.
__global__ void k_hit_prev_points(const float4 *__restrict__ hits, const float *__restrict__ points, int n, const float4 *__restrict__ tris,
                                  const float4 *__restrict__ prevTris, int nTris, float *__restrict__ prevPoints) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 h = hits[i];
    const int prim = __float_as_int(h.y);
    float out[3] = {0.0f, 0.0f, 0.0f};
    if (prim >= 0 && prim < nTris) {
        const float *p = points + (size_t)i * 3;
        const float x[3] = {p[0], p[1], p[2]};
        const float4 *T = tris + (size_t)prim * 3, *P = prevTris + (size_t)prim * 3;
        const float4 t0 = T[0], t1 = T[1], t2 = T[2], p0 = P[0], p1 = P[1], p2 = P[2];
        const float Tf[12] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w};
        const float Pf[12] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w};
        rtmotion::prev_point(Tf, Pf, h.z, h.w, x, out);
    }
    float *o = prevPoints + (size_t)i * 3;
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
}

inline unsigned blocks_for(size_t n) { return (unsigned)std::max<size_t>(1, (n + 255) / 256); }

}  // namespace

namespace rtl {

void motion_launch_scatter(hipStream_t st, const float4 *tris, const int *perm, const int *outOfPos, int nTris, float4 *byInput) {
    hipLaunchKernelGGL(k_prev_scatter, dim3(blocks_for((size_t)nTris)), dim3(256), 0, st, tris, perm, outOfPos, nTris, byInput);
}

void motion_launch_gather(hipStream_t st, const float4 *byInput, const int *perm, const int *outOfPos, int nTris, float4 *prev) {
    hipLaunchKernelGGL(k_prev_gather, dim3(blocks_for((size_t)nTris)), dim3(256), 0, st, byInput, perm, outOfPos, nTris, prev);
}

void motion_launch_hit_prev_points(hipStream_t st, const void *hits, const float *points, int n, const float4 *tris, const float4 *prevTris, int nTris,
                                   float *prevPoints) {
    hipLaunchKernelGGL(k_hit_prev_points, dim3(blocks_for((size_t)n)), dim3(256), 0, st, static_cast<const float4 *>(hits), points, n, tris, prevTris, nTris,
                       prevPoints);
}

}  // namespace rtl
