// rt_mesh_refit.hip -- the device kernels of the refit: the tree of the last rebuild kept, everything that depends on coordinates
// recomputed.  A translation unit of its own, so that the code object of rt_mesh.hip -- the rebuild's kernels and the radix sort instantiated there --
// stays the machine code it was (tools/isa_diff.py).  rt_mesh.hip owns the mesh, the tables and the order of the launches; this file only launches.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include <hip/hip_runtime.h>

#include "rt_mesh.hpp"

#pragma clang fp contract(off)

namespace {

struct Mat16 { float m[16]; };

// the sortable key of rt_bvh_build.hpp: unsigned order = float order, with -0 below +0
__device__ __forceinline__ uint32_t f2sortable(float f) { uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

// Triangles: k_mesh_gather's expression for the input triangle perm[i], written as k_emit_tris writes it to the row that triangle had.
__global__ void k_refit_tris(const float *__restrict__ pos, const uint32_t *__restrict__ idx, const int *__restrict__ perm, const int *__restrict__ outOfPos,
                             int nTris, Mat16 M, float4 *__restrict__ t12) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nTris) return;
    const int tri = perm[i];
    float v[3][3];
    for (int c = 0; c < 3; ++c) {
        const float *p = pos + (size_t)idx[(size_t)tri * 3 + c] * 3;
        const float x = p[0], y = p[1], z = p[2];
        for (int k = 0; k < 3; ++k) v[c][k] = (M.m[k] * x + M.m[4 + k] * y) + (M.m[8 + k] * z + M.m[12 + k] * 1.0f);
    }
    float4 *o = t12 + (size_t)outOfPos[i] * 3;
    o[0] = make_float4(v[0][0], v[0][1], v[0][2], 0.0f);
    o[1] = make_float4(v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2], 0.0f);
    o[2] = make_float4(v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2], 0.0f);
}

// Leaf boxes from the leaf's own rows (<= 8, contiguous): per triangle k_tri_prep's corners v0, v0 + e1, v0 + e2, reduced as sortable uints -- the
// order k_level_bounds' atomics reduce in, so -0 lies below +0.  One thread per leaf; thread 0 clears the quantiser's status word (k_mesh_init's job).
__global__ void k_refit_leaves(const float4 *__restrict__ t12, const rtl::RefitLeaf *__restrict__ tab, int nLeaves, uint32_t *__restrict__ bounds,
                               uint32_t *__restrict__ status) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0) *status = 0u;
    if (j >= nLeaves) return;
    const rtl::RefitLeaf lf = tab[j];
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    for (int k = 0; k < lf.count; ++k) {
        const float4 a = t12[(size_t)(lf.first + k) * 3], b = t12[(size_t)(lf.first + k) * 3 + 1], c = t12[(size_t)(lf.first + k) * 3 + 2];
        const float v0[3] = {a.x, a.y, a.z}, e1[3] = {b.x, b.y, b.z}, e2[3] = {c.x, c.y, c.z};
        for (int ax = 0; ax < 3; ++ax) {
            const uint32_t s0 = f2sortable(v0[ax]), s1 = f2sortable(v0[ax] + e1[ax]), s2 = f2sortable(v0[ax] + e2[ax]);
            lo[ax] = min(lo[ax], min(s0, min(s1, s2)));
            hi[ax] = max(hi[ax], max(s0, max(s1, s2)));
        }
    }
    uint32_t *o = bounds + (size_t)lf.slot * 6;
    for (int ax = 0; ax < 3; ++ax) { o[ax] = lo[ax]; o[3 + ax] = hi[ax]; }
}

// Inner boxes of one level = the union of their two children's, which the launches before this one finished (deeper levels, the leaves).
__global__ void k_refit_inner(const rtl::RefitKids *__restrict__ kids, int firstSlot, int nSlots, uint32_t *__restrict__ bounds) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nSlots) return;
    const int slot = firstSlot + j;
    const rtl::RefitKids k = kids[slot];
    if (k.l < 0) return;
    const uint32_t *a = bounds + (size_t)k.l * 6, *b = bounds + (size_t)k.r * 6;
    uint32_t *o = bounds + (size_t)slot * 6;
    for (int c = 0; c < 3; ++c) { o[c] = min(a[c], b[c]); o[3 + c] = max(a[3 + c], b[3 + c]); }
}

// order[row] = the input triangle in that row of the triangle array (rt_build_bvh_order's meaning)
__global__ void k_mesh_order(const int *__restrict__ perm, const int *__restrict__ outOfPos, int nTris, int *__restrict__ order) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nTris) order[outOfPos[i]] = perm[i];
}

inline unsigned blocks_for(size_t n) { return (unsigned)std::max<size_t>(1, (n + 255) / 256); }

}  // namespace

namespace rtl {

void refit_launch_tris(hipStream_t st, const float *pos, const uint32_t *idx, const int *perm, const int *outOfPos, int nTris, const float *M16, float4 *t12) {
    Mat16 M;
    std::memcpy(M.m, M16, sizeof M.m);
    hipLaunchKernelGGL(k_refit_tris, dim3(blocks_for((size_t)nTris)), dim3(256), 0, st, pos, idx, perm, outOfPos, nTris, M, t12);
}

void refit_launch_leaves(hipStream_t st, const float4 *t12, const RefitLeaf *leaves, int nLeaves, uint32_t *bounds, uint32_t *status) {
    hipLaunchKernelGGL(k_refit_leaves, dim3(blocks_for((size_t)nLeaves)), dim3(256), 0, st, t12, leaves, nLeaves, bounds, status);
}

void refit_launch_inner(hipStream_t st, const RefitKids *kids, int firstSlot, int nSlots, uint32_t *bounds) {
    hipLaunchKernelGGL(k_refit_inner, dim3(blocks_for((size_t)nSlots)), dim3(256), 0, st, kids, firstSlot, nSlots, bounds);
}

void refit_launch_order(hipStream_t st, const int *perm, const int *outOfPos, int nTris, int *order) {
    hipLaunchKernelGGL(k_mesh_order, dim3(blocks_for((size_t)nTris)), dim3(256), 0, st, perm, outOfPos, nTris, order);
}

}  // namespace rtl
