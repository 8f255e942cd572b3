// rt_mesh_normals.hip -- smooth vertex normals of the dynamic mesh: recomputed from the rows of the triangle array behind every
// update, and the query that blends them at a hit.  The gather of the corner rows is the one all corner attributes share (k_corner_rows<NormalAttr>,
// rt_mesh_corner.hip).  A translation unit of its own for the reason rt_mesh_skin.hip is one: the code objects of the other mesh files stay the
// machine code they were.  rt_mesh.hip owns the arrays.
//
// Two kernels run behind the new rows and in front of the gather, a store pass and a per-destination sum pass through an inverted index, so the sums
// have one fixed order and no atomics:
//   k_face_vectors    one thread per row: e1 and e2 as two 16-byte loads, cross(e1, e2) as one 16-byte store to faceByInput[order[row]];
//   k_vertex_normals  one thread per vertex, one wave per slice of the packed adjacency (rt_normal_pack.hpp): the slice's entry range comes from two
//                     scalar loads and the walk has a wave-uniform trip count; a step is 256 consecutive bytes of triangle numbers per wave and one
//                     16-byte gather per lane from faceByInput.  The sums form a chain in entry order, but no load depends on them: four steps'
//                     numbers are loaded, then their four face vectors, before the first is added.  A pad entry gathers face 0 and is dropped by a
//                     select.  One float4 stored, xyz the normal and w = 0.
// k_hit_normals: one thread per hit -- the 16-byte RtHit, the row (for the fallback) and the row's three corner normals as three 16-byte loads each,
// issued together, 12 bytes stored.  No LDS, no atomics, no scratch.  The arithmetic is rt_mesh_normals.hpp's, operation for operation.
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/rt_mi355.h"
#include "rt_mesh.hpp"
#include "rt_mesh_normals.hpp"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void k_face_vectors(const float4 *__restrict__ tris, const int *__restrict__ order, int nTris, float4 *__restrict__ faceByInput) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nTris) return;
    const float4 e1 = tris[(size_t)r * 3 + 1], e2 = tris[(size_t)r * 3 + 2];
    const float a[3] = {e1.x, e1.y, e1.z}, b[3] = {e2.x, e2.y, e2.z};
    float f[3];
    rtnormal::cross3(a, b, f);
    const int k = order[r];
    if (k >= 0 && k < nTris) faceByInput[k] = make_float4(f[0], f[1], f[2], 0.0f);   // (order is a bijection of [0, nTris): the guard never fails)
}

struct Sum { float x, y, z; bool any; };

// one entry: the first face vector initialises the sum, a pad entry is dropped
__device__ __forceinline__ void add_face(Sum &s, int k, float4 f) {
    const bool use = k >= 0;
    const float sx = s.any ? s.x + f.x : f.x, sy = s.any ? s.y + f.y : f.y, sz = s.any ? s.z + f.z : f.z;
    s.x = use ? sx : s.x; s.y = use ? sy : s.y; s.z = use ? sz : s.z;
    s.any = s.any || use;
}
__device__ __forceinline__ int face_slot(int k, int nTris) { return (k >= 0 && k < nTris) ? k : 0; }

__global__ __launch_bounds__(256) void k_vertex_normals(const uint32_t *__restrict__ sliceFirst, const int *__restrict__ entries, const float4 *__restrict__ faceByInput,
                                                        int nTris, int nVerts, int nSlices, float4 *__restrict__ vertNrm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int slice = __builtin_amdgcn_readfirstlane(i >> 6);   // a wave is a slice
    if (slice >= nSlices) return;                               // a whole wave behind the last slice
    const uint32_t e0 = sliceFirst[slice], e1 = sliceFirst[slice + 1];
    Sum s = {0.0f, 0.0f, 0.0f, false};
    const int *e = entries + (size_t)e0 + (threadIdx.x & 63);
    uint32_t j = e0;
    for (; j + 4 * 64 <= e1; j += 4 * 64, e += 4 * 64) {
        const int k0 = e[0], k1 = e[64], k2 = e[128], k3 = e[192];
        const float4 f0 = faceByInput[face_slot(k0, nTris)], f1 = faceByInput[face_slot(k1, nTris)], f2 = faceByInput[face_slot(k2, nTris)],
                     f3 = faceByInput[face_slot(k3, nTris)];
        add_face(s, k0, f0); add_face(s, k1, f1); add_face(s, k2, f2); add_face(s, k3, f3);
    }
    for (; j < e1; j += 64, e += 64) {
        const int k = e[0];
        add_face(s, k, faceByInput[face_slot(k, nTris)]);
    }
    if (i >= nVerts) return;                                    // a lane behind the last vertex walked pad entries
    const float S[3] = {s.x, s.y, s.z};
    float n[3];
    rtnormal::vertex_normal(S, n);
    vertNrm[i] = make_float4(n[0], n[1], n[2], 0.0f);
}

// A prim outside [0, nTris) -- a miss, an analytic hit, a stale record -- reads neither array and answers zeros.
__global__ __launch_bounds__(256) void k_hit_normals(const float4 *__restrict__ hits, int n, const float4 *__restrict__ tris, const float4 *__restrict__ nrmRows,
                                                     int nTris, float *__restrict__ normals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 h = hits[i];
    const int prim = __float_as_int(h.y);
    float out[3] = {0.0f, 0.0f, 0.0f};
    if (prim >= 0 && prim < nTris) {
        const float4 *T = tris + (size_t)prim * 3, *N = nrmRows + (size_t)prim * 3;
        const float4 t0 = T[0], t1 = T[1], t2 = T[2], c0 = N[0], c1 = N[1], c2 = N[2];
        const float Tf[12] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w};
        const float n0[3] = {c0.x, c0.y, c0.z}, n1[3] = {c1.x, c1.y, c1.z}, n2[3] = {c2.x, c2.y, c2.z};
        rtnormal::hit_normal(Tf, n0, n1, n2, h.z, h.w, out);
    }
    float *o = normals + (size_t)i * 3;
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
}

inline unsigned blocks_for(size_t n) { return (unsigned)std::max<size_t>(1, (n + 255) / 256); }

}  // namespace

namespace rtl {

void normals_launch_update(hipStream_t st, const float4 *tris, const int *order, int nTris, const uint32_t *sliceFirst, const int32_t *entries, int nVerts,
                           float4 *faceByInput, float4 *vertNrm) {
    const int nSlices = (nVerts + 63) / 64;
    hipLaunchKernelGGL(k_face_vectors, dim3(blocks_for((size_t)nTris)), dim3(256), 0, st, tris, order, nTris, faceByInput);
    hipLaunchKernelGGL(k_vertex_normals, dim3(blocks_for((size_t)nVerts)), dim3(256), 0, st, sliceFirst, entries, faceByInput, nTris, nVerts, nSlices, vertNrm);
}

void normals_launch_hit_normals(hipStream_t st, const void *hits, int n, const float4 *tris, const float4 *nrmRows, int nTris, float *normals) {
    hipLaunchKernelGGL(k_hit_normals, dim3(blocks_for((size_t)n)), dim3(256), 0, st, static_cast<const float4 *>(hits), n, tris, nrmRows, nTris, normals);
}

}  // namespace rtl
