// rt_mesh_corner.hip -- the corner attributes of the dynamic mesh (14.13 - 14.15): smooth normals, colours and UVs are each a per-vertex
// array and, row for row beside the triangle array, the three corner values of the row's input triangle.  One gather fills the rows and one query
// blends them at a hit; an attribute is a traits type (NormalAttr, ColorAttr, UvAttr) that says what a vertex is and how a row is packed.
// rt_mesh.hip owns the arrays.
//   k_corner_rows<Attr>  one thread per row: order[row], three indices, three vertex values (16 bytes each; UVs: 8), the row as 16-byte stores --
//                        normals three float4 as loaded, colours three (r, g, b, 0), UVs (u0, v0, u1, v1) and (u2, v2, 0, 0);
//   k_hit_blend<Attr>    colours and UVs, one thread per hit: the 16-byte RtHit and the row as 16-byte loads, 12 or 8 bytes stored (the normals' query
//                        is k_hit_normals, rt_mesh_normals.hip: it normalises, and falls back to the face normal);
//   k_hit_texels         one thread per hit: the UV as k_hit_blend<UvAttr> has it, then up to four 4-byte texel loads and the decode table, 12 bytes stored;
//   k_color_fill         one thread per vertex: one 16-byte store of (0.85, 0.85, 0.85, 0), when colours are enabled.
// No LDS, no atomics.  Every index is checked against its array before use.  The arithmetic is rt_mesh_corner.hpp's and rt_mesh_uvs.hpp's, operation
// for operation.
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/rt_mi355.h"
#include "rt_mesh.hpp"
#include "rt_mesh_colors.hpp"
#include "rt_mesh_uvs.hpp"

#pragma clang fp contract(off)

namespace {

// An attribute: Vert, what a vertex holds; kRowVecs, the float4 of a row; pack, the row of three corner values; and, where k_hit_blend serves it,
// kChannels and unpack, the three corners of a row as kChannels floats each.
struct NormalAttr {
    using Vert = float4;
    static constexpr int kRowVecs = 3;
    static __device__ void pack(float4 *o, const Vert &c0, const Vert &c1, const Vert &c2) { o[0] = c0; o[1] = c1; o[2] = c2; }
};
struct ColorAttr {
    using Vert = float4;
    static constexpr int kRowVecs = 3, kChannels = 3;
    static __device__ void pack(float4 *o, Vert c0, Vert c1, Vert c2) {
        o[0] = make_float4(c0.x, c0.y, c0.z, 0.0f); o[1] = make_float4(c1.x, c1.y, c1.z, 0.0f); o[2] = make_float4(c2.x, c2.y, c2.z, 0.0f);
    }
    static __device__ void unpack(const float4 *R, float *c0, float *c1, float *c2) {
        const float4 r0 = R[0], r1 = R[1], r2 = R[2];
        c0[0] = r0.x; c0[1] = r0.y; c0[2] = r0.z; c1[0] = r1.x; c1[1] = r1.y; c1[2] = r1.z; c2[0] = r2.x; c2[1] = r2.y; c2[2] = r2.z;
    }
};
struct UvAttr {
    using Vert = float2;
    static constexpr int kRowVecs = 2, kChannels = 2;
    static __device__ void pack(float4 *o, Vert c0, Vert c1, Vert c2) { o[0] = make_float4(c0.x, c0.y, c1.x, c1.y); o[1] = make_float4(c2.x, c2.y, 0.0f, 0.0f); }
    static __device__ void unpack(const float4 *R, float *c0, float *c1, float *c2) {
        const float4 r0 = R[0], r1 = R[1];
        c0[0] = r0.x; c0[1] = r0.y; c1[0] = r0.z; c1[1] = r0.w; c2[0] = r1.x; c2[1] = r1.y;
    }
};

template <class Attr>
__global__ __launch_bounds__(256) void k_corner_rows(const int *__restrict__ order, const uint32_t *__restrict__ idx, const typename Attr::Vert *__restrict__ vert, int nTris,
                                                     int nVerts, float4 *__restrict__ rows) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nTris) return;
    const int k = order[r];
    typename Attr::Vert c0(0.0f), c1 = c0, c2 = c0;
    if (k >= 0 && k < nTris) {
        const uint32_t *ix = idx + (size_t)k * 3;
        const uint32_t i0 = ix[0], i1 = ix[1], i2 = ix[2];
        if (i0 < (uint32_t)nVerts && i1 < (uint32_t)nVerts && i2 < (uint32_t)nVerts) { c0 = vert[i0]; c1 = vert[i1]; c2 = vert[i2]; }   // (validated on upload)
    }
    Attr::pack(rows + (size_t)r * Attr::kRowVecs, c0, c1, c2);
}

// the attribute of hit record h on its row; false (and zeros) for a prim outside [0, nTris) -- a miss, an analytic hit, a stale record -- with nothing read
template <class Attr> __device__ inline bool hit_blend(const float4 h, const float4 *__restrict__ rows, int nTris, float *out) {
    const int prim = __float_as_int(h.y);
    for (int c = 0; c < Attr::kChannels; ++c) out[c] = 0.0f;
    if (prim < 0 || prim >= nTris) return false;
    float c0[Attr::kChannels], c1[Attr::kChannels], c2[Attr::kChannels];
    Attr::unpack(rows + (size_t)prim * Attr::kRowVecs, c0, c1, c2);
    rtcorner::blend_corners<Attr::kChannels>(c0, c1, c2, h.z, h.w, out);
    return true;
}

template <class Attr>
__global__ __launch_bounds__(256) void k_hit_blend(const float4 *__restrict__ hits, int n, const float4 *__restrict__ rows, int nTris, float *__restrict__ values) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float out[Attr::kChannels];
    (void)hit_blend<Attr>(hits[i], rows, nTris, out);
    float *o = values + (size_t)i * Attr::kChannels;
    for (int c = 0; c < Attr::kChannels; ++c) o[c] = out[c];
}

__global__ __launch_bounds__(256) void k_hit_texels(const float4 *__restrict__ hits, int n, const float4 *__restrict__ uvRows, int nTris, rtuv::Texture tex,
                                                    float *__restrict__ texels) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float uv[2], out[3] = {0.0f, 0.0f, 0.0f};
    if (hit_blend<UvAttr>(hits[i], uvRows, nTris, uv)) rtuv::sample(tex, uv[0], uv[1], out);   // (sample keeps every texel index inside W x H)
    float *o = texels + (size_t)i * 3;
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
}

__global__ __launch_bounds__(256) void k_color_fill(float4 *__restrict__ vertCol, int nVerts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nVerts) vertCol[i] = make_float4(rtcolor::kGrey, rtcolor::kGrey, rtcolor::kGrey, 0.0f);
}

inline unsigned blocks_for(size_t n) { return (unsigned)std::max<size_t>(1, (n + 255) / 256); }

template <class Attr> void launch_rows(hipStream_t st, const int *order, const uint32_t *idx, const void *vert, int nTris, int nVerts, float4 *rows) {
    hipLaunchKernelGGL(k_corner_rows<Attr>, dim3(blocks_for((size_t)nTris)), dim3(256), 0, st, order, idx, static_cast<const typename Attr::Vert *>(vert), nTris, nVerts, rows);
}
template <class Attr> void launch_hit_blend(hipStream_t st, const void *hits, int n, const float4 *rows, int nTris, float *values) {
    hipLaunchKernelGGL(k_hit_blend<Attr>, dim3(blocks_for((size_t)n)), dim3(256), 0, st, static_cast<const float4 *>(hits), n, rows, nTris, values);
}

}  // namespace

namespace rtl {

const CornerKind &corner_kind(Corner which) {
    static const CornerKind kinds[] = {   // indexed by Corner
        {sizeof(NormalAttr::Vert), NormalAttr::kRowVecs * sizeof(float4), launch_rows<NormalAttr>, nullptr},
        {sizeof(ColorAttr::Vert), ColorAttr::kRowVecs * sizeof(float4), launch_rows<ColorAttr>, launch_hit_blend<ColorAttr>},
        {sizeof(UvAttr::Vert), UvAttr::kRowVecs * sizeof(float4), launch_rows<UvAttr>, launch_hit_blend<UvAttr>},
    };
    return kinds[(int)which];
}

void corner_launch_hit_texels(hipStream_t st, const void *hits, int n, const float4 *uvRows, int nTris, const rtuv::Texture &tex, float *texels) {
    hipLaunchKernelGGL(k_hit_texels, dim3(blocks_for((size_t)n)), dim3(256), 0, st, static_cast<const float4 *>(hits), n, uvRows, nTris, tex, texels);
}

void corner_launch_color_fill(hipStream_t st, float4 *vertCol, int nVerts) {
    hipLaunchKernelGGL(k_color_fill, dim3(blocks_for((size_t)nVerts)), dim3(256), 0, st, vertCol, nVerts);
}

}  // namespace rtl
