// rt_mesh_corner.hpp -- what the corner attributes of the dynamic mesh share: the bit tests and the blend of a row's three corner values
// at a hit, once, for smooth normals (rt_mesh_normals.hpp), the previous pose (rt_mesh_motion.hpp), colours (rt_mesh_colors.hpp) and UVs
// (rt_mesh_uvs.hpp).  Plain host + device C++, no HIP header: the host definitions link on their own.
//
// A corner attribute is a per-vertex array and, row for row beside the triangle array, the three corner values of the row's input triangle.  At a hit
// with barycentrics (a, b) the corner values are blended channel by channel; a channel whose three corner values are bit-equal hands that value back
// bit for bit -- so three bit-equal corners hand their value back and a channel that is constant over the mesh is not disturbed by the others -- and
// non-finite barycentrics give the first corner.  fp32, every product and sum rounded on its own, nothing fused.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_CORNER_HD __host__ __device__
#else
#define RT_CORNER_HD
#endif

#pragma clang fp contract(off)

namespace rtcorner {

RT_CORNER_HD inline bool same_bits(float p, float q) {
    uint32_t u, v;
    __builtin_memcpy(&u, &p, 4); __builtin_memcpy(&v, &q, 4);
    return u == v;
}

// finite: neither NaN nor an infinity, on the bits (no comparison that a fast-math flag could fold)
RT_CORNER_HD inline bool finite_bits(float p) {
    uint32_t u;
    __builtin_memcpy(&u, &p, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
}

// the blend of a row's three corner values of C channels at barycentrics (a, b)
template <int C> RT_CORNER_HD inline void blend_corners(const float *c0, const float *c1, const float *c2, float a, float b, float *out) {
    const bool first = !finite_bits(a) || !finite_bits(b);
    const float w = (1.0f - a) - b;
    for (int c = 0; c < C; ++c) {
        const bool flat = same_bits(c0[c], c1[c]) && same_bits(c0[c], c2[c]);
        const float m = (c0[c] * w + c1[c] * a) + c2[c] * b;
        out[c] = (first || flat) ? c0[c] : m;
    }
}

}  // namespace rtcorner
