// rt_mesh_colors.hpp -- per-vertex colours of the dynamic mesh, once, for the host definitions (rt_hit_colors and rt_color_rows,
// rt_mesh_colors.cpp), the device kernels (rt_mesh_colors.hip) and the frames (hitColor, rt_device_shade.hpp).
//
// A vertex colour is three floats, the linear RGB albedo that stands where the reference's directLightBVH writes 0.85 in all three channels.  At a hit
// with barycentrics (a, b) the three corner colours are blended channel by channel; a channel whose three corner values are bit-equal hands that value
// back bit for bit -- so three bit-equal corners hand their colour back, a mesh of one colour shades exactly as a constant does, and a channel that is
// constant over the mesh is not disturbed by the others -- and non-finite barycentrics give the first corner.  fp32, every product and sum rounded on
// its own, nothing fused.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_COLOR_HD __host__ __device__
#else
#define RT_COLOR_HD
#endif

#pragma clang fp contract(off)

namespace rtcolor {

// the albedo of a mesh hit without colours: the reference's constant (directLightBVH, rt_lighting.glsl)
constexpr float kGrey = 0.85f;

RT_COLOR_HD inline bool same_bits(float p, float q) {
    uint32_t u, v;
    __builtin_memcpy(&u, &p, 4); __builtin_memcpy(&v, &q, 4);
    return u == v;
}

// finite: neither NaN nor an infinity, on the bits (no comparison that a fast-math flag could fold)
RT_COLOR_HD inline bool finite_bits(float p) {
    uint32_t u;
    __builtin_memcpy(&u, &p, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
}

// the blend of a row's three corner colours at barycentrics (a, b)
RT_COLOR_HD inline void blend_colors(const float *c0, const float *c1, const float *c2, float a, float b, float *out) {
    const bool first = !finite_bits(a) || !finite_bits(b);
    const float w = (1.0f - a) - b;
    for (int c = 0; c < 3; ++c) {
        const bool flat = same_bits(c0[c], c1[c]) && same_bits(c0[c], c2[c]);
        const float m = (c0[c] * w + c1[c] * a) + c2[c] * b;
        out[c] = (first || flat) ? c0[c] : m;
    }
}

}  // namespace rtcolor
