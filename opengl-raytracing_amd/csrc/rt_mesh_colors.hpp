// rt_mesh_colors.hpp -- per-vertex colours of the dynamic mesh, once, for the host definitions (rt_hit_colors and rt_color_rows,
// rt_mesh_colors.cpp), the device kernels (rt_mesh_corner.hip) and the frames (hitColor, rt_device_shade.hpp).
//
// A vertex colour is three floats, the linear RGB albedo that stands where the reference's directLightBVH writes 0.85 in all three channels.  At a hit
// the three corner colours are blended under rt_mesh_corner.hpp's rule, so a mesh of one colour shades exactly as a constant does.
#pragma once
#include "rt_mesh_corner.hpp"

namespace rtcolor {

// the albedo of a mesh hit without colours: the reference's constant (directLightBVH, rt_lighting.glsl)
constexpr float kGrey = 0.85f;

// the blend of a row's three corner colours at barycentrics (a, b)
RT_CORNER_HD inline void blend_colors(const float *c0, const float *c1, const float *c2, float a, float b, float *out) { rtcorner::blend_corners<3>(c0, c1, c2, a, b, out); }

}  // namespace rtcolor
