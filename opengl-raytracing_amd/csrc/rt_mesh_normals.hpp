// rt_mesh_normals.hpp -- smooth vertex normals of the dynamic mesh, once, for the host definitions (rt_vertex_normals and
// rt_hit_normals, rt_normal_pack.cpp), the device kernels (rt_mesh_normals.hip, rt_mesh_corner.hip) and the frames (hitNormal, rt_device_shade.hpp).
//
// A row of the triangle array is [v0 -][e1 -][e2 -].  Its face vector is cross(e1, e2) in rt_device_math.hpp's expression, not normalised, so a vertex
// sum weights by area; a vertex normal is the sum under normalize's expression, or three +0 where the sum has no direction.  At a hit with barycentrics
// (a, b) the three corner normals are blended and normalised; three bit-equal corners hand their normal back bit for bit -- a flat region shades exactly
// as the reference's face normal does -- and whatever has no direction falls back to the row's face normal, tri_normal's expression.  fp32, rounded
// products and sums, nothing fused except where cross and dot write an fmaf.
#pragma once
#include <cstdint>

#include "rt_mesh_corner.hpp"

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_NORMAL_HD __host__ __device__
#else
#define RT_NORMAL_HD
#endif

#pragma clang fp contract(off)

namespace rtnormal {

// cross and dot of rt_device_math.hpp, operation for operation
RT_NORMAL_HD inline void cross3(const float *a, const float *b, float *o) {
    o[0] = __builtin_fmaf(a[1], b[2], -(a[2] * b[1]));
    o[1] = __builtin_fmaf(a[2], b[0], -(a[0] * b[2]));
    o[2] = __builtin_fmaf(a[0], b[1], -(a[1] * b[0]));
}
RT_NORMAL_HD inline float dot3(const float *a, const float *b) { return __builtin_fmaf(a[2], b[2], __builtin_fmaf(a[1], b[1], a[0] * b[0])); }

// v * (1 / sqrt(dot(v, v))) when dot(v, v) > 0 and finite: normalize's expression.  false: v has no direction, o is untouched.
RT_NORMAL_HD inline bool unit3(const float *v, float *o) {
    const float d = dot3(v, v);
    if (!(d > 0.0f) || !(d < __builtin_inff())) return false;
    const float inv = 1.0f / __builtin_sqrtf(d);
    o[0] = v[0] * inv; o[1] = v[1] * inv; o[2] = v[2] * inv;
    return true;
}

// the face vector of a row (12 floats): cross(e1, e2)
RT_NORMAL_HD inline void face_vector(const float *row, float *f) { cross3(row + 4, row + 8, f); }

// the vertex normal of a finished sum
RT_NORMAL_HD inline void vertex_normal(const float *S, float *n) {
    float u[3];
    const bool ok = unit3(S, u);
    n[0] = ok ? u[0] : 0.0f; n[1] = ok ? u[1] : 0.0f; n[2] = ok ? u[2] : 0.0f;
}

// the blend of a row's three corner normals at barycentrics (a, b); false: it has no answer (zero bit-equal corners, a zero or non-finite sum, NaN
// barycentrics), out is untouched and the row's face normal is the answer
RT_NORMAL_HD inline bool blend_normals(const float *n0, const float *n1, const float *n2, float a, float b, float *out) {
    bool same = true;
    for (int c = 0; c < 3; ++c) same = same && rtcorner::same_bits(n0[c], n1[c]) && rtcorner::same_bits(n0[c], n2[c]);
    if (same) {
        if (n0[0] == 0.0f && n0[1] == 0.0f && n0[2] == 0.0f) return false;
        out[0] = n0[0]; out[1] = n0[1]; out[2] = n0[2];
        return true;
    }
    const float w = (1.0f - a) - b;
    float m[3];
    for (int c = 0; c < 3; ++c) m[c] = (n0[c] * w + n1[c] * a) + n2[c] * b;
    return unit3(m, out);
}

// tri_normal (rt_device_shade.hpp): normalize(cross(e1, e2)), whatever that is for a degenerate row
RT_NORMAL_HD inline void face_normal(const float *e1, const float *e2, float *out) {
    float f[3];
    cross3(e1, e2, f);
    const float inv = 1.0f / __builtin_sqrtf(dot3(f, f));
    out[0] = f[0] * inv; out[1] = f[1] * inv; out[2] = f[2] * inv;
}

// the shading normal at barycentrics (a, b) of a row (12 floats) whose corners carry n0, n1, n2
RT_NORMAL_HD inline void hit_normal(const float *row, const float *n0, const float *n1, const float *n2, float a, float b, float *out) {
    if (!blend_normals(n0, n1, n2, a, b, out)) face_normal(row + 4, row + 8, out);
}

}  // namespace rtnormal
