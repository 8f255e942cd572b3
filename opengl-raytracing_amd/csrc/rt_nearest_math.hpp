// rt_nearest_math.hpp -- the float operations of the nearest-point definitions: pd, lb(box, p), closestUV, the point v0 + u e1 + v e2
// and e(t).  One text for both sides: compiled as HIP its functions are device functions over rtd::V3 (rt_nearest.hip,
// rt_nearest_multi.hip, rt_overlap_query.hip), compiled as plain C++ inline host functions over its own V (rt_nearest.cpp, rt_nearest_multi.cpp,
// rt_overlap_query.cpp).  Only the primitives differ by side: the vector type with its ld and sub, the fused multiply-add, min, max and dot.  Written in
// the float model of DESIGN.md 2: a fused multiply-add exactly where dot and cross have it, nothing contracted.
#pragma once
#if defined(__HIP__)
#include "rt_device_math.hpp"
#define RT_Q __device__ __forceinline__
namespace rtnear {
using V = rtd::V3;
using rtd::dot;
using rtd::fmaxr;   // a NaN operand is ignored
using rtd::fminr;
RT_Q V ld(const float *p) { return rtd::ld3(p); }
RT_Q V sub(V a, V b) { return a - b; }
RT_Q float fmar(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
}  // namespace rtnear
#else
#include <cmath>
#define RT_Q inline
namespace rtnear {
struct V { float x, y, z; };
inline V ld(const float *p) { return V{p[0], p[1], p[2]}; }
inline V sub(V a, V b) { return V{a.x - b.x, a.y - b.y, a.z - b.z}; }
inline float fmar(float a, float b, float c) { return std::fmaf(a, b, c); }
inline float dot(V a, V b) { return fmar(a.z, b.z, fmar(a.y, b.y, a.x * b.x)); }
inline float fmaxr(float a, float b) { return std::fmax(a, b); }   // a NaN operand is ignored
inline float fminr(float a, float b) { return std::fmin(a, b); }
inline bool finite3(V p) { return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z); }
}  // namespace rtnear
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rtnear {

RT_Q float pd(float a, float b, float c, float d) { return fmar(a, b, -(c * d)); }   // a b - c d, the idiom of cross

// lb(box, p): the squared distance from p to the box, 0 inside
RT_Q float box_lb(V lo, V hi, V p) {
    const V d = {fmaxr(fmaxr(lo.x - p.x, p.x - hi.x), 0.0f), fmaxr(fmaxr(lo.y - p.y, p.y - hi.y), 0.0f), fmaxr(fmaxr(lo.z - p.z, p.z - hi.z), 0.0f)};
    return dot(d, d);
}

// closestUV: Ericson, Real-Time Collision Detection 5.1.5, over the row as stored (ab = e1, ac = e2); the nearest point is v0 + u e1 + v e2
RT_Q void closest_uv(V p, V v0, V e1, V e2, float &u, float &v) {
    const V ap = sub(p, v0);
    const float d1 = dot(e1, ap), d2 = dot(e2, ap);
    if (d1 <= 0.0f && d2 <= 0.0f) { u = 0.0f; v = 0.0f; return; }                                        // A
    const V bp = sub(ap, e1);
    const float d3 = dot(e1, bp), d4 = dot(e2, bp);
    if (d3 >= 0.0f && d4 <= d3) { u = 1.0f; v = 0.0f; return; }                                          // B
    const float vc = pd(d1, d4, d3, d2);
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { u = d1 / (d1 - d3); v = 0.0f; return; }                // AB
    const V cp = sub(ap, e2);
    const float d5 = dot(e1, cp), d6 = dot(e2, cp);
    if (d6 >= 0.0f && d5 <= d6) { u = 0.0f; v = 1.0f; return; }                                          // C
    const float vb = pd(d5, d2, d1, d6);
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { u = 0.0f; v = d2 / (d2 - d6); return; }                // AC
    const float va = pd(d3, d6, d5, d4);
    const float s = d4 - d3, r = d5 - d6;
    if (va <= 0.0f && s >= 0.0f && r >= 0.0f) { v = s / (s + r); u = 1.0f - v; return; }                 // BC
    const float den = 1.0f / ((va + vb) + vc);                                                           // interior
    u = vb * den;
    v = vc * den;
}
RT_Q V point_at(V v0, V e1, V e2, float u, float v) {
    return V{fmar(v, e2.x, fmar(u, e1.x, v0.x)), fmar(v, e2.y, fmar(u, e1.y, v0.y)), fmar(v, e2.z, fmar(u, e1.z, v0.z))};
}

// e(t): the row's squared distance from p, raised to pathLB, the largest box bound above it.  A NaN distance stays NaN
RT_Q float row_e(V p, V v0, V e1, V e2, float pathLB) {
    float u, v;
    closest_uv(p, v0, e1, e2, u, v);
    const V diff = sub(p, point_at(v0, e1, e2, u, v));
    const float d2 = dot(diff, diff);
    return (d2 < pathLB) ? pathLB : d2;
}

}  // namespace rtnear
