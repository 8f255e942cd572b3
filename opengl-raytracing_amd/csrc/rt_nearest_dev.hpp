// rt_nearest_dev.hpp -- the device forms of the nearest-point definitions' float operations and the walks' stack entry, for
// rt_nearest.hip and rt_nearest_multi.hip: operation for operation what rt_nearest_math.hpp has for the host.
#pragma once
#include "rt_frame.hpp"

#pragma clang fp contract(off)

namespace rtd {
namespace nearest {

RT_DEV float pd(float a, float b, float c, float d) { return __builtin_fmaf(a, b, -(c * d)); }   // a b - c d, the idiom of cross
RT_DEV unsigned long long entry(int ref, float lbEff) { return (unsigned long long)(uint32_t)ref | ((unsigned long long)f2u(lbEff) << 32); }   // a stack entry
RT_DEV bool finite1(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }

// lb(box, p): the squared distance from p to the box, 0 inside
RT_DEV float box_lb(V3 lo, V3 hi, V3 p) {
    const V3 d = mk3(fmaxr(fmaxr(lo.x - p.x, p.x - hi.x), 0.0f), fmaxr(fmaxr(lo.y - p.y, p.y - hi.y), 0.0f), fmaxr(fmaxr(lo.z - p.z, p.z - hi.z), 0.0f));
    return dot(d, d);
}

// closestUV of DESIGN.md 21.1, operation for operation as rt_nearest.cpp has it
RT_DEV void closest_uv(V3 p, V3 v0, V3 e1, V3 e2, float &u, float &v) {
    const V3 ap = p - v0;
    const float d1 = dot(e1, ap), d2 = dot(e2, ap);
    if (d1 <= 0.0f && d2 <= 0.0f) { u = 0.0f; v = 0.0f; return; }                                        // A
    const V3 bp = ap - e1;
    const float d3 = dot(e1, bp), d4 = dot(e2, bp);
    if (d3 >= 0.0f && d4 <= d3) { u = 1.0f; v = 0.0f; return; }                                          // B
    const float vc = pd(d1, d4, d3, d2);
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { u = d1 / (d1 - d3); v = 0.0f; return; }                // AB
    const V3 cp = ap - e2;
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
RT_DEV V3 point_at(V3 v0, V3 e1, V3 e2, float u, float v) {
    return mk3(__builtin_fmaf(v, e2.x, __builtin_fmaf(u, e1.x, v0.x)), __builtin_fmaf(v, e2.y, __builtin_fmaf(u, e1.y, v0.y)),
               __builtin_fmaf(v, e2.z, __builtin_fmaf(u, e1.z, v0.z)));
}

}  // namespace nearest
}  // namespace rtd
