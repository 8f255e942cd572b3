// rt_bvh_cost.hpp -- the expressions of the BVH quality metric, once, for the host definition (rt_bvh_cost, rt_host.cpp), the
// device measurement (rt_mesh_quality.hip) and the host code that turns the device's integer sums into the record (rt_api.hip).
//
// The metric is the surface-area heuristic with both unit costs 1: sum over inner nodes of area / root area, plus sum over leaves of count x area /
// root area.  It has to come out bit for bit alike whatever order waves and blocks add in, so nothing floating-point is ever summed over nodes: every
// node's half-area is scaled by a power of two taken from the root's half-area, floored to an integer q <= 2^32, and the integers are added.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_COST_HD __host__ __device__
#else
#define RT_COST_HD
#endif

#pragma clang fp contract(off)

namespace rtcost {

// half the surface area of a box from its fp32 extents: widened to double every product is exact (two 24-bit significands), fp32 would overflow
RT_COST_HD inline double half_area(float dx, float dy, float dz) {
    const double x = (double)dx, y = (double)dy, z = (double)dz;
    return (x * y + y * z) + z * x;
}

// frexp's exponent of the root's half-area A > 0: A = m * 2^e with m in [0.5, 1)
RT_COST_HD inline int root_exp(double A) { int e = 0; (void)frexp(A, &e); return e; }

// a <= A < 2^e, so q <= 2^32
RT_COST_HD inline uint64_t quantise(double a, int e) { return (uint64_t)floor(ldexp(a, 32 - e)); }

// an integer sum back to units of the root's half-area
inline double from_sum(uint64_t sumQ, int e, double A) { return ldexp((double)sumQ, e - 32) / A; }

}  // namespace rtcost
