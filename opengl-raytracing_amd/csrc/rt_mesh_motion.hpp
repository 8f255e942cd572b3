// rt_mesh_motion.hpp -- where a hit point of the dynamic mesh was in the previous pose, once, for the host definition (rt_hit_motion,
// rt_host.cpp), the device query (rt_mesh_motion.hip) and the frames (prevHitPoint, rt_device_shade.hpp).
//
// T is the hit triangle's row of the triangle array, P the row the same input triangle had before the most recent update, both [v0 -][e1 -][e2 -];
// (a, b) are the hit's barycentrics on T and x the hit point.  A row whose nine geometry floats did not change hands x back bit for bit (-0 and NaN
// included), so an unchanged pose gives exactly the reference's motion; otherwise the point moves by the difference of the two rows at (a, b), which
// keeps the precision of a displacement that is small against the coordinates.  fp32, rounded products and sums, nothing fused.
#pragma once
#include <cstdint>

#include "rt_mesh_corner.hpp"

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_MOTION_HD __host__ __device__
#else
#define RT_MOTION_HD
#endif

#pragma clang fp contract(off)

namespace rtmotion {

RT_MOTION_HD inline void prev_point(const float *T, const float *P, float a, float b, const float *x, float *prev) {
    bool same = true;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) same = same && rtcorner::same_bits(T[4 * r + c], P[4 * r + c]);
    for (int c = 0; c < 3; ++c) {
        const float d = ((P[c] - T[c]) + (P[4 + c] - T[4 + c]) * a) + (P[8 + c] - T[8 + c]) * b;
        prev[c] = same ? x[c] : x[c] + d;
    }
}

}  // namespace rtmotion
