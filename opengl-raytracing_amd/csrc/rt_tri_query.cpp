// rt_tri_query.cpp -- rt_tri_overlaps (include/rt_mi355.h): the definition of the triangle query.  Host only, no context, no GPU.
//
// For one query triangle (p0, p1, p2) with the box [qlo, qhi] of its points, the list is the rows t that lie under nodes whose boxes overlap [qlo, qhi]
// all the way from the root and that the 20-axis separating-axis test below cannot part from the query, in the order of a depth-first walk that takes
// the right child before the left and the rows of a leaf ascending: the walk of rt_box_overlaps for the box [qlo, qhi].  Nothing culls, so list and count
// are functions of the tree and the query alone; the device walk (rt_tri_query.hip) makes the same tests and is held to this answer bit for bit.
// DESIGN.md 24.1 has every operation; pd, dot and sub are rt_nearest_math.hpp's.
#include <climits>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/rt_mi355.h"
#include "rt_bvh_tree.hpp"
#include "rt_nearest_math.hpp"

using namespace rtnear;

namespace {

inline float fminr(float a, float b) { return std::fmin(a, b); }   // a NaN operand is ignored, as fmaxr
inline float min3(float a, float b, float c) { return fminr(fminr(a, b), c); }
inline float max3(float a, float b, float c) { return fmaxr(fmaxr(a, b), c); }

// closed boxes: comparisons only
inline bool boxes_overlap(V bmin, V bmax, V lo, V hi) {
    return !(bmax.x < lo.x) && !(hi.x < bmin.x) && !(bmax.y < lo.y) && !(hi.y < bmin.y) && !(bmax.z < lo.z) && !(hi.z < bmin.z);
}

inline V cross(V x, V y) { return V{pd(x.y, y.z, x.z, y.y), pd(x.z, y.x, x.x, y.z), pd(x.x, y.y, x.y, y.x)}; }
inline V add(V a, V b) { return V{a.x + b.x, a.y + b.y, a.z + b.z}; }

// The query's own values: its points, its edges g1 = p1 - p0, g2 = p2 - p1, g3 = p2 - p0, its normal m = cross(g1, g3) and the box of its points
struct Query {
    V p0, p1, p2, g1, g2, g3, m, lo, hi;
};

inline Query make_query(const float *q) {
    Query Q;
    Q.p0 = ld(q); Q.p1 = ld(q + 3); Q.p2 = ld(q + 6);
    Q.g1 = sub(Q.p1, Q.p0); Q.g2 = sub(Q.p2, Q.p1); Q.g3 = sub(Q.p2, Q.p0);
    Q.m = cross(Q.g1, Q.g3);
    Q.lo = V{min3(Q.p0.x, Q.p1.x, Q.p2.x), min3(Q.p0.y, Q.p1.y, Q.p2.y), min3(Q.p0.z, Q.p1.z, Q.p2.z)};
    Q.hi = V{max3(Q.p0.x, Q.p1.x, Q.p2.x), max3(Q.p0.y, Q.p1.y, Q.p2.y), max3(Q.p0.z, Q.p1.z, Q.p2.z)};
    return Q;
}

inline bool has_nan(const float *q) {
    for (int k = 0; k < 9; ++k)
        if (q[k] != q[k]) return true;
    return false;
}

// One projected axis: the row's points and the query's points through the same dot.  True when the axis separates; a NaN never does
inline bool axis_separates(V ax, V a, V b, V c, const Query &Q) {
    const float ta = dot(ax, a), tb = dot(ax, b), tc = dot(ax, c);
    const float q0 = dot(ax, Q.p0), q1 = dot(ax, Q.p1), q2 = dot(ax, Q.p2);
    const float tmin = min3(ta, tb, tc), tmax = max3(ta, tb, tc), qmin = min3(q0, q1, q2), qmax = max3(q0, q1, q2);
    return tmax < qmin || qmax < tmin;
}

// The triangle test of DESIGN.md 24.1: true when none of the 20 axes separates the row from the query
inline bool tri_overlaps(V v0, V e1, V e2, const Query &Q) {
    const V a = v0, b = add(v0, e1), c = add(v0, e2);
    const V tmin = {min3(a.x, b.x, c.x), min3(a.y, b.y, c.y), min3(a.z, b.z, c.z)}, tmax = {max3(a.x, b.x, c.x), max3(a.y, b.y, c.y), max3(a.z, b.z, c.z)};
    if (!boxes_overlap(tmin, tmax, Q.lo, Q.hi)) return false;
    const V f1 = e1, f2 = sub(e2, e1), f3 = e2;
    const V n = cross(e1, e2);
    if (axis_separates(n, a, b, c, Q)) return false;
    if (axis_separates(Q.m, a, b, c, Q)) return false;
    if (axis_separates(cross(f1, Q.g1), a, b, c, Q) || axis_separates(cross(f1, Q.g2), a, b, c, Q) || axis_separates(cross(f1, Q.g3), a, b, c, Q)) return false;
    if (axis_separates(cross(f2, Q.g1), a, b, c, Q) || axis_separates(cross(f2, Q.g2), a, b, c, Q) || axis_separates(cross(f2, Q.g3), a, b, c, Q)) return false;
    if (axis_separates(cross(f3, Q.g1), a, b, c, Q) || axis_separates(cross(f3, Q.g2), a, b, c, Q) || axis_separates(cross(f3, Q.g3), a, b, c, Q)) return false;
    if (axis_separates(cross(n, f1), a, b, c, Q) || axis_separates(cross(n, f2), a, b, c, Q) || axis_separates(cross(n, f3), a, b, c, Q)) return false;
    return !(axis_separates(cross(Q.m, Q.g1), a, b, c, Q) || axis_separates(cross(Q.m, Q.g2), a, b, c, Q) || axis_separates(cross(Q.m, Q.g3), a, b, c, Q));
}

}  // namespace

extern "C" int rt_tri_overlaps(const float *nodes12, int nNodes, const float *tris12, int nTris, const float *qtris, int stride, int n, const int32_t *offsets,
                               int cap, int32_t *prims, int32_t *counts) {
    if (n < 0 || nNodes < 0 || nTris < 0 || stride < 9) return RT_ERR_INVALID;
    if ((nNodes > 0 && !nodes12) || (nTris > 0 && !tris12)) return RT_ERR_INVALID;
    if (n > 0 && (!qtris || (!prims && !counts))) return RT_ERR_INVALID;
    if (prims && !offsets && (cap < 0 || (uint64_t)n * (uint64_t)cap > (uint64_t)INT32_MAX)) return RT_ERR_INVALID;
    try {
        const bool scene = nNodes > 0 && nTris > 0;
        if (scene && !rtbvh::is_tree(nodes12, nNodes, nTris)) return RT_ERR_INVALID;
        std::vector<int> stack;
        for (int i = 0; i < n; ++i) {
            const float *q = qtris + (size_t)i * stride;
            int32_t *out = nullptr;   // the slot: `room` entries from `out`
            int64_t room = 0;
            if (prims && offsets) {
                const int32_t o0 = offsets[i], o1 = offsets[i + 1];
                if (o0 >= 0 && o1 > o0) { out = prims + o0; room = (int64_t)o1 - o0; }   // (a negative start holds nothing, as a negative length)
            } else if (prims) {
                out = prims + (size_t)i * (size_t)cap;
                room = cap;
            }
            int64_t found = 0;
            if (scene && !has_nan(q)) {   // a NaN component: an empty slot
                const Query Q = make_query(q);
                stack.assign(1, 0);
                while (!stack.empty()) {
                    const int ni = stack.back();
                    stack.pop_back();
                    const float *nd = nodes12 + (size_t)ni * 12;
                    if (!boxes_overlap(ld(nd), ld(nd + 4), Q.lo, Q.hi)) continue;
                    const rtbvh::Node N = rtbvh::node_fetch(nd);
                    if (N.count > 0) {
                        for (int k = 0; k < N.count; ++k) {
                            const float *t = tris12 + (size_t)(N.first + k) * 12;
                            if (!tri_overlaps(ld(t), ld(t + 4), ld(t + 8), Q)) continue;
                            if (found < room) out[found] = N.first + k;
                            found++;
                        }
                    } else {
                        stack.push_back(N.left);
                        stack.push_back(N.right);   // popped first: the right child before the left
                    }
                }
            }
            if (counts) counts[i] = (int32_t)found;
        }
    } catch (const std::bad_alloc &) {
        return RT_ERR_IO;
    }
    return RT_OK;
}
