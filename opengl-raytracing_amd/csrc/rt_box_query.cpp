// rt_box_query.cpp -- rt_box_overlaps (include/rt_mi355.h): the definition of the box query.  Host only, no context, no GPU.
//
// For one closed box Q = [lo, hi], the list is the rows t that lie under nodes whose boxes overlap Q all the way from the root and that the 13-axis
// separating-axis test below cannot part from Q, in the order of a depth-first walk that takes the right child before the left and the rows of a leaf
// ascending.  Nothing culls, so list and count are functions of the tree and the box alone; the device walk (rt_box_query.hip) makes the same tests
// in the same order and is held to this answer bit for bit.  DESIGN.md 23.1 has every operation; pd and dot are rt_nearest_math.hpp's.
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

// One axis cross(unit_k, f): components n1, n2 on the coordinates i, j != k.  a1 .. c2: the vertices' coordinates i and j; l1 .. h2: the box's.
// A point projects to fmaf(p_j, n2, p_i * n1); the box to the least and the greatest of its corners under the same two steps, the least and the greatest
// product kept after the first.  Both steps are monotone, so a vertex inside the closed box never projects outside it.  True when the axis separates.
inline bool edge_axis_separates(float n1, float n2, float a1, float a2, float b1, float b2, float c1, float c2, float l1, float h1, float l2, float h2) {
    const float pa = std::fmaf(a2, n2, a1 * n1), pb = std::fmaf(b2, n2, b1 * n1), pc = std::fmaf(c2, n2, c1 * n1);
    const float tmin = min3(pa, pb, pc), tmax = max3(pa, pb, pc);
    const float l1p = l1 * n1, h1p = h1 * n1;
    const float m1 = fminr(l1p, h1p), M1 = fmaxr(l1p, h1p);
    const float bmin = fminr(std::fmaf(l2, n2, m1), std::fmaf(h2, n2, m1)), bmax = fmaxr(std::fmaf(l2, n2, M1), std::fmaf(h2, n2, M1));
    return tmax < bmin || bmax < tmin;
}

// The three axes cross(unit_x, f), cross(unit_y, f), cross(unit_z, f) = (0, -f.z, f.y), (f.z, 0, -f.x), (-f.y, f.x, 0)
inline bool edge_separates(V f, V a, V b, V c, V lo, V hi) {
    return edge_axis_separates(-f.z, f.y, a.y, a.z, b.y, b.z, c.y, c.z, lo.y, hi.y, lo.z, hi.z) ||
           edge_axis_separates(-f.x, f.z, a.z, a.x, b.z, b.x, c.z, c.x, lo.z, hi.z, lo.x, hi.x) ||
           edge_axis_separates(-f.y, f.x, a.x, a.y, b.x, b.y, c.x, c.y, lo.x, hi.x, lo.y, hi.y);
}

// The triangle test of DESIGN.md 23.1: true when none of the 13 axes separates the row from [lo, hi]
inline bool tri_overlaps(V v0, V e1, V e2, V lo, V hi) {
    const V a = v0, b = {v0.x + e1.x, v0.y + e1.y, v0.z + e1.z}, c = {v0.x + e2.x, v0.y + e2.y, v0.z + e2.z};
    const V tmin = {min3(a.x, b.x, c.x), min3(a.y, b.y, c.y), min3(a.z, b.z, c.z)}, tmax = {max3(a.x, b.x, c.x), max3(a.y, b.y, c.y), max3(a.z, b.z, c.z)};
    if (!boxes_overlap(tmin, tmax, lo, hi)) return false;
    const V n = {pd(e1.y, e2.z, e1.z, e2.y), pd(e1.z, e2.x, e1.x, e2.z), pd(e1.x, e2.y, e1.y, e2.x)};
    const float d = dot(n, a);
    const float lx = n.x * lo.x, hx = n.x * hi.x;   // the box's corners through dot's own three steps, the least and the greatest kept at each
    const float mx = fminr(lx, hx), Mx = fmaxr(lx, hx);
    const float my = fminr(std::fmaf(n.y, lo.y, mx), std::fmaf(n.y, hi.y, mx)), My = fmaxr(std::fmaf(n.y, lo.y, Mx), std::fmaf(n.y, hi.y, Mx));
    const float bmin = fminr(std::fmaf(n.z, lo.z, my), std::fmaf(n.z, hi.z, my)), bmax = fmaxr(std::fmaf(n.z, lo.z, My), std::fmaf(n.z, hi.z, My));
    if (d < bmin || bmax < d) return false;
    if (edge_separates(e1, a, b, c, lo, hi)) return false;
    if (edge_separates(sub(e2, e1), a, b, c, lo, hi)) return false;
    return !edge_separates(e2, a, b, c, lo, hi);
}

}  // namespace

extern "C" int rt_box_overlaps(const float *nodes12, int nNodes, const float *tris12, int nTris, const float *boxes, int stride, int n, const int32_t *offsets,
                               int cap, int32_t *prims, int32_t *counts) {
    if (n < 0 || nNodes < 0 || nTris < 0 || stride < 6) return RT_ERR_INVALID;
    if ((nNodes > 0 && !nodes12) || (nTris > 0 && !tris12)) return RT_ERR_INVALID;
    if (n > 0 && (!boxes || (!prims && !counts))) return RT_ERR_INVALID;
    if (prims && !offsets && (cap < 0 || (uint64_t)n * (uint64_t)cap > (uint64_t)INT32_MAX)) return RT_ERR_INVALID;
    try {
        const bool scene = nNodes > 0 && nTris > 0;
        if (scene && !rtbvh::is_tree(nodes12, nNodes, nTris)) return RT_ERR_INVALID;
        std::vector<int> stack;
        for (int i = 0; i < n; ++i) {
            const float *q = boxes + (size_t)i * stride;
            const V lo = ld(q), hi = ld(q + 3);
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
            if (scene && lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z) {   // a NaN component or lo > hi: an empty slot
                stack.assign(1, 0);
                while (!stack.empty()) {
                    const int ni = stack.back();
                    stack.pop_back();
                    const float *nd = nodes12 + (size_t)ni * 12;
                    if (!boxes_overlap(ld(nd), ld(nd + 4), lo, hi)) continue;
                    const rtbvh::Node N = rtbvh::node_fetch(nd);
                    if (N.count > 0) {
                        for (int k = 0; k < N.count; ++k) {
                            const float *t = tris12 + (size_t)(N.first + k) * 12;
                            if (!tri_overlaps(ld(t), ld(t + 4), ld(t + 8), lo, hi)) continue;
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
