// rt_overlap_query.cpp -- rt_box_overlaps, rt_tri_overlaps and rt_hull_overlaps (include/rt_mi355.h): the definitions of the box
// query, of the triangle query and of the hull query.  Host only, no context, no GPU.
//
// For one query with the closed box [lo, hi] -- the box itself, or the box of a query triangle's three points or of a hull's eight corners -- the list
// is the rows t that lie under nodes that pass the shape's node test all the way from the root -- their boxes overlap [lo, hi] and, for a hull, none of
// its six face normals parts them from it -- and that the shape's separating-axis test cannot part from the query (13 axes for a box, DESIGN.md 23.1;
// 20 for a triangle; 46 for a hull), in the order of a depth-first walk that takes the right child before the left
// and the rows of a leaf ascending.  Nothing culls by what was found, so list and count are functions of the tree and the query alone; the device walk (rt_overlap_query.hip) makes
// the same tests in the same order and is held to this answer bit for bit.  The shapes and every float operation are rt_overlap_math.hpp's, the text
// the device compiles too.
#include <climits>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/rt_mi355.h"
#include "rt_bvh_tree.hpp"
#include "rt_overlap_math.hpp"

using namespace rtoverlap;

namespace {

// minFloats: the floats of one query
template <class Shape>
int overlaps(int minFloats, const float *nodes12, int nNodes, const float *tris12, int nTris, const float *queries, int stride, int n, const int32_t *offsets,
             int cap, int32_t *prims, int32_t *counts) {
    if (n < 0 || nNodes < 0 || nTris < 0 || stride < minFloats) return RT_ERR_INVALID;
    if ((nNodes > 0 && !nodes12) || (nTris > 0 && !tris12)) return RT_ERR_INVALID;
    if (n > 0 && (!queries || (!prims && !counts))) return RT_ERR_INVALID;
    if (prims && !offsets && (cap < 0 || (uint64_t)n * (uint64_t)cap > (uint64_t)INT32_MAX)) return RT_ERR_INVALID;
    try {
        const bool scene = nNodes > 0 && nTris > 0;
        if (scene && !rtbvh::is_tree(nodes12, nNodes, nTris)) return RT_ERR_INVALID;
        std::vector<int> stack;
        for (int i = 0; i < n; ++i) {
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
            Shape S;
            if (scene && S.load(queries + (size_t)i * stride)) {   // else an empty slot
                S.prepare();
                stack.assign(1, 0);
                while (!stack.empty()) {
                    const int ni = stack.back();
                    stack.pop_back();
                    const float *nd = nodes12 + (size_t)ni * 12;
                    if (!S.node(ld(nd), ld(nd + 4))) continue;
                    const rtbvh::Node N = rtbvh::node_fetch(nd);
                    if (N.count > 0) {
                        for (int k = 0; k < N.count; ++k) {
                            const float *t = tris12 + (size_t)(N.first + k) * 12;
                            if (!S.row(ld(t), ld(t + 4), ld(t + 8))) continue;
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

}  // namespace

extern "C" int rt_box_overlaps(const float *nodes12, int nNodes, const float *tris12, int nTris, const float *boxes, int stride, int n, const int32_t *offsets,
                               int cap, int32_t *prims, int32_t *counts) {
    return overlaps<BoxShape>(6, nodes12, nNodes, tris12, nTris, boxes, stride, n, offsets, cap, prims, counts);
}

extern "C" int rt_tri_overlaps(const float *nodes12, int nNodes, const float *tris12, int nTris, const float *qtris, int stride, int n, const int32_t *offsets,
                               int cap, int32_t *prims, int32_t *counts) {
    return overlaps<TriShape>(9, nodes12, nNodes, tris12, nTris, qtris, stride, n, offsets, cap, prims, counts);
}

extern "C" int rt_hull_overlaps(const float *nodes12, int nNodes, const float *tris12, int nTris, const float *hulls, int stride, int n, const int32_t *offsets,
                                int cap, int32_t *prims, int32_t *counts) {
    return overlaps<HullShape>(24, nodes12, nNodes, tris12, nTris, hulls, stride, n, offsets, cap, prims, counts);
}
