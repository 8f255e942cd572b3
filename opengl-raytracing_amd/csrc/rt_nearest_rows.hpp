// rt_nearest_rows.hpp -- the walk of the nearest-point definitions, for rt_nearest.cpp and rt_nearest_multi.cpp: every row of the tree
// with its e(t).  Host only, header only.
#pragma once
#include <utility>
#include <vector>

#include "rt_bvh_tree.hpp"
#include "rt_nearest_math.hpp"

namespace rtnear {

// Calls row(prim, e) for every row t, e = e(t): the row's squared distance from p raised to the largest box bound lb(box(n), p) on the way from the
// root to its leaf.  e(t) is a function of the row and the point alone, so the walk visits every node, carries the running maximum and culls
// nothing: the order nodes are visited in does not matter.  stack: the caller's, kept across points
template <class Row>
void for_each_row(const float *nodes12, const float *tris12, V p, std::vector<std::pair<int, float>> &stack, Row row) {
    stack.assign(1, {0, 0.0f});   // (node, the largest lb above it)
    while (!stack.empty()) {
        const int ni = stack.back().first;
        const float above = stack.back().second;
        stack.pop_back();
        const float *q = nodes12 + (size_t)ni * 12;
        const float pathLB = fmaxr(above, box_lb(ld(q), ld(q + 4), p));
        const rtbvh::Node N = rtbvh::node_fetch(q);
        if (N.count > 0) {
            for (int k = 0; k < N.count; ++k) {
                const float *t = tris12 + (size_t)(N.first + k) * 12;
                row(N.first + k, row_e(p, ld(t), ld(t + 4), ld(t + 8), pathLB));
            }
        } else {
            stack.push_back({N.right, pathLB});
            stack.push_back({N.left, pathLB});
        }
    }
}

}  // namespace rtnear
