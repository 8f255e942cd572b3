// rt_bvh_tree.hpp -- what the host definitions of the queries with a traversal of their own (rt_multi_hit.cpp, rt_nearest.cpp) read of nodes12: a
// node's links as the reference's nodeFetch reads them, and the check that the nodes are a tree over the rows.  Header only: each definition links
// without any other object of the library.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rtbvh {

struct Node { int left, right, first, count; };   // nodeFetch, rt_bvh.glsl:91-102
inline int to_index(float f) { return (f >= 0.0f && f < 2147483520.0f) ? (int)(f + 0.5f) : -1; }   // int(f + 0.5) of an index; -1 for what is none (negative, huge, NaN)
inline Node node_fetch(const float *p) { return Node{to_index(p[3]), to_index(p[7]), to_index(p[8]), to_index(p[9])}; }

// Every node is reached once from node 0, children and triangle ranges lie inside the arrays: a walk from node 0 then ends and reads nothing else
inline bool is_tree(const float *nodes12, int nNodes, int nTris) {
    std::vector<uint8_t> seen((size_t)nNodes, 0);
    std::vector<int> stack{0};
    while (!stack.empty()) {
        const int ni = stack.back();
        stack.pop_back();
        if (ni < 0 || ni >= nNodes || seen[(size_t)ni]) return false;
        seen[(size_t)ni] = 1;
        const Node N = node_fetch(nodes12 + (size_t)ni * 12);
        if (N.count > 0) {
            if (N.first < 0 || N.count > nTris || N.first > nTris - N.count) return false;
        } else {
            stack.push_back(N.left);
            stack.push_back(N.right);
        }
    }
    return true;
}

}  // namespace rtbvh
