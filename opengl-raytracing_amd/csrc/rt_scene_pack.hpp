// rt_scene_pack.hpp -- the host packers of the BVH scene: every device record form of rt_upload_bvh as plain arithmetic over the
// reference's two float arrays.  No HIP, no context: rt_api.hip uploads what pack_scene made, rt_debug_pack_scene hands it out without a device, and
// rt_mesh.hip lays its index tables out with the topology helpers below instead of with copies of them.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace rtl {

constexpr size_t kQNodesAbove = (size_t)4 << 20;   // bytes of 112-byte any-hit nodes beyond which the quantised nodes are built and walked

struct PackOptions {
    int qnodes = -1;                // quantised any-hit nodes: -1 by the size of the tree (kQNodesAbove), 0 never, > 0 always
    bool fused = false;             // fused closest-hit records
    bool implicit = false;          // implicit records, where every leaf sits at one depth
    bool anyhitSah = false;         // EXPERIMENT: the four-wide tree from a binned SAH build over the leaves
    bool sparseLeafBoxes = false;   // EXPERIMENT: one leaf-box slot per pair record
    bool verbose = false;
};
// The one place that reads RT_QNODES, RT_FUSED, RT_IMPLICIT, RT_ANYHIT_TREE, RT_QNODES_SPARSE_BOXES and RT_VERBOSE for the packers.
PackOptions pack_options_from_env();
// "Build the quantised form?" for a four-wide tree of nWide4 records whose root reference is rootRef4 (0: an inner root)
inline bool want_quantised(const PackOptions &o, size_t nWide4, int rootRef4) {
    return rootRef4 == 0 && (o.qnodes > 0 || (o.qnodes < 0 && nWide4 * 112 > kQNodesAbove));
}

struct PackedScene {
    std::vector<float> pairs, wn, wnW, w4, leafBox, wF, iN2, iPairs, iN4, iLeafBox;
    std::vector<uint32_t> q4, iQ4;
    int nInner = 0, depth = 0;
    int rootRef = 0, rootRefW = 0, rootRef4 = 0;
    int anyStack = 0;
    uint32_t leafBoxMagic = 0;
    size_t nLeafBoxes = 0;
    int implD = 0, implR = 0;
    int flags = 0;                  // RT_SCENE_QNODES_REJECTED, RT_SCENE_NOT_FUSED
    float rootMin[3] = {0, 0, 0}, rootMax[3] = {0, 0, 0};
    bool collapsed4 = true;         // w4 is the binary tree collapsed (false: the SAH tree, which the bounce probe must not walk)
};

// nodes12 / tris12: the reference's texture-buffer arrays, nNodes > 0 and nTris > 0.  RT_OK, or the code and message (err) of rt_upload_bvh.
int pack_scene(const float *nodes12, int nNodes, const float *tris12, int nTris, const PackOptions &opt, PackedScene &out, std::string &err);

// ---- topology helpers, shared with rtl::mesh_create (which applies them to the skeleton instead of to decoded nodes)

// One four-wide node of the collapsed tree: the binary nodes that became its children (-1: absent) and their references (RT_NO_CHILD: absent)
struct Wide4 { int kid[4]; int ref[4]; };

// 4-wide nodes for any-hit rays: every binary inner node at an even level absorbs its inner children, so one
// 128-byte record holds up to four grandchild boxes -- stored component-wise, so that the 28 payload floats take 7 of the
// record's 8 sixteen-byte pieces and a visit costs 7 gather loads.  A child box is only skipped (never tested) when it is an
// intermediate node; by monotonicity of the slab arithmetic a grandchild that passes its own test also passes
// its parent's, so the set of triangles tested -- and hence every any-hit answer -- is unchanged.
// left(i), right(i), count(i): the binary tree (count > 0: a leaf), node 0 an inner node; leafRef(i): the reference of leaf i.
template <class Left, class Right, class Count, class LeafRef>
std::vector<Wide4> collapse_to_four(Left left, Right right, Count count, LeafRef leafRef) {
    struct Job { int bin; size_t at; };   // fill node `at` from binary node `bin`
    std::vector<Job> jobs{{0, 0}};
    std::vector<Wide4> w4(1);
    while (!jobs.empty()) {
        const Job jb = jobs.back();
        jobs.pop_back();
        int kids[4], nk = 0;
        for (int ch : {left(jb.bin), right(jb.bin)}) {
            if (count(ch) > 0) kids[nk++] = ch;
            else { kids[nk++] = left(ch); kids[nk++] = right(ch); }
        }
        for (int i = 0; i < 4; ++i) {
            int ref = 0x7fffffff, kid = -1;   // RT_NO_CHILD
            if (i < nk) {
                kid = kids[i];
                if (count(kid) > 0) ref = leafRef(kid);
                else { ref = (int)w4.size(); w4.push_back(Wide4{}); jobs.push_back({kid, (size_t)ref}); }
            }
            w4[jb.at].kid[i] = kid; w4[jb.at].ref[i] = ref;
        }
    }
    return w4;
}

// Exact stack need of the any-hit walk (round 4): a visit of a node with nc children pushes at most nc - 1 entries (one child is gone on with),
// so S(node) = nc - 1 + max over its inner children S(child).  Round 3 sized the stack as 3 per two binary levels INCLUDING the leaf level: 24 entries
// for the bench mesh, where 21 are enough -- and 21 x 4 B x 256 threads let seven workgroups share a CU's 160 KB of LDS instead of six.
// refAt(node, i): child reference i of four-wide node `node` of n4 (root: node 0).
template <class RefAt>
int any_stack_need(size_t n4, RefAt refAt) {
    std::vector<int> need(n4, -1);
    std::vector<std::pair<size_t, int>> st{{0, 0}};   // (node, next child to look at)
    while (!st.empty()) {
        auto &[nn, ci] = st.back();
        if (ci < 4) {
            const int ref = refAt(nn, ci);
            ++ci;
            if (ref >= 0 && ref != 0x7fffffff && (size_t)ref < n4 && need[(size_t)ref] < 0) st.push_back({(size_t)ref, 0});
            continue;
        }
        int nc = 0, deepest = 0;
        for (int i = 0; i < 4; ++i) {
            const int ref = refAt(nn, i);
            if (ref == 0x7fffffff) continue;
            ++nc;
            if (ref >= 0 && (size_t)ref < n4) deepest = std::max(deepest, need[(size_t)ref]);
        }
        need[nn] = std::max(nc - 1, 0) + deepest;
        st.pop_back();
    }
    return std::max(need[0], 1);
}

// A leaf's box sits at index first / R, R = the smallest number of pair records any leaf owns: consecutive leaves are at least R records apart,
// so the quotient is distinct per leaf, and the array is dense when the leaves are alike (a median-split tree: record counts differ by at most one).
// The kernel divides by multiplying with ceil(2^32 / R) (exact for first < 2^28, R <= 8); R = 1: the identity (magic 0).
struct LeafBoxRule {
    int rmin;         // R (1 under sparseLeafBoxes: one slot per pair record, as first built)
    uint32_t magic;
    LeafBoxRule(int minLeafRecords, bool sparse) : rmin(sparse ? 1 : minLeafRecords), magic(rmin <= 1 ? 0u : (uint32_t)((((uint64_t)1 << 32) + (uint64_t)rmin - 1) / (uint64_t)rmin)) {}
    size_t index(size_t firstPairRecord) const { return magic ? (size_t)(((uint64_t)firstPairRecord * magic) >> 32) : firstPairRecord; }
    size_t floats(size_t pairRecordsWithPadding) const { return (pairRecordsWithPadding / (size_t)std::max(rmin, 1) + 1) * 8; }   // the array's length
};

}  // namespace rtl
