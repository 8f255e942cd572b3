// rt_scene_pack.cpp -- the host packers of the BVH scene (rt_scene_pack.hpp): one function per record form, called in order by pack_scene.
#include "rt_scene_pack.hpp"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/rt_mi355.h"
#include "rt_qnode.hpp"

namespace rtl {

PackOptions pack_options_from_env() {
    PackOptions o;
    auto on = [](const char *name) { const char *e = getenv(name); return e && atoi(e) != 0; };
    if (const char *e = getenv("RT_QNODES")) o.qnodes = atoi(e);
    o.fused = on("RT_FUSED");
    o.implicit = on("RT_IMPLICIT");
    if (const char *e = getenv("RT_ANYHIT_TREE")) o.anyhitSah = std::string(e) == "sah";
    o.sparseLeafBoxes = getenv("RT_QNODES_SPARSE_BOXES") != nullptr;
    o.verbose = getenv("RT_VERBOSE") != nullptr;
    return o;
}

namespace {

int fail(std::string &err, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

struct N { int left, right, first, count; };
// the decoded tree every stage reads: links, the compact index of every inner node, the pair-record reference of every leaf
struct Tree {
    const float *nodes12, *tris12;
    int nNodes, nTris, nInner = 0;
    std::vector<N> nd;
    std::vector<int> innerIdx, pairRefOf;
    const float *box(int node) const { return nodes12 + (size_t)node * 12; }
    bool leaf(int node) const { return nd[(size_t)node].count > 0; }
    int refOf(int node) const {
        const N &n = nd[(size_t)node];
        return (n.count > 0) ? -(((n.first << 3) | (n.count - 1)) + 1) : innerIdx[(size_t)node];
    }
    int refOfW(int node) const { return leaf(node) ? pairRefOf[(size_t)node] : innerIdx[(size_t)node]; }
};

const float kQnan = std::nanf("");

// Decode the reference's float-encoded links exactly as nodeFetch does (rt_bvh.glsl:97-100).
int decode_links(Tree &t, std::string &err) {
    t.nd.resize((size_t)t.nNodes);
    t.innerIdx.assign((size_t)t.nNodes, -1);
    for (int i = 0; i < t.nNodes; ++i) {
        const float *p = t.box(i);
        t.nd[(size_t)i] = {(int)(p[3] + 0.5f), (int)(p[7] + 0.5f), (int)(p[8] + 0.5f), (int)(p[9] + 0.5f)};
        const N &n = t.nd[(size_t)i];
        if (n.count > 0) {
            if (n.count > 8 || n.first < 0 || n.first + n.count > t.nTris)
                return fail(err, RT_ERR_UNSUPPORTED, "rt_upload_bvh: leaf %d has first=%d count=%d (leaves hold 1..8 triangles)", i, n.first, n.count);
        } else {
            if (n.left <= 0 || n.right <= 0 || n.left >= t.nNodes || n.right >= t.nNodes)
                return fail(err, RT_ERR_INVALID, "rt_upload_bvh: inner node %d has children %d,%d", i, n.left, n.right);
            t.innerIdx[(size_t)i] = t.nInner++;
        }
    }
    return RT_OK;
}

// Triangle PAIR records for the wavefront pipeline's traversal kernels: what bounds them is the number of 16-byte gather
// loads per ray, and a 48-byte triangle record carries only 36 bytes of payload.  Two triangles of a leaf are
// packed into 80 bytes = 5 loads instead of 6: floats [0..8] = v0,e1,e2 of the first, [9..17] of the second, [18] = index of the
// first in the reference's triangle array (closest-hit results name triangles by it), [19] unused.  A leaf owns
// ceil(count/2) consecutive records; its reference in the wavefront node arrays addresses the first of them.
int pack_pairs(Tree &t, std::vector<float> &pairs, std::string &err) {
    t.pairRefOf.assign((size_t)t.nNodes, 0);
    for (int i = 0; i < t.nNodes; ++i) {
        const N &n = t.nd[(size_t)i];
        if (n.count <= 0) continue;
        const size_t rec = pairs.size() / 20;
        if (rec + 8 >= ((size_t)1 << 28)) return fail(err, RT_ERR_UNSUPPORTED, "rt_upload_bvh: pair records exceed the 2^28 leaf encoding");
        t.pairRefOf[(size_t)i] = -((int)((rec << 3) | (size_t)(n.count - 1)) + 1);
        for (int k = 0; k < n.count; k += 2) {
            float r[20] = {0};
            for (int h = 0; h < 2 && k + h < n.count; ++h) {
                const float *q = t.tris12 + (size_t)(n.first + k + h) * 12;
                const float nine[9] = {q[0], q[1], q[2], q[4], q[5], q[6], q[8], q[9], q[10]};
                std::memcpy(&r[9 * h], nine, sizeof nine);
            }
            const uint32_t orig = (uint32_t)(n.first + k);
            std::memcpy(&r[18], &orig, 4);
            if (k + 1 >= n.count) std::memcpy(&r[9], &orig, 4);   // a record with one triangle: the index again in the unused tenth float (3-load fetch)
            pairs.insert(pairs.end(), r, r + 20);
        }
    }
    pairs.resize(pairs.size() + 8 * 20, 0.0f);   // groups are fetched without a bounds branch
    return RT_OK;
}

// 64-byte two-child records, one per inner node: [L.min, ref L][L.max, ref R][R.min, 0][R.max, 0].  wn names leaves by their rows of the triangle array.
void pack_two_child(const Tree &t, std::vector<float> &wn, std::vector<float> &wnW) {
    wn.assign((size_t)std::max(t.nInner, 1) * 16, 0.0f);
    for (int i = 0; i < t.nNodes; ++i) {
        if (t.innerIdx[(size_t)i] < 0) continue;
        const float *L = t.box(t.nd[(size_t)i].left), *R = t.box(t.nd[(size_t)i].right);
        float *o = &wn[(size_t)t.innerIdx[(size_t)i] * 16];
        int rl = t.refOf(t.nd[(size_t)i].left), rr = t.refOf(t.nd[(size_t)i].right);
        o[0] = L[0]; o[1] = L[1]; o[2] = L[2]; std::memcpy(&o[3], &rl, 4);
        o[4] = L[4]; o[5] = L[5]; o[6] = L[6]; std::memcpy(&o[7], &rr, 4);
        o[8] = R[0]; o[9] = R[1]; o[10] = R[2];
        o[12] = R[4]; o[13] = R[5]; o[14] = R[6];
    }
    wnW = wn;   // the same records with pair-record leaf references (wavefront closest-hit kernels)
    for (int i = 0; i < t.nNodes; ++i) {
        if (t.innerIdx[(size_t)i] < 0) continue;
        float *o = &wnW[(size_t)t.innerIdx[(size_t)i] * 16];
        int rl = t.refOfW(t.nd[(size_t)i].left), rr = t.refOfW(t.nd[(size_t)i].right);
        std::memcpy(&o[3], &rl, 4);
        std::memcpy(&o[7], &rr, 4);
    }
}

// depth of the tree (iterative), bounds the traversal stack: one deferred sibling per level
int tree_depth(const Tree &t, int &depth, std::string &err) {
    depth = 0;
    std::vector<std::pair<int, int>> st{{0, 1}};
    size_t visited = 0;
    while (!st.empty()) {
        auto [n, d] = st.back();
        st.pop_back();
        if (++visited > (size_t)t.nNodes) return fail(err, RT_ERR_INVALID, "rt_upload_bvh: node links form a cycle");
        depth = std::max(depth, d);
        if (!t.leaf(n)) { st.push_back({t.nd[(size_t)n].left, d + 1}); st.push_back({t.nd[(size_t)n].right, d + 1}); }
    }
    if (depth > 32) return fail(err, RT_ERR_UNSUPPORTED, "rt_upload_bvh: tree depth %d exceeds the 32-entry traversal stack", depth);
    return RT_OK;
}

// child i of a four-wide record: its box component-wise, its reference in piece 6
void put_child4(float *o, int i, const float *lo, const float *hi, int ref) {
    // SoA: [min.x x4][min.y x4][min.z x4][max.x x4][max.y x4][max.z x4][ref x4][-]
    // absent child (lo == null): NaN box -- (NaN - ro) * rdInv = NaN, v_min/v_max drop NaN operands, tmax = NaN, and
    // "tmax >= tmin" is false, so the traversal kernel needs no child-present branch
    for (int a = 0; a < 3; ++a) { o[4 * a + i] = lo ? lo[a] : kQnan; o[12 + 4 * a + i] = hi ? hi[a] : kQnan; }
    std::memcpy(&o[24 + i], &ref, 4);
}

// The binary tree collapsed to four children (collapse_to_four, rt_scene_pack.hpp), as 128-byte records.  A single-leaf root has no four-wide tree:
// one empty record, and the root reference names the leaf.
void pack_four_wide(const Tree &t, std::vector<float> &w4, int &rootRef4) {
    rootRef4 = t.refOfW(0);
    if (t.leaf(0)) { w4.assign(32, 0.0f); return; }
    rootRef4 = 0;
    const std::vector<Wide4> c4 = collapse_to_four([&](int i) { return t.nd[(size_t)i].left; }, [&](int i) { return t.nd[(size_t)i].right; },
                                                   [&](int i) { return t.nd[(size_t)i].count; }, [&](int i) { return t.refOfW(i); });
    w4.assign(c4.size() * 32, 0.0f);
    for (size_t nn = 0; nn < c4.size(); ++nn)
        for (int i = 0; i < 4; ++i) {
            const float *b = c4[nn].kid[i] >= 0 ? t.box(c4[nn].kid[i]) : nullptr;
            put_child4(&w4[nn * 32], i, b, b ? b + 4 : nullptr, c4[nn].ref[i]);
        }
}

// EXPERIMENT (RT_ANYHIT_TREE=sah): any-hit answers do not depend on the tree, only on which reference leaves pass their own
// exact box test -- so the 4-wide tree may be ANY tree over the reference's leaves whose inner boxes contain their leaves' boxes.  Binned SAH
// (16 bins, cost = area x triangles) over the leaves, collapsed to four children by pulling up the child of largest area.  Off by default: it
// needs more node visits than the collapse of the balanced median-split tree on the bench mesh.
// Returns whether s4 holds the tree (false: deeper than the any-hit stack allows; the collapsed tree stays).
bool pack_four_wide_sah(const Tree &t, std::vector<float> &s4) {
    struct Leaf { float lo[3], hi[3], cen[3]; int ref; float w; };
    std::vector<Leaf> leaves;
    for (int i = 0; i < t.nNodes; ++i) if (t.leaf(i)) {
        Leaf L;
        const float *b = t.box(i);
        for (int a = 0; a < 3; ++a) { L.lo[a] = b[a]; L.hi[a] = b[4 + a]; L.cen[a] = 0.5f * (b[a] + b[4 + a]); }
        L.ref = t.refOfW(i); L.w = (float)t.nd[(size_t)i].count;
        leaves.push_back(L);
    }
    struct BNode { float lo[3], hi[3]; int left, right, leaf; };
    std::vector<BNode> B;
    std::vector<int> ids(leaves.size());
    for (size_t i = 0; i < ids.size(); ++i) ids[i] = (int)i;
    auto area = [](const float *lo, const float *hi) { float ex = std::max(hi[0] - lo[0], 0.0f), ey = std::max(hi[1] - lo[1], 0.0f), ez = std::max(hi[2] - lo[2], 0.0f); return 2.0f * (ex * ey + ey * ez + ez * ex); };
    struct Job { int begin, end, node, depth; };
    std::vector<Job> todo;
    B.push_back(BNode{});
    todo.push_back({0, (int)ids.size(), 0, 0});
    constexpr int NB = 16;
    while (!todo.empty()) {
        const Job jb = todo.back();
        todo.pop_back();
        BNode bn{};
        for (int a = 0; a < 3; ++a) { bn.lo[a] = 3.0e38f; bn.hi[a] = -3.0e38f; }
        float clo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, chi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
        for (int i = jb.begin; i < jb.end; ++i) {
            const Leaf &L = leaves[(size_t)ids[(size_t)i]];
            for (int a = 0; a < 3; ++a) { bn.lo[a] = std::min(bn.lo[a], L.lo[a]); bn.hi[a] = std::max(bn.hi[a], L.hi[a]); clo[a] = std::min(clo[a], L.cen[a]); chi[a] = std::max(chi[a], L.cen[a]); }
        }
        bn.left = bn.right = -1; bn.leaf = -1;
        if (jb.end - jb.begin == 1) { bn.leaf = ids[(size_t)jb.begin]; B[(size_t)jb.node] = bn; continue; }
        int bestAxis = -1, bestSplit = -1;
        float bestCost = 3.0e38f;
        for (int a = 0; a < 3 && jb.depth < 40; ++a) {
            const float ext = chi[a] - clo[a];
            if (!(ext > 0.0f)) continue;
            float blo[NB][3], bhi[NB][3], bw[NB];
            for (int k = 0; k < NB; ++k) { bw[k] = 0.0f; for (int q = 0; q < 3; ++q) { blo[k][q] = 3.0e38f; bhi[k][q] = -3.0e38f; } }
            for (int i = jb.begin; i < jb.end; ++i) {
                const Leaf &L = leaves[(size_t)ids[(size_t)i]];
                const int k = std::min(NB - 1, (int)((L.cen[a] - clo[a]) / ext * NB));
                bw[k] += L.w;
                for (int q = 0; q < 3; ++q) { blo[k][q] = std::min(blo[k][q], L.lo[q]); bhi[k][q] = std::max(bhi[k][q], L.hi[q]); }
            }
            float rlo[NB][3], rhi[NB][3], rw[NB];
            float alo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, ahi[3] = {-3.0e38f, -3.0e38f, -3.0e38f}, aw = 0.0f;
            for (int k = NB - 1; k >= 0; --k) {
                aw += bw[k];
                for (int q = 0; q < 3; ++q) { alo[q] = std::min(alo[q], blo[k][q]); ahi[q] = std::max(ahi[q], bhi[k][q]); rlo[k][q] = alo[q]; rhi[k][q] = ahi[q]; }
                rw[k] = aw;
            }
            float llo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, lhi[3] = {-3.0e38f, -3.0e38f, -3.0e38f}, lw = 0.0f;
            for (int k = 0; k + 1 < NB; ++k) {
                lw += bw[k];
                for (int q = 0; q < 3; ++q) { llo[q] = std::min(llo[q], blo[k][q]); lhi[q] = std::max(lhi[q], bhi[k][q]); }
                if (lw == 0.0f || rw[k + 1] == 0.0f) continue;
                const float cost = area(llo, lhi) * lw + area(rlo[k + 1], rhi[k + 1]) * rw[k + 1];
                if (cost < bestCost) { bestCost = cost; bestAxis = a; bestSplit = k; }
            }
        }
        int mid;
        if (bestAxis < 0) {   // degenerate centroids or the depth cap: median by index
            mid = (jb.begin + jb.end) / 2;
        } else {
            const float ext = chi[bestAxis] - clo[bestAxis];
            auto it = std::partition(ids.begin() + jb.begin, ids.begin() + jb.end, [&](int id) {
                return std::min(NB - 1, (int)((leaves[(size_t)id].cen[bestAxis] - clo[bestAxis]) / ext * NB)) <= bestSplit; });
            mid = (int)(it - ids.begin());
            if (mid == jb.begin || mid == jb.end) mid = (jb.begin + jb.end) / 2;
        }
        bn.left = (int)B.size(); B.push_back(BNode{});
        bn.right = (int)B.size(); B.push_back(BNode{});
        B[(size_t)jb.node] = bn;
        todo.push_back({jb.begin, mid, bn.left, jb.depth + 1});
        todo.push_back({mid, jb.end, bn.right, jb.depth + 1});
    }
    // collapse to four children
    s4.assign(32, 0.0f);
    struct J4 { int bin; size_t at; int depth; };
    std::vector<J4> jobs4{{0, 0, 1}};
    int depth4 = 1;
    while (!jobs4.empty()) {
        const J4 jb = jobs4.back();
        jobs4.pop_back();
        depth4 = std::max(depth4, jb.depth);
        std::vector<int> kids{B[(size_t)jb.bin].left, B[(size_t)jb.bin].right};
        while (kids.size() < 4) {
            int pick = -1;
            float best = -1.0f;
            for (size_t i = 0; i < kids.size(); ++i) if (B[(size_t)kids[i]].leaf < 0) { const float ar = area(B[(size_t)kids[i]].lo, B[(size_t)kids[i]].hi); if (ar > best) { best = ar; pick = (int)i; } }
            if (pick < 0) break;
            const int k = kids[(size_t)pick];
            kids.erase(kids.begin() + pick);
            kids.push_back(B[(size_t)k].left); kids.push_back(B[(size_t)k].right);
        }
        for (int i = 0; i < 4; ++i) {
            if (i >= (int)kids.size()) { put_child4(&s4[jb.at * 32], i, nullptr, nullptr, RT_NO_CHILD); continue; }
            const BNode &kb = B[(size_t)kids[(size_t)i]];
            int ref;
            if (kb.leaf >= 0) ref = leaves[(size_t)kb.leaf].ref;
            else { ref = (int)(s4.size() / 32); s4.resize(s4.size() + 32, 0.0f); jobs4.push_back({kids[(size_t)i], (size_t)ref, jb.depth + 1}); }
            // a leaf child carries the reference's exact leaf box (the test that decides which triangles are tested); an inner child the union of its leaves' boxes
            const float *lo = kb.leaf >= 0 ? leaves[(size_t)kb.leaf].lo : kb.lo, *hi = kb.leaf >= 0 ? leaves[(size_t)kb.leaf].hi : kb.hi;
            put_child4(&s4[jb.at * 32], i, lo, hi, ref);
        }
    }
    return 3 * depth4 <= 60;
}

int ref_of4(const std::vector<float> &w4, size_t node, int i) {
    int ref;
    std::memcpy(&ref, &w4[node * 32 + 24 + (size_t)i], 4);
    return ref;
}

// Round 4: the any-hit tree once more with QUANTISED child boxes -- 64 bytes per 4-wide node instead of 112, four gather loads per
// visit instead of seven.  Only the reference's LEAVES need their exact boxes (an any-hit answer is the OR over the leaves that pass their own box test);
// an inner box may be any box that contains them, and the slab arithmetic is monotonic in the box, so a decoded box that is checked HERE, in the very
// float expression the kernel decodes with (fmaf(q, 2^e, origin)), to contain the child's box passes whenever the child's does.  A leaf child passes
// the quantised test first and its exact box -- kept in `leafBox`, indexed from the leaf's first pair record (below) -- in the leaf phase.
// Built (and walked: rt_trace_build.cpp trace_build, rt_trace.hpp launch_trace) when the 112-byte nodes outgrow one XCD's 4 MB L2 (kQNodesAbove): the decode costs 48 VALU operations per
// visit and a wave per SIMD, which a cache-resident tree does not earn back -- any-hit launch per frame, exact / quantised nodes, one launch set in flight:
// 20 k triangles 0.57 / 0.63-0.66 ms, 82 k (bench mesh, 0.6 MB of nodes) 0.66 / 0.74, 328 k (2.4 MB) 0.81 / 0.83-0.84, 1 M (9.8 MB) 15.9 / 13.6
// (profiles/r04_experiments.txt 19).  RT_QNODES=0 / 2 forces either.
//   piece 0: origin.xyz (float), biased exponents ex | ey << 8 | ez << 16       piece 1: lo.x lo.y lo.z hi.x, one byte per child
//   piece 2: hi.y hi.z - -                                                       piece 3: the four child references of the 112-byte node
bool quantise_four_wide(const std::vector<float> &w4, std::vector<uint32_t> &q4) {
    const size_t n4 = w4.size() / 32;
    q4.assign(n4 * 16, 0u);
    for (size_t nn = 0; nn < n4; ++nn) {
        int refs[4];
        std::memcpy(refs, &w4[nn * 32 + 24], 16);
        if (!rt_quantise_node4(&w4[nn * 32], refs, &q4[nn * 16])) return false;
        std::memcpy(&q4[nn * 16 + 12], refs, 16);
    }
    return true;
}

// The leaves' exact boxes for the quantised walk, placed by LeafBoxRule (rt_scene_pack.hpp).
bool pack_leaf_boxes(const Tree &t, const PackOptions &opt, size_t pairRecords, PackedScene &s) {
    int rmin = 8;
    for (int i = 0; i < t.nNodes; ++i) if (t.leaf(i)) rmin = std::min(rmin, (t.nd[(size_t)i].count + 1) / 2);
    const LeafBoxRule rule(rmin, opt.sparseLeafBoxes);
    s.leafBoxMagic = rule.magic;
    s.leafBox.assign(rule.floats(pairRecords), 0.0f);
    std::vector<char> taken(s.leafBox.size() / 8, 0);   // (host only: nothing but boxes is uploaded)
    s.nLeafBoxes = 0;
    for (int i = 0; i < t.nNodes; ++i) if (t.leaf(i)) {
        ++s.nLeafBoxes;
        const size_t at = rule.index((size_t)(-t.pairRefOf[(size_t)i] - 1) >> 3);
        const float *b = t.box(i);
        const float box[8] = {b[0], b[1], b[2], b[4], b[5], b[6], 0.0f, 0.0f};
        if (at * 8 + 8 > s.leafBox.size() || taken[at]) return false;   // (cannot happen: distinct quotients)
        std::memcpy(&s.leafBox[at * 8], box, sizeof box);
        taken[at] = 1;
    }
    return true;
}

// Round 5 -- fused closest-hit records.  The closest-hit walk must keep the reference's visiting order (rt_bvh.glsl:205-241: near child first, far
// child behind the pop-time cull; ties and triangles a rounding in front of their leaf box make the answer depend on it), but nothing says it
// must spend one dependent memory round trip per binary node.  Whenever the walk enters a child X of a node N it visits X next, and X's record (the
// boxes of X's children) is known as soon as N's index is -- so the records of N's two children are stored TOGETHER under N's index, 128 bytes = one
// cache line per even-level inner node N ("hub"):
//     pieces 0-3: [A1.min, ref A1] [A1.max, ref A2] [A2.min, -] [A2.max, -]      A = N.left,  A1 / A2 = A's children
//     pieces 4-7: the same for B = N.right
// A leaf child X is stored as a half with ONE box: [X.min, leaf ref] [X.max, RT_NO_CHILD] [NaN box].  References are hub indices (>= 0) or the pair-record
// leaf codes of wnodesW (< 0).  The kernel (k_trace<.., FUSE>) fetches the eight pieces in one round trip and makes the reference's two steps from them:
// the step at N needs the boxes of A and B themselves, which are not stored -- they are the unions of their children's boxes, and the slab values of a
// union follow from the children's by min / max (per axis: tsm = min(tsm1, tsm2), tbg = max(tbg1, tbg2); tests/test_fused_nodes.py pins that identity
// against the slab test of the union box, signed zeros, infinities and the NaN of 0 * inf included).  That needs every inner box to BE the union of its children's, bit for bit --
// true of the reference's builder (bounds over a range = the union of the bounds over its halves, bvh.cpp:41-60) and of rt_build_bvh_gpu, checked
// here for whatever was uploaded; a tree that fails the check keeps the 64-byte records (RT_SCENE_NOT_FUSED in RtSceneInfo.flags).
// Built only where the option is on (both forms are measured options, off by default: no second and third copy of the tree in device memory otherwise).
bool pack_fused(const Tree &t, std::vector<float> &wF) {
    for (int i = 0; i < t.nNodes; ++i) {
        if (t.leaf(i)) continue;
        const float *P = t.box(i), *L = t.box(t.nd[(size_t)i].left), *R = t.box(t.nd[(size_t)i].right);
        for (int a = 0; a < 3; ++a)
            if (!(P[a] == std::min(L[a], R[a])) || !(P[4 + a] == std::max(L[4 + a], R[4 + a]))) return false;
    }
    struct Job { int bin; size_t at; };
    std::vector<Job> jobs{{0, 0}};
    wF.assign(32, 0.0f);
    while (!jobs.empty()) {
        const Job jb = jobs.back();
        jobs.pop_back();
        for (int h = 0; h < 2; ++h) {
            const int X = h == 0 ? t.nd[(size_t)jb.bin].left : t.nd[(size_t)jb.bin].right;
            int kids[2] = {X, -1};
            if (!t.leaf(X)) { kids[0] = t.nd[(size_t)X].left; kids[1] = t.nd[(size_t)X].right; }
            int refs[2] = {RT_NO_CHILD, RT_NO_CHILD};
            for (int k = 0; k < 2; ++k) {
                float box[6] = {kQnan, kQnan, kQnan, kQnan, kQnan, kQnan};
                if (kids[k] >= 0) {
                    const float *b = t.box(kids[k]);
                    box[0] = b[0]; box[1] = b[1]; box[2] = b[2]; box[3] = b[4]; box[4] = b[5]; box[5] = b[6];
                    if (t.leaf(kids[k])) refs[k] = t.refOfW(kids[k]);
                    else {
                        refs[k] = (int)(wF.size() / 32);
                        if ((size_t)refs[k] >= ((size_t)1 << 29)) { wF.clear(); return false; }
                        wF.resize(wF.size() + 32, 0.0f);
                        jobs.push_back({kids[k], (size_t)refs[k]});
                    }
                }
                float *o = &wF[jb.at * 32 + (size_t)h * 16 + (size_t)k * 8];
                o[0] = box[0]; o[1] = box[1]; o[2] = box[2]; o[4] = box[3]; o[5] = box[4]; o[6] = box[5];
            }
            float *o = &wF[jb.at * 32 + (size_t)h * 16];
            std::memcpy(&o[3], &refs[0], 4);
            std::memcpy(&o[7], &refs[1], 4);
        }
    }
    return true;
}

// Round 5 -- implicit records.  What the traversal launches cost is their 16-byte lane-loads (one vector-L1 lookup each), and a 64-byte
// two-child record spends one of its four on two child references.  The reference's builder splits every range at its middle and stops at <= 8 triangles
// (bvh.cpp:62-76), so whenever n / 2^D falls into [4.5, 8] for some D every leaf sits at depth D and the tree is a perfect binary tree: a node is named by
// (depth d, path p = the left / right turns from the root as a binary number), its children are (d + 1, 2p) and (d + 1, 2p + 1), the leaves are p = 0 ..
// 2^D - 1 at depth D -- no reference needs to be stored.  Records: 48 bytes = the two child boxes = THREE loads, at the node's pre-order position
// d - popcount(p) + (p << (D - d)) (a left child sits next to its parent, as in the reference's own numbering); a leaf's triangle-pair records at
// p * R (R = the most records any leaf owns), the leaf's triangle count in the spare word of its first record.  Visiting order, boxes and triangle tests
// are those of the 64-byte records.  Checked here for whatever tree was uploaded (all leaves at one depth <= 23); others keep the explicit records.
void pack_implicit(const Tree &t, PackedScene &s) {
    struct E { int node; int d; uint32_t p; };
    std::vector<E> st{{0, 0, 0u}};
    std::vector<int> nodeD((size_t)t.nNodes, -1);
    std::vector<uint32_t> nodeP((size_t)t.nNodes, 0u);
    int leafDepth = -1, maxRec = 0;
    bool uniform = true;
    while (!st.empty() && uniform) {
        const E e = st.back();
        st.pop_back();
        nodeD[(size_t)e.node] = e.d; nodeP[(size_t)e.node] = e.p;
        const N &n = t.nd[(size_t)e.node];
        if (n.count > 0) {
            if (leafDepth < 0) leafDepth = e.d;
            if (e.d != leafDepth) uniform = false;
            maxRec = std::max(maxRec, (n.count + 1) / 2);
        } else {
            if (e.d >= 23) { uniform = false; break; }
            st.push_back({n.left, e.d + 1, e.p * 2u});
            st.push_back({n.right, e.d + 1, e.p * 2u + 1u});
        }
    }
    if (!uniform || leafDepth < 1) return;
    const int D = leafDepth;
    auto slot = [D](int d, uint32_t p) { return (size_t)d - (size_t)__builtin_popcount(p) + ((size_t)p << (D - d)); };
    s.iN2.assign((((size_t)1 << D) - 1) * 12, 0.0f);
    s.iPairs.assign((((size_t)1 << D) * (size_t)maxRec + 8) * 20, 0.0f);
    for (int i = 0; i < t.nNodes; ++i) {
        if (nodeD[(size_t)i] < 0) continue;             // (unreachable nodes: none in a valid tree)
        const N &n = t.nd[(size_t)i];
        const uint32_t pth = nodeP[(size_t)i];
        if (n.count <= 0) {
            const float *L = t.box(n.left), *R = t.box(n.right);
            const float rec[12] = {L[0], L[1], L[2], L[4], L[5], L[6], R[0], R[1], R[2], R[4], R[5], R[6]};
            std::memcpy(&s.iN2[slot(nodeD[(size_t)i], pth) * 12], rec, sizeof rec);
        } else {
            // the leaf's records as `pairs` holds them, at p * R; the count in the spare word of the first
            const size_t src = (size_t)(-t.pairRefOf[(size_t)i] - 1) >> 3, nrec = (size_t)(n.count + 1) / 2;
            float *o = &s.iPairs[(size_t)pth * (size_t)maxRec * 20];
            std::memcpy(o, &s.pairs[src * 20], nrec * 20 * sizeof(float));
            const uint32_t cnt = (uint32_t)n.count;
            std::memcpy(&o[19], &cnt, 4);
        }
    }
    s.implD = D; s.implR = maxRec;
    // ... and the any-hit walk's four-wide records in the same naming: an even-depth node (d, p) has the children (d + 2, 4p + j), j = 0..3 (or, when d + 1 == D,
    // the two leaves 2p, 2p + 1), so the record is the four child boxes alone, component-wise: 96 bytes, SIX loads instead of seven, at the node's own
    // pre-order position (odd-depth slots of the array stay empty and are never touched).  Where the quantised form is walked (trees beyond the L2) the same
    // record in bytes: [origin.xyz, exponents] [lo.x lo.y lo.z hi.x] [hi.y hi.z - -] = 48 bytes, THREE loads instead of four, and the leaves' exact boxes at
    // their ordinal p.
    const bool wantQ = !s.q4.empty();
    s.iN4.assign((((size_t)1 << D) - 1) * 24, 0.0f);
    if (wantQ) { s.iQ4.assign((((size_t)1 << D) - 1) * 12, 0u); s.iLeafBox.assign(((size_t)1 << D) * 8, 0.0f); }
    bool okI = true;
    for (int i = 0; i < t.nNodes && okI; ++i) {
        const int d = nodeD[(size_t)i];
        if (d < 0) continue;
        const N &n = t.nd[(size_t)i];
        const uint32_t pth = nodeP[(size_t)i];
        if (n.count > 0) {
            if (wantQ) { const float *b = t.box(i); const float box[8] = {b[0], b[1], b[2], b[4], b[5], b[6], 0.0f, 0.0f}; std::memcpy(&s.iLeafBox[(size_t)pth * 8], box, sizeof box); }
            continue;
        }
        if (d & 1) continue;
        int kids[4] = {-1, -1, -1, -1};
        if (d + 1 == D) { kids[0] = n.left; kids[1] = n.right; }
        else { kids[0] = t.nd[(size_t)n.left].left; kids[1] = t.nd[(size_t)n.left].right; kids[2] = t.nd[(size_t)n.right].left; kids[3] = t.nd[(size_t)n.right].right; }
        const size_t at = slot(d, pth);
        float *o = &s.iN4[at * 24];
        int present[4];
        for (int k = 0; k < 4; ++k) {
            const float *b = kids[k] >= 0 ? t.box(kids[k]) : nullptr;
            for (int a = 0; a < 3; ++a) { o[4 * a + k] = b ? b[a] : kQnan; o[12 + 4 * a + k] = b ? b[4 + a] : kQnan; }
            present[k] = kids[k] >= 0 ? 0 : RT_NO_CHILD;
        }
        // quantise as the explicit form does (rt_qnode.hpp)
        if (wantQ) okI = rt_quantise_node4(o, present, &s.iQ4[at * 12]);
    }
    if (!okI) { s.iQ4.clear(); s.iLeafBox.clear(); }      // (the explicit quantised form passed the same checks, so this does not happen)
}

}  // namespace

int pack_scene(const float *nodes12, int nNodes, const float *tris12, int nTris, const PackOptions &opt, PackedScene &s, std::string &err) {
    s = PackedScene{};
    if (nTris >= (1 << 28)) return fail(err, RT_ERR_UNSUPPORTED, "rt_upload_bvh: %d triangles exceed the 2^28 leaf encoding", nTris);
    Tree t{nodes12, tris12, nNodes, nTris};
    if (int rc = decode_links(t, err)) return rc;
    if (int rc = pack_pairs(t, s.pairs, err)) return rc;
    pack_two_child(t, s.wn, s.wnW);
    if (int rc = tree_depth(t, s.depth, err)) return rc;
    pack_four_wide(t, s.w4, s.rootRef4);
    if (opt.anyhitSah && !t.leaf(0)) {
        std::vector<float> s4;
        if (pack_four_wide_sah(t, s4)) { s.w4.swap(s4); s.collapsed4 = false; }   // not the binary tree collapsed: no bounce probe
    }
    if (s.rootRef4 == 0) s.anyStack = any_stack_need(s.w4.size() / 32, [&](size_t nn, int i) { return ref_of4(s.w4, nn, i); });
    if (want_quantised(opt, s.w4.size() / 32, s.rootRef4)) {
        if (!quantise_four_wide(s.w4, s.q4) || !pack_leaf_boxes(t, opt, s.pairs.size() / 20, s)) {
            // asked for and not built: say so instead of falling back silently
            s.q4.clear(); s.leafBox.clear(); s.leafBoxMagic = 0; s.nLeafBoxes = 0;
            s.flags |= RT_SCENE_QNODES_REJECTED;
            if (opt.verbose) fprintf(stderr, "[rt_upload_bvh] quantised any-hit nodes rejected (exponent range or leaf-box index collision): walking the exact 112-byte nodes\n");
        }
    }
    if (opt.fused && !t.leaf(0) && !pack_fused(t, s.wF)) { s.wF.clear(); s.flags |= RT_SCENE_NOT_FUSED; }
    if (opt.implicit && !t.leaf(0)) pack_implicit(t, s);
    s.nInner = t.nInner;
    s.rootRef = t.refOf(0); s.rootRefW = t.refOfW(0);
    std::memcpy(s.rootMin, nodes12, 12);
    std::memcpy(s.rootMax, nodes12 + 4, 12);
    return RT_OK;
}

}  // namespace rtl
