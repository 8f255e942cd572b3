// The box query's definition (csrc/rt_overlap_query.cpp: rt_box_overlaps) driven over its edge cases under AddressSanitizer + UBSan on the CPU
// (tests/test_box_query_host_sanitizers.py).  Linked with rt_overlap_query.cpp alone.  Every array is exactly as long as the call may read or write: a
// strided box array ends with its last box's sixth float, offsets hold n + 1 entries, prims offsets[n] or n * cap entries (none at all for cap = 0),
// counts n.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "query_sanitize.hpp"
#include "rt_mi355.h"

// n boxes with the given stride in an array that ends with the last box's sixth float; every seventh an empty slot
struct Boxes { std::vector<float> b; int n, stride; };
static Boxes boxes_about(int n, int stride, unsigned seed) {
    Boxes B;
    B.n = n; B.stride = stride;
    B.b.assign((size_t)(n - 1) * stride + 6, 0.0f);
    std::mt19937 r(seed);
    for (int i = 0; i < n; ++i) {
        float *q = &B.b[(size_t)i * stride];
        for (int a = 0; a < 3; ++a) {
            const float c = (float)((int)(r() % 640u) - 320) / 8.0f * (a == 1 ? 0.05f : 1.0f), h = (float)(r() % 200u) / 8.0f;
            q[a] = c - h; q[3 + a] = c + h;
        }
        if (i % 7 == 3) q[4] = q[1] - 1.0f;   // lo > hi
    }
    return B;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const int32_t mark = -77;
    // ---- one leaf: two triangles, no inner node
    Tree one = tree_of({-0.75f, 0.25f, -0.75f, 2, 0, 0, 1, 1.5f, -0.2f, -0.75f, 0.25f, 1.25f, 2, 0, 0, 1, 1.5f, -0.5f});
    CHECK(one.nNodes == 1 && one.nTris == 2);
    // ---- the layer stack: six layers of three coincident copies of a quad, 36 triangles
    std::vector<float> t9;
    for (int k = 0; k < 6; ++k)
        for (int c = 0; c < 3; ++c) {
            const float y = (float)(0.25 * k + 0.1);
            const float edges[2][6] = {{60, 0, 0, 60, 0, 60}, {60, 0, 60, 0, 0, 60}};
            for (const auto &e : edges) {
                t9.insert(t9.end(), {-30.0f, y, -30.0f});
                t9.insert(t9.end(), e, e + 6);
            }
        }
    Tree stack = tree_of(t9);
    CHECK(stack.nTris == 36 && stack.nNodes > 1);
    for (const Tree *T : {&one, &stack})
        for (int stride : {6, 7, 12})
            for (int n : {1, 2, 65}) {
                Boxes B = boxes_about(n, stride, 7u + (unsigned)(stride + n));
                std::vector<int32_t> counts((size_t)n, mark);
                // the counts alone
                CHECK(rt_box_overlaps(T->nodes.data(), T->nNodes, T->tris.data(), T->nTris, B.b.data(), stride, n, nullptr, 0, nullptr, counts.data()) == RT_OK);
                for (int i = 0; i < n; ++i) {
                    CHECK(counts[(size_t)i] >= 0 && counts[(size_t)i] <= T->nTris);
                    if (i % 7 == 3) CHECK(counts[(size_t)i] == 0);
                }
                // the exact list: count, scan, list -- with and without the counts again
                std::vector<int32_t> offsets((size_t)n + 1, 0);
                for (int i = 0; i < n; ++i) offsets[(size_t)i + 1] = offsets[(size_t)i] + counts[(size_t)i];
                for (int withCounts = 0; withCounts < 2; ++withCounts) {
                    std::vector<int32_t> prims((size_t)offsets[(size_t)n], mark), again((size_t)n, mark);
                    // (a vector without elements may hand out any pointer: an empty list array is passed as one spare word no slot reaches)
                    int32_t spare = mark;
                    CHECK(rt_box_overlaps(T->nodes.data(), T->nNodes, T->tris.data(), T->nTris, B.b.data(), stride, n, offsets.data(), 0,
                                          prims.empty() ? &spare : prims.data(), withCounts ? again.data() : nullptr) == RT_OK);
                    CHECK(spare == mark);
                    for (int i = 0; i < n; ++i) {
                        check_slot(*T, prims.data() + offsets[(size_t)i], counts[(size_t)i], counts[(size_t)i], mark);
                        if (withCounts) CHECK(again[(size_t)i] == counts[(size_t)i]);
                    }
                }
                // fixed capacities
                for (int cap : {0, 1, 3, 8}) {
                    std::vector<int32_t> prims((size_t)n * cap, mark), again((size_t)n, mark);
                    int32_t spare = mark;
                    CHECK(rt_box_overlaps(T->nodes.data(), T->nNodes, T->tris.data(), T->nTris, B.b.data(), stride, n, nullptr, cap, cap ? prims.data() : &spare,
                                          again.data()) == RT_OK);
                    CHECK(spare == mark);
                    for (int i = 0; i < n; ++i) {
                        CHECK(again[(size_t)i] == counts[(size_t)i]);
                        check_slot(*T, prims.data() + (size_t)i * cap, cap, counts[(size_t)i], mark);
                    }
                }
            }
    // ---- degenerate boxes: NaN and infinite components, denormals, huge values, lo == hi; a zero-area triangle among the rows
    {
        Tree flat = tree_of({0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1});
        const float sp[] = {nan, inf, -inf, 0.0f, -0.0f, 1e-41f, 3.0f, 3e38f, -3e38f};
        std::vector<float> b;
        for (float a : sp) for (float c : sp) for (float d : sp) for (float e : sp) b.insert(b.end(), {a, c, -1.0f, d, e, d});
        const int n = (int)b.size() / 6, cap = 3;
        std::vector<int32_t> prims((size_t)n * cap), counts((size_t)n);
        for (const Tree *T : {&one, &stack, &flat}) {
            std::fill(prims.begin(), prims.end(), mark);
            std::fill(counts.begin(), counts.end(), mark);
            CHECK(rt_box_overlaps(T->nodes.data(), T->nNodes, T->tris.data(), T->nTris, b.data(), 6, n, nullptr, cap, prims.data(), counts.data()) == RT_OK);
            for (int i = 0; i < n; ++i) {
                const float *q = &b[(size_t)i * 6];
                const bool live = q[0] <= q[3] && q[1] <= q[4] && q[2] <= q[5];
                if (!live) CHECK(counts[(size_t)i] == 0);
                check_slot(*T, prims.data() + (size_t)i * cap, cap, counts[(size_t)i], mark);
            }
        }
        // the box that spans everything lists everything, in walk order: the split by index and the right child first give descending leaves
        const float all[6] = {-inf, -inf, -inf, inf, inf, inf};
        std::vector<int32_t> list((size_t)stack.nTris, mark);
        int32_t count = mark;
        CHECK(rt_box_overlaps(stack.nodes.data(), stack.nNodes, stack.tris.data(), stack.nTris, all, 6, 1, nullptr, stack.nTris, list.data(), &count) == RT_OK);
        CHECK(count == stack.nTris);
        std::vector<int32_t> sorted = list;
        std::sort(sorted.begin(), sorted.end());
        for (int i = 0; i < stack.nTris; ++i) CHECK(sorted[(size_t)i] == i);
        CHECK(list[0] > list[(size_t)stack.nTris - 1]);
    }
    // ---- slots of negative length or with a negative start hold nothing
    {
        Boxes B = boxes_about(5, 6, 3u);
        const int32_t odd[6] = {3, 1, 1, -5, 2, 2};
        int32_t prims[4] = {mark, mark, mark, mark}, counts[5];
        CHECK(rt_box_overlaps(stack.nodes.data(), stack.nNodes, stack.tris.data(), stack.nTris, B.b.data(), 6, 5, odd, 0, prims, counts) == RT_OK);
        CHECK(prims[0] == mark && prims[1] == mark && prims[2] == mark && prims[3] == mark);
    }
    // ---- refusals: nothing is read or written
    {
        Boxes B = boxes_about(2, 6, 1u);
        int32_t prims[8], cnt[2] = {mark, mark};
        const int32_t off[3] = {0, 4, 8};
        std::fill(prims, prims + 8, mark);
        auto call = [&](const Tree &T, int n, int stride, const float *b, const int32_t *o, int cap, int32_t *p, int32_t *c) {
            return rt_box_overlaps(T.nodes.data(), T.nNodes, T.tris.data(), T.nTris, b, stride, n, o, cap, p, c);
        };
        CHECK(call(stack, -1, 6, B.b.data(), off, 0, prims, cnt) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 5, B.b.data(), off, 0, prims, cnt) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 6, nullptr, off, 0, prims, cnt) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 6, B.b.data(), off, 0, nullptr, nullptr) == RT_ERR_INVALID);          // prims and counts both NULL
        CHECK(call(stack, 2, 6, B.b.data(), nullptr, -1, prims, cnt) == RT_ERR_INVALID);            // prims without offsets, cap < 0
        CHECK(call(stack, INT_MAX / 4 + 1, 6, B.b.data(), nullptr, 4, prims, cnt) == RT_ERR_INVALID);   // n * cap beyond INT32_MAX
        CHECK(call(stack, 0, 6, nullptr, nullptr, 0, nullptr, nullptr) == RT_OK);                   // n == 0: a no-op
        CHECK(rt_box_overlaps(nullptr, stack.nNodes, stack.tris.data(), stack.nTris, B.b.data(), 6, 2, off, 0, prims, cnt) == RT_ERR_INVALID);
        CHECK(rt_box_overlaps(stack.nodes.data(), stack.nNodes, nullptr, stack.nTris, B.b.data(), 6, 2, off, 0, prims, cnt) == RT_ERR_INVALID);
        CHECK(rt_box_overlaps(stack.nodes.data(), -1, stack.tris.data(), stack.nTris, B.b.data(), 6, 2, off, 0, prims, cnt) == RT_ERR_INVALID);
        // nodes that are no tree over the rows: a child off the array, a cycle, a range beyond the rows, huge and NaN links
        for (float link : {-1.0f, 1e9f, nan, (float)stack.nNodes, 0.0f}) {
            Tree bad = stack;
            bad.nodes[3] = link;
            CHECK(call(bad, 2, 6, B.b.data(), off, 0, prims, cnt) == RT_ERR_INVALID);
        }
        Tree bad = one;
        bad.nodes[9] = 3.0f;
        CHECK(call(bad, 2, 6, B.b.data(), off, 0, prims, cnt) == RT_ERR_INVALID);
        bad.nodes[8] = 2e9f; bad.nodes[9] = 1.0f;
        CHECK(call(bad, 2, 6, B.b.data(), off, 0, prims, cnt) == RT_ERR_INVALID);
        CHECK(cnt[0] == mark && cnt[1] == mark && std::all_of(prims, prims + 8, [&](int32_t v) { return v == mark; }));
        // an empty scene overlaps nothing
        CHECK(rt_box_overlaps(nullptr, 0, nullptr, 0, B.b.data(), 6, 2, off, 0, prims, cnt) == RT_OK && cnt[0] == 0 && cnt[1] == 0 && prims[0] == mark);
    }
    if (g_fail) { std::printf("box query host: %d checks FAILED\n", g_fail); return 1; }
    std::printf("box query host: all checks passed\n");
    return 0;
}
