// The hull query's definition (csrc/rt_overlap_query.cpp: rt_hull_overlaps) and the corner makers (csrc/rt_hull_corners.cpp: rt_box_corners,
// rt_rect_frusta) driven over their edge cases under AddressSanitizer + UBSan on the CPU (tests/test_hull_query_host_sanitizers.py).  Linked with those
// two files alone.  Every array is exactly as long as the call may read or write: a strided query array ends with its last hull's 24th float (a box
// array with its last box's sixth, a rect array with its last rect's fourth), offsets hold n + 1 entries, prims offsets[n] or n * cap entries (none at
// all for cap = 0), counts n, corners n * 24.
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

// n hulls with the given stride in an array that ends with the last hull's 24th float: sheared boxes about random centres; every seventh an empty
// slot (a NaN that rotates through the 24 floats)
struct Queries { std::vector<float> q; int n, stride; };
static Queries queries_about(int n, int stride, unsigned seed) {
    Queries Q;
    Q.n = n; Q.stride = stride;
    Q.q.assign((size_t)(n - 1) * stride + 24, 0.0f);
    std::mt19937 r(seed);
    auto unit = [&]() { return (float)(r() % 65u) / 32.0f - 1.0f; };
    for (int i = 0; i < n; ++i) {
        float *q = &Q.q[(size_t)i * stride];
        float c[3], ax[3][3];
        for (int a = 0; a < 3; ++a) c[a] = (float)((int)(r() % 640u) - 320) / 8.0f * (a == 1 ? 0.05f : 1.0f);
        const float h = (float)(r() % 200u) / 8.0f;
        for (auto &v : ax)
            for (float &x : v) x = h * unit();
        for (int k = 0; k < 8; ++k)
            for (int a = 0; a < 3; ++a) q[3 * k + a] = c[a] + ((k & 1) ? ax[0][a] : -ax[0][a]) + ((k & 2) ? ax[1][a] : -ax[1][a]) + ((k & 4) ? ax[2][a] : -ax[2][a]);
        if (i % 7 == 3) q[(i / 7) % 24] = std::numeric_limits<float>::quiet_NaN();
    }
    return Q;
}

static int hulls(const Tree &T, const float *q, int stride, int n, const int32_t *o, int cap, int32_t *p, int32_t *c) {
    return rt_hull_overlaps(T.nodes.data(), T.nNodes, T.tris.data(), T.nTris, q, stride, n, o, cap, p, c);
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
        for (int stride : {24, 25, 32})
            for (int n : {1, 2, 65}) {
                Queries Q = queries_about(n, stride, 7u + (unsigned)(stride + n));
                std::vector<int32_t> counts((size_t)n, mark);
                // the counts alone
                CHECK(hulls(*T, Q.q.data(), stride, n, nullptr, 0, nullptr, counts.data()) == RT_OK);
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
                    CHECK(hulls(*T, Q.q.data(), stride, n, offsets.data(), 0, prims.empty() ? &spare : prims.data(), withCounts ? again.data() : nullptr) == RT_OK);
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
                    CHECK(hulls(*T, Q.q.data(), stride, n, nullptr, cap, cap ? prims.data() : &spare, again.data()) == RT_OK);
                    CHECK(spare == mark);
                    for (int i = 0; i < n; ++i) {
                        CHECK(again[(size_t)i] == counts[(size_t)i]);
                        check_slot(*T, prims.data() + (size_t)i * cap, cap, counts[(size_t)i], mark);
                    }
                }
            }
    // ---- degenerate hulls: NaN and infinite components, denormals, huge values; collapsed to a quad, a segment and a point; zero-area rows
    {
        Tree flat = tree_of({0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1});
        const float sp[] = {nan, inf, -inf, 0.0f, -0.0f, 1e-41f, 3.0f, 3e38f, -3e38f};
        std::vector<float> b;
        for (float a : sp) for (float c : sp) for (float d : sp) for (float e : sp)
            b.insert(b.end(), {a, c, -1.0f, d, c, -1.0f, a, e, -1.0f, d, e, -1.0f, a, c, 0.25f, d, c, e, a, e, 0.25f, d, e, a});
        for (float a : sp) for (float c : sp) for (int k = 0; k < 8; ++k) b.insert(b.end(), {a, c, a});                                   // points
        for (float a : sp) for (float c : sp) for (int k = 0; k < 8; ++k) b.insert(b.end(), {k & 4 ? a : c, 0.25f, k & 4 ? c : a});       // segments
        for (float a : sp) for (float c : sp) for (int k = 0; k < 8; ++k) b.insert(b.end(), {k & 1 ? a : -1.0f, k & 2 ? c : 0.0f, 0.1f});  // quads
        const int n = (int)b.size() / 24, cap = 3;
        std::vector<int32_t> prims((size_t)n * cap), counts((size_t)n);
        for (const Tree *T : {&one, &stack, &flat}) {
            std::fill(prims.begin(), prims.end(), mark);
            std::fill(counts.begin(), counts.end(), mark);
            CHECK(hulls(*T, b.data(), 24, n, nullptr, cap, prims.data(), counts.data()) == RT_OK);
            for (int i = 0; i < n; ++i) {
                const float *q = &b[(size_t)i * 24];
                bool live = true;
                for (int k = 0; k < 24; ++k) live = live && q[k] == q[k];
                if (!live) CHECK(counts[(size_t)i] == 0);
                check_slot(*T, prims.data() + (size_t)i * cap, cap, counts[(size_t)i], mark);
            }
        }
        // a hull collapsed to a row's own point lists that row, a zero-area row and a point row included
        for (int t = 0; t < flat.nTris; ++t)
            for (int v = 0; v < 3; ++v) {
                const float *r = &flat.tris[(size_t)t * 12];
                const float p[3] = {v ? r[0] + r[4 * v] : r[0], v ? r[1] + r[4 * v + 1] : r[1], v ? r[2] + r[4 * v + 2] : r[2]};
                float own[24];
                for (int k = 0; k < 24; ++k) own[k] = p[k % 3];
                int32_t list[3] = {mark, mark, mark}, count = mark;
                CHECK(hulls(flat, own, 24, 1, nullptr, 3, list, &count) == RT_OK);
                CHECK(count >= 1 && std::find(list, list + std::min(count, 3), t) != list + std::min(count, 3));
            }
        // a box over everything lists everything, in walk order: the split by index and the right child first give descending leaves
        const float everything[6] = {-100, -100, -100, 100, 100, 100};
        float all[24];
        CHECK(rt_box_corners(everything, 6, 1, nullptr, 0, all) == RT_OK);
        std::vector<int32_t> list((size_t)stack.nTris, mark);
        int32_t count = mark;
        CHECK(hulls(stack, all, 24, 1, nullptr, stack.nTris, list.data(), &count) == RT_OK);
        CHECK(count == stack.nTris);
        std::vector<int32_t> sorted = list;
        std::sort(sorted.begin(), sorted.end());
        for (int i = 0; i < stack.nTris; ++i) CHECK(sorted[(size_t)i] == i);
        CHECK(list[0] > list[(size_t)stack.nTris - 1]);
    }
    // ---- slots of negative length or with a negative start hold nothing
    {
        Queries Q = queries_about(5, 24, 3u);
        const int32_t odd[6] = {3, 1, 1, -5, 2, 2};
        int32_t prims[4] = {mark, mark, mark, mark}, counts[5];
        CHECK(hulls(stack, Q.q.data(), 24, 5, odd, 0, prims, counts) == RT_OK);
        CHECK(prims[0] == mark && prims[1] == mark && prims[2] == mark && prims[3] == mark);
    }
    // ---- refusals: nothing is read or written
    {
        Queries Q = queries_about(2, 24, 1u);
        int32_t prims[8], cnt[2] = {mark, mark};
        const int32_t off[3] = {0, 4, 8};
        std::fill(prims, prims + 8, mark);
        CHECK(hulls(stack, Q.q.data(), 24, -1, off, 0, prims, cnt) == RT_ERR_INVALID);
        CHECK(hulls(stack, Q.q.data(), 23, 2, off, 0, prims, cnt) == RT_ERR_INVALID);
        CHECK(hulls(stack, nullptr, 24, 2, off, 0, prims, cnt) == RT_ERR_INVALID);
        CHECK(hulls(stack, Q.q.data(), 24, 2, off, 0, nullptr, nullptr) == RT_ERR_INVALID);          // prims and counts both NULL
        CHECK(hulls(stack, Q.q.data(), 24, 2, nullptr, -1, prims, cnt) == RT_ERR_INVALID);            // prims without offsets, cap < 0
        CHECK(hulls(stack, Q.q.data(), 24, INT_MAX / 4 + 1, nullptr, 4, prims, cnt) == RT_ERR_INVALID);   // n * cap beyond INT32_MAX
        CHECK(hulls(stack, nullptr, 24, 0, nullptr, 0, nullptr, nullptr) == RT_OK);                   // n == 0: a no-op
        CHECK(rt_hull_overlaps(nullptr, stack.nNodes, stack.tris.data(), stack.nTris, Q.q.data(), 24, 2, off, 0, prims, cnt) == RT_ERR_INVALID);
        CHECK(rt_hull_overlaps(stack.nodes.data(), stack.nNodes, nullptr, stack.nTris, Q.q.data(), 24, 2, off, 0, prims, cnt) == RT_ERR_INVALID);
        CHECK(rt_hull_overlaps(stack.nodes.data(), -1, stack.tris.data(), stack.nTris, Q.q.data(), 24, 2, off, 0, prims, cnt) == RT_ERR_INVALID);
        for (float link : {-1.0f, 1e9f, nan, (float)stack.nNodes, 0.0f}) {   // nodes that are no tree over the rows
            Tree bad = stack;
            bad.nodes[3] = link;
            CHECK(hulls(bad, Q.q.data(), 24, 2, off, 0, prims, cnt) == RT_ERR_INVALID);
        }
        CHECK(cnt[0] == mark && cnt[1] == mark && std::all_of(prims, prims + 8, [&](int32_t v) { return v == mark; }));
        // an empty scene overlaps nothing
        CHECK(rt_hull_overlaps(nullptr, 0, nullptr, 0, Q.q.data(), 24, 2, off, 0, prims, cnt) == RT_OK && cnt[0] == 0 && cnt[1] == 0 && prims[0] == mark);
    }
    // ---- the corner makers: strided inputs that end with their last element's last float, outputs of n * 24 floats
    {
        const int n = 9;
        for (int stride : {6, 7}) {
            std::vector<float> boxes((size_t)(n - 1) * stride + 6), M((size_t)n * 16, 0.0f), out((size_t)n * 24, -77.0f);
            for (int i = 0; i < n; ++i) {
                for (int a = 0; a < 3; ++a) { boxes[(size_t)i * stride + a] = -1.0f - (float)i; boxes[(size_t)i * stride + 3 + a] = 2.0f + (float)a; }
                for (int d = 0; d < 4; ++d) M[(size_t)i * 16 + 5 * d] = 1.0f + (float)i;
                M[(size_t)i * 16 + 12] = 3.0f;
            }
            boxes[(size_t)2 * stride + 1] = nan;              // empty slots: a NaN, lo > hi
            boxes[(size_t)4 * stride + 5] = -100.0f;
            boxes[(size_t)5 * stride + 3] = inf;
            boxes[(size_t)6 * stride + 0] = -3e38f; boxes[(size_t)6 * stride + 3] = 3e38f;
            for (int form = 0; form < 3; ++form) {
                CHECK(rt_box_corners(boxes.data(), stride, n, form ? M.data() : nullptr, form == 2 ? 16 : 0, out.data()) == RT_OK);
                for (int i = 0; i < n; ++i) {
                    const bool empty = i == 2 || i == 4;
                    for (int k = 0; k < 24; ++k) CHECK(empty == (out[(size_t)i * 24 + k] != out[(size_t)i * 24 + k]) || (i >= 5 && i <= 6));
                }
            }
            CHECK(out[0] == (-1.0f) * 1.0f + 3.0f);           // box 0, corner 0, x under its own matrix
            std::fill(out.begin(), out.end(), -77.0f);
            CHECK(rt_box_corners(boxes.data(), 5, n, nullptr, 0, out.data()) == RT_ERR_INVALID);
            CHECK(rt_box_corners(boxes.data(), stride, -1, nullptr, 0, out.data()) == RT_ERR_INVALID);
            CHECK(rt_box_corners(boxes.data(), stride, n, M.data(), 8, out.data()) == RT_ERR_INVALID);
            CHECK(rt_box_corners(nullptr, stride, n, nullptr, 0, out.data()) == RT_ERR_INVALID);
            CHECK(rt_box_corners(boxes.data(), stride, n, nullptr, 0, nullptr) == RT_ERR_INVALID);
            CHECK(rt_box_corners(nullptr, stride, 0, nullptr, 0, nullptr) == RT_OK);
            CHECK(std::all_of(out.begin(), out.end(), [](float v) { return v == -77.0f; }));
        }
        RtUniforms u;
        std::memset(&u, 0, sizeof u);
        u.camPos[2] = 5.0f; u.camRight[0] = 1.0f; u.camUp[1] = 1.0f; u.camFwd[2] = -1.0f;
        u.tanHalfFov = 0.5f; u.aspect = 4.0f / 3.0f; u.resolution[0] = 48.0f; u.resolution[1] = 36.0f;
        const float rootMin[3] = {-1, -1, -1}, rootMax[3] = {1, 1, 1};
        for (int stride : {4, 5})
            for (int jitter = 0; jitter < 2; ++jitter) {
                u.enableJitter = jitter; u.jitter[0] = 0.3f; u.jitter[1] = -0.2f;
                std::vector<float> rects((size_t)(n - 1) * stride + 4), out((size_t)n * 24, -77.0f);
                for (int i = 0; i < n; ++i) {
                    float *r = &rects[(size_t)i * stride];
                    r[0] = (float)(5 * i) - 8.0f; r[1] = (float)(3 * i) - 4.0f; r[2] = r[0] + (float)i; r[3] = r[1] + 2.0f;
                }
                rects[(size_t)2 * stride + 2] = nan;
                rects[(size_t)4 * stride + 3] = -100.0f;          // y1 < y0
                rects[(size_t)5 * stride + 2] = inf;
                rects[(size_t)6 * stride + 0] = -3e38f;
                for (float tFar : {-1.0f, 0.0f, 4.0f, 1e30f, inf})
                    for (float tNear : {0.0f, 0.5f, 20.0f}) {
                        CHECK(rt_rect_frusta(&u, rootMin, rootMax, rects.data(), stride, n, tNear, tFar, out.data()) == RT_OK);
                        for (int i = 0; i < n; ++i)
                            if (i == 2 || i == 4) for (int k = 0; k < 24; ++k) CHECK(out[(size_t)i * 24 + k] != out[(size_t)i * 24 + k]);
                        if (tNear == 0.0f) CHECK(out[0] == 0.0f && out[1] == 0.0f && out[2] == 5.0f);   // the pyramid's apex is the eye
                        if (tFar < 0.0f && tNear < 1.0f) CHECK(out[14] < -1.0f && out[14] > -1.1f);     // "to the far side": just beyond the root box
                        // the hulls serve as queries as they stand
                        std::vector<int32_t> counts((size_t)n, mark);
                        CHECK(hulls(stack, out.data(), 24, n, nullptr, 0, nullptr, counts.data()) == RT_OK);
                        CHECK(counts[2] == 0 && counts[4] == 0);
                    }
                std::fill(out.begin(), out.end(), -77.0f);
                RtUniforms bad = u;
                bad.resolution[1] = 0.0f;
                CHECK(rt_rect_frusta(nullptr, rootMin, rootMax, rects.data(), stride, n, 0.0f, -1.0f, out.data()) == RT_ERR_INVALID);
                CHECK(rt_rect_frusta(&bad, rootMin, rootMax, rects.data(), stride, n, 0.0f, -1.0f, out.data()) == RT_ERR_INVALID);
                CHECK(rt_rect_frusta(&u, nullptr, rootMax, rects.data(), stride, n, 0.0f, -1.0f, out.data()) == RT_ERR_INVALID);
                CHECK(rt_rect_frusta(&u, rootMin, nullptr, rects.data(), stride, n, 0.0f, -1.0f, out.data()) == RT_ERR_INVALID);
                CHECK(rt_rect_frusta(&u, rootMin, rootMax, nullptr, stride, n, 0.0f, -1.0f, out.data()) == RT_ERR_INVALID);
                CHECK(rt_rect_frusta(&u, rootMin, rootMax, rects.data(), 3, n, 0.0f, -1.0f, out.data()) == RT_ERR_INVALID);
                CHECK(rt_rect_frusta(&u, rootMin, rootMax, rects.data(), stride, -1, 0.0f, -1.0f, out.data()) == RT_ERR_INVALID);
                CHECK(rt_rect_frusta(&u, rootMin, rootMax, rects.data(), stride, n, -0.5f, -1.0f, out.data()) == RT_ERR_INVALID);
                CHECK(rt_rect_frusta(&u, rootMin, rootMax, rects.data(), stride, n, nan, -1.0f, out.data()) == RT_ERR_INVALID);
                CHECK(rt_rect_frusta(&u, rootMin, rootMax, rects.data(), stride, n, 0.0f, nan, out.data()) == RT_ERR_INVALID);
                CHECK(rt_rect_frusta(&u, rootMin, rootMax, rects.data(), stride, n, 0.0f, -1.0f, nullptr) == RT_ERR_INVALID);
                CHECK(rt_rect_frusta(&u, rootMin, rootMax, nullptr, stride, 0, 0.0f, -1.0f, nullptr) == RT_OK);
                CHECK(std::all_of(out.begin(), out.end(), [](float v) { return v == -77.0f; }));
            }
    }
    if (g_fail) { std::printf("hull query host: %d checks FAILED\n", g_fail); return 1; }
    std::printf("hull query host: all checks passed\n");
    return 0;
}
