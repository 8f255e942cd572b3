// The proximity definition (csrc/rt_nearest_multi.cpp: rt_nearest_points_multi) driven over its edge cases under AddressSanitizer + UBSan on the CPU
// (tests/test_nearest_multi_host_sanitizers.py).  Linked with rt_nearest_multi.cpp alone.  Every array is exactly as long as the call may read or
// write: a strided point array ends with its last point's third float, hits hold n * K records, closest 3 n K floats, counts n; with K = 0 hits and
// closest have no element at all.
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

// n points with the given stride in an array that ends with the last point's third float
struct Points { std::vector<float> p, md; int n, stride; };
static Points points_about(int n, int stride, unsigned seed) {
    Points P;
    P.n = n; P.stride = stride;
    P.p.assign((size_t)(n - 1) * stride + 3, 0.0f); P.md.assign((size_t)n, 0.0f);
    std::mt19937 r(seed);
    for (int i = 0; i < n; ++i) {
        float *p = &P.p[(size_t)i * stride];
        p[0] = (float)((int)(r() % 640u) - 320) / 8.0f; p[1] = (float)((int)(r() % 64u) - 16) / 8.0f; p[2] = (float)((int)(r() % 640u) - 320) / 8.0f;
        P.md[(size_t)i] = (i % 7 == 0) ? -1.0f : (float)(r() % 100u) / 10.0f;
    }
    return P;
}

// The records of every point: min(K, count) of them ascending under (e, prim) and within the limit, then misses; closest at the stated distance
static void check_answer(const Tree &T, const Points &P, bool limited, int K, const RtHit *hits, const int32_t *counts, const float *closest) {
    const float inf = std::numeric_limits<float>::infinity();
    for (int i = 0; i < P.n; ++i) {
        int kept = 0;
        for (int j = 0; j < K; ++j) {
            const RtHit &h = hits[(size_t)i * K + j];
            const float *c = closest ? closest + ((size_t)i * K + j) * 3 : nullptr;
            if (h.prim < 0) {
                CHECK(h.prim == -1 && h.t == inf && h.u == 0.0f && h.v == 0.0f);
                if (c) CHECK(c[0] == 0.0f && c[1] == 0.0f && c[2] == 0.0f);
                continue;
            }
            CHECK(kept == j);   // no record behind a miss
            kept++;
            CHECK(h.prim < T.nTris && h.t >= 0.0f && h.u >= 0.0f && h.v >= 0.0f && h.u + h.v <= 1.0f + 1e-6f);
            if (j > 0) { const RtHit &g = hits[(size_t)i * K + j - 1]; CHECK(g.t < h.t || (g.t == h.t && g.prim < h.prim)); }
            if (limited) CHECK(!(P.md[(size_t)i] < 0.0f) && h.t <= P.md[(size_t)i] * P.md[(size_t)i]);
            if (c) {
                const float *p = &P.p[(size_t)i * P.stride];
                double d2 = 0;
                for (int a = 0; a < 3; ++a) d2 += ((double)p[a] - c[a]) * ((double)p[a] - c[a]);
                CHECK(std::fabs(d2 - h.t) <= 1e-4 * (1.0 + h.t));
            }
        }
        if (counts) {
            CHECK(counts[i] >= 0 && counts[i] <= T.nTris && kept == std::min(K, counts[i]));
            if (!limited) CHECK(counts[i] == T.nTris);   // without a limit every row of a finite point is accepted (no row here has a NaN e)
            if (limited && P.md[(size_t)i] < 0.0f) CHECK(counts[i] == 0);
        }
    }
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // ---- one leaf: two triangles, no inner node
    Tree one = tree_of({-0.75f, 0.25f, -0.75f, 2, 0, 0, 1, 1.5f, -0.2f, -0.75f, 0.25f, 1.25f, 2, 0, 0, 1, 1.5f, -0.5f});
    CHECK(one.nNodes == 1 && one.nTris == 2);
    // ---- the layer stack: six layers of three coincident copies of a quad, 36 triangles -- every point has exact ties
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
        for (int stride : {3, 4, 8})
            for (int n : {1, 2, 65})
                for (int K : {0, 1, 3, 32}) {
                    Points P = points_about(n, stride, 7u + (unsigned)(stride + n));
                    std::vector<RtHit> hits((size_t)n * K);
                    std::vector<float> closest((size_t)n * K * 3);
                    std::vector<int32_t> counts((size_t)n);
                    for (int limited = 0; limited < 2; ++limited)
                        for (int withCounts = (K == 0); withCounts < 2; ++withCounts)
                            for (int withClosest = 0; withClosest < 2; ++withClosest) {
                                // (a vector without elements may hand out any pointer: K = 0 passes NULL for the arrays it may not touch)
                                RtHit *h = K ? hits.data() : nullptr;
                                float *c = withClosest && K ? closest.data() : nullptr;
                                CHECK(rt_nearest_points_multi(T->nodes.data(), T->nNodes, T->tris.data(), T->nTris, P.p.data(), P.stride, limited ? P.md.data() : nullptr,
                                                              n, K, h, withCounts ? counts.data() : nullptr, c) == RT_OK);
                                check_answer(*T, P, limited != 0, K, h, withCounts ? counts.data() : nullptr, c);
                            }
                }
    // ---- ties: above the layer stack the three coincident copies tie exactly, and prim decides
    {
        const float p[3] = {1.0f, 5.0f, 2.0f};
        RtHit h[4]; int32_t count = -1;
        CHECK(rt_nearest_points_multi(stack.nodes.data(), stack.nNodes, stack.tris.data(), stack.nTris, p, 3, nullptr, 1, 4, h, &count, nullptr) == RT_OK);
        CHECK(count == 36 && h[0].t == h[1].t && h[1].t == h[2].t && h[0].prim < h[1].prim && h[1].prim < h[2].prim && h[3].t >= h[2].t);
    }
    // ---- degenerate points and limits: NaN and infinite components, denormals, huge values; a zero-area triangle among the rows
    {
        Tree flat = tree_of({0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1});
        const float sp[] = {nan, inf, -inf, 0.0f, -0.0f, 1e-41f, 3.0f, 3e38f};
        std::vector<float> p, md;
        for (float a : sp) for (float b : sp) for (float c : sp) { p.insert(p.end(), {a, b, c}); md.push_back(c); }
        const int n = (int)md.size(), K = 3;
        std::vector<RtHit> hits((size_t)n * K);
        std::vector<float> closest((size_t)n * K * 3);
        std::vector<int32_t> counts((size_t)n);
        for (const Tree *T : {&one, &stack, &flat})
            for (int limited = 0; limited < 2; ++limited) {
                RtHit mark; mark.t = -7.5f; mark.prim = -9; mark.u = mark.v = -7.5f;
                std::fill(hits.begin(), hits.end(), mark);
                std::fill(counts.begin(), counts.end(), -9);
                CHECK(rt_nearest_points_multi(T->nodes.data(), T->nNodes, T->tris.data(), T->nTris, p.data(), 3, limited ? md.data() : nullptr, n, K, hits.data(),
                                              counts.data(), closest.data()) == RT_OK);
                for (int i = 0; i < n; ++i) {
                    const bool finite = std::isfinite(p[3 * i]) && std::isfinite(p[3 * i + 1]) && std::isfinite(p[3 * i + 2]);
                    CHECK(counts[(size_t)i] >= 0 && counts[(size_t)i] <= T->nTris);
                    if (!finite || (limited && !(md[(size_t)i] >= 0.0f))) CHECK(counts[(size_t)i] == 0);   // an empty slot, or a NaN limit: nothing accepted
                    for (int j = 0; j < K; ++j) {
                        const RtHit &h = hits[(size_t)i * K + j];
                        CHECK(h.prim != -9 && h.prim >= -1 && h.prim < T->nTris);   // no slot is left unwritten
                        CHECK((h.prim >= 0) == (j < counts[(size_t)i]));
                        if (h.prim >= 0) CHECK(!(h.t != h.t));                      // a NaN e is never accepted
                    }
                }
            }
    }
    // ---- refusals: nothing is read or written
    {
        Points P = points_about(2, 3, 1u);
        RtHit h[8]; float c[24]; int32_t cnt[2] = {-9, -9};
        std::memset(h, 0x55, sizeof h);
        auto call = [&](const Tree &T, int n, int stride, int K, const float *p, RtHit *hh, int32_t *cc) {
            return rt_nearest_points_multi(T.nodes.data(), T.nNodes, T.tris.data(), T.nTris, p, stride, nullptr, n, K, hh, cc, c);
        };
        CHECK(call(stack, 2, 3, -1, P.p.data(), h, cnt) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 3, RT_NEAREST_MULTI_MAX + 1, P.p.data(), h, cnt) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 3, 0, P.p.data(), h, nullptr) == RT_ERR_INVALID);              // K = 0 without counts
        CHECK(call(stack, INT_MAX / 4 + 1, 3, 4, P.p.data(), h, cnt) == RT_ERR_INVALID);    // n * K beyond INT32_MAX
        CHECK(call(stack, -1, 3, 4, P.p.data(), h, cnt) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 2, 4, P.p.data(), h, cnt) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 3, 4, nullptr, h, cnt) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 3, 4, P.p.data(), nullptr, cnt) == RT_ERR_INVALID);
        CHECK(call(stack, INT_MAX, 8, 1, P.p.data(), h, cnt) == RT_ERR_INVALID);            // beyond 2^32 floats
        CHECK(call(stack, 0, 3, 4, nullptr, nullptr, nullptr) == RT_OK);
        CHECK(rt_nearest_points_multi(nullptr, stack.nNodes, stack.tris.data(), stack.nTris, P.p.data(), 3, nullptr, 2, 4, h, cnt, c) == RT_ERR_INVALID);
        CHECK(rt_nearest_points_multi(stack.nodes.data(), stack.nNodes, nullptr, stack.nTris, P.p.data(), 3, nullptr, 2, 4, h, cnt, c) == RT_ERR_INVALID);
        CHECK(rt_nearest_points_multi(stack.nodes.data(), -1, stack.tris.data(), stack.nTris, P.p.data(), 3, nullptr, 2, 4, h, cnt, c) == RT_ERR_INVALID);
        // nodes that are no tree over the rows: a child off the array, a cycle, a range beyond the rows, huge and NaN links
        for (float link : {-1.0f, 1e9f, nan, (float)stack.nNodes, 0.0f}) {
            Tree bad = stack;
            bad.nodes[3] = link;
            CHECK(call(bad, 2, 3, 4, P.p.data(), h, cnt) == RT_ERR_INVALID);
        }
        Tree bad = one;
        bad.nodes[9] = 3.0f;
        CHECK(call(bad, 2, 3, 4, P.p.data(), h, cnt) == RT_ERR_INVALID);
        bad.nodes[8] = 2e9f; bad.nodes[9] = 1.0f;
        CHECK(call(bad, 2, 3, 4, P.p.data(), h, cnt) == RT_ERR_INVALID);
        CHECK(cnt[0] == -9 && cnt[1] == -9 && h[0].prim == 0x55555555 && h[7].prim == 0x55555555);
        // K = 0 with counts: the counts alone, no record array at all
        CHECK(call(stack, 2, 3, 0, P.p.data(), nullptr, cnt) == RT_OK && cnt[0] == 36 && cnt[1] == 36 && h[0].prim == 0x55555555);
        // an empty scene has no surface
        CHECK(rt_nearest_points_multi(nullptr, 0, nullptr, 0, P.p.data(), 3, nullptr, 2, 4, h, cnt, c) == RT_OK && h[0].prim == -1 && h[7].prim == -1 && h[7].t == inf &&
              c[23] == 0.0f && cnt[0] == 0 && cnt[1] == 0);
        // the block size of the device launch lives in the same file
        int threads = 0; int64_t lds = 0;
        CHECK(rt_debug_nearest_multi_block(64, 32, &threads, &lds) == RT_OK && threads == 128 && lds == 98304);
        CHECK(rt_debug_nearest_multi_block(0, 32, &threads, &lds) == RT_ERR_INVALID && rt_debug_nearest_multi_block(8, 4, nullptr, &lds) == RT_ERR_INVALID);
    }
    if (g_fail) { std::printf("nearest multi host: %d checks FAILED\n", g_fail); return 1; }
    std::printf("nearest multi host: all checks passed\n");
    return 0;
}
