// The nearest-point definition (csrc/rt_nearest.cpp: rt_nearest_points) driven over its edge cases under AddressSanitizer + UBSan on the CPU
// (tests/test_nearest_host_sanitizers.py).  Linked with rt_nearest.cpp alone.  Every array is exactly as long as the call may read or write: a
// strided point array ends with its last point's third float, hits hold n records, closest 3 n floats.
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

static void check_answer(const Tree &T, const Points &P, bool limited, const std::vector<RtHit> &hits, const float *closest) {
    const float inf = std::numeric_limits<float>::infinity();
    for (int i = 0; i < P.n; ++i) {
        const RtHit &h = hits[(size_t)i];
        if (h.prim < 0) {
            CHECK(h.prim == -1 && h.t == inf && h.u == 0.0f && h.v == 0.0f);
            if (closest) CHECK(closest[3 * i] == 0.0f && closest[3 * i + 1] == 0.0f && closest[3 * i + 2] == 0.0f);
            CHECK(limited);   // without a limit every finite point has an answer
            continue;
        }
        CHECK(h.prim < T.nTris && h.t >= 0.0f && h.u >= 0.0f && h.v >= 0.0f && h.u + h.v <= 1.0f + 1e-6f);
        if (limited) CHECK(!(P.md[(size_t)i] < 0.0f) && h.t <= P.md[(size_t)i] * P.md[(size_t)i]);
        if (closest) {   // the point lies at the distance the record states, to rounding
            const float *p = &P.p[(size_t)i * P.stride];
            double d2 = 0;
            for (int a = 0; a < 3; ++a) d2 += ((double)p[a] - closest[3 * i + a]) * ((double)p[a] - closest[3 * i + a]);
            CHECK(std::fabs(d2 - h.t) <= 1e-4 * (1.0 + h.t));
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
            for (int n : {1, 2, 65}) {
                Points P = points_about(n, stride, 7u + (unsigned)(stride + n));
                std::vector<RtHit> hits((size_t)n);
                std::vector<float> closest((size_t)n * 3);
                for (int limited = 0; limited < 2; ++limited)
                    for (int withClosest = 0; withClosest < 2; ++withClosest) {
                        CHECK(rt_nearest_points(T->nodes.data(), T->nNodes, T->tris.data(), T->nTris, P.p.data(), P.stride, limited ? P.md.data() : nullptr, n,
                                                hits.data(), withClosest ? closest.data() : nullptr) == RT_OK);
                        check_answer(*T, P, limited != 0, hits, withClosest ? closest.data() : nullptr);
                        if (limited) for (int i = 0; i < n; i += 7) CHECK(hits[(size_t)i].prim == -1);
                    }
            }
    // ---- degenerate points and limits: NaN and infinite components, denormals, huge values; a zero-area triangle among the rows
    {
        Tree flat = tree_of({0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1});
        const float sp[] = {nan, inf, -inf, 0.0f, -0.0f, 1e-41f, 3.0f, 3e38f};
        std::vector<float> p, md;
        for (float a : sp) for (float b : sp) for (float c : sp) { p.insert(p.end(), {a, b, c}); md.push_back(c); }
        const int n = (int)md.size();
        std::vector<RtHit> hits((size_t)n);
        std::vector<float> closest((size_t)n * 3);
        for (const Tree *T : {&one, &stack, &flat})
            for (int limited = 0; limited < 2; ++limited) {
                RtHit mark; mark.t = -7.5f; mark.prim = -9; mark.u = mark.v = -7.5f;
                std::fill(hits.begin(), hits.end(), mark);
                CHECK(rt_nearest_points(T->nodes.data(), T->nNodes, T->tris.data(), T->nTris, p.data(), 3, limited ? md.data() : nullptr, n, hits.data(),
                                        closest.data()) == RT_OK);
                for (int i = 0; i < n; ++i) {
                    const RtHit &h = hits[(size_t)i];
                    CHECK(h.prim != -9 && h.prim >= -1 && h.prim < T->nTris);   // no slot is left unwritten
                    const bool finite = std::isfinite(p[3 * i]) && std::isfinite(p[3 * i + 1]) && std::isfinite(p[3 * i + 2]);
                    if (!finite) CHECK(h.prim == -1 && h.t == inf);
                    if (h.prim >= 0) CHECK(!(h.t != h.t));                      // a NaN e is never accepted
                }
            }
    }
    // ---- refusals: nothing is read or written
    {
        Points P = points_about(2, 3, 1u);
        RtHit h[2]; float c[6];
        auto call = [&](const Tree &T, int n, int stride, const float *p, RtHit *hh) {
            return rt_nearest_points(T.nodes.data(), T.nNodes, T.tris.data(), T.nTris, p, stride, nullptr, n, hh, c);
        };
        CHECK(call(stack, -1, 3, P.p.data(), h) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 2, P.p.data(), h) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 3, nullptr, h) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 3, P.p.data(), nullptr) == RT_ERR_INVALID);
        CHECK(call(stack, INT_MAX, 8, P.p.data(), h) == RT_ERR_INVALID);
        CHECK(call(stack, 0, 3, nullptr, nullptr) == RT_OK);
        // nodes that are no tree over the rows: a child off the array, a cycle, a range beyond the rows, huge and NaN links
        for (float link : {-1.0f, 1e9f, nan, (float)stack.nNodes, 0.0f}) {
            Tree bad = stack;
            bad.nodes[3] = link;
            CHECK(call(bad, 2, 3, P.p.data(), h) == RT_ERR_INVALID);
        }
        Tree bad = one;
        bad.nodes[9] = 3.0f;
        CHECK(call(bad, 2, 3, P.p.data(), h) == RT_ERR_INVALID);
        bad.nodes[8] = 2e9f; bad.nodes[9] = 1.0f;
        CHECK(call(bad, 2, 3, P.p.data(), h) == RT_ERR_INVALID);
        // an empty scene has no surface
        CHECK(rt_nearest_points(nullptr, 0, nullptr, 0, P.p.data(), 3, nullptr, 2, h, c) == RT_OK && h[0].prim == -1 && h[1].prim == -1 && h[1].t == inf && c[5] == 0.0f);
    }
    if (g_fail) { std::printf("nearest host: %d checks FAILED\n", g_fail); return 1; }
    std::printf("nearest host: all checks passed\n");
    return 0;
}
