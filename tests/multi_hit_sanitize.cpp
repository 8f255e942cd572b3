// The multi-hit definition (csrc/rt_multi_hit.cpp: rt_multi_hits) driven over its edge cases under AddressSanitizer + UBSan on the CPU
// (tests/test_multi_hit_host_sanitizers.py).  Linked with rt_multi_hit.cpp alone.  Every array is exactly as long as the call may read or write:
// strided ray arrays end with their last ray's third float, hits hold n * maxHits records.
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

// n rays with the given strides in arrays that end with the last ray's third float
struct Rays { std::vector<float> o, d, tm; int n, os, ds; };
static Rays rays_down(int n, int os, int ds, unsigned seed) {
    Rays R;
    R.n = n; R.os = os; R.ds = ds;
    R.o.assign((size_t)(n - 1) * os + 3, 0.0f); R.d.assign((size_t)(n - 1) * ds + 3, 0.0f); R.tm.assign((size_t)n, 0.0f);
    std::mt19937 r(seed);
    for (int i = 0; i < n; ++i) {
        float *o = &R.o[(size_t)i * os], *d = &R.d[(size_t)i * ds];
        o[0] = (float)((int)(r() % 80u) - 40) / 8.0f; o[1] = (float)(16 + (int)(r() % 48u)) / 8.0f; o[2] = (float)((int)(r() % 80u) - 40) / 8.0f;
        const float dx = (i & 1) ? (float)((int)(r() % 5u) - 2) : 0.0f, dz = (i & 1) ? (float)((int)(r() % 5u) - 2) : 0.0f;
        const float inv = 1.0f / std::sqrt(dx * dx + 1.0f + dz * dz);
        d[0] = dx * inv; d[1] = -inv; d[2] = dz * inv;
        R.tm[(size_t)i] = (i % 7 == 0) ? -1.0f : (float)(r() % 100u) / 10.0f;
    }
    return R;
}

static void check_answer(const Rays &R, int K, const std::vector<RtHit> &hits, const std::vector<int32_t> &counts, float inf, int nTris) {
    for (int i = 0; i < R.n; ++i) {
        const int c = counts[(size_t)i];
        CHECK(c >= 0 && c <= nTris);
        for (int j = 0; j < K; ++j) {
            const RtHit &h = hits[(size_t)i * K + j];
            if (j < std::min(c, K)) {
                CHECK(h.prim >= 0 && h.prim < nTris);
                if (j > 0) { const RtHit &p = hits[(size_t)i * K + j - 1]; CHECK(p.t < h.t || (p.t == h.t && p.prim < h.prim)); }
            } else CHECK(h.t == inf && h.prim == -1 && h.u == 0.0f && h.v == 0.0f);
        }
    }
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
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
        for (int K : {0, 1, 4, 18, RT_MULTI_HIT_MAX})
            for (auto st : {std::pair<int, int>{3, 3}, {4, 3}, {8, 8}})
                for (int n : {1, 2, 65}) {
                    Rays R = rays_down(n, st.first, st.second, 7u + (unsigned)(K + n));
                    std::vector<RtHit> hits((size_t)n * K);
                    std::vector<int32_t> counts((size_t)n, -5);
                    for (int useTm = 0; useTm < 2; ++useTm) {
                        CHECK(rt_multi_hits(T->nodes.data(), T->nNodes, T->tris.data(), T->nTris, R.o.data(), R.os, R.d.data(), R.ds, useTm ? R.tm.data() : nullptr, 1e-4f,
                                            1e30f, n, K, K ? hits.data() : nullptr, counts.data()) == RT_OK);
                        check_answer(R, K, hits, counts, 1e30f, T->nTris);
                        if (!useTm && T == &stack) for (int c : counts) CHECK(c == 18 || c == 36);
                        if (useTm) for (int i = 0; i < n; i += 7) CHECK(counts[(size_t)i] == 0);
                    }
                    if (K) CHECK(rt_multi_hits(T->nodes.data(), T->nNodes, T->tris.data(), T->nTris, R.o.data(), R.os, R.d.data(), R.ds, nullptr, 0.0f, 1e30f, n, K, hits.data(),
                                               nullptr) == RT_OK);   // counts may be null
                }
    // ---- degenerate rays: NaN and infinite components, zero directions, a NaN limit
    {
        const float sp[] = {nan, inf, -inf, 0.0f, -0.0f, 1e-41f, 3.0f};
        std::vector<float> o, d, tm;
        for (float a : sp) for (float b : sp) for (float c : sp) { o.insert(o.end(), {a, 4.0f, b}); d.insert(d.end(), {b, c, a}); tm.push_back(c); }
        const int n = (int)tm.size();
        std::vector<RtHit> hits((size_t)n * RT_MULTI_HIT_MAX);
        std::vector<int32_t> counts((size_t)n);
        for (const Tree *T : {&one, &stack}) {
            RtHit mark; mark.t = -7.5f; mark.prim = -9; mark.u = mark.v = -7.5f;
            std::fill(hits.begin(), hits.end(), mark);
            CHECK(rt_multi_hits(T->nodes.data(), T->nNodes, T->tris.data(), T->nTris, o.data(), 3, d.data(), 3, tm.data(), 1e-4f, 1e30f, n, RT_MULTI_HIT_MAX, hits.data(),
                                counts.data()) == RT_OK);
            for (const RtHit &h : hits) CHECK(h.prim != -9);   // no slot is left unwritten
            for (int c : counts) CHECK(c >= 0 && c <= T->nTris);
        }
    }
    // ---- refusals: nothing is read or written
    {
        Rays R = rays_down(2, 3, 3, 1u);
        RtHit h[8]; int32_t c[2];
        auto call = [&](const Tree &T, int n, int K, int os, int ds, const float *o, const float *d, RtHit *hh, int32_t *cc) {
            return rt_multi_hits(T.nodes.data(), T.nNodes, T.tris.data(), T.nTris, o, os, d, ds, nullptr, 1e-4f, 1e30f, n, K, hh, cc);
        };
        CHECK(call(stack, 2, -1, 3, 3, R.o.data(), R.d.data(), h, c) == RT_ERR_INVALID);
        CHECK(call(stack, 2, RT_MULTI_HIT_MAX + 1, 3, 3, R.o.data(), R.d.data(), h, c) == RT_ERR_INVALID);
        CHECK(call(stack, -1, 4, 3, 3, R.o.data(), R.d.data(), h, c) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 4, 2, 3, R.o.data(), R.d.data(), h, c) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 4, 3, 2, R.o.data(), R.d.data(), h, c) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 4, 3, 3, nullptr, R.d.data(), h, c) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 4, 3, 3, R.o.data(), nullptr, h, c) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 4, 3, 3, R.o.data(), R.d.data(), nullptr, c) == RT_ERR_INVALID);
        CHECK(call(stack, 2, 0, 3, 3, R.o.data(), R.d.data(), nullptr, nullptr) == RT_ERR_INVALID);
        CHECK(call(stack, INT_MAX, RT_MULTI_HIT_MAX, 3, 3, R.o.data(), R.d.data(), h, c) == RT_ERR_INVALID);
        CHECK(call(stack, 0, 4, 3, 3, nullptr, nullptr, nullptr, nullptr) == RT_OK);
        // nodes that are no tree over the rows: a child off the array, a cycle, a range beyond the rows, huge and NaN links
        for (float link : {-1.0f, 1e9f, nan, (float)stack.nNodes, 0.0f}) {
            Tree bad = stack;
            bad.nodes[3] = link;
            CHECK(call(bad, 2, 4, 3, 3, R.o.data(), R.d.data(), h, c) == RT_ERR_INVALID);
        }
        Tree bad = one;
        bad.nodes[9] = 3.0f;
        CHECK(call(bad, 2, 4, 3, 3, R.o.data(), R.d.data(), h, c) == RT_ERR_INVALID);
        bad.nodes[8] = 2e9f; bad.nodes[9] = 1.0f;
        CHECK(call(bad, 2, 4, 3, 3, R.o.data(), R.d.data(), h, c) == RT_ERR_INVALID);
        // an empty scene has no occluders
        CHECK(rt_multi_hits(nullptr, 0, nullptr, 0, R.o.data(), 3, R.d.data(), 3, nullptr, 1e-4f, 1e30f, 2, 4, h, c) == RT_OK && c[0] == 0 && c[1] == 0 && h[7].prim == -1);
    }
    if (g_fail) { std::printf("multi-hit host: %d checks FAILED\n", g_fail); return 1; }
    std::printf("multi-hit host: all checks passed\n");
    return 0;
}
