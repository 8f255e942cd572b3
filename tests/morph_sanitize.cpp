// The morph-target host code (csrc/rt_morph_pack.cpp: the checks, the packer of the sliced layout and rt_morph_positions, the definition) driven over
// its edge cases under AddressSanitizer + UBSan on the CPU (tests/test_morph_host_sanitizers.py).  Linked with rt_morph_pack.cpp alone.
#include "rt_mi355.h"
#include "../opengl-raytracing_amd/csrc/rt_morph_pack.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_fail; } } while (0)

struct Targets { std::vector<int32_t> first; std::vector<uint32_t> vi; std::vector<float> d; };

// nt targets over nv vertices: the given targets empty, vertex `hub` in every other one (twice in the even ones), signed zeros among the deltas
static Targets make(int nv, int nt, std::mt19937 &r, int emptyEvery) {
    Targets T;
    std::uniform_real_distribution<float> U(-1, 1);
    const uint32_t hub = (uint32_t)(nv / 2);
    T.first.push_back(0);
    for (int t = 0; t < nt; ++t) {
        if (!(emptyEvery && t % emptyEvery == 0)) {
            for (int v = nv - 1; v >= 0; --v)
                if ((uint32_t)v != hub && r() % 3 == 0) T.vi.push_back((uint32_t)v);
            T.vi.push_back(hub);
            if (t % 2 == 0) T.vi.push_back(hub);
        }
        T.first.push_back((int32_t)T.vi.size());
    }
    T.d.resize(T.vi.size() * 3);
    for (size_t i = 0; i < T.d.size(); ++i) T.d[i] = i % 5 == 0 ? 0.0f : i % 7 == 2 ? -0.0f : U(r);
    return T;
}

static int pack(int nv, const Targets &T, int nt, int which, std::vector<unsigned char> &out) {
    size_t n = 0;
    int rc = rt_debug_morph_pack(nv, T.first.data(), T.vi.data(), T.d.data(), nt, which, nullptr, 0, &n);
    if (rc != RT_OK) return rc;
    out.assign(n, 0xAB);   // exactly the size asked for: a write past it is the sanitizer's to find
    return rt_debug_morph_pack(nv, T.first.data(), T.vi.data(), T.d.data(), nt, which, out.data(), out.size(), &n);
}

int main() {
    std::mt19937 r(1);
    for (int nv : {1, 2, 63, 64, 65, 257, 1000})
        for (int nt : {1, 3, 40}) {
            const Targets T = make(nv, nt, r, nt >= 3 ? 3 : 0);
            std::vector<unsigned char> sf, ent, inf;
            CHECK(pack(nv, T, nt, RT_MORPH_ARRAY_SLICE_FIRST, sf) == RT_OK);
            CHECK(pack(nv, T, nt, RT_MORPH_ARRAY_ENTRIES, ent) == RT_OK);
            CHECK(pack(nv, T, nt, RT_MORPH_ARRAY_INFO, inf) == RT_OK && inf.size() == sizeof(RtMorphInfo));
            RtMorphInfo I;
            std::memcpy(&I, inf.data(), sizeof I);
            CHECK(I.nVerts == nv && I.nTargets == nt && I.nSlices == (nv + 63) / 64 && I.entries == T.vi.size());
            CHECK(sf.size() == ((size_t)I.nSlices + 1) * 4 && ent.size() == I.paddedEntries * 16 && I.paddedEntries % 64 == 0);
            // the definition from the packed form, row by row, equals rt_morph_positions on the lists
            std::vector<float> base((size_t)nv * 3), w((size_t)nt), want((size_t)nv * 3), got;
            std::uniform_real_distribution<float> U(-2, 2);
            for (auto &x : base) x = U(r);
            base[0] = -0.0f;
            for (int t = 0; t < nt; ++t) w[(size_t)t] = t % 4 == 0 ? 0.0f : t % 4 == 1 ? -0.0f : U(r);
            CHECK(rt_morph_positions(base.data(), nv, T.first.data(), T.vi.data(), T.d.data(), nt, w.data(), want.data()) == RT_OK);
            got = base;
            std::vector<uint32_t> first(sf.size() / 4);
            std::memcpy(first.data(), sf.data(), sf.size());
            size_t real = 0;
            for (int v = 0; v < nv; ++v)
                for (uint32_t k = first[(size_t)v / 64]; k < first[(size_t)v / 64 + 1]; ++k) {
                    rtl::MorphRecord rec;
                    std::memcpy(&rec, ent.data() + ((size_t)k * 64 + (size_t)v % 64) * 16, 16);
                    if (rec.target == rtl::kMorphPadTarget) { CHECK(rec.dx == 0 && rec.dy == 0 && rec.dz == 0); continue; }
                    ++real;
                    CHECK(rec.target < (uint32_t)nt);
                    const float wt = w[rec.target];
                    if (wt == 0.0f) continue;
                    float d[3];
                    std::memcpy(d, &rec, 12);
                    for (int c = 0; c < 3; ++c) { const float term = wt * d[c]; got[(size_t)v * 3 + c] = got[(size_t)v * 3 + c] + term; }
                }
            CHECK(real == T.vi.size());
            CHECK(std::memcmp(got.data(), want.data(), got.size() * 4) == 0);
            std::vector<float> alias = base;   // out may be base
            CHECK(rt_morph_positions(alias.data(), nv, T.first.data(), T.vi.data(), T.d.data(), nt, w.data(), alias.data()) == RT_OK);
            CHECK(std::memcmp(alias.data(), want.data(), want.size() * 4) == 0);
        }
    {   // every target empty: no record, and a positions call that copies the base
        Targets T;
        T.first.assign(6, 0);
        T.vi.assign(1, 0); T.d.assign(3, 0.0f);   // never read
        std::vector<unsigned char> ent, sf;
        CHECK(pack(130, T, 5, RT_MORPH_ARRAY_ENTRIES, ent) == RT_OK && ent.empty());
        CHECK(pack(130, T, 5, RT_MORPH_ARRAY_SLICE_FIRST, sf) == RT_OK && sf.size() == 16);
        std::vector<float> base(390, -0.0f), out(390, 1.0f), w(5, 1.0f);
        CHECK(rt_morph_positions(base.data(), 130, T.first.data(), T.vi.data(), T.d.data(), 5, w.data(), out.data()) == RT_OK);
        CHECK(std::memcmp(base.data(), out.data(), 390 * 4) == 0);
    }
    {   // what must be refused, by the definition and by the packer alike
        const int nv = 65, nt = 3;
        Targets G = make(nv, nt, r, 0);
        std::vector<float> base((size_t)nv * 3, 0.5f), out((size_t)nv * 3), w(70000, 0.5f);
        size_t n = 7;
        auto both = [&](const Targets &T, int verts, int targets, int want) {
            CHECK(rt_morph_positions(base.data(), verts, T.first.data(), T.vi.data(), T.d.data(), targets, w.data(), out.data()) == want);
            CHECK(rt_debug_morph_pack(verts, T.first.data(), T.vi.data(), T.d.data(), targets, RT_MORPH_ARRAY_ENTRIES, nullptr, 0, &n) == want);
        };
        both(G, nv, nt, RT_OK);
        both(G, 0, nt, RT_ERR_INVALID);
        both(G, -5, nt, RT_ERR_INVALID);
        both(G, nv, 0, RT_ERR_INVALID);
        both(G, nv, -1, RT_ERR_INVALID);
        both(G, nv, RT_MAX_MORPH_TARGETS + 1, RT_ERR_INVALID);   // refused before targetFirst is read
        Targets B = G; B.first[0] = 1; both(B, nv, nt, RT_ERR_INVALID);
        B = G; B.first[2] = B.first[1] - 1; both(B, nv, nt, RT_ERR_INVALID);
        B = G; B.first[1] = -4; both(B, nv, nt, RT_ERR_INVALID);
        B = G; B.vi[3] = (uint32_t)nv; both(B, nv, nt, RT_ERR_INVALID);
        B = G; B.vi.back() = 0xFFFFFFFFu; both(B, nv, nt, RT_ERR_INVALID);
        B = G; B.d.back() = std::numeric_limits<float>::quiet_NaN(); both(B, nv, nt, RT_ERR_INVALID);
        B = G; B.d[1] = std::numeric_limits<float>::infinity(); both(B, nv, nt, RT_ERR_INVALID);
        CHECK(rt_morph_positions(nullptr, nv, G.first.data(), G.vi.data(), G.d.data(), nt, w.data(), out.data()) == RT_ERR_INVALID);
        CHECK(rt_morph_positions(base.data(), nv, nullptr, G.vi.data(), G.d.data(), nt, w.data(), out.data()) == RT_ERR_INVALID);
        CHECK(rt_morph_positions(base.data(), nv, G.first.data(), nullptr, G.d.data(), nt, w.data(), out.data()) == RT_ERR_INVALID);
        CHECK(rt_morph_positions(base.data(), nv, G.first.data(), G.vi.data(), nullptr, nt, w.data(), out.data()) == RT_ERR_INVALID);
        CHECK(rt_morph_positions(base.data(), nv, G.first.data(), G.vi.data(), G.d.data(), nt, nullptr, out.data()) == RT_ERR_INVALID);
        CHECK(rt_morph_positions(base.data(), nv, G.first.data(), G.vi.data(), G.d.data(), nt, w.data(), nullptr) == RT_ERR_INVALID);
        CHECK(rt_debug_morph_pack(nv, G.first.data(), G.vi.data(), G.d.data(), nt, RT_MORPH_ARRAY_INFO, nullptr, 0, nullptr) == RT_ERR_INVALID);
        CHECK(rt_debug_morph_pack(nv, G.first.data(), G.vi.data(), G.d.data(), nt, 55, nullptr, 0, &n) == RT_ERR_INVALID && n == 0);
        std::vector<unsigned char> small(8);
        CHECK(rt_debug_morph_pack(nv, G.first.data(), G.vi.data(), G.d.data(), nt, RT_MORPH_ARRAY_ENTRIES, small.data(), small.size(), &n) == RT_ERR_INVALID);
        std::vector<int32_t> many((size_t)RT_MAX_MORPH_TARGETS + 1, 0);   // the largest count, every target empty
        CHECK(rt_morph_positions(base.data(), nv, many.data(), G.vi.data(), G.d.data(), RT_MAX_MORPH_TARGETS, w.data(), out.data()) == RT_OK);
    }
    {   // one vertex named 2^20 times: a plan of 2^20 rows for its slice; the 2^31 refusal from the plan alone, through a vertex list that repeats
        const int n = 1 << 20;
        Targets T;
        T.first = {0, n};
        T.vi.assign((size_t)n, 3u);
        T.d.assign((size_t)n * 3, 0.25f);
        std::vector<unsigned char> inf;
        CHECK(pack(64, T, 1, RT_MORPH_ARRAY_INFO, inf) == RT_OK);
        RtMorphInfo I;
        std::memcpy(&I, inf.data(), sizeof I);
        CHECK(I.maxPerVertex == n && I.paddedEntries == (uint64_t)n * 64);
        rtl::MorphPlan plan;
        std::string err;
        std::vector<int32_t> first = {0};
        for (int t = 0; t < 32; ++t) first.push_back(first.back() + n);   // 32 targets of 2^20 entries each = 2^25 entries of one vertex
        std::vector<uint32_t> vi((size_t)n * 32, 3u);
        CHECK(rtl::morph_plan(64, first.data(), vi.data(), 32, plan, err) == RT_ERR_UNSUPPORTED && !err.empty());
        first.back() -= 1;
        CHECK(rtl::morph_plan(64, first.data(), vi.data(), 32, plan, err) == RT_OK && plan.info.paddedEntries == (1ull << 31) - 64);
    }
    std::printf(g_fail ? "morph host: %d checks FAILED\n" : "morph host: all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
}
