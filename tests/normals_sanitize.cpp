// The smooth-normal host code (csrc/rt_normal_pack.cpp: the check, the packer of the sliced adjacency, rt_vertex_normals and rt_hit_normals, the
// definitions) driven over its edge cases under AddressSanitizer + UBSan on the CPU (tests/test_normals_host_sanitizers.py).  Linked with
// rt_normal_pack.cpp alone.
#include "rt_mi355.h"
#include "../opengl-raytracing_amd/csrc/rt_normal_pack.hpp"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <vector>

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_fail; } } while (0)

struct MeshCase { std::vector<float> tris; std::vector<int32_t> order; std::vector<uint32_t> idx; int nVerts; };

// nTris triangles over nVerts vertices: vertex `hub` in every third triangle (twice in some), random rows, the rows in a shuffled order
static MeshCase make(int nVerts, int nTris, std::mt19937 &r) {
    MeshCase M;
    M.nVerts = nVerts;
    std::uniform_real_distribution<float> U(-1, 1);
    const uint32_t hub = (uint32_t)(nVerts / 2);
    for (int k = 0; k < nTris; ++k) {
        uint32_t a = r() % (uint32_t)nVerts, b = r() % (uint32_t)nVerts, c = r() % (uint32_t)nVerts;
        if (k % 3 == 0) a = hub;
        if (k % 9 == 0) c = hub;
        if (k == nTris - 1) c = (uint32_t)nVerts - 1;   // the last vertex, in the last lane of its slice
        M.idx.insert(M.idx.end(), {a, b, c});
    }
    M.tris.resize((size_t)nTris * 12);
    for (size_t i = 0; i < M.tris.size(); ++i) M.tris[i] = i % 4 == 3 ? 7.0f : i % 5 == 0 ? 0.0f : i % 7 == 2 ? -0.0f : U(r);
    M.order.resize((size_t)nTris);
    std::iota(M.order.begin(), M.order.end(), 0);
    for (int i = nTris - 1; i > 0; --i) std::swap(M.order[(size_t)i], M.order[r() % (uint32_t)(i + 1)]);
    return M;
}

static int pack(const MeshCase &M, int which, std::vector<unsigned char> &out) {
    size_t n = 0;
    int rc = rt_debug_normal_pack(M.idx.data(), (int)M.idx.size(), M.nVerts, which, nullptr, 0, &n);
    if (rc != RT_OK) return rc;
    out.assign(n, 0xAB);   // exactly the size asked for: a write past it is the sanitizer's to find
    return rt_debug_normal_pack(M.idx.data(), (int)M.idx.size(), M.nVerts, which, out.data(), out.size(), &n);
}

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0; }

int main() {
    std::mt19937 r(1);
    for (int nv : {1, 2, 63, 64, 65, 129, 257, 1000})
        for (int nt : {1, 2, 7, 200, 1000}) {
            const MeshCase M = make(nv, nt, r);
            std::vector<unsigned char> sf, ent, inf;
            CHECK(pack(M, RT_NORMAL_ARRAY_SLICE_FIRST, sf) == RT_OK);
            CHECK(pack(M, RT_NORMAL_ARRAY_ENTRIES, ent) == RT_OK);
            CHECK(pack(M, RT_NORMAL_ARRAY_INFO, inf) == RT_OK && inf.size() == sizeof(RtNormalInfo));
            RtNormalInfo I;
            std::memcpy(&I, inf.data(), sizeof I);
            CHECK(I.nVerts == nv && I.nTris == nt && I.nSlices == (nv + 63) / 64 && I.incidences == (uint64_t)nt * 3);
            CHECK(sf.size() == ((size_t)I.nSlices + 1) * 4 && ent.size() == I.paddedEntries * 4 && I.paddedEntries % 64 == 0);
            // the vertex sums walked from the packed form, lane by lane as the device walks it, equal rt_vertex_normals on the index buffer
            std::vector<float> want((size_t)nv * 3, 5.0f), got((size_t)nv * 3, 0.0f);
            CHECK(rt_vertex_normals(M.tris.data(), M.order.data(), nt, M.idx.data(), nv, want.data()) == RT_OK);
            std::vector<float> face((size_t)nt * 3);
            for (int row = 0; row < nt; ++row) {
                const float *T = M.tris.data() + (size_t)row * 12;
                float *f = face.data() + (size_t)M.order[(size_t)row] * 3;
                f[0] = std::fmaf(T[5], T[10], -(T[6] * T[9])); f[1] = std::fmaf(T[6], T[8], -(T[4] * T[10])); f[2] = std::fmaf(T[4], T[9], -(T[5] * T[8]));
            }
            const uint32_t *first = reinterpret_cast<const uint32_t *>(sf.data());
            const int32_t *e = reinterpret_cast<const int32_t *>(ent.data());
            size_t real = 0;
            for (int v = 0; v < I.nSlices * 64; ++v) {
                const int s = v / 64, l = v % 64;
                float S[3] = {0, 0, 0};
                bool any = false, padSeen = false;
                for (uint32_t at = first[s] + (uint32_t)l; at < first[s + 1]; at += 64) {
                    const int32_t k = e[at];
                    if (k < 0) { padSeen = true; continue; }
                    CHECK(!padSeen && k < nt && v < nv);   // pad entries only behind a vertex's incidences, and only real vertices have any
                    ++real;
                    for (int c = 0; c < 3; ++c) S[c] = any ? S[c] + face[(size_t)k * 3 + c] : face[(size_t)k * 3 + c];
                    any = true;
                }
                if (v >= nv) continue;
                const float d = std::fmaf(S[2], S[2], std::fmaf(S[1], S[1], S[0] * S[0]));
                const bool ok = d > 0.0f && d < std::numeric_limits<float>::infinity();
                const float inv = 1.0f / std::sqrt(d);
                for (int c = 0; c < 3; ++c) got[(size_t)v * 3 + c] = ok ? S[c] * inv : 0.0f;
            }
            CHECK(real == (size_t)nt * 3);
            CHECK(same_bits(got, want));
            // hits: every row, corners and edges, NaN and infinite barycentrics, prims off the mesh; the last hit on exactly-sized arrays
            std::vector<RtHit> hits;
            for (int p = 0; p < nt; ++p) hits.push_back({1.0f, p, (p % 5) * 0.2f, (p % 3) * 0.1f});
            hits.push_back({1.0f, 0, std::numeric_limits<float>::quiet_NaN(), 0.5f});
            hits.push_back({1.0f, nt - 1, 0.5f, std::numeric_limits<float>::infinity()});
            hits.push_back({1.0f, nt - 1, -std::numeric_limits<float>::infinity(), 0.25f});
            const size_t off = hits.size();
            for (int p : {-1, nt, INT_MAX, INT_MIN}) hits.push_back({1.0f, p, 0.25f, 0.25f});
            std::vector<float> out(hits.size() * 3, 9.0f);
            CHECK(rt_hit_normals(M.tris.data(), M.order.data(), nt, M.idx.data(), want.data(), nv, hits.data(), (int)hits.size(), out.data()) == RT_OK);
            for (size_t i = off * 3; i < out.size(); ++i) CHECK(out[i] == 0.0f && !std::signbit(out[i]));
            for (size_t i = 0; i < off * 3; ++i) CHECK(out[i] != 9.0f);
        }
    {   // a fan of valence 200 beside valence-1 vertices: one wide slice, the others one entry wide
        MeshCase F;
        F.nVerts = 401;
        for (uint32_t k = 0; k < 200; ++k) F.idx.insert(F.idx.end(), {0u, 2 * k + 2, 2 * k + 1});
        std::vector<unsigned char> sf, inf;
        CHECK(pack(F, RT_NORMAL_ARRAY_SLICE_FIRST, sf) == RT_OK && pack(F, RT_NORMAL_ARRAY_INFO, inf) == RT_OK);
        RtNormalInfo I;
        std::memcpy(&I, inf.data(), sizeof I);
        const uint32_t *first = reinterpret_cast<const uint32_t *>(sf.data());
        CHECK(I.nSlices == 7 && I.maxPerVertex == 200 && first[1] == 200u * 64u && I.paddedEntries == 200u * 64u + 6u * 64u);
    }
    {   // what must be refused, and the size-query convention
        const MeshCase G = make(65, 7, r);
        size_t n = 77;
        const int nIdx = (int)G.idx.size();
        CHECK(rt_debug_normal_pack(nullptr, nIdx, 65, RT_NORMAL_ARRAY_INFO, nullptr, 0, &n) == RT_ERR_INVALID && n == 0);
        CHECK(rt_debug_normal_pack(G.idx.data(), 0, 65, RT_NORMAL_ARRAY_INFO, nullptr, 0, &n) == RT_ERR_INVALID);
        CHECK(rt_debug_normal_pack(G.idx.data(), nIdx - 1, 65, RT_NORMAL_ARRAY_INFO, nullptr, 0, &n) == RT_ERR_INVALID);
        CHECK(rt_debug_normal_pack(G.idx.data(), nIdx, 0, RT_NORMAL_ARRAY_INFO, nullptr, 0, &n) == RT_ERR_INVALID);
        CHECK(rt_debug_normal_pack(G.idx.data(), nIdx, 64, RT_NORMAL_ARRAY_INFO, nullptr, 0, &n) == RT_ERR_INVALID);   // the last triangle names vertex 64
        CHECK(rt_debug_normal_pack(G.idx.data(), nIdx, 65, RT_NORMAL_ARRAY_INFO, nullptr, 0, nullptr) == RT_ERR_INVALID);
        CHECK(rt_debug_normal_pack(G.idx.data(), nIdx, 65, 55, nullptr, 0, &n) == RT_ERR_INVALID && n == 0);
        std::vector<unsigned char> small(8);
        CHECK(rt_debug_normal_pack(G.idx.data(), nIdx, 65, RT_NORMAL_ARRAY_ENTRIES, small.data(), small.size(), &n) == RT_ERR_INVALID);
        std::vector<float> out(65 * 3);
        CHECK(rt_vertex_normals(G.tris.data(), G.order.data(), 7, G.idx.data(), 64, out.data()) == RT_ERR_INVALID);
        CHECK(rt_vertex_normals(nullptr, G.order.data(), 7, G.idx.data(), 65, out.data()) == RT_ERR_INVALID);
        CHECK(rt_vertex_normals(G.tris.data(), G.order.data(), 0, G.idx.data(), 65, out.data()) == RT_ERR_INVALID);
        std::vector<int32_t> badOrder = G.order;
        badOrder[2] = 7;
        CHECK(rt_vertex_normals(G.tris.data(), badOrder.data(), 7, G.idx.data(), 65, out.data()) == RT_ERR_INVALID);
        badOrder[2] = INT_MIN;
        CHECK(rt_vertex_normals(G.tris.data(), badOrder.data(), 7, G.idx.data(), 65, out.data()) == RT_ERR_INVALID);
        CHECK(rt_vertex_normals(G.tris.data(), G.order.data(), 7, G.idx.data(), 65, out.data()) == RT_OK);
        const RtHit h = {1.0f, 2, 0.25f, 0.25f};
        float o3[3];
        CHECK(rt_hit_normals(G.tris.data(), badOrder.data(), 7, G.idx.data(), out.data(), 65, &h, 1, o3) == RT_ERR_INVALID);
        CHECK(rt_hit_normals(G.tris.data(), G.order.data(), 7, G.idx.data(), out.data(), 65, &h, -1, o3) == RT_ERR_INVALID);
        CHECK(rt_hit_normals(G.tris.data(), G.order.data(), 7, G.idx.data(), out.data(), 65, nullptr, 1, o3) == RT_ERR_INVALID);
        CHECK(rt_hit_normals(G.tris.data(), G.order.data(), 7, G.idx.data(), out.data(), 65, nullptr, 0, nullptr) == RT_OK);
    }
    {   // one vertex named 2^25 + 1 times: its slice of 64 would be 2^31 + 64 entries
        const int nIdx = (1 << 25) + 1;
        std::vector<uint32_t> idx((size_t)nIdx, 0u);
        size_t n = 0;
        CHECK(rt_debug_normal_pack(idx.data(), nIdx, 1, RT_NORMAL_ARRAY_ENTRIES, nullptr, 0, &n) == RT_ERR_UNSUPPORTED && n == 0);
        CHECK(rt_debug_normal_pack(idx.data(), nIdx - 3, 1, RT_NORMAL_ARRAY_INFO, nullptr, 0, &n) == RT_OK && n == sizeof(RtNormalInfo));
    }
    if (g_fail) { std::printf("normals host: %d checks FAILED\n", g_fail); return 1; }
    std::printf("normals host: all checks passed\n");
    return 0;
}
