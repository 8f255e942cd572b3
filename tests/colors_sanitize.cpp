// The per-vertex colour host code (csrc/rt_mesh_colors.cpp: rt_hit_colors and rt_color_rows, the definitions, with the arithmetic of
// csrc/rt_mesh_colors.hpp) driven over its edge cases under AddressSanitizer + UBSan on the CPU (tests/test_colors_host_sanitizers.py).  Linked with
// rt_mesh_colors.cpp alone.
#include "rt_mi355.h"

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

struct MeshCase { std::vector<int32_t> order; std::vector<uint32_t> idx; std::vector<float> colors; int nVerts, nTris; };

// nTris triangles over nVerts vertices, random colours, the rows in a shuffled order; every array exactly as long as the call may read
static MeshCase make(int nVerts, int nTris, std::mt19937 &r) {
    MeshCase M;
    M.nVerts = nVerts; M.nTris = nTris;
    std::uniform_real_distribution<float> U(0, 1);
    for (int k = 0; k < nTris; ++k) {
        uint32_t a = r() % (uint32_t)nVerts, b = r() % (uint32_t)nVerts, c = r() % (uint32_t)nVerts;
        if (k == nTris - 1) c = (uint32_t)nVerts - 1;   // the last vertex: its colour ends the array
        M.idx.insert(M.idx.end(), {a, b, c});
    }
    M.colors.resize((size_t)nVerts * 3);
    for (float &c : M.colors) c = U(r);
    M.order.resize((size_t)nTris);
    std::iota(M.order.begin(), M.order.end(), 0);
    for (int i = nTris - 1; i > 0; --i) std::swap(M.order[(size_t)i], M.order[r() % (uint32_t)(i + 1)]);
    return M;
}

static RtHit hit(int prim, float u, float v) { RtHit h; h.t = 1.0f; h.prim = prim; h.u = u; h.v = v; return h; }
static bool same(const float *a, const float *b, int n) { return std::memcmp(a, b, (size_t)n * 4) == 0; }

int main() {
    std::mt19937 r(1);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (int nv : {1, 2, 3, 63, 64, 65, 257, 1000})
        for (int nt : {1, 2, 7, 200, 1000}) {
            const MeshCase M = make(nv, nt, r);
            std::vector<float> rows((size_t)nt * 12, 7.0f);
            CHECK(rt_color_rows(M.order.data(), M.idx.data(), M.colors.data(), nt, nv, rows.data()) == RT_OK);
            for (int i = 0; i < nt; ++i)
                for (int c = 0; c < 3; ++c) {
                    const uint32_t v = M.idx[3 * (size_t)M.order[(size_t)i] + c];
                    CHECK(same(&rows[(size_t)i * 12 + 4 * c], &M.colors[(size_t)v * 3], 3) && rows[(size_t)i * 12 + 4 * c + 3] == 0.0f);
                }
            // hits on every row, on the last row, with barycentrics that are not finite, and off the mesh
            std::vector<RtHit> hits;
            for (int i = 0; i < nt; ++i) hits.push_back(hit(i, 0.25f, 0.5f));
            hits.push_back(hit(nt - 1, 0.0f, 1.0f));
            const size_t special = hits.size();
            for (float a : {nan, inf, -inf}) { hits.push_back(hit(0, a, 0.25f)); hits.push_back(hit(nt - 1, 0.25f, a)); }
            const size_t off = hits.size();
            for (int p : {-1, nt, INT_MAX, INT_MIN}) hits.push_back(hit(p, 0.3f, 0.3f));
            std::vector<float> out(hits.size() * 3, 7.0f);
            CHECK(rt_hit_colors(nullptr, nt, M.order.data(), M.idx.data(), M.colors.data(), nv, hits.data(), (int)hits.size(), out.data()) == RT_OK);
            for (size_t i = 0; i < hits.size(); ++i) {
                const float *o = &out[i * 3];
                if (i >= off) { CHECK(o[0] == 0.0f && o[1] == 0.0f && o[2] == 0.0f); continue; }
                const uint32_t *ix = &M.idx[3 * (size_t)M.order[(size_t)hits[i].prim]];
                const float *c0 = &M.colors[(size_t)ix[0] * 3], *c1 = &M.colors[(size_t)ix[1] * 3], *c2 = &M.colors[(size_t)ix[2] * 3];
                if (i >= special) { CHECK(same(o, c0, 3)); continue; }
                const float a = hits[i].u, b = hits[i].v, w = (1.0f - a) - b;
                for (int c = 0; c < 3; ++c) {
                    volatile float p0 = c0[c] * w, p1 = c1[c] * a, p2 = c2[c] * b, s = p0 + p1, m = s + p2;   // every operation rounded on its own
                    const bool flat = same(c0 + c, c1 + c, 1) && same(c0 + c, c2 + c, 1);   // a channel with three bit-equal corner values: c0's
                    CHECK(flat ? same(o + c, c0 + c, 1) : o[c] == m);
                }
            }
            // the flat rule: one colour at every vertex comes back bit for bit, a + b above 1 included
            std::vector<float> flat((size_t)nv * 3);
            for (int v = 0; v < nv; ++v) { flat[(size_t)v * 3] = 0.85f; flat[(size_t)v * 3 + 1] = 0.1f; flat[(size_t)v * 3 + 2] = 0.7f; }
            std::vector<RtHit> fh = {hit(0, 0.5000001f, 0.5000001f), hit(nt - 1, 0.3333333f, 0.3333334f), hit(nt / 2, 1.5f, -0.25f)};
            std::vector<float> fo(fh.size() * 3);
            CHECK(rt_hit_colors(nullptr, nt, M.order.data(), M.idx.data(), flat.data(), nv, fh.data(), (int)fh.size(), fo.data()) == RT_OK);
            for (size_t i = 0; i < fh.size(); ++i) CHECK(same(&fo[i * 3], flat.data(), 3));
            // refusals read nothing they should not
            CHECK(rt_hit_colors(nullptr, nt, M.order.data(), M.idx.data(), M.colors.data(), nv, hits.data(), 0, nullptr) == RT_OK);
            CHECK(rt_hit_colors(nullptr, nt, M.order.data(), M.idx.data(), M.colors.data(), nv, nullptr, 0, nullptr) == RT_OK);
            CHECK(rt_hit_colors(nullptr, nt, nullptr, M.idx.data(), M.colors.data(), nv, hits.data(), 1, out.data()) == RT_ERR_INVALID);
            CHECK(rt_hit_colors(nullptr, nt, M.order.data(), nullptr, M.colors.data(), nv, hits.data(), 1, out.data()) == RT_ERR_INVALID);
            CHECK(rt_hit_colors(nullptr, nt, M.order.data(), M.idx.data(), nullptr, nv, hits.data(), 1, out.data()) == RT_ERR_INVALID);
            CHECK(rt_hit_colors(nullptr, nt, M.order.data(), M.idx.data(), M.colors.data(), nv, nullptr, 1, out.data()) == RT_ERR_INVALID);
            CHECK(rt_hit_colors(nullptr, nt, M.order.data(), M.idx.data(), M.colors.data(), nv, hits.data(), 1, nullptr) == RT_ERR_INVALID);
            CHECK(rt_hit_colors(nullptr, 0, M.order.data(), M.idx.data(), M.colors.data(), nv, hits.data(), 1, out.data()) == RT_ERR_INVALID);
            CHECK(rt_hit_colors(nullptr, nt, M.order.data(), M.idx.data(), M.colors.data(), 0, hits.data(), 1, out.data()) == RT_ERR_INVALID);
            CHECK(rt_hit_colors(nullptr, nt, M.order.data(), M.idx.data(), M.colors.data(), nv, hits.data(), -1, out.data()) == RT_ERR_INVALID);
            if (nv > 1) {   // the last vertex is named by the last triangle: one vertex fewer is refused before anything past the colours is read
                std::vector<float> fewer(M.colors.begin(), M.colors.end() - 3);
                CHECK(rt_color_rows(M.order.data(), M.idx.data(), fewer.data(), nt, nv - 1, rows.data()) == RT_ERR_INVALID);
                std::vector<RtHit> last = {hit(0, 0.1f, 0.1f)};
                for (int i = 0; i < nt; ++i) if (M.order[(size_t)i] == nt - 1) last[0].prim = i;
                CHECK(rt_hit_colors(nullptr, nt, M.order.data(), M.idx.data(), fewer.data(), nv - 1, last.data(), 1, out.data()) == RT_ERR_INVALID);
            }
            for (int bad : {-1, nt, INT_MAX, INT_MIN}) {
                std::vector<int32_t> o2 = M.order;
                o2[(size_t)(nt / 2)] = bad;
                CHECK(rt_color_rows(o2.data(), M.idx.data(), M.colors.data(), nt, nv, rows.data()) == RT_ERR_INVALID);
                std::vector<RtHit> one = {hit(nt / 2, 0.1f, 0.1f)};
                CHECK(rt_hit_colors(nullptr, nt, o2.data(), M.idx.data(), M.colors.data(), nv, one.data(), 1, out.data()) == RT_ERR_INVALID);
            }
            CHECK(rt_color_rows(nullptr, M.idx.data(), M.colors.data(), nt, nv, rows.data()) == RT_ERR_INVALID);
            CHECK(rt_color_rows(M.order.data(), M.idx.data(), M.colors.data(), nt, nv, nullptr) == RT_ERR_INVALID);
            CHECK(rt_color_rows(M.order.data(), M.idx.data(), M.colors.data(), -1, nv, rows.data()) == RT_ERR_INVALID);
        }
    if (g_fail) { std::printf("colors host: %d checks FAILED\n", g_fail); return 1; }
    std::printf("colors host: all checks passed\n");
    return 0;
}
