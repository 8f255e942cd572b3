// The UV and texture host code (csrc/rt_mesh_uvs.cpp: rt_uv_rows, rt_hit_uvs, rt_srgb_table, rt_sample_texture and rt_load_obj_uv, with the arithmetic
// of csrc/rt_mesh_uvs.hpp) driven over its edge cases under AddressSanitizer + UBSan on the CPU (tests/test_uvs_host_sanitizers.py).  Linked with
// rt_mesh_uvs.cpp alone.  Every array is exactly as long as the call may read.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "rt_mi355.h"

void rt_free(void *p) { std::free(p); }   // (rt_host.cpp's; the loader's buffers are malloc'ed)

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_fail; } } while (0)

static bool same(const float *a, const float *b, int n) { return std::memcmp(a, b, (size_t)n * 4) == 0; }

struct MeshCase { std::vector<int32_t> order; std::vector<uint32_t> idx; std::vector<float> uvs; int nVerts, nTris; };

static MeshCase strip(int nVerts, unsigned seed) {
    MeshCase M;
    M.nVerts = nVerts; M.nTris = nVerts - 2;
    std::mt19937 r(seed);
    std::uniform_real_distribution<float> U(-1.5f, 2.5f);
    for (int t = 0; t < M.nTris; ++t) { M.idx.push_back((uint32_t)t); M.idx.push_back((uint32_t)t + 1); M.idx.push_back((uint32_t)t + 2); }
    for (int t = 0; t < M.nTris; ++t) M.order.push_back(t);
    for (int t = M.nTris - 1; t > 0; --t) std::swap(M.order[(size_t)t], M.order[(size_t)(r() % (unsigned)(t + 1))]);
    M.uvs.resize((size_t)nVerts * 2);
    for (float &c : M.uvs) c = U(r);
    return M;
}

int main(int argc, char **argv) {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (int nv : {3, 4, 63, 64, 65, 1002}) {
        MeshCase M = strip(nv, 11u + (unsigned)nv);
        const int nt = M.nTris;
        std::vector<float> rows((size_t)nt * 8);
        CHECK(rt_uv_rows(M.order.data(), M.idx.data(), M.uvs.data(), nt, nv, rows.data()) == RT_OK);
        for (int i = 0; i < nt; ++i) {
            for (int c = 0; c < 3; ++c) CHECK(same(&rows[(size_t)i * 8 + 2 * c], &M.uvs[(size_t)M.idx[3 * (size_t)M.order[(size_t)i] + c] * 2], 2));
            CHECK(rows[(size_t)i * 8 + 6] == 0.0f && rows[(size_t)i * 8 + 7] == 0.0f);
        }
        std::vector<RtHit> hits;
        const int prims[] = {0, nt - 1, nt / 2, -1, nt, INT_MAX, INT_MIN};
        const float ab[][2] = {{0.25f, 0.5f}, {0.0f, 0.0f}, {1.0f, 0.0f}, {nan, 0.5f}, {0.5f, nan}, {inf, 0.0f}, {0.0f, -inf}, {-0.1f, 1.5f}};
        for (int p : prims)
            for (auto &c : ab) { RtHit h; h.t = 1.0f; h.prim = p; h.u = c[0]; h.v = c[1]; hits.push_back(h); }
        std::vector<float> out(hits.size() * 2, 7.0f);
        CHECK(rt_hit_uvs(hits.data(), (int)hits.size(), M.order.data(), M.idx.data(), M.uvs.data(), nt, nv, out.data()) == RT_OK);
        for (size_t i = 0; i < hits.size(); ++i) {
            const int p = hits[i].prim;
            if (p < 0 || p >= nt) { CHECK(out[2 * i] == 0.0f && out[2 * i + 1] == 0.0f); continue; }
            if (!std::isfinite(hits[i].u) || !std::isfinite(hits[i].v)) CHECK(same(&out[2 * i], &M.uvs[(size_t)M.idx[3 * (size_t)M.order[(size_t)p]] * 2], 2));
        }
        CHECK(rt_hit_uvs(hits.data(), 0, M.order.data(), M.idx.data(), M.uvs.data(), nt, nv, nullptr) == RT_OK);
        CHECK(rt_hit_uvs(nullptr, 0, M.order.data(), M.idx.data(), M.uvs.data(), nt, nv, nullptr) == RT_OK);
        CHECK(rt_hit_uvs(hits.data(), 1, nullptr, M.idx.data(), M.uvs.data(), nt, nv, out.data()) == RT_ERR_INVALID);
        CHECK(rt_hit_uvs(hits.data(), 1, M.order.data(), nullptr, M.uvs.data(), nt, nv, out.data()) == RT_ERR_INVALID);
        CHECK(rt_hit_uvs(hits.data(), 1, M.order.data(), M.idx.data(), nullptr, nt, nv, out.data()) == RT_ERR_INVALID);
        CHECK(rt_hit_uvs(nullptr, 1, M.order.data(), M.idx.data(), M.uvs.data(), nt, nv, out.data()) == RT_ERR_INVALID);
        CHECK(rt_hit_uvs(hits.data(), 1, M.order.data(), M.idx.data(), M.uvs.data(), nt, nv, nullptr) == RT_ERR_INVALID);
        CHECK(rt_hit_uvs(hits.data(), 1, M.order.data(), M.idx.data(), M.uvs.data(), 0, nv, out.data()) == RT_ERR_INVALID);
        CHECK(rt_hit_uvs(hits.data(), 1, M.order.data(), M.idx.data(), M.uvs.data(), nt, 0, out.data()) == RT_ERR_INVALID);
        CHECK(rt_hit_uvs(hits.data(), -1, M.order.data(), M.idx.data(), M.uvs.data(), nt, nv, out.data()) == RT_ERR_INVALID);
        {   // one vertex fewer: the corner that names the last vertex is refused, not read
            std::vector<float> fewer(M.uvs.begin(), M.uvs.end() - 2);
            CHECK(rt_uv_rows(M.order.data(), M.idx.data(), fewer.data(), nt, nv - 1, rows.data()) == RT_ERR_INVALID);
            int row = 0;
            for (int i = 0; i < nt; ++i) if (M.order[(size_t)i] == nt - 1) row = i;
            RtHit last; last.t = 1.0f; last.prim = row; last.u = 0.2f; last.v = 0.3f;
            CHECK(rt_hit_uvs(&last, 1, M.order.data(), M.idx.data(), fewer.data(), nt, nv - 1, out.data()) == RT_ERR_INVALID);
        }
        for (int bad : {-1, nt, INT_MAX, INT_MIN}) {
            std::vector<int32_t> o2 = M.order;
            o2[0] = bad;
            CHECK(rt_uv_rows(o2.data(), M.idx.data(), M.uvs.data(), nt, nv, rows.data()) == RT_ERR_INVALID);
            RtHit one; one.t = 1.0f; one.prim = 0; one.u = 0.2f; one.v = 0.3f;
            CHECK(rt_hit_uvs(&one, 1, o2.data(), M.idx.data(), M.uvs.data(), nt, nv, out.data()) == RT_ERR_INVALID);
        }
        CHECK(rt_uv_rows(nullptr, M.idx.data(), M.uvs.data(), nt, nv, rows.data()) == RT_ERR_INVALID);
        CHECK(rt_uv_rows(M.order.data(), M.idx.data(), M.uvs.data(), nt, nv, nullptr) == RT_ERR_INVALID);
        CHECK(rt_uv_rows(M.order.data(), M.idx.data(), M.uvs.data(), -1, nv, rows.data()) == RT_ERR_INVALID);
    }
    // ---- the decode table
    float srgb[256];
    CHECK(rt_srgb_table(srgb) == RT_OK && srgb[0] == 0.0f && srgb[255] == 1.0f);
    for (int c = 1; c < 256; ++c) CHECK(srgb[c] > srgb[c - 1]);
    CHECK(rt_srgb_table(nullptr) == RT_ERR_INVALID);
    // ---- samples: every size and flag combination over the special coordinates, on texel arrays of exactly W * H * 4 bytes
    const float special[] = {0.0f, 1.0f, -1.4e-45f, -0.25f, 3.75f, 1e9f, -1e9f, nan, inf, -inf, 0.5f, 0.999999f, 1e-7f, 0.25f, 1.0f / 3.0f, -0.0f, 2.0f, -1.0f};
    std::vector<float> uv;
    for (float u : special) for (float v : special) { uv.push_back(u); uv.push_back(v); }
    const int n = (int)uv.size() / 2;
    const int sizes[][2] = {{1, 1}, {2, 2}, {3, 5}, {1, 7}, {64, 64}, {RT_TEX_MAX_SIZE, 1}, {1, RT_TEX_MAX_SIZE}};
    std::mt19937 r(5);
    for (auto &s : sizes) {
        const int W = s[0], H = s[1];
        std::vector<uint8_t> tex((size_t)W * H * 4), white((size_t)W * H * 4, 255);
        for (uint8_t &b : tex) b = (uint8_t)(r() & 255u);
        for (int flags = 0; flags < 8; ++flags) {
            std::vector<float> out((size_t)n * 3, -1.0f);
            CHECK(rt_sample_texture(tex.data(), W, H, flags, uv.data(), n, out.data()) == RT_OK);
            for (float x : out) CHECK(x >= 0.0f && x <= 1.0f);
            CHECK(rt_sample_texture(white.data(), W, H, flags, uv.data(), n, out.data()) == RT_OK);
            for (float x : out) CHECK(x == 1.0f);   // the white anchor
        }
    }
    {
        std::vector<uint8_t> tex(3 * 5 * 4, 9);
        std::vector<float> out((size_t)n * 3);
        CHECK(rt_sample_texture(tex.data(), 3, 5, 0, uv.data(), 0, nullptr) == RT_OK);
        CHECK(rt_sample_texture(nullptr, 3, 5, 0, uv.data(), n, out.data()) == RT_ERR_INVALID);
        CHECK(rt_sample_texture(tex.data(), 3, 5, 0, nullptr, n, out.data()) == RT_ERR_INVALID);
        CHECK(rt_sample_texture(tex.data(), 3, 5, 0, uv.data(), n, nullptr) == RT_ERR_INVALID);
        CHECK(rt_sample_texture(tex.data(), 0, 5, 0, uv.data(), n, out.data()) == RT_ERR_INVALID);
        CHECK(rt_sample_texture(tex.data(), 3, -1, 0, uv.data(), n, out.data()) == RT_ERR_INVALID);
        CHECK(rt_sample_texture(tex.data(), RT_TEX_MAX_SIZE + 1, 1, 0, uv.data(), n, out.data()) == RT_ERR_INVALID);
        CHECK(rt_sample_texture(tex.data(), 3, 5, 8, uv.data(), n, out.data()) == RT_ERR_INVALID);
        CHECK(rt_sample_texture(tex.data(), 3, 5, -1, uv.data(), n, out.data()) == RT_ERR_INVALID);
        CHECK(rt_sample_texture(tex.data(), 3, 5, 0, uv.data(), -1, out.data()) == RT_ERR_INVALID);
    }
    // ---- the .obj reader, on texts written here (argv[1]: a directory to write them in)
    if (argc > 1) {
        const std::string path = std::string(argv[1]) + "/uvs_sanitize.obj";
        const char *texts[] = {
            "v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nvt 0.5 0.5\nf 1/1 2/2 3/3\nf 2/4 4/2 3/3\n",
            "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 0 1\nf 1/1/1 2/2/1 3/3 4/4/1\n",
            "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0.25 0.5\nvt 0.75 0.5\nvt 0.5 1\nf -3/-3 -2/-2 -1/-1\n",
            "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0.5 0.5\nf 1 2 3\nf 1/1 2//1 3\n",
            "", "f\nvt\nv\n# nothing\n", "v 0 0 0\nf 1/ 1/ 1/\n"};
        const int wantVerts[] = {5, 4, 3, 4, 0, 0, 1}, wantIdx[] = {6, 6, 3, 6, 0, 0, 3};
        for (size_t k = 0; k < sizeof texts / sizeof texts[0]; ++k) {
            FILE *f = std::fopen(path.c_str(), "wb");
            CHECK(f != nullptr);
            if (!f) break;
            std::fputs(texts[k], f);
            std::fclose(f);
            float *pos = nullptr, *uvs = nullptr; uint32_t *idx = nullptr; int nv = -1, ni = -1;
            CHECK(rt_load_obj_uv(path.c_str(), &pos, &uvs, &nv, &idx, &ni) == RT_OK);
            CHECK(nv == wantVerts[k] && ni == wantIdx[k]);
            for (int i = 0; i < ni; ++i) CHECK(idx[i] < (uint32_t)nv);
            float acc = 0.0f;
            for (int i = 0; i < nv * 3; ++i) acc += pos[i];
            for (int i = 0; i < nv * 2; ++i) acc += uvs[i];
            CHECK(std::isfinite(acc));
            rt_free(pos); rt_free(uvs); rt_free(idx);
        }
        for (const char *bad : {"v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/2 2/1 3/1\n", "v 0 0 0\nf 1 2 3\n", "v 0 0 0\nvt 0 0\nf 1/-2 1/1 1/1\n"}) {
            FILE *f = std::fopen(path.c_str(), "wb");
            CHECK(f != nullptr);
            if (!f) break;
            std::fputs(bad, f);
            std::fclose(f);
            float *pos = nullptr, *uvs = nullptr; uint32_t *idx = nullptr; int nv = -1, ni = -1;
            CHECK(rt_load_obj_uv(path.c_str(), &pos, &uvs, &nv, &idx, &ni) == RT_ERR_IO);
            CHECK(pos == nullptr && uvs == nullptr && idx == nullptr);
        }
        std::remove(path.c_str());
        float *pos = nullptr, *uvs = nullptr; uint32_t *idx = nullptr; int nv = -1, ni = -1;
        CHECK(rt_load_obj_uv(path.c_str(), &pos, &uvs, &nv, &idx, &ni) == RT_ERR_IO);
        CHECK(rt_load_obj_uv(nullptr, &pos, &uvs, &nv, &idx, &ni) == RT_ERR_INVALID);
        CHECK(rt_load_obj_uv(path.c_str(), &pos, nullptr, &nv, &idx, &ni) == RT_ERR_INVALID);
    }
    if (g_fail) { std::printf("uvs host: %d checks FAILED\n", g_fail); return 1; }
    std::printf("uvs host: all checks passed\n");
    return 0;
}
