// The beam cull's host definition (csrc/rt_beam.cpp: rt_debug_beam_cull, rt_debug_beam_slab, rt_debug_beam_walk) driven over its edge cases under
// AddressSanitizer + UBSan on the CPU (tests/test_beam_cull_host_sanitizers.py).  Linked with rt_beam.cpp alone.  Every array is exactly as long as the call
// may read or write.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_mi355.h"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

static float as_ref(int ref) { float f; std::memcpy(&f, &ref, 4); return f; }

// a complete tree of `depth` levels of inner nodes over the unit cube cut along x: node i has children 2 i + 1, 2 i + 2; the last level's children are leaves
static std::vector<float> make_tree(int depth, int &nInner) {
    nInner = (1 << depth) - 1;
    std::vector<float> rec((size_t)nInner * 16);
    struct Span { float lo, hi; };
    std::vector<Span> span((size_t)nInner);
    span[0] = {0.0f, 1.0f};
    for (int i = 0; i < nInner; ++i) {
        const float mid = 0.5f * (span[i].lo + span[i].hi);
        const int l = 2 * i + 1, r = 2 * i + 2;
        const bool leaf = l >= nInner;
        float *q = &rec[(size_t)i * 16];
        q[0] = span[i].lo; q[1] = 0; q[2] = 0; q[3] = as_ref(leaf ? -(i * 2 + 1) : l);
        q[4] = mid; q[5] = 1; q[6] = 1; q[7] = as_ref(leaf ? -(i * 2 + 2) : r);
        q[8] = mid; q[9] = 0; q[10] = 0; q[11] = 0;
        q[12] = span[i].hi; q[13] = 1; q[14] = 1; q[15] = 0;
        if (!leaf) { span[l] = {span[i].lo, mid}; span[r] = {mid, span[i].hi}; }
    }
    return rec;
}

static RtUniforms make_uniforms(int w, int h, float px, float py, float pz) {
    RtUniforms u;
    std::memset(&u, 0, sizeof u);
    u.camPos[0] = px; u.camPos[1] = py; u.camPos[2] = pz;
    u.camRight[0] = 1; u.camUp[1] = 1; u.camFwd[2] = -1;
    u.tanHalfFov = 0.5f; u.aspect = (float)w / (float)h;
    u.resolution[0] = (float)w; u.resolution[1] = (float)h;
    u.enableJitter = 1; u.nodeCount = 1; u.triCount = 1;
    return u;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    int nInner = 0;
    const std::vector<float> tree = make_tree(8, nInner);      // 255 records, 128 inner nodes in the last level
    const float rootMin[3] = {0, 0, 0}, rootMax[3] = {1, 1, 1};
    // frames: sizes that are no multiple of the tile, one pixel, ranks of a world, batches of 1 and 16
    for (int w : {1, 17, 64}) for (int h : {1, 33}) for (int world : {1, 3}) for (int rank = 0; rank < world; ++rank) for (int batch : {1, 16}) {
        const int tiles = ((w + 15) / 16) * ((h + 15) / 16);
        int nl = (tiles - rank + world - 1) / world; if (nl < 0) nl = 0;
        RtUniforms u = make_uniforms(w, h, 0.3f, 0.4f, 3.0f);
        std::vector<float> jit((size_t)batch * 2);
        for (int k = 0; k < batch; ++k) { jit[2 * k] = 0.03f * (float)k - 0.2f; jit[2 * k + 1] = 0.2f - 0.02f * (float)k; }
        std::vector<uint8_t> dead((size_t)nl, 7);
        std::vector<float> rd((size_t)batch * w * h * 3);
        RtBeamCullStats st;
        CHECK(rt_debug_beam_cull(&u, jit.data(), batch, rank, world, tree.data(), nInner, 0, rootMin, rootMax, dead.data(), nl, &st, rd.data()) == RT_OK);
        CHECK(st.tiles == (uint64_t)nl);
        uint64_t d = 0; for (uint8_t v : dead) { CHECK(v <= 1); d += v; }
        CHECK(d == st.deadTiles);
        CHECK(rt_debug_beam_cull(&u, batch > 1 ? jit.data() : nullptr, batch, rank, world, tree.data(), nInner, 0, rootMin, rootMax, dead.data(), nl, nullptr, nullptr) == RT_OK);   // (one frame: u.jitter)
        CHECK(rt_debug_beam_cull(&u, jit.data(), batch, rank, world, tree.data(), nInner, 0, rootMin, rootMax, dead.data(), nl + 1, nullptr, nullptr) == RT_ERR_INVALID);
    }
    {   // a camera that looks away: every tile dead at the root box; a root that is a leaf; no tree at all; hasBVH == 0
        RtUniforms u = make_uniforms(32, 32, 0.5f, 0.5f, -3.0f);
        u.camFwd[0] = 0.8f; u.camFwd[1] = 0.8f;     // (no axis changes sign inside a tile)
        uint8_t dead[4]; RtBeamCullStats st;
        CHECK(rt_debug_beam_cull(&u, nullptr, 1, 0, 1, tree.data(), nInner, 0, rootMin, rootMax, dead, 4, &st, nullptr) == RT_OK && st.deadTiles == 4 && st.levels == 0);
        CHECK(rt_debug_beam_cull(&u, nullptr, 1, 0, 1, nullptr, 0, -1, rootMin, rootMax, dead, 4, &st, nullptr) == RT_OK && st.deadTiles == 4);
        u.nodeCount = 0;
        CHECK(rt_debug_beam_cull(&u, nullptr, 1, 0, 1, tree.data(), nInner, 0, rootMin, rootMax, dead, 4, &st, nullptr) == RT_OK && st.deadTiles == 0);
        u.nodeCount = 1;
        CHECK(rt_debug_beam_cull(nullptr, nullptr, 1, 0, 1, tree.data(), nInner, 0, rootMin, rootMax, dead, 4, &st, nullptr) == RT_ERR_INVALID);
        CHECK(rt_debug_beam_cull(&u, nullptr, 2, 0, 1, tree.data(), nInner, 0, rootMin, rootMax, dead, 4, &st, nullptr) == RT_ERR_INVALID);
        CHECK(rt_debug_beam_cull(&u, nullptr, 17, 0, 1, tree.data(), nInner, 0, rootMin, rootMax, dead, 4, &st, nullptr) == RT_ERR_INVALID);
        CHECK(rt_debug_beam_cull(&u, nullptr, 1, 1, 1, tree.data(), nInner, 0, rootMin, rootMax, dead, 4, &st, nullptr) == RT_ERR_INVALID);
        CHECK(rt_debug_beam_cull(&u, nullptr, 1, 0, 1, nullptr, 3, 0, rootMin, rootMax, dead, 4, &st, nullptr) == RT_ERR_INVALID);
    }
    {   // the walk: a narrow beam dies or finds a leaf, a beam over the whole cube overflows the 64-node frontier, references outside the records keep the beam
        const float ro[3] = {3.0f, 2.5f, 4.0f};
        auto rinv = [&](float x, float y, float z, float *out) { const float d[3] = {x - ro[0], y - ro[1], z - ro[2]}; const float n = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]); for (int a = 0; a < 3; ++a) out[a] = 1.0f / (d[a] / n); };
        float L[3] = {0, 0, 0}, H[3] = {0, 0, 0}, r[3];
        bool first = true;
        for (int i = 0; i < 8; ++i) {
            rinv((float)(i & 1), (float)((i >> 1) & 1), (float)(i >> 2), r);
            for (int a = 0; a < 3; ++a) { if (first || r[a] < L[a]) L[a] = r[a]; if (first || r[a] > H[a]) H[a] = r[a]; }
            first = false;
        }
        uint8_t v = 9; int32_t lv = -1;
        CHECK(rt_debug_beam_walk(1, ro, L, H, tree.data(), nInner, 0, rootMin, rootMax, &v, &lv) == RT_OK && v == 2 && lv == 7);
        rinv(0.51f, 0.5f, 0.5f, r);     // one ray, but it crosses every cut of the cube: 128 cells
        CHECK(rt_debug_beam_walk(1, ro, r, r, tree.data(), nInner, 0, rootMin, rootMax, &v, &lv) == RT_OK && v == 2 && lv == 7);
        {   // a ray that stays inside a cell or two: down to a leaf
            const float ro2[3] = {0.511f, 2.5f, 4.0f}, d2[3] = {0.001f, -2.0f, -3.5f};
            const float n2 = std::sqrt(d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2]);
            float r2[3];
            for (int a = 0; a < 3; ++a) r2[a] = 1.0f / (d2[a] / n2);
            CHECK(rt_debug_beam_walk(1, ro2, r2, r2, tree.data(), nInner, 0, rootMin, rootMax, &v, &lv) == RT_OK && v == 1 && lv == 8);
        }
        rinv(5.0f, 0.5f, 0.5f, r);     // past the cube
        CHECK(rt_debug_beam_walk(1, ro, r, r, tree.data(), nInner, 0, rootMin, rootMax, &v, nullptr) == RT_OK && v == 0);
        rinv(0.51f, 0.5f, 0.5f, r);
        CHECK(rt_debug_beam_walk(1, ro, r, r, tree.data(), 3, 0, rootMin, rootMax, &v, &lv) == RT_OK && v == 1 && lv == 2);      // children 3 .. 6 lie outside 3 records
        CHECK(rt_debug_beam_walk(1, ro, r, r, tree.data(), nInner, nInner, rootMin, rootMax, &v, &lv) == RT_OK && v == 1 && lv == 0);
        CHECK(rt_debug_beam_walk(1, ro, r, r, nullptr, 0, -1, rootMin, rootMax, &v, &lv) == RT_OK && v == 1);
        CHECK(rt_debug_beam_walk(0, nullptr, nullptr, nullptr, nullptr, 0, -1, rootMin, rootMax, nullptr, nullptr) == RT_OK);
        CHECK(rt_debug_beam_walk(1, ro, r, r, nullptr, 2, 0, rootMin, rootMax, &v, &lv) == RT_ERR_INVALID);
        CHECK(rt_debug_beam_walk(-1, ro, r, r, tree.data(), nInner, 0, rootMin, rootMax, &v, &lv) == RT_ERR_INVALID);
    }
    {   // the slab: what the argument does not cover is kept, with NaN bounds
        const float ro[3] = {0, 0, 0}, lo[3] = {10, 10, 10}, hi[3] = {11, 11, 11};
        const float bad[][2] = {{0.0f, 1.0f}, {-1.0f, 0.0f}, {-1.0f, 1.0f}, {1.0f, inf}, {-inf, -1.0f}, {nan, 1.0f}, {1.0f, nan}, {1e-41f, 1.0f}, {-1.0f, -1e-41f}, {2.0f, 1.0f}, {-0.0f, -0.0f}};
        for (const auto &b : bad) for (int a = 0; a < 3; ++a) {
            float L[3] = {-2, -2, -2}, H[3] = {-1, -1, -1}, bounds[4]; uint8_t f = 9;
            L[a] = b[0]; H[a] = b[1];
            CHECK(rt_debug_beam_slab(1, ro, lo, hi, L, H, &f, bounds) == RT_OK && f == 0 && std::isnan(bounds[0]) && std::isnan(bounds[3]));
        }
        float L[3] = {-2, -2, -2}, H[3] = {-1, -1, -1}, bounds[4]; uint8_t f = 9;
        CHECK(rt_debug_beam_slab(1, ro, lo, hi, L, H, &f, bounds) == RT_OK && f == 1 && bounds[3] < bounds[0]);
        CHECK(rt_debug_beam_slab(1, ro, lo, hi, L, H, &f, nullptr) == RT_OK && f == 1);
        const float huge[3] = {3e38f, 3e38f, 3e38f}, mhuge[3] = {-3e38f, -3e38f, -3e38f}, nlo[3] = {nan, 10, 10};
        CHECK(rt_debug_beam_slab(1, mhuge, lo, huge, L, H, &f, bounds) == RT_OK && f == 0);      // hi - ro overflows: not finite
        CHECK(rt_debug_beam_slab(1, ro, nlo, hi, L, H, &f, bounds) == RT_OK && f == 0);
        CHECK(rt_debug_beam_slab(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RT_OK);
        CHECK(rt_debug_beam_slab(1, ro, lo, hi, L, H, nullptr, bounds) == RT_ERR_INVALID);
        CHECK(rt_debug_beam_slab(-1, ro, lo, hi, L, H, &f, bounds) == RT_ERR_INVALID);
    }
    if (failures == 0) std::printf("beam cull host: all checks passed\n");
    return failures == 0 ? 0 : 1;
}
