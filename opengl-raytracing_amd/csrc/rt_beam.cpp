// rt_beam.cpp -- rt_debug_beam_cull / rt_debug_beam_slab (include/rt_mi355.h; DESIGN.md 4.2 "Beam cull"): the definition of the beam cull on the host.  No context, no
// GPU, links alone.  The tile walk and the interval arithmetic are rt_beam.hpp's, the functions k_beam_cull runs; what is restated here is what the device takes from
// its own headers: the tile deal of rt_frame.hpp and the primary ray of rt.frag:58-68 (primaryDirJ) with primary_pixel's three divisions, operation for operation in
// the float model of DESIGN.md 2 (the Makefile compiles host sources with -ffp-contract=off).
#include <cmath>
#include <cstdint>

#include "../../include/rt_mi355.h"
#include "rt_beam.hpp"

using namespace rtbeam;

namespace {
constexpr int kTile = 16, kRowShift = 11;   // RT_TILE_DIM, kTileRowShift (rt_frame.hpp)

// 1 / primaryDirJ(u, x + 0.5, y + 0.5, jx, jy), per component
void primary_rd_inv(const RtUniforms &u, int x, int y, float jitterX, float jitterY, float *out) {
    const float fcx = (float)x + 0.5f, fcy = (float)y + 0.5f;
    const float jx = (u.enableJitter == 1) ? jitterX : 0.0f, jy = (u.enableJitter == 1) ? jitterY : 0.0f;
    const float uvx = (fcx + jx) / u.resolution[0], uvy = (fcy + jy) / u.resolution[1];
    const float nx = uvx * 2.0f - 1.0f, ny = uvy * 2.0f - 1.0f;
    const float sx = u.tanHalfFov * u.aspect, sy = u.tanHalfFov;
    float d[3];
    for (int a = 0; a < 3; ++a) d[a] = (u.camFwd[a] + (nx * u.camRight[a]) * sx) + (ny * u.camUp[a]) * sy;
    const float inv = 1.0f / std::sqrt(std::fmaf(d[2], d[2], std::fmaf(d[1], d[1], d[0] * d[0])));
    for (int a = 0; a < 3; ++a) out[a] = 1.0f / (d[a] * inv);
}
}  // namespace

extern "C" int rt_debug_beam_cull(const RtUniforms *u, const float *jitters, int batch, int rank, int world, const float *records, int nInner, int rootRef,
                                  const float *rootMin, const float *rootMax, uint8_t *dead, int nLocalTiles, RtBeamCullStats *stats, float *rdInvOut) {
    if (!u || (!dead && nLocalTiles > 0) || !rootMin || !rootMax || batch < 1 || batch > 16 || world < 1 || rank < 0 || rank >= world || nInner < 0 || (nInner > 0 && !records)) return RT_ERR_INVALID;
    if (batch > 1 && !jitters) return RT_ERR_INVALID;
    const int W = (int)u->resolution[0], H = (int)u->resolution[1];
    if (W <= 0 || H <= 0) return RT_ERR_INVALID;
    const int tilesX = (W + kTile - 1) / kTile, tilesY = (H + kTile - 1) / kTile, nTiles = tilesX * tilesY;
    int nl = (nTiles - rank + world - 1) / world;
    if (nl < 0) nl = 0;
    if (nLocalTiles != nl) return RT_ERR_INVALID;
    const bool hasBVH = u->nodeCount > 0 && u->triCount > 0;
    RtBeamCullStats s = {};
    for (int lt = 0; lt < nl; ++lt) {
        const int t = lt * world + rank, ty = t / tilesX, shift = world > 1 ? (ty * kRowShift) % tilesX : 0, tx = (t % tilesX + tilesX - shift) % tilesX;
        Interval I;
        interval_clear(I);
        for (int k = 0; k < batch; ++k) {
            const float jx = jitters ? jitters[2 * k] : u->jitter[0], jy = jitters ? jitters[2 * k + 1] : u->jitter[1];
            for (int y = ty * kTile; y < ty * kTile + kTile && y < H; ++y)
                for (int x = tx * kTile; x < tx * kTile + kTile && x < W; ++x) {
                    float r[3];
                    primary_rd_inv(*u, x, y, jx, jy, r);
                    interval_add(I, r);
                    if (rdInvOut) { float *o = rdInvOut + (((size_t)k * H + y) * W + x) * 3; o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; }
                }
        }
        int levels = 0;
        const Verdict v = hasBVH ? beam_cull_tile(records, nInner, rootRef, rootMin, rootMax, u->camPos, I, &levels) : kAlive;
        dead[lt] = v == kDead ? 1 : 0;
        s.tiles++; s.deadTiles += v == kDead; s.overflowTiles += v == kOverflow; s.levels += (uint64_t)levels;
    }
    if (stats) *stats = s;
    return RT_OK;
}

// n beams from one origin: verdict[i] = beam_cull_tile of the interval (L + 3 i, H + 3 i) -- 0 dead, 1 alive, 2 kept by overflow --, levels[i] the levels walked
extern "C" int rt_debug_beam_walk(int n, const float *ro, const float *L, const float *H, const float *records, int nInner, int rootRef, const float *rootMin,
                                  const float *rootMax, uint8_t *verdict, int32_t *levels) {
    if (n < 0 || nInner < 0 || (nInner > 0 && !records) || !rootMin || !rootMax || (n > 0 && (!ro || !L || !H || !verdict))) return RT_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        Interval I;
        for (int a = 0; a < 3; ++a) { I.L[a] = L[(size_t)i * 3 + a]; I.H[a] = H[(size_t)i * 3 + a]; }
        int lv = 0;
        verdict[i] = (uint8_t)beam_cull_tile(records, nInner, rootRef, rootMin, rootMax, ro, I, &lv);
        if (levels) levels[i] = lv;
    }
    return RT_OK;
}

// n boxes against n intervals: fails[i] = beam_slab_fails, bounds[4 i ..] = {tminLo, tminHi, tmaxLo, tmaxHi} (NaN x 4 where the argument does not apply)
extern "C" int rt_debug_beam_slab(int n, const float *ro, const float *lo, const float *hi, const float *L, const float *H, uint8_t *fails, float *bounds) {
    if (n < 0 || (n > 0 && (!ro || !lo || !hi || !L || !H || !fails))) return RT_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        const size_t o = (size_t)i * 3;
        fails[i] = beam_slab_fails(ro + o, lo + o, hi + o, L + o, H + o) ? 1 : 0;
        if (bounds) {
            float b[4];
            const bool ok = interval_ok(L + o, H + o) && slab_bounds(ro + o, lo + o, hi + o, L + o, H + o, b);
            for (int j = 0; j < 4; ++j) bounds[(size_t)i * 4 + j] = ok ? b[j] : std::nanf("");
        }
    }
    return RT_OK;
}
