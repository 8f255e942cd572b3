// rt_nearest.cpp -- rt_nearest_points (include/rt_mi355.h): the definition of the nearest-point query.  Host only, no context, no GPU.
//
// For one point p the answer is the triangle least under (e(t), prim) among those with e(t) <= L, where e(t) is the triangle's squared distance d2(t)
// raised to the largest box bound lb(box(n), p) on the way from the root to its leaf (one line per operation; rt_nearest_math.hpp,
// which the device compiles too, and the walk of rt_nearest_rows.hpp, shared with rt_nearest_multi.cpp, are that text).  e(t) is a function of the
// triangle and the point alone, so that walk visits every node, carries the running maximum and culls nothing: the order nodes are visited in does
// not matter and none is kept.  The device walk (rt_nearest.hip) culls against its best and is held to this answer bit for
// bit; DESIGN.md 21.2 has the proof that it may.  Written in the float model of DESIGN.md 2: fmaf exactly where dot and cross have it, nothing
// contracted (the Makefile compiles host sources with -ffp-contract=off).
#include <cmath>
#include <cstdint>
#include <new>
#include <utility>
#include <vector>

#include "../../include/rt_mi355.h"
#include "rt_nearest_rows.hpp"

using namespace rtnear;

extern "C" int rt_nearest_points(const float *nodes12, int nNodes, const float *tris12, int nTris, const float *points, int stride, const float *maxDist, int n,
                                 RtHit *hits, float *closest) {
    if (n < 0 || nNodes < 0 || nTris < 0 || stride < 3) return RT_ERR_INVALID;
    if ((nNodes > 0 && !nodes12) || (nTris > 0 && !tris12)) return RT_ERR_INVALID;
    if (n > 0 && (!points || !hits)) return RT_ERR_INVALID;
    if ((uint64_t)(n > 0 ? n - 1 : 0) * (uint64_t)stride + 3 > ((uint64_t)1 << 32)) return RT_ERR_INVALID;
    try {
        const bool scene = nNodes > 0 && nTris > 0;
        if (scene && !rtbvh::is_tree(nodes12, nNodes, nTris)) return RT_ERR_INVALID;
        std::vector<std::pair<int, float>> stack;
        for (int i = 0; i < n; ++i) {
            const V p = ld(points + (size_t)i * stride);
            const float md = maxDist ? maxDist[i] : 0.0f;
            const float L = maxDist ? md * md : INFINITY;
            bool have = false;
            float best = 0.0f;
            int bprim = -1;
            if (scene && !(maxDist && md < 0.0f) && finite3(p))   // maxDist[i] < 0 or a non-finite coordinate: an empty slot
                for_each_row(nodes12, tris12, p, stack, [&](int prim, float e) {
                    if (!(e <= L)) return;   // (a NaN e too)
                    if (!have || e < best || (e == best && prim < bprim)) { have = true; best = e; bprim = prim; }
                });
            V c = {0.0f, 0.0f, 0.0f};
            if (have) {   // u, v and c of the winner alone: the same closest_uv on the same operands
                const float *t = tris12 + (size_t)bprim * 12;
                const V v0 = ld(t), e1 = ld(t + 4), e2 = ld(t + 8);
                float u, v;
                closest_uv(p, v0, e1, e2, u, v);
                c = point_at(v0, e1, e2, u, v);
                hits[i] = RtHit{best, bprim, u, v};
            } else hits[i] = RtHit{INFINITY, -1, 0.0f, 0.0f};
            if (closest) { closest[(size_t)i * 3] = c.x; closest[(size_t)i * 3 + 1] = c.y; closest[(size_t)i * 3 + 2] = c.z; }
        }
    } catch (const std::bad_alloc &) {
        return RT_ERR_IO;
    }
    return RT_OK;
}
