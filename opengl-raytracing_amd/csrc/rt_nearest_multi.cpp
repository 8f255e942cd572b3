// rt_nearest_multi.cpp -- rt_nearest_points_multi (include/rt_mi355.h): the definition of the proximity query, and the block size of its
// device launch.  Host only, no context, no GPU.
//
// For one point p, S is the set of rows t with e(t) <= L, e(t) exactly rt_nearest_points' (rt_nearest.cpp): the row's squared distance
// d2(t) raised to the largest box bound on the way from the root to its leaf.  The count is |S|; the records are the maxHits least elements of S under
// (e(t), prim).  e(t) is a function of the row and the point alone, so the walk (rt_nearest_rows.hpp, shared with rt_nearest.cpp) visits every node,
// carries the running maximum and culls nothing; this file collects S and sorts it.  The device walk (rt_nearest_multi.hip) culls against its K-th
// best and is held to this answer bit for bit; DESIGN.md 22.2 has the proof that it may.  The float operations are rt_nearest_math.hpp's, the text
// the device compiles too.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <new>
#include <utility>
#include <vector>

#include "../../include/rt_mi355.h"
#include "rt_nearest_multi_block.hpp"
#include "rt_nearest_rows.hpp"

using namespace rtnear;

extern "C" int rt_nearest_points_multi(const float *nodes12, int nNodes, const float *tris12, int nTris, const float *points, int stride, const float *maxDist,
                                       int n, int maxHits, RtHit *hits, int32_t *counts, float *closest) {
    if (maxHits < 0 || maxHits > RT_NEAREST_MULTI_MAX) return RT_ERR_INVALID;
    if (n < 0 || nNodes < 0 || nTris < 0 || stride < 3) return RT_ERR_INVALID;
    if ((nNodes > 0 && !nodes12) || (nTris > 0 && !tris12)) return RT_ERR_INVALID;
    if (n > 0 && (!points || (maxHits > 0 && !hits) || (maxHits == 0 && !counts))) return RT_ERR_INVALID;
    if ((uint64_t)n * (uint64_t)maxHits > (uint64_t)INT32_MAX) return RT_ERR_INVALID;
    if ((uint64_t)(n > 0 ? n - 1 : 0) * (uint64_t)stride + 3 > ((uint64_t)1 << 32)) return RT_ERR_INVALID;
    try {
        const bool scene = nNodes > 0 && nTris > 0;
        if (scene && !rtbvh::is_tree(nodes12, nNodes, nTris)) return RT_ERR_INVALID;
        const size_t K = (size_t)maxHits;
        std::vector<std::pair<int, float>> stack;
        std::vector<std::pair<float, int>> S;       // (e, prim) of the accepted rows: std::pair orders as (e, prim), no e is NaN
        for (int i = 0; i < n; ++i) {
            const V p = ld(points + (size_t)i * stride);
            const float md = maxDist ? maxDist[i] : 0.0f;
            const float L = maxDist ? md * md : INFINITY;
            S.clear();
            if (scene && !(maxDist && md < 0.0f) && finite3(p))   // maxDist[i] < 0 or a non-finite coordinate: an empty slot
                for_each_row(nodes12, tris12, p, stack, [&](int prim, float e) {
                    if (e <= L) S.push_back({e, prim});
                });
            if (counts) counts[i] = (int32_t)S.size();
            const size_t kept = std::min(K, S.size());
            std::partial_sort(S.begin(), S.begin() + (ptrdiff_t)kept, S.end());
            for (size_t j = 0; j < K; ++j) {
                const size_t slot = (size_t)i * K + j;
                V c = {0.0f, 0.0f, 0.0f};
                if (j < kept) {   // u, v and c of the winners alone: the same closest_uv on the same operands
                    const float *t = tris12 + (size_t)S[j].second * 12;
                    const V v0 = ld(t), e1 = ld(t + 4), e2 = ld(t + 8);
                    float u, v;
                    closest_uv(p, v0, e1, e2, u, v);
                    c = point_at(v0, e1, e2, u, v);
                    hits[slot] = RtHit{S[j].first, S[j].second, u, v};
                } else hits[slot] = RtHit{INFINITY, -1, 0.0f, 0.0f};
                if (closest) { closest[slot * 3] = c.x; closest[slot * 3 + 1] = c.y; closest[slot * 3 + 2] = c.z; }
            }
        }
    } catch (const std::bad_alloc &) {
        return RT_ERR_IO;
    }
    return RT_OK;
}

extern "C" int rt_debug_nearest_multi_block(int stackEntries, int maxHits, int *threads, int64_t *ldsBytes) {
    if (stackEntries < 1 || stackEntries > RT_NEAREST_MULTI_STACK_MAX || maxHits < 0 || maxHits > RT_NEAREST_MULTI_MAX || !threads || !ldsBytes) return RT_ERR_INVALID;
    *threads = rt_nearest_multi_block(stackEntries, maxHits);
    *ldsBytes = (int64_t)rt_nearest_multi_lds(*threads, stackEntries, maxHits);
    return RT_OK;
}
