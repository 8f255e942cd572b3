// rt_multi_hit.cpp -- rt_multi_hits (include/rt_mi355.h): the definition of the multi-hit query.  Host only, no context, no GPU.
//
// For one ray the answer is the set S of triangles traceBVHShadow's loop (shaders/rt/rt_bvh.glsl:260-304) would accept at the limit T with its
// `return true` removed: the root and every node on the way to the triangle's leaf pass aabbHit(...) && tmin <= T, the triangle passes
// triHit(ro, rd, T_i, T).  counts = |S|, hits = the K smallest of S under (key(t), prim).  Nothing is culled against a found hit, so
// the order nodes are visited in does not matter and none is kept.  Written in the float model of DESIGN.md 2: fmaf exactly where dot and cross have
// it, nothing contracted (the Makefile compiles host sources with -ffp-contract=off).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/rt_mi355.h"
#include "rt_bvh_tree.hpp"

namespace {

struct V { float x, y, z; };
inline V ld(const float *p) { return V{p[0], p[1], p[2]}; }
inline V sub(V a, V b) { return V{a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V mulv(V a, V b) { return V{a.x * b.x, a.y * b.y, a.z * b.z}; }
inline float dot(V a, V b) { return std::fmaf(a.z, b.z, std::fmaf(a.y, b.y, a.x * b.x)); }
inline V cross(V a, V b) { return V{std::fmaf(a.y, b.z, -(a.z * b.y)), std::fmaf(a.z, b.x, -(a.x * b.z)), std::fmaf(a.x, b.y, -(a.y * b.x))}; }

// aabbHit, rt_bvh.glsl:124-134 (min / max ignore a NaN operand, as GLSL's on the reference's hardware and the oracle's fmin / fmax)
inline bool aabb_hit(V ro, V rdInv, V bmin, V bmax, float &tminOut) {
    const V t0 = mulv(sub(bmin, ro), rdInv), t1 = mulv(sub(bmax, ro), rdInv);
    const V tsm = {std::fmin(t0.x, t1.x), std::fmin(t0.y, t1.y), std::fmin(t0.z, t1.z)};
    const V tbg = {std::fmax(t0.x, t1.x), std::fmax(t0.y, t1.y), std::fmax(t0.z, t1.z)};
    const float tmin = std::fmax(std::fmax(tsm.x, tsm.y), std::fmax(tsm.z, 0.0f));
    const float tmax = std::fmin(std::fmin(tbg.x, tbg.y), tbg.z);
    tminOut = tmin;
    return tmax >= tmin;
}

// triHit, rt_bvh.glsl:154-170, with uEPS = eps; u, v as it computes them
inline bool tri_hit(V ro, V rd, const float *tri12, float eps, float tMax, float &t, float &uOut, float &vOut) {
    const V v0 = ld(tri12), e1 = ld(tri12 + 4), e2 = ld(tri12 + 8);
    const V pvec = cross(rd, e2);
    const float det = dot(e1, pvec);
    if (std::fabs(det) < 1e-8f) return false;
    const float invDet = 1.0f / det;
    const V tvec = sub(ro, v0);
    const float u = dot(tvec, pvec) * invDet;
    if (u < 0.0f || u > 1.0f) return false;
    const V qvec = cross(tvec, e1);
    const float v = dot(rd, qvec) * invDet;
    if (v < 0.0f || u + v > 1.0f) return false;
    const float tt = dot(e2, qvec) * invDet;
    if (tt < eps || tt > tMax) return false;
    t = tt; uOut = u; vOut = v;
    return true;
}

using rtbvh::Node;   // a node's links, and the tree check rt_nearest.cpp shares (rt_bvh_tree.hpp)
using rtbvh::node_fetch;
using rtbvh::is_tree;

// The monotone map of a float's bits: ascending keys are ascending t, -0 before +0, negative NaNs first and positive NaNs last
inline uint32_t key_of(float t) {
    uint32_t b;
    std::memcpy(&b, &t, 4);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

struct Found { uint32_t key; int32_t prim; float t, u, v; };

}  // namespace

extern "C" int rt_multi_hits(const float *nodes12, int nNodes, const float *tris12, int nTris, const float *origins, int originStride, const float *dirs,
                             int dirStride, const float *tMax, float eps, float inf, int n, int maxHits, RtHit *hits, int32_t *counts) {
    if (maxHits < 0 || maxHits > RT_MULTI_HIT_MAX || n < 0 || nNodes < 0 || nTris < 0 || originStride < 3 || dirStride < 3) return RT_ERR_INVALID;
    if ((nNodes > 0 && !nodes12) || (nTris > 0 && !tris12)) return RT_ERR_INVALID;
    if (n > 0 && (!origins || !dirs || (maxHits > 0 && !hits) || (maxHits == 0 && !counts))) return RT_ERR_INVALID;
    if ((uint64_t)n * (uint64_t)maxHits > (uint64_t)INT32_MAX) return RT_ERR_INVALID;
    try {
        const bool scene = nNodes > 0 && nTris > 0;   // traceBVHShadow: uNodeCount <= 0 || uTriCount <= 0 -> no occluders
        if (scene && !is_tree(nodes12, nNodes, nTris)) return RT_ERR_INVALID;
        const size_t K = (size_t)maxHits;
        std::vector<Found> found;
        std::vector<int> stack;
        for (int i = 0; i < n; ++i) {
            found.clear();
            const float T = tMax ? tMax[i] : inf;
            if (scene && !(tMax && T < 0.0f)) {   // tMax[i] < 0: an empty slot
                const V ro = ld(origins + (size_t)i * originStride), rd = ld(dirs + (size_t)i * dirStride);
                const V rdInv = {1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z};
                stack.assign(1, 0);
                while (!stack.empty()) {
                    const int ni = stack.back();
                    stack.pop_back();
                    const float *p = nodes12 + (size_t)ni * 12;
                    float tminBox;
                    if (!(aabb_hit(ro, rdInv, ld(p), ld(p + 4), tminBox) && tminBox <= T)) continue;
                    const Node N = node_fetch(p);
                    if (N.count > 0) {
                        for (int k = 0; k < N.count; ++k) {
                            Found f;
                            f.prim = N.first + k;
                            if (tri_hit(ro, rd, tris12 + (size_t)f.prim * 12, eps, T, f.t, f.u, f.v)) { f.key = key_of(f.t); found.push_back(f); }
                        }
                    } else {
                        stack.push_back(N.right);
                        stack.push_back(N.left);
                    }
                }
            }
            if (counts) counts[i] = (int32_t)found.size();
            std::sort(found.begin(), found.end(), [](const Found &a, const Found &b) { return a.key != b.key ? a.key < b.key : a.prim < b.prim; });
            for (size_t j = 0; j < K; ++j) {
                RtHit &h = hits[(size_t)i * K + j];
                if (j < found.size()) h = RtHit{found[j].t, found[j].prim, found[j].u, found[j].v};
                else h = RtHit{inf, -1, 0.0f, 0.0f};
            }
        }
    } catch (const std::bad_alloc &) {
        return RT_ERR_IO;
    }
    return RT_OK;
}
