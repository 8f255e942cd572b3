// rt_raster.hip -- the raster preview of the reference (renderRaster, src/render/render.cpp:244-295): flat-coloured meshes through
// basic.vert / basic.frag with GL_LESS on a D24 buffer.  The rules (mirrored by tests/raster_ref.py) are exact integer /
// fixed-order fp32 arithmetic, so every triangle's contribution to a pixel is a 64-bit key (d24 << 32 | global primitive index) and a
// pixel keeps the smallest: the kernels may visit triangles in any order and the frame is still GL's in-order result.
//   k_rs_part_mvp  (draws of a slot bound to the dynamic mesh in parts mode) one lane per part: the part's MVP from the device matrix table
//   k_rs_setup   one lane per triangle of one draw: index fetch, MVP, clip (near + guard band), snap, tile rectangle, record; a template over where
//                the MVP and the colour come from (StaticDraw: the kernel arguments; PartsDraw: the triangle's part)
//   scan         rocprim exclusive scan of the per-triangle tile counts
//   k_rs_scatter (tile, triangle) pairs at the scanned offsets; a triangle whose pairs would pass the capacity writes none
//   sort         rocprim radix sort of the pairs by tile (stable: triangle order inside a tile)
//   k_rs_ranges  [begin, end) of every tile's pairs
//   k_rs_raster  one wave per 16 x 16 tile, four pixels per lane, running minimum key in registers over the tile's triangles (and over
//                the triangles past the capacity, tested against their tile rectangle), then the resolve to RGBA8 / primId / depth24
// No global atomics on the raster path (the setup tallies for RtRasterStats are one atomic per wave).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt_mi355.h"
#include "rt_wave.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kTile = 16;                 // raster tile: 16 x 16 pixels, one wave of 64 lanes, four pixels per lane
constexpr int kMaxPoly = 8;               // a triangle clipped by five planes has at most 3 + 5 vertices
constexpr int kVertInts = kMaxPoly * 3;   // record vertices: (x, y) in 1/256 pixel + z_w bits
constexpr float kGuardPixels2 = 2097152.0f;   // 2 x the guard band (2^20 pixels beyond each side of the viewport), see DESIGN.md 11
constexpr uint32_t kBg = 0xFFFFFFFFu;

// Where a draw's triangles, MVP and colour come from: the source policy of k_rs_setup (QuerySrc / SceneSrc in rt_wave.hip are the pattern).
// StaticDraw: one MVP and one colour for the whole draw, in the kernel arguments -- a static slot, or the dynamic mesh's own arrays bound with
// RT_RASTER_BIND_SINGLE.  `m` is read through a pointer into the kernel arguments, so it stays in scalar registers.
struct StaticDraw {
    float m[16];               // MVP = P * V * M, column-major
    const float *pos;          // 3 floats per vertex
    const uint32_t *idx;       // validated < nVerts on upload
    uint32_t triBase, nTris;   // global index of the draw's first triangle, triangles in the draw
    uint32_t rgba;
    __device__ __forceinline__ const float *mvp(uint32_t, float *) const { return m; }
    __device__ __forceinline__ uint32_t color(uint32_t) const { return rgba; }
};
// PartsDraw: the dynamic mesh bound with RT_RASTER_BIND_PARTS.  Thread i owns input triangle i: one coalesced 2-byte load of its part, then the part's
// 64-byte entry of the call's MVP table (k_rs_part_mvp) as four 16-byte loads, then the part's packed colour when a colour table is set.
struct PartsDraw {
    const float *pos;
    const uint32_t *idx;
    uint32_t triBase, nTris;
    uint32_t rgba;                 // the draw's own colour (partRGBA == null)
    const uint16_t *partOf;        // [input triangle] -> part
    const float4 *partMvp;         // [part] -> MVP, four float4 columns
    const uint32_t *partRGBA;      // [part] -> packed colour, or null
    __device__ __forceinline__ const float *mvp(uint32_t i, float *tmp) const {
        const float4 *M = partMvp + (size_t)partOf[i] * 4;
        const float4 c0 = M[0], c1 = M[1], c2 = M[2], c3 = M[3];
        tmp[0] = c0.x; tmp[1] = c0.y; tmp[2] = c0.z; tmp[3] = c0.w; tmp[4] = c1.x; tmp[5] = c1.y; tmp[6] = c1.z; tmp[7] = c1.w;
        tmp[8] = c2.x; tmp[9] = c2.y; tmp[10] = c2.z; tmp[11] = c2.w; tmp[12] = c3.x; tmp[13] = c3.y; tmp[14] = c3.z; tmp[15] = c3.w;
        return tmp;
    }
    __device__ __forceinline__ uint32_t color(uint32_t i) const { return partRGBA ? partRGBA[partOf[i]] : rgba; }
};

struct Mat16 { float m[16]; };
// rt_mat4_mul (mat_mul of rt_host.cpp): column-major, the same association and operation order, contraction off
__device__ __forceinline__ void mat_mul_dev(const float *a, const float *b, float *out) {
    for (int col = 0; col < 4; ++col)
        for (int row = 0; row < 4; ++row)
            out[col * 4 + row] = a[0 * 4 + row] * b[col * 4 + 0] + a[1 * 4 + row] * b[col * 4 + 1] + a[2 * 4 + row] * b[col * 4 + 2] + a[3 * 4 + row] * b[col * 4 + 3];
}
// One lane per part: mvp[p] = mat_mul(vp, mat_mul(model, table[p])) with the matrix table as it stands on the stream (it may have been written on
// the device, so the product cannot be formed on the host).  Table entries and results are 64-byte aligned: four 16-byte loads, four 16-byte stores.
__global__ __launch_bounds__(256) void k_rs_part_mvp(Mat16 vp, Mat16 model, const float4 *__restrict__ table, uint32_t nParts, float4 *__restrict__ mvp) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= nParts) return;
    const float4 *T = table + (size_t)p * 4;
    const float4 c0 = T[0], c1 = T[1], c2 = T[2], c3 = T[3];
    const float t[16] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
    float mt[16], r[16];
    mat_mul_dev(model.m, t, mt);
    mat_mul_dev(vp.m, mt, r);
    float4 *o = mvp + (size_t)p * 4;
    for (int c = 0; c < 4; ++c) o[c] = make_float4(r[4 * c], r[4 * c + 1], r[4 * c + 2], r[4 * c + 3]);
}

struct CV { float x, y, z, w; };

__device__ __forceinline__ CV lerp_cv(const CV &in, const CV &out, float t) {
    // always from the inside vertex towards the outside one: two triangles sharing an edge get the same point
    CV r;
    r.x = in.x + t * (out.x - in.x);
    r.y = in.y + t * (out.y - in.y);
    r.z = in.z + t * (out.z - in.z);
    r.w = in.w + t * (out.w - in.w);
    return r;
}
__device__ __forceinline__ float plane_dist(const CV &v, int p, float gx, float gy) {
    switch (p) {
        case 0: return v.z + v.w;          // near: z >= -w
        case 1: return gx * v.w - v.x;     // x <= gx w
        case 2: return gx * v.w + v.x;     // x >= -gx w
        case 3: return gy * v.w - v.y;
        default: return gy * v.w + v.y;
    }
}

__device__ __forceinline__ uint32_t wave_add(bool pred) { return (uint32_t)__popcll(__ballot(pred)); }

// stats[0] dropped, [1] clipped, [2] set up, [3] bin entries, [4] first triangle past the capacity, [5] tiles per row
template <class Draw>
__global__ __launch_bounds__(256) void k_rs_setup(Draw d, int W, int H, float gx, float gy, uint4 *__restrict__ hdr, int *__restrict__ verts,
                                                  uint32_t *__restrict__ counts, unsigned long long *__restrict__ stats) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < d.nTris;
    bool dropped = false, clipped = false;
    if (live) {
        const uint32_t t = d.triBase + i;
        CV v[kMaxPoly];
        bool finite = true;
        float mtmp[16];
        const float *m = d.mvp(i, mtmp);
        const uint32_t rgba = d.color(i);
        for (int k = 0; k < 3; ++k) {
            const uint32_t vi = d.idx[3u * i + (uint32_t)k];
            const float px = d.pos[3u * vi + 0], py = d.pos[3u * vi + 1], pz = d.pos[3u * vi + 2];
            v[k].x = ((m[0] * px + m[4] * py) + m[8] * pz) + m[12];
            v[k].y = ((m[1] * px + m[5] * py) + m[9] * pz) + m[13];
            v[k].z = ((m[2] * px + m[6] * py) + m[10] * pz) + m[14];
            v[k].w = ((m[3] * px + m[7] * py) + m[11] * pz) + m[15];
            finite = finite && __builtin_isfinite(v[k].x) && __builtin_isfinite(v[k].y) && __builtin_isfinite(v[k].z) && __builtin_isfinite(v[k].w);
        }
        int n = 3;
        if (finite) {
            bool allIn = true;
            for (int k = 0; k < 3; ++k)
                for (int p = 0; p < 5; ++p) allIn = allIn && plane_dist(v[k], p, gx, gy) >= 0.0f;
            if (!allIn) {
                clipped = true;
                // Sutherland-Hodgman, planes in order near, +x, -x, +y, -y.  A convex polygon gains at most one vertex per plane (3 + 5 = 8),
                // but rounding can add sign changes for vertices lying almost on a plane: a polygon that would pass kMaxPoly vertices
                // is not stored past the array, the triangle is dropped
                for (int p = 0; p < 5 && n > 0; ++p) {
                    CV o[kMaxPoly];
                    int m = 0;
                    for (int k = 0; k < n; ++k) {
                        const CV &a = v[k], &b = v[k + 1 == n ? 0 : k + 1];
                        const float da = plane_dist(a, p, gx, gy), db = plane_dist(b, p, gx, gy);
                        const bool ia = da >= 0.0f, ib = db >= 0.0f;
                        if (ia) { if (m < kMaxPoly) o[m] = a; ++m; }
                        if (ia != ib) { if (m < kMaxPoly) o[m] = ia ? lerp_cv(a, b, da / (da - db)) : lerp_cv(b, a, db / (db - da)); ++m; }
                    }
                    if (m > kMaxPoly) { n = 0; break; }
                    n = m;
                    for (int k = 0; k < n; ++k) v[k] = o[k];
                }
            }
        }
        // project, snap to 1/256 pixel; any non-finite window coordinate drops the triangle
        int xs[kMaxPoly], ys[kMaxPoly];
        float zs[kMaxPoly];
        bool ok = finite && n >= 3;
        for (int k = 0; k < kMaxPoly; ++k) {
            if (k >= n || !ok) break;
            const float xw = ((v[k].x / v[k].w) * 0.5f + 0.5f) * (float)W;
            const float yw = ((v[k].y / v[k].w) * 0.5f + 0.5f) * (float)H;
            const float zw = (v[k].z / v[k].w) * 0.5f + 0.5f;
            const float sx = __builtin_rintf(xw * 256.0f), sy = __builtin_rintf(yw * 256.0f);
            ok = __builtin_isfinite(sx) && __builtin_isfinite(sy) && __builtin_isfinite(zw) && __builtin_fabsf(sx) < 536870912.0f &&
                 __builtin_fabsf(sy) < 536870912.0f;
            xs[k] = (int)sx; ys[k] = (int)sy; zs[k] = zw;
        }
        // drawable pieces of the fan (nonzero area), bounding box of their pixel centres
        int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -0x7fffffff, y1 = -0x7fffffff;
        bool any = false;
        if (ok)
            for (int k = 1; k + 1 < n; ++k) {
                const long long ar = (long long)(xs[k] - xs[0]) * (ys[k + 1] - ys[0]) - (long long)(ys[k] - ys[0]) * (xs[k + 1] - xs[0]);
                if (ar == 0) continue;
                any = true;
                x0 = min(x0, min(xs[0], min(xs[k], xs[k + 1]))); x1 = max(x1, max(xs[0], max(xs[k], xs[k + 1])));
                y0 = min(y0, min(ys[0], min(ys[k], ys[k + 1]))); y1 = max(y1, max(ys[0], max(ys[k], ys[k + 1])));
            }
        uint32_t cnt = 0, rx = 0, ry = 0;
        dropped = !any;
        if (any) {
            // pixels whose centre 256 p + 128 lies in [min, max]
            const int px0 = max(0, (x0 - 128 + 255) >> 8), px1 = min(W - 1, (x1 - 128) >> 8);
            const int py0 = max(0, (y0 - 128 + 255) >> 8), py1 = min(H - 1, (y1 - 128) >> 8);
            if (px0 <= px1 && py0 <= py1) {
                const uint32_t tx0 = (uint32_t)px0 / kTile, tx1 = (uint32_t)px1 / kTile, ty0 = (uint32_t)py0 / kTile, ty1 = (uint32_t)py1 / kTile;
                cnt = (tx1 - tx0 + 1) * (ty1 - ty0 + 1);
                rx = tx0 | (tx1 << 16); ry = ty0 | (ty1 << 16);
            }
            int *vo = verts + (size_t)t * kVertInts;
            for (int k = 0; k < kMaxPoly; ++k) {
                if (k >= n) break;
                vo[3 * k + 0] = xs[k]; vo[3 * k + 1] = ys[k]; vo[3 * k + 2] = __float_as_int(zs[k]);
            }
        }
        hdr[t] = make_uint4(any ? (uint32_t)n : 0u, rgba, rx, ry);
        counts[t] = cnt;
    }
    const uint32_t nd = wave_add(live && dropped), nc = wave_add(live && clipped), ns = wave_add(live && !dropped);
    if ((threadIdx.x & 63) == 0) {
        if (nd) atomicAdd(&stats[0], (unsigned long long)nd);
        if (nc) atomicAdd(&stats[1], (unsigned long long)nc);
        if (ns) atomicAdd(&stats[2], (unsigned long long)ns);
    }
}

// A lane writes the pairs of its own triangle when they are few; the pairs of a large triangle (a screen-filling one is a pair in
// every tile) are written by its whole wave, 64 at a time.
constexpr uint32_t kScatterAlone = 32;
__global__ __launch_bounds__(256) void k_rs_scatter(uint32_t n, const uint4 *__restrict__ hdr, const uint32_t *__restrict__ counts,
                                                    const unsigned long long *__restrict__ offs, unsigned long long cap, uint32_t *__restrict__ keys,
                                                    uint32_t *__restrict__ vals, unsigned long long *__restrict__ stats) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t tilesX = (uint32_t)stats[5];
    unsigned long long off = 0, cnt = 0;
    uint4 h = make_uint4(0, 0, 0, 0);
    if (t < n) {
        off = offs[t]; cnt = counts[t];
        if (t == n - 1) stats[3] = off + cnt;
        if (off + cnt > cap) cnt = 0;   // past the capacity: k_rs_raster takes it from the triangle list
        if (cnt) h = hdr[t];
    }
    if (cnt && cnt <= kScatterAlone) {
        const uint32_t tx0 = h.z & 0xffffu, tx1 = h.z >> 16, ty0 = h.w & 0xffffu, ty1 = h.w >> 16;
        unsigned long long o = off;
        for (uint32_t ty = ty0; ty <= ty1; ++ty)
            for (uint32_t tx = tx0; tx <= tx1; ++tx, ++o) { keys[o] = ty * tilesX + tx; vals[o] = t; }
    }
    unsigned long long big = __ballot(cnt > kScatterAlone);
    while (big) {
        const int l = __ffsll((long long)big) - 1;
        big &= big - 1;
        const uint32_t bt = __shfl(t, l), bz = __shfl(h.z, l), bw = __shfl(h.w, l);
        const unsigned long long bo = __shfl(off, l), bc = __shfl(cnt, l);
        const uint32_t tx0 = bz & 0xffffu, w = (bz >> 16) - tx0 + 1, ty0 = bw & 0xffffu;
        for (unsigned long long j = lane; j < bc; j += 64) {
            const uint32_t jj = (uint32_t)j;
            keys[bo + j] = (ty0 + jj / w) * tilesX + tx0 + jj % w;
            vals[bo + j] = bt;
        }
    }
}

// stats[4] = first triangle past the capacity: the one whose pairs end past cap while those of its predecessors (offs[t]) did not.
// Every later triangle is past it too, so k_rs_raster's fallback is the suffix [stats[4], n).
__global__ __launch_bounds__(256) void k_rs_first_over(uint32_t n, const uint32_t *__restrict__ counts, const unsigned long long *__restrict__ offs,
                                                       unsigned long long cap, unsigned long long *__restrict__ stats) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    if (offs[t] + counts[t] > cap && offs[t] <= cap) stats[4] = t;
}

__global__ void k_rs_init(unsigned long long *stats, unsigned long long nTris, unsigned long long tilesX) {
    if (threadIdx.x == 0) { stats[0] = stats[1] = stats[2] = stats[3] = 0; stats[4] = nTris; stats[5] = tilesX; }
}

__global__ __launch_bounds__(256) void k_rs_ranges(uint32_t cap, uint32_t nTiles, const uint32_t *__restrict__ keys, uint32_t *__restrict__ begin,
                                                   uint32_t *__restrict__ end) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= cap) return;
    const uint32_t k = keys[i];
    if (k >= nTiles) return;
    if (i == 0 || keys[i - 1] != k) begin[k] = i;
    if (i + 1 == cap || keys[i + 1] != k) end[k] = i + 1;
}

struct Lane4 { unsigned long long key[4]; };

// one piece (a, b, c) of triangle t's fan against this lane's four pixels (column px, rows py + 4 k, 1/256 pixel centres)
__device__ __forceinline__ void raster_piece(Lane4 &L, int ax, int ay, float az, int bx, int by, float bz, int cx, int cy, float cz, uint32_t prim,
                                             int px, int py, int tileX0, int tileY0) {
    long long area = (long long)(bx - ax) * (cy - ay) - (long long)(by - ay) * (cx - ax);
    if (area == 0) return;
    if (area < 0) { int tx = bx; bx = cx; cx = tx; int ty = by; by = cy; cy = ty; float tz = bz; bz = cz; cz = tz; area = -area; }
    // reject pieces whose box misses the tile (centres of the tile's pixels span [tile0 + 128, tile0 + 15 * 256 + 128])
    const int mnx = min(ax, min(bx, cx)), mxx = max(ax, max(bx, cx)), mny = min(ay, min(by, cy)), mxy = max(ay, max(by, cy));
    if (mxx < tileX0 + 128 || mnx > tileX0 + (kTile - 1) * 256 + 128 || mxy < tileY0 + 128 || mny > tileY0 + (kTile - 1) * 256 + 128) return;
    // edges opposite a, b, c: b->c, c->a, a->b; top-left (y-up, counter-clockwise): dy < 0, or dy == 0 and dx < 0
    const int d0x = cx - bx, d0y = cy - by, d1x = ax - cx, d1y = ay - cy, d2x = bx - ax, d2y = by - ay;
    const long long b0 = (d0y < 0 || (d0y == 0 && d0x < 0)) ? 0 : 1, b1 = (d1y < 0 || (d1y == 0 && d1x < 0)) ? 0 : 1,
                    b2 = (d2y < 0 || (d2y == 0 && d2x < 0)) ? 0 : 1;
    long long e0 = (long long)d0x * (py - by) - (long long)d0y * (px - bx);
    long long e1 = (long long)d1x * (py - cy) - (long long)d1y * (px - cx);
    long long e2 = (long long)d2x * (py - ay) - (long long)d2y * (px - ax);
    const long long s0 = (long long)d0x * (4 * 256), s1 = (long long)d1x * (4 * 256), s2 = (long long)d2x * (4 * 256);
    const float fa = (float)area;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (e0 >= b0 && e1 >= b1 && e2 >= b2) {
            const float z = (((float)e0 * az + (float)e1 * bz) + (float)e2 * cz) / fa;
            if (z <= 1.0f) {
                const uint32_t d24 = (uint32_t)__builtin_rintf(fmaxf(z, 0.0f) * 16777215.0f);
                const unsigned long long key = ((unsigned long long)d24 << 32) | prim;
                if (d24 < 0xFFFFFFu && key < L.key[k]) L.key[k] = key;
            }
        }
        e0 += s0; e1 += s1; e2 += s2;
    }
}

// A list of triangles 64 at a time: each lane fetches one triangle's id, vertex count and first three vertices into LDS (one round of
// dependent loads per 64 triangles instead of one per triangle), then the wave walks them from LDS.  kSuffix: the list is the
// triangle range [b, e) itself and a triangle counts only if its tile rectangle holds this tile; otherwise the tile's bin pairs.
template <bool kSuffix>
__device__ __forceinline__ void walk_list(Lane4 &L, uint32_t b, uint32_t e, const uint32_t *__restrict__ vals, const uint4 *__restrict__ hdr,
                                          const int *__restrict__ verts, uint32_t *sT, uint32_t *sN, int (*sV)[9], int lane, int tx, int ty, int px, int py,
                                          int tileX0, int tileY0) {
    for (uint32_t base = b; base < e; base += 64) {
        const uint32_t cnt = min(64u, e - base);
        if ((uint32_t)lane < cnt) {
            const uint32_t t = kSuffix ? base + lane : vals[base + lane];
            uint32_t n = hdr[t].x;
            if (kSuffix) {
                const uint4 h = hdr[t];
                const uint32_t tx0 = h.z & 0xffffu, tx1 = h.z >> 16, ty0 = h.w & 0xffffu, ty1 = h.w >> 16;
                if ((uint32_t)tx < tx0 || (uint32_t)tx > tx1 || (uint32_t)ty < ty0 || (uint32_t)ty > ty1) n = 0;
            }
            sT[lane] = t; sN[lane] = n;
            if (!kSuffix || n) {
                const int *v = verts + (size_t)t * kVertInts;
#pragma unroll
                for (int q = 0; q < 9; ++q) sV[lane][q] = v[q];
            }
        }
        __syncthreads();
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t t = sT[j], n = sN[j];
            if (kSuffix && n == 0) continue;
            const int *v = sV[j];
            const int ax = v[0], ay = v[1];
            const float az = __int_as_float(v[2]);
            raster_piece(L, ax, ay, az, v[3], v[4], __int_as_float(v[5]), v[6], v[7], __int_as_float(v[8]), t, px, py, tileX0, tileY0);
            if (n > 3) {   // the rest of a clipped triangle's fan from the record itself
                const int *g = verts + (size_t)t * kVertInts;
                for (uint32_t k = 2; k + 1 < n; ++k)
                    raster_piece(L, ax, ay, az, g[3 * k], g[3 * k + 1], __int_as_float(g[3 * k + 2]), g[3 * k + 3], g[3 * k + 4], __int_as_float(g[3 * k + 5]), t,
                                 px, py, tileX0, tileY0);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_rs_raster(int W, int H, int tilesX, const uint32_t *__restrict__ begin, const uint32_t *__restrict__ end,
                                                  const uint32_t *__restrict__ vals, const uint4 *__restrict__ hdr, const int *__restrict__ verts,
                                                  const unsigned long long *__restrict__ stats, uint32_t nTris, uint32_t bgRGBA, uint32_t *__restrict__ outRGBA,
                                                  uint32_t *__restrict__ outPrim, uint32_t *__restrict__ outDepth) {
    const int tile = blockIdx.x, tx = tile % tilesX, ty = tile / tilesX;
    const int lane = threadIdx.x;
    const int x = tx * kTile + (lane & 15), y0 = ty * kTile + (lane >> 4);
    const int px = x * 256 + 128, py = y0 * 256 + 128, tileX0 = tx * kTile * 256, tileY0 = ty * kTile * 256;
    Lane4 L;
#pragma unroll
    for (int k = 0; k < 4; ++k) L.key[k] = ~0ull;
    // Two lists: the tile's bin pairs [begin, end), then the triangles past the bin capacity [stats[4], nTris) (none unless the
    // capacity was too small), which are tested against their tile rectangle.
    __shared__ uint32_t sT[64], sN[64];
    __shared__ int sV[64][9];
    walk_list<false>(L, begin[tile], end[tile], vals, hdr, verts, sT, sN, sV, lane, tx, ty, px, py, tileX0, tileY0);
    walk_list<true>(L, (uint32_t)stats[4], nTris, vals, hdr, verts, sT, sN, sV, lane, tx, ty, px, py, tileX0, tileY0);
    if (x >= W) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = y0 + 4 * k;
        if (y >= H) break;
        const size_t o = (size_t)y * W + x;
        const unsigned long long key = L.key[k];
        if (key == ~0ull) { outRGBA[o] = bgRGBA; outPrim[o] = kBg; outDepth[o] = 0xFFFFFFu; }
        else { const uint32_t p = (uint32_t)key; outRGBA[o] = hdr[p].y; outPrim[o] = p; outDepth[o] = (uint32_t)(key >> 32); }
    }
}

uint32_t unorm8(float x) {   // rt_present.hip unorm8 on the host
    float c = std::min(std::max(x, 0.0f), 1.0f);
    if (c != c) c = 0.0f;
    return (uint32_t)std::nearbyintf(c * 255.0f);
}
uint32_t pack_rgba(const float *c) { return unorm8(c[0]) | (unorm8(c[1]) << 8) | (unorm8(c[2]) << 16) | (255u << 24); }

}  // namespace

struct RtRaster {
    std::string err;
    // a slot holds an uploaded mesh (pos != null), or is bound to the context's dynamic mesh (bind = RT_RASTER_BIND_*), or is empty
    struct Mesh {
        float *pos = nullptr; uint32_t *idx = nullptr; int nVerts = 0, nIdx = 0;
        int bind = -1;
        uint32_t *partRGBA = nullptr; int nPartColors = 0;   // parts mode: packed colour per part on the device (null: the draw's colour)
    } mesh[RT_MAX_RASTER_MESHES];
    float4 *dPartMvp = nullptr; size_t nMvpCap = 0;          // per-call MVP table of the bound parts draws: 64 bytes per part
    hipStream_t last = nullptr;          // stream of the last rt_render_raster
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool rendered = false;
    bool boundPending = false;           // a call that read the dynamic mesh may still be running (ev1 behind it has not been seen complete)
    // frame buffers (W x H)
    int W = 0, H = 0;
    uint32_t *dRGBA = nullptr, *dPrim = nullptr, *dDepth = nullptr;
    // per-triangle arrays (capacity nTriCap)
    size_t nTriCap = 0;
    uint4 *dHdr = nullptr; int *dVerts = nullptr; uint32_t *dCounts = nullptr; unsigned long long *dOffs = nullptr;
    // bins
    size_t binCap = 0, binGrowTo = 0;
    size_t forcedCap = 0;                // rt_debug_raster_bin_capacity: pairs the bin arrays hold (0: sized as DESIGN.md 11.2 says)
    uint32_t *dKeys[2] = {}, *dVals[2] = {};
    uint32_t *dBegin = nullptr, *dEnd = nullptr; size_t nTileCap = 0;
    void *dTemp = nullptr; size_t tempBytes = 0;
    unsigned long long *dStats = nullptr;
    uint64_t lastTris = 0, lastCap = 0;
    size_t bytes = 0;
};

#define RS_TRY(r, expr)                                                                                           \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) { (r)->err = std::string(#expr " failed: ") + hipGetErrorString(e_); return RT_ERR_HIP; } \
    } while (0)

static void rs_free(void *&p) { if (p) (void)hipFree(p); p = nullptr; }
template <class T> static void rs_free(T *&p) { void *q = p; rs_free(q); p = nullptr; }

RtRaster *rt_raster_create() { return new RtRaster(); }
const char *rt_raster_error(const RtRaster *r) { return r ? r->err.c_str() : ""; }

void rt_raster_destroy(RtRaster *r) {
    if (!r) return;
    if (r->last) (void)hipStreamSynchronize(r->last);
    for (auto &m : r->mesh) { rs_free(m.pos); rs_free(m.idx); rs_free(m.partRGBA); }
    rs_free(r->dPartMvp);
    rs_free(r->dRGBA); rs_free(r->dPrim); rs_free(r->dDepth);
    rs_free(r->dHdr); rs_free(r->dVerts); rs_free(r->dCounts); rs_free(r->dOffs);
    for (int i = 0; i < 2; ++i) { rs_free(r->dKeys[i]); rs_free(r->dVals[i]); }
    rs_free(r->dBegin); rs_free(r->dEnd); rs_free(r->dTemp); rs_free(r->dStats);
    if (r->ev0) (void)hipEventDestroy(r->ev0);
    if (r->ev1) (void)hipEventDestroy(r->ev1);
    delete r;
}

void rt_raster_force_bin_capacity(RtRaster *r, size_t pairs) { r->forcedCap = pairs; }

int rt_raster_set_mesh(RtRaster *r, int slot, const float *pos, int nVerts, const uint32_t *idx, int nIdx) {
    if (slot < 0 || slot >= RT_MAX_RASTER_MESHES) { r->err = "rt_raster_mesh: slot " + std::to_string(slot) + " outside 0.." + std::to_string(RT_MAX_RASTER_MESHES - 1); return RT_ERR_INVALID; }
    if (nVerts < 0 || nIdx < 0 || (nVerts > 0 && (!pos || !idx))) { r->err = "rt_raster_mesh: bad arguments"; return RT_ERR_INVALID; }
    if (nVerts > 0) {
        if (nIdx % 3 != 0) { r->err = "rt_raster_mesh: nIdx = " + std::to_string(nIdx) + " is not a multiple of 3"; return RT_ERR_INVALID; }
        for (int i = 0; i < nIdx; ++i)
            if (idx[i] >= (uint32_t)nVerts) {
                r->err = "rt_raster_mesh: index " + std::to_string(idx[i]) + " at " + std::to_string(i) + " >= nVerts = " + std::to_string(nVerts);
                return RT_ERR_INVALID;
            }
    }
    if (r->last) RS_TRY(r, hipStreamSynchronize(r->last));   // a raster call in flight may still read the slot
    RtRaster::Mesh &m = r->mesh[slot];
    rs_free(m.pos); rs_free(m.idx); rs_free(m.partRGBA);
    m.nVerts = m.nIdx = m.nPartColors = 0;
    m.bind = -1;   // an upload replaces a binding, nVerts == 0 unbinds
    if (nVerts == 0) return RT_OK;
    RS_TRY(r, hipMalloc(&m.pos, (size_t)nVerts * 12));
    RS_TRY(r, hipMalloc(&m.idx, std::max<size_t>((size_t)nIdx * 4, 4)));
    RS_TRY(r, hipMemcpy(m.pos, pos, (size_t)nVerts * 12, hipMemcpyHostToDevice));
    if (nIdx > 0) RS_TRY(r, hipMemcpy(m.idx, idx, (size_t)nIdx * 4, hipMemcpyHostToDevice));
    m.nVerts = nVerts; m.nIdx = nIdx;
    return RT_OK;
}

int rt_raster_bind_dynamic(RtRaster *r, int slot, int mode) {
    if (slot < 0 || slot >= RT_MAX_RASTER_MESHES) { r->err = "rt_raster_mesh_dynamic: slot " + std::to_string(slot) + " outside 0.." + std::to_string(RT_MAX_RASTER_MESHES - 1); return RT_ERR_INVALID; }
    if (mode != RT_RASTER_BIND_SINGLE && mode != RT_RASTER_BIND_PARTS) { r->err = "rt_raster_mesh_dynamic: mode = " + std::to_string(mode); return RT_ERR_INVALID; }
    RtRaster::Mesh &m = r->mesh[slot];
    if (m.pos || m.partRGBA) {
        if (r->last) RS_TRY(r, hipStreamSynchronize(r->last));   // a raster call in flight may still read what the slot holds
        rs_free(m.pos); rs_free(m.idx); rs_free(m.partRGBA);
    }
    m.nVerts = m.nIdx = m.nPartColors = 0;
    m.bind = mode;
    return RT_OK;
}

int rt_raster_set_part_colors(RtRaster *r, int slot, const float *rgb, int nParts) {
    if (slot < 0 || slot >= RT_MAX_RASTER_MESHES) { r->err = "rt_raster_part_colors: slot " + std::to_string(slot) + " outside 0.." + std::to_string(RT_MAX_RASTER_MESHES - 1); return RT_ERR_INVALID; }
    RtRaster::Mesh &m = r->mesh[slot];
    if (m.bind != RT_RASTER_BIND_PARTS) { r->err = "rt_raster_part_colors: slot " + std::to_string(slot) + " is not bound with RT_RASTER_BIND_PARTS"; return RT_ERR_INVALID; }
    if (nParts < 0) { r->err = "rt_raster_part_colors: nParts = " + std::to_string(nParts); return RT_ERR_INVALID; }
    if (nParts > RT_MAX_MESH_PARTS) { r->err = "rt_raster_part_colors: " + std::to_string(nParts) + " parts (a mesh has at most " + std::to_string(RT_MAX_MESH_PARTS) + ")"; return RT_ERR_INVALID; }
    if (!rgb) nParts = 0;
    if (m.partRGBA || nParts) {
        if (r->last) RS_TRY(r, hipStreamSynchronize(r->last));   // a raster call in flight may still read the table
    }
    if (nParts != m.nPartColors) { rs_free(m.partRGBA); m.nPartColors = 0; }
    if (nParts == 0) return RT_OK;
    std::vector<uint32_t> packed((size_t)nParts);
    for (int p = 0; p < nParts; ++p) packed[(size_t)p] = pack_rgba(rgb + 3 * (size_t)p);
    if (!m.partRGBA) RS_TRY(r, hipMalloc(&m.partRGBA, (size_t)nParts * 4));
    m.nPartColors = nParts;
    RS_TRY(r, hipMemcpy(m.partRGBA, packed.data(), (size_t)nParts * 4, hipMemcpyHostToDevice));
    return RT_OK;
}

// The second half of the event scheme: `s` is about to carry writes to the dynamic mesh -- rt_mesh_set_positions /
// rt_mesh_set_part_matrices on it, or it has just become rt_stream()'s stream, on which the caller orders device writes of their own.  If a raster
// call that read the mesh may still be running on another stream, `s` waits for the event behind that call.  The wait is enqueued here, when a
// writer on another stream exists, and not on every lane by the raster call itself: a wait enqueued for the event of a call costs that call's own
// stream time on this runtime (measured: 0.06 ms per waiting lane and call), and an application in raster mode never changes streams.
int rt_raster_order_after(RtRaster *r, hipStream_t s) {
    if (!r->boundPending || s == r->last) return RT_OK;
    const hipError_t q = hipEventQuery(r->ev1);
    if (q == hipSuccess) { r->boundPending = false; return RT_OK; }
    if (q == hipErrorNotReady) (void)hipGetLastError();
    RS_TRY(r, hipStreamWaitEvent(s, r->ev1, 0));
    return RT_OK;
}

template <class T> static int rs_grow(RtRaster *r, T *&p, size_t have, size_t want, size_t elemBytes) {
    if (p && have >= want) return RT_OK;
    if (p) { r->bytes -= have * elemBytes; rs_free(p); }
    RS_TRY(r, hipMalloc(&p, std::max<size_t>(want, 1) * elemBytes));
    r->bytes += std::max<size_t>(want, 1) * elemBytes;
    return RT_OK;
}
#define RS_GROW(p, have, want, eb) do { int rc_ = rs_grow(r, p, have, want, eb); if (rc_ != RT_OK) return rc_; } while (0)

int rt_raster_render(RtRaster *r, hipStream_t st, int W, int H, const RtRasterDraw *draws, int nDraws, const float *view, const float *proj,
                     const RtRasterDynamic *dyn) {
    // validate the draw list first: nothing is enqueued for a bad one
    uint64_t nTris = 0;
    bool anyBound = false;     // some draw names a bound slot: the call reads the dynamic mesh
    size_t mvpEntries = 0;     // the largest part count of the bound parts draws
    for (int i = 0; i < nDraws; ++i) {
        const int s = draws[i].mesh;
        if (s < 0 || s >= RT_MAX_RASTER_MESHES) { r->err = "rt_render_raster: draw " + std::to_string(i) + " names slot " + std::to_string(s); return RT_ERR_INVALID; }
        const RtRaster::Mesh &m = r->mesh[s];
        if (m.bind >= 0) {
            if (!dyn) {
                r->err = "rt_render_raster: draw " + std::to_string(i) + " names slot " + std::to_string(s) + ", bound to the dynamic mesh, and there is no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)";
                return RT_ERR_STATE;
            }
            if (m.bind == RT_RASTER_BIND_PARTS) {
                if (m.partRGBA && m.nPartColors != dyn->nParts) {
                    r->err = "rt_render_raster: draw " + std::to_string(i) + ": the colour table of slot " + std::to_string(s) + " has " + std::to_string(m.nPartColors) + " entries, the mesh has " +
                             std::to_string(dyn->nParts) + " parts (rt_raster_part_colors again)";
                    return RT_ERR_STATE;
                }
                mvpEntries = std::max(mvpEntries, (size_t)dyn->nParts);
            }
            anyBound = true;
            nTris += (uint64_t)dyn->nTris;
            continue;
        }
        if (!m.pos) { r->err = "rt_render_raster: draw " + std::to_string(i) + " names empty mesh slot " + std::to_string(s); return RT_ERR_STATE; }
        nTris += (uint64_t)m.nIdx / 3;
    }
    if (nTris >= 0x7fffffffull) { r->err = "rt_render_raster: more than 2^31 triangles"; return RT_ERR_UNSUPPORTED; }
    if (W > 65536 || H > 65536) { r->err = "rt_render_raster: framebuffer above 65536 pixels a side (guard band, DESIGN.md 11)"; return RT_ERR_UNSUPPORTED; }
    const int tilesX = (W + kTile - 1) / kTile, tilesY = (H + kTile - 1) / kTile;
    const uint32_t nTiles = (uint32_t)(tilesX * tilesY);
    if (!r->ev0) { RS_TRY(r, hipEventCreate(&r->ev0)); RS_TRY(r, hipEventCreate(&r->ev1)); }
    if (!r->dStats) { RS_TRY(r, hipMalloc(&r->dStats, 8 * sizeof(unsigned long long))); r->bytes += 64; }
    if (r->last && r->last != st) RS_TRY(r, hipStreamWaitEvent(st, r->ev1, 0));   // the previous call's buffers are reused
    // what the previous call needed: grow the bin arrays to it (+ 25 %) when it has finished (no wait: a call that finds no room
    // rasterises the pairs that did not fit from the triangle list)
    if (r->rendered && hipEventQuery(r->ev1) == hipSuccess) {
        unsigned long long s[8];
        RS_TRY(r, hipMemcpy(s, r->dStats, sizeof s, hipMemcpyDeviceToHost));
        r->binGrowTo = std::max<size_t>(r->binGrowTo, (size_t)(s[3] + s[3] / 4));
    }
    size_t want = std::max<size_t>({(size_t)(2 * nTris + 2 * (uint64_t)nTiles + 4096), r->binGrowTo, r->binCap});
    if (r->forcedCap) want = r->forcedCap;   // diagnostics: exercise the path past the capacity
    want = std::min<size_t>(want, (size_t)1 << 31);
    // buffers
    if (W != r->W || H != r->H) {
        const size_t np = (size_t)W * H, old = (size_t)r->W * r->H;
        if (r->dRGBA) r->bytes -= old * 12;
        rs_free(r->dRGBA); rs_free(r->dPrim); rs_free(r->dDepth);
        RS_TRY(r, hipMalloc(&r->dRGBA, np * 4)); RS_TRY(r, hipMalloc(&r->dPrim, np * 4)); RS_TRY(r, hipMalloc(&r->dDepth, np * 4));
        r->bytes += np * 12;
        r->W = W; r->H = H;
    }
    const size_t nt = (size_t)nTris;
    if (!r->dHdr || r->nTriCap < nt) {
        RS_GROW(r->dHdr, r->nTriCap, nt, 16); RS_GROW(r->dVerts, r->nTriCap, nt, (size_t)kVertInts * 4);
        RS_GROW(r->dCounts, r->nTriCap, nt, 4); RS_GROW(r->dOffs, r->nTriCap, nt, 8);
        r->nTriCap = std::max<size_t>(nt, 1);
    }
    if (mvpEntries && (!r->dPartMvp || r->nMvpCap < mvpEntries)) {
        RS_GROW(r->dPartMvp, r->nMvpCap, mvpEntries, 64);
        r->nMvpCap = mvpEntries;
    }
    if (!r->dBegin || r->nTileCap < nTiles) {
        RS_GROW(r->dBegin, r->nTileCap, nTiles, 4); RS_GROW(r->dEnd, r->nTileCap, nTiles, 4);
        r->nTileCap = nTiles;
    }
    if (!r->dKeys[0] || r->binCap != want) {
        for (int i = 0; i < 2; ++i) {
            if (r->dKeys[i]) { r->bytes -= r->binCap * 8; rs_free(r->dKeys[i]); rs_free(r->dVals[i]); }
            RS_TRY(r, hipMalloc(&r->dKeys[i], want * 4)); RS_TRY(r, hipMalloc(&r->dVals[i], want * 4));
            r->bytes += want * 8;
        }
        r->binCap = want;
    }
    int bits = 1;
    while (((1u << bits) - 1u) < nTiles) ++bits;   // the sentinel key 0xFFFFFFFF keeps its place above every tile in bits [0, bits)
    size_t tScan = 0, tSort = 0;
    RS_TRY(r, rocprim::exclusive_scan(nullptr, tScan, r->dCounts, r->dOffs, 0ull, std::max<size_t>(nt, 1), rocprim::plus<unsigned long long>(), st));
    {
        rocprim::double_buffer<uint32_t> kb(r->dKeys[0], r->dKeys[1]), vb(r->dVals[0], r->dVals[1]);
        RS_TRY(r, rocprim::radix_sort_pairs(nullptr, tSort, kb, vb, r->binCap, 0, bits, st));
    }
    const size_t tNeed = std::max<size_t>({tScan, tSort, 16});
    if (r->tempBytes < tNeed) {
        if (r->dTemp) r->bytes -= r->tempBytes;
        rs_free(r->dTemp);
        RS_TRY(r, hipMalloc(&r->dTemp, tNeed));
        r->tempBytes = tNeed; r->bytes += tNeed;
    }
    float vp[16], mvp[16];
    rt_mat4_mul(proj, view, vp);
    const float gx = 1.0f + kGuardPixels2 / (float)W, gy = 1.0f + kGuardPixels2 / (float)H;
    float bgc[3] = {0.1f, 0.0f, 0.2f};
    const uint32_t bg = pack_rgba(bgc);
    // launches.  A call that names a bound slot reads the mesh where the caller's writes and the mesh updates put it, and those were ordered on
    // rt_stream()'s stream as it was then: the setup work waits for every other lane (the first half of 14.4's scheme)
    if (anyBound)
        for (int i = 0; i < dyn->nOthers; ++i) {
            RS_TRY(r, hipEventRecord(dyn->evOther[i], dyn->others[i]));
            RS_TRY(r, hipStreamWaitEvent(st, dyn->evOther[i], 0));
        }
    RS_TRY(r, hipEventRecord(r->ev0, st));
    hipLaunchKernelGGL(k_rs_init, dim3(1), dim3(64), 0, st, r->dStats, (unsigned long long)nTris, (unsigned long long)tilesX);
    uint32_t base = 0;
    for (int i = 0; i < nDraws; ++i) {
        const RtRaster::Mesh &m = r->mesh[draws[i].mesh];
        if (m.bind == RT_RASTER_BIND_PARTS) {
            // the parts' MVPs on the device, then one setup launch over all index triples: parts are contiguous and in order, so input triangle t is
            // primitive base + t.  The table is reused by the next bound draw of the call: the stream orders its launches
            PartsDraw a;
            Mat16 mvpM, modelM;
            std::memcpy(mvpM.m, vp, 64); std::memcpy(modelM.m, draws[i].model, 64);
            a.pos = dyn->pos; a.idx = dyn->idx; a.triBase = base; a.nTris = (uint32_t)dyn->nTris; a.rgba = pack_rgba(draws[i].color);
            a.partOf = dyn->partOf; a.partMvp = r->dPartMvp; a.partRGBA = m.partRGBA;
            if (a.nTris) {
                hipLaunchKernelGGL(k_rs_part_mvp, dim3(((unsigned)dyn->nParts + 255) / 256), dim3(256), 0, st, mvpM, modelM, reinterpret_cast<const float4 *>(dyn->partM),
                                   (uint32_t)dyn->nParts, r->dPartMvp);
                hipLaunchKernelGGL(k_rs_setup<PartsDraw>, dim3((a.nTris + 255) / 256), dim3(256), 0, st, a, W, H, gx, gy, r->dHdr, r->dVerts, r->dCounts, r->dStats);
            }
            base += a.nTris;
        } else {
            StaticDraw a;
            rt_mat4_mul(vp, draws[i].model, mvp);
            std::memcpy(a.m, mvp, 64);
            if (m.bind == RT_RASTER_BIND_SINGLE) { a.pos = dyn->pos; a.idx = dyn->idx; a.nTris = (uint32_t)dyn->nTris; }
            else { a.pos = m.pos; a.idx = m.idx; a.nTris = (uint32_t)(m.nIdx / 3); }
            a.triBase = base; a.rgba = pack_rgba(draws[i].color);
            if (a.nTris) hipLaunchKernelGGL(k_rs_setup<StaticDraw>, dim3((a.nTris + 255) / 256), dim3(256), 0, st, a, W, H, gx, gy, r->dHdr, r->dVerts, r->dCounts, r->dStats);
            base += a.nTris;
        }
    }
    RS_TRY(r, hipGetLastError());
    RS_TRY(r, hipMemsetAsync(r->dKeys[0], 0xFF, r->binCap * 4, st));
    RS_TRY(r, hipMemsetAsync(r->dBegin, 0, (size_t)nTiles * 4, st));
    RS_TRY(r, hipMemsetAsync(r->dEnd, 0, (size_t)nTiles * 4, st));
    uint32_t sortedIdx = 0;
    if (nt > 0) {
        size_t tb = r->tempBytes;
        RS_TRY(r, rocprim::exclusive_scan(r->dTemp, tb, r->dCounts, r->dOffs, 0ull, nt, rocprim::plus<unsigned long long>(), st));
        const unsigned g = (unsigned)((nt + 255) / 256);
        hipLaunchKernelGGL(k_rs_first_over, dim3(g), dim3(256), 0, st, (uint32_t)nt, r->dCounts, r->dOffs, (unsigned long long)r->binCap, r->dStats);
        hipLaunchKernelGGL(k_rs_scatter, dim3(g), dim3(256), 0, st, (uint32_t)nt, r->dHdr, r->dCounts, r->dOffs, (unsigned long long)r->binCap, r->dKeys[0],
                           r->dVals[0], r->dStats);
        RS_TRY(r, hipGetLastError());
        rocprim::double_buffer<uint32_t> kb(r->dKeys[0], r->dKeys[1]), vb(r->dVals[0], r->dVals[1]);
        tb = r->tempBytes;
        RS_TRY(r, rocprim::radix_sort_pairs(r->dTemp, tb, kb, vb, r->binCap, 0, bits, st));
        sortedIdx = kb.current() == r->dKeys[0] ? 0 : 1;
        hipLaunchKernelGGL(k_rs_ranges, dim3((unsigned)((r->binCap + 255) / 256)), dim3(256), 0, st, (uint32_t)r->binCap, nTiles, r->dKeys[sortedIdx], r->dBegin,
                           r->dEnd);
    }
    hipLaunchKernelGGL(k_rs_raster, dim3(nTiles), dim3(64), 0, st, W, H, tilesX, r->dBegin, r->dEnd, r->dVals[sortedIdx], r->dHdr, r->dVerts, r->dStats,
                       (uint32_t)nt, bg, r->dRGBA, r->dPrim, r->dDepth);
    RS_TRY(r, hipGetLastError());
    RS_TRY(r, hipEventRecord(r->ev1, st));
    // ... and whatever writes the mesh after this call on another stream than this one waits for ev1 first (the second half): rt_raster_order_after
    if (anyBound) r->boundPending = true;
    r->last = st;
    r->rendered = true;
    r->lastTris = nTris;
    r->lastCap = r->binCap;
    return RT_OK;
}

int rt_raster_read(RtRaster *r, int W, int H, uint8_t *rgba, uint32_t *prim, uint32_t *depth) {
    if (!r->rendered) { r->err = "rt_read_raster before rt_render_raster"; return RT_ERR_STATE; }
    if (W != r->W || H != r->H) {   // the caller's buffers are sized by the framebuffer (rt_resize); the raster frame is older
        r->err = "rt_read_raster: the framebuffer is " + std::to_string(W) + "x" + std::to_string(H) + " but the last raster frame is " + std::to_string(r->W) + "x" +
                 std::to_string(r->H) + " (rt_resize since rt_render_raster): render it again";
        return RT_ERR_STATE;
    }
    RS_TRY(r, hipStreamSynchronize(r->last));
    const size_t np = (size_t)r->W * r->H;
    if (rgba) RS_TRY(r, hipMemcpy(rgba, r->dRGBA, np * 4, hipMemcpyDeviceToHost));
    if (prim) RS_TRY(r, hipMemcpy(prim, r->dPrim, np * 4, hipMemcpyDeviceToHost));
    if (depth) RS_TRY(r, hipMemcpy(depth, r->dDepth, np * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_raster_buffers(RtRaster *r, int W, int H, void **rgba, void **prim, void **depth, size_t *bytesEach) {
    if (!r->rendered) { r->err = "rt_raster_targets before rt_render_raster"; return RT_ERR_STATE; }
    if (W != r->W || H != r->H) {
        r->err = "rt_raster_targets: the framebuffer is " + std::to_string(W) + "x" + std::to_string(H) + " but the last raster frame is " + std::to_string(r->W) + "x" +
                 std::to_string(r->H) + " (rt_resize since rt_render_raster): render it again";
        return RT_ERR_STATE;
    }
    if (rgba) *rgba = r->dRGBA;
    if (prim) *prim = r->dPrim;
    if (depth) *depth = r->dDepth;
    if (bytesEach) *bytesEach = (size_t)r->W * r->H * 4;
    return RT_OK;
}

int rt_raster_stats(RtRaster *r, RtRasterStats *out) {
    std::memset(out, 0, sizeof *out);
    if (!r) return RT_OK;
    out->rasterBytes = r->bytes;
    for (auto &m : r->mesh) {
        if (m.pos) out->rasterBytes += (uint64_t)m.nVerts * 12 + (uint64_t)m.nIdx * 4;
        if (m.partRGBA) out->rasterBytes += (uint64_t)m.nPartColors * 4;
    }
    if (!r->rendered) return RT_OK;
    RS_TRY(r, hipStreamSynchronize(r->last));
    unsigned long long s[8];
    RS_TRY(r, hipMemcpy(s, r->dStats, sizeof s, hipMemcpyDeviceToHost));
    out->trianglesIn = r->lastTris; out->trianglesDropped = s[0]; out->trianglesClipped = s[1]; out->trianglesSetUp = s[2];
    out->binEntries = s[3]; out->binCapacity = r->lastCap;
    float ms = 0.0f;
    RS_TRY(r, hipEventElapsedTime(&ms, r->ev0, r->ev1));
    out->deviceMs = ms;
    return RT_OK;
}
