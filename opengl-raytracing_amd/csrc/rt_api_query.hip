// rt_api_query.hip -- the query part of the C ABI (include/rt_mi355.h): rt_trace_rays, rt_trace_scene_rays, rt_pick_pixels,
// rt_trace_rays_multi, rt_pick_pixels_multi, rt_query_nearest, rt_query_nearest_multi, rt_query_boxes, rt_query_tris, rt_query_hulls, rt_pick_rects and their _host twins.  Host code only: rt_wave.hip,
// rt_scene_query.hip, rt_multi_hit.hip, rt_nearest.hip, rt_nearest_multi.hip and rt_overlap_query.hip launch, this file checks arguments and orders the queries on rt_stream()'s stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "rt_context.hpp"
#include "rt_multi_hit.hpp"
#include "rt_nearest.hpp"
#include "rt_nearest_multi.hpp"
#include "rt_overlap_query.hpp"

using namespace rtd;
using namespace rtapi;

namespace {

// What every query checks of its arguments, in the order the entry points have always checked it.  flags: the scene queries' (0 otherwise); xy != null: pixel
// rays (rt_pick_pixels), else origins / dirs.  ownBVH: rt_trace_rays, which checks the ray arrays' 2^32-float bound last and needs an uploaded BVH.
int query_args(RtContext *c, const char *what, int kind, int flags, const float *origins, int originStride, const float *dirs, int dirStride, const int32_t *xy,
               const float *tMax, int n, const RtHit *hits, const uint8_t *occluded, bool ownBVH) {
    if (kind != RT_QUERY_CLOSEST && kind != RT_QUERY_ANY) return fail(c, RT_ERR_INVALID, "%s: kind %d (RT_QUERY_CLOSEST or RT_QUERY_ANY)", what, kind);
    if (flags & ~(RT_QUERY_SKIP_GLASS | RT_QUERY_SKIP_MARKER)) return fail(c, RT_ERR_INVALID, "%s: flags 0x%x (RT_QUERY_SKIP_*)", what, flags);
    if (n < 0) return fail(c, RT_ERR_INVALID, "%s: n = %d", what, n);
    if (xy) {
        if ((size_t)n * 2 > ((size_t)1 << 32)) return fail(c, RT_ERR_INVALID, "%s: the pixel array exceeds 2^32 entries", what);
    } else {
        if (originStride < 3 || dirStride < 3) return fail(c, RT_ERR_INVALID, "%s: strides %d / %d floats (at least 3)", what, originStride, dirStride);
        if (n > 0 && (!origins || !dirs)) return fail(c, RT_ERR_INVALID, "%s: null ray arrays", what);
    }
    const bool tooLong = !xy && (size_t)(n > 0 ? n - 1 : 0) * (size_t)std::max(originStride, dirStride) + 3 > ((size_t)1 << 32);
    if (tooLong && !ownBVH) return fail(c, RT_ERR_INVALID, "%s: the ray arrays exceed 2^32 floats", what);
    if (kind == RT_QUERY_ANY && !tMax) return fail(c, RT_ERR_INVALID, "%s: any-hit queries need tMax", what);
    if (n > 0 && kind == RT_QUERY_CLOSEST && !hits) return fail(c, RT_ERR_INVALID, "%s: closest-hit queries need hits", what);
    if (n > 0 && kind == RT_QUERY_ANY && !occluded) return fail(c, RT_ERR_INVALID, "%s: any-hit queries need occluded", what);
    if (tooLong) return fail(c, RT_ERR_INVALID, "%s: the ray arrays exceed 2^32 floats", what);
    if (ownBVH && (c->nNodes <= 0 || c->nTris <= 0)) return fail(c, RT_ERR_STATE, "%s: no BVH uploaded", what);
    return RT_OK;
}

// The query scratch (allocated on the first query) and rt_stream()'s stream, which first waits for the previous query if that ran on another stream
int query_begin(RtContext *c, hipStream_t &st) {
    (void)hipSetDevice(c->cfg.device);
    st = api_stream(c);   // rt_stream()
    if (!c->dQueryFrame) {
        HIP_TRY(c, hipMalloc(&c->dQueryFrame, sizeof(DevFrame)));
        HIP_TRY(c, hipMalloc(&c->dQueryHeads, rt_wave_head_words() * sizeof(uint32_t)));
        // on the query's own stream: the lanes do not synchronise with the null stream, and a memset there can land after the first query's kernels
        // have written their uniforms into the scratch
        HIP_TRY(c, hipMemsetAsync(c->dQueryFrame, 0, sizeof(DevFrame), st));
        HIP_TRY(c, hipEventCreateWithFlags(&c->queryDone, hipEventDisableTiming));
    }
    if (c->queryStream && c->queryStream != st) HIP_TRY(c, hipStreamWaitEvent(st, c->queryDone, 0));   // the scratch is free again
    return RT_OK;
}
int query_end(RtContext *c, hipStream_t st) {
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->queryDone, st));
    c->queryStream = st;
    return RT_OK;
}
// One query by a traversal of its own: `call` enqueues it on `st` between query_begin and query_end and returns its hipError_t
template <class Launch>
int query_run(RtContext *c, const char *expr, Launch launch) {
    hipStream_t st = nullptr;
    const int br = query_begin(c, st);
    if (br != RT_OK) return br;
    const hipError_t e = launch(st);
    if (e != hipSuccess) return fail(c, RT_ERR_HIP, "%s failed: %s", expr, hipGetErrorString(e));   // (HIP_TRY's words)
    return query_end(c, st);
}
#define QUERY_RUN(c, call) query_run(c, #call, [&](hipStream_t st) { return call; })

// ---- scene queries and pixel picking: the analytic leg (rt_scene_query.hip) into the caller's outputs, then the mesh leg through the frames'
// persistent traversal launch (SceneSrc).  Shares rt_trace_rays' scratch; touches no frame state.
// Checks everything before any device work; `mesh` = the scene has a mesh leg.
int scene_query_args(RtContext *c, const char *what, const RtUniforms *u, int kind, int flags, const float *origins, int originStride, const float *dirs,
                     int dirStride, const int32_t *xy, const float *tMax, int n, const RtHit *hits, const uint8_t *occluded, bool &mesh) {
    if (!u) return fail(c, RT_ERR_INVALID, "%s: null uniforms", what);
    const int rc = query_args(c, what, kind, flags, origins, originStride, dirs, dirStride, xy, tMax, n, hits, occluded, false);
    if (rc != RT_OK) return rc;
    // the mesh as render_frames_impl sees it
    const bool meshMode = u->useBVH == 1 || u->useBVH == RT_SCENE_HYBRID;
    mesh = meshMode && u->nodeCount > 0 && u->triCount > 0;
    if (mesh && (c->nNodes == 0 || u->nodeCount > c->nNodes || u->triCount > c->nTris))
        return fail(c, RT_ERR_STATE, "%s: uniforms name %d nodes / %d tris, uploaded %d / %d", what, u->nodeCount, u->triCount, c->nNodes, c->nTris);
    return RT_OK;
}

int scene_query(RtContext *c, const char *what, const RtUniforms *u, int kind, int flags, const float *origins, int originStride, const float *dirs, int dirStride,
                const int32_t *xy, const float *tMax, int n, RtHit *hits, int32_t *objects, float *normals, float *points, uint8_t *occluded) {
    bool mesh = false;
    const int rc = scene_query_args(c, what, u, kind, flags, origins, originStride, dirs, dirStride, xy, tMax, n, hits, occluded, mesh);
    if (rc != RT_OK || n == 0) return rc;
    if (((uintptr_t)origins | (uintptr_t)dirs | (uintptr_t)xy | (uintptr_t)tMax | (uintptr_t)objects | (uintptr_t)normals | (uintptr_t)points) & 3u)
        return fail(c, RT_ERR_INVALID, "%s: float and int32 arrays must be 4-byte aligned", what);
    if (kind == RT_QUERY_CLOSEST && ((uintptr_t)hits & 15u)) return fail(c, RT_ERR_INVALID, "%s: hits must be 16-byte aligned (one 16-byte store per ray)", what);
    hipStream_t st = nullptr;
    const int br = query_begin(c, st);
    if (br != RT_OK) return br;
    DevScene sc = make_dev_scene(c);
    if (!mesh) sc.hasBVH = 0;
    const bool any = kind == RT_QUERY_ANY;
    SceneRays r;
    r.o = xy ? nullptr : origins; r.d = xy ? nullptr : dirs; r.os = originStride; r.ds = dirStride; r.xy = xy; r.tm = tMax; r.n = (uint32_t)n;
    r.hits = any ? nullptr : reinterpret_cast<float4 *>(hits);
    r.objects = any ? nullptr : objects; r.normals = any ? nullptr : normals; r.points = any ? nullptr : points; r.occ = any ? occluded : nullptr;
    rt_scene_query_analytic(st, *u, sc, flags, r, c->dQueryFrame, c->dQueryHeads);
    const uint32_t built = mesh ? rt_wave_trace_scene(st, c->cus, c->treeDepth, c->dQueryFrame, sc, u->useBVH == RT_SCENE_HYBRID, r, u->inf, c->dQueryHeads) : 1u;
    const int end = query_end(c, st);
    return end != RT_OK || built ? end : fail(c, RT_ERR_UNSUPPORTED, "scene query: the library holds no k_trace build for the chosen options");
}

// host arrays: staged through the context's buffer (origins | dirs | xy | tMax | hits / occluded | objects | normals | points; the ray arrays keep their
// strides), then synchronised
int scene_query_host(RtContext *c, const char *what, const RtUniforms *u, int kind, int flags, const float *origins, int originStride, const float *dirs,
                     int dirStride, const int32_t *xy, const float *tMax, int n, RtHit *hits, int32_t *objects, float *normals, float *points, uint8_t *occluded) {
    bool mesh = false;
    const int rc = scene_query_args(c, what, u, kind, flags, origins, originStride, dirs, dirStride, xy, tMax, n, hits, occluded, mesh);
    if (rc != RT_OK || n == 0) return rc;
    const bool any = kind == RT_QUERY_ANY;
    const size_t N = (size_t)n;
    const StageSeg segs[] = {{origins, xy ? 0 : ((N - 1) * originStride + 3) * 4, false}, {dirs, xy ? 0 : ((N - 1) * dirStride + 3) * 4, false},
                             {xy, xy ? N * 8 : 0, false}, {tMax, tMax ? N * 4 : 0, false},
                             {any ? (void *)occluded : (void *)hits, any ? N : N * sizeof(RtHit), true}, {objects, (!any && objects) ? N * 4 : 0, true},
                             {normals, (!any && normals) ? N * 12 : 0, true}, {points, (!any && points) ? N * 12 : 0, true}};
    return staged(c, what, segs, [&](void *const *d) {
        return scene_query(c, what, u, kind, flags, (const float *)d[0], originStride, (const float *)d[1], dirStride, (const int32_t *)d[2], (const float *)d[3], n,
                           any ? nullptr : (RtHit *)d[4], (int32_t *)d[5], (float *)d[6], (float *)d[7], any ? (uint8_t *)d[4] : nullptr);
    });
}

// ---- multi-hit queries: the K nearest hits and the hit count per ray, by a traversal of their own (rt_multi_hit.hip).  Share the queries'
// scratch and event; touch no frame state.
// What both multi-hit entries check of their outputs and counts, before anything is enqueued or written
int multi_args(RtContext *c, const char *what, int n, int maxHits, const RtHit *hits, const int32_t *counts) {
    if (maxHits < 0 || maxHits > RT_MULTI_HIT_MAX) return fail(c, RT_ERR_INVALID, "%s: maxHits = %d (0 .. RT_MULTI_HIT_MAX = %d)", what, maxHits, RT_MULTI_HIT_MAX);
    if (n < 0) return fail(c, RT_ERR_INVALID, "%s: n = %d", what, n);
    if (n > 0 && maxHits > 0 && !hits) return fail(c, RT_ERR_INVALID, "%s: maxHits > 0 needs hits", what);
    if (n > 0 && maxHits == 0 && !counts) return fail(c, RT_ERR_INVALID, "%s: maxHits == 0 asks for the counts alone and needs counts", what);
    if ((uint64_t)n * (uint64_t)maxHits > (uint64_t)INT32_MAX) return fail(c, RT_ERR_INVALID, "%s: n * maxHits exceeds INT32_MAX records", what);
    return RT_OK;
}
int multi_aligned(RtContext *c, const char *what, const void *a, const void *b, const void *tMax, const RtHit *hits, const int32_t *counts) {
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)tMax | (uintptr_t)counts) & 3u) return fail(c, RT_ERR_INVALID, "%s: float and int32 arrays must be 4-byte aligned", what);
    if ((uintptr_t)hits & 15u) return fail(c, RT_ERR_INVALID, "%s: hits must be 16-byte aligned (one 16-byte store per record)", what);
    return RT_OK;
}
int multi_rays_args(RtContext *c, const char *what, const float *origins, int originStride, const float *dirs, int dirStride, int n, int maxHits, const RtHit *hits,
                    const int32_t *counts) {
    const int rc = multi_args(c, what, n, maxHits, hits, counts);
    if (rc != RT_OK) return rc;
    if (originStride < 3 || dirStride < 3) return fail(c, RT_ERR_INVALID, "%s: strides %d / %d floats (at least 3)", what, originStride, dirStride);
    if (n > 0 && (!origins || !dirs)) return fail(c, RT_ERR_INVALID, "%s: null ray arrays", what);
    if ((size_t)(n > 0 ? n - 1 : 0) * (size_t)std::max(originStride, dirStride) + 3 > ((size_t)1 << 32)) return fail(c, RT_ERR_INVALID, "%s: the ray arrays exceed 2^32 floats", what);
    if (c->nNodes <= 0 || c->nTris <= 0) return fail(c, RT_ERR_STATE, "%s: no BVH uploaded", what);
    return RT_OK;
}
// The pixel form: the frame's BVH scene only; u->nodeCount / u->triCount as scene_query_args checks them.  `mesh` = the scene has one.
int multi_pick_args(RtContext *c, const char *what, const RtUniforms *u, const int32_t *xy, int n, int maxHits, const RtHit *hits, const int32_t *counts, bool &mesh) {
    if (!u) return fail(c, RT_ERR_INVALID, "%s: null uniforms", what);
    int rc = multi_args(c, what, n, maxHits, hits, counts);
    if (rc != RT_OK) return rc;
    if (n > 0 && !xy) return fail(c, RT_ERR_INVALID, "%s: null pixel array", what);
    if (u->useBVH != 1) return fail(c, RT_ERR_INVALID, "%s: useBVH = %d -- multi-hit picking answers for the BVH scene only (useBVH == 1)", what, u->useBVH);
    mesh = u->nodeCount > 0 && u->triCount > 0;
    if (mesh && (c->nNodes == 0 || u->nodeCount > c->nNodes || u->triCount > c->nTris))
        return fail(c, RT_ERR_STATE, "%s: uniforms name %d nodes / %d tris, uploaded %d / %d", what, u->nodeCount, u->triCount, c->nNodes, c->nTris);
    return RT_OK;
}
int multi_launch(RtContext *c, bool mesh, const MultiHitQuery &q) {
    return QUERY_RUN(c, rt_multi_hit_launch(st, c->treeDepth, c->dQueryFrame, make_dev_scene(c), mesh, q));
}

// ---- nearest-point queries: the closest surface point per point, by a traversal of their own (rt_nearest.hip).  Share the queries' scratch
// and event; touch no frame state.
// What the entries check, before anything is enqueued or written.  needHits: the call writes records (not so the proximity query's counts alone)
int nearest_args(RtContext *c, const char *what, const float *points, int stride, int n, const RtHit *hits, bool needHits) {
    if (n < 0) return fail(c, RT_ERR_INVALID, "%s: n = %d", what, n);
    if (stride < 3) return fail(c, RT_ERR_INVALID, "%s: stride %d floats (at least 3)", what, stride);
    if (n > 0 && !points) return fail(c, RT_ERR_INVALID, "%s: null point array", what);
    if (n > 0 && needHits && !hits) return fail(c, RT_ERR_INVALID, "%s: the query needs hits", what);
    if ((size_t)(n > 0 ? n - 1 : 0) * (size_t)stride + 3 > ((size_t)1 << 32)) return fail(c, RT_ERR_INVALID, "%s: the point array exceeds 2^32 floats", what);
    if (c->nNodes <= 0 || c->nTris <= 0) return fail(c, RT_ERR_STATE, "%s: no BVH uploaded", what);
    return RT_OK;
}

// ---- proximity queries: the K nearest rows and the count within the limit per point, by a traversal of their own (rt_nearest_multi.hip).
// Share the queries' scratch and event; touch no frame state.
// What both entries check, before anything is enqueued or written: the records and counts first, then what nearest_args checks
int nearest_multi_args(RtContext *c, const char *what, const float *points, int stride, int n, int maxHits, const RtHit *hits, const int32_t *counts) {
    if (maxHits < 0 || maxHits > RT_NEAREST_MULTI_MAX)
        return fail(c, RT_ERR_INVALID, "%s: maxHits = %d (0 .. RT_NEAREST_MULTI_MAX = %d)", what, maxHits, RT_NEAREST_MULTI_MAX);
    if (n > 0 && maxHits == 0 && !counts) return fail(c, RT_ERR_INVALID, "%s: maxHits == 0 asks for the counts alone and needs counts", what);
    if (n > 0 && (uint64_t)n * (uint64_t)maxHits > (uint64_t)INT32_MAX) return fail(c, RT_ERR_INVALID, "%s: n * maxHits exceeds INT32_MAX records", what);
    return nearest_args(c, what, points, stride, n, hits, maxHits > 0);
}

// ---- box queries, triangle queries and hull queries: the rows overlapping an axis-aligned box, intersected
// by a query triangle, or overlapping a convex hexahedron, per query, by one traversal over three shapes (rt_overlap_query.hip).  Share the queries' scratch and event; touch no frame state.
// What tells the two apart in the checks, in the staging and in the launch: the floats of one query, the words of the messages, and the shape
struct OverlapKind { int floats; const char *layout, *noun; OverlapShape shape; };
constexpr OverlapKind kBoxes = {6, "lo.xyz, hi.xyz", "box", RT_OVERLAP_BOX}, kTris = {9, "p0.xyz, p1.xyz, p2.xyz", "triangle", RT_OVERLAP_TRI},
                      kHulls = {24, "c0.xyz .. c7.xyz", "hull", RT_OVERLAP_HULL};

// What all four entries check, before anything is enqueued or written.  offsets is the caller's to get right: device memory for the device entries
int overlap_args(RtContext *c, const char *what, const OverlapKind &k, const float *queries, int stride, int n, const int32_t *offsets, int cap, const int32_t *prims,
                 const int32_t *counts) {
    if (n < 0) return fail(c, RT_ERR_INVALID, "%s: n = %d", what, n);
    if (stride < k.floats) return fail(c, RT_ERR_INVALID, "%s: stride %d floats (at least %d: %s)", what, stride, k.floats, k.layout);
    if (n > 0 && !queries) return fail(c, RT_ERR_INVALID, "%s: null %s array", what, k.noun);
    if (n > 0 && !prims && !counts) return fail(c, RT_ERR_INVALID, "%s: the query needs prims or counts", what);
    if (prims && !offsets && cap < 0) return fail(c, RT_ERR_INVALID, "%s: cap = %d without offsets", what, cap);
    if (prims && !offsets && (uint64_t)n * (uint64_t)cap > (uint64_t)INT32_MAX) return fail(c, RT_ERR_INVALID, "%s: n * cap exceeds INT32_MAX entries", what);
    if ((size_t)(n > 0 ? n - 1 : 0) * (size_t)stride + (size_t)k.floats > ((size_t)1 << 32)) return fail(c, RT_ERR_INVALID, "%s: the %s array exceeds 2^32 floats", what, k.noun);
    if (c->nNodes <= 0 || c->nTris <= 0) return fail(c, RT_ERR_STATE, "%s: no BVH uploaded", what);
    return RT_OK;
}

// The device entry (rt_query_boxes, rt_query_tris or rt_query_hulls)
int overlap_query(RtContext *c, const char *what, const OverlapKind &k, const float *queries, int stride, int n, const int32_t *offsets, int cap, int32_t *prims,
                  int32_t *counts, int32_t *visits) {
    if (!c) return RT_ERR_INVALID;
    const int rc = overlap_args(c, what, k, queries, stride, n, offsets, cap, prims, counts);
    if (rc != RT_OK || n == 0) return rc;
    if (((uintptr_t)queries | (uintptr_t)offsets | (uintptr_t)prims | (uintptr_t)counts | (uintptr_t)visits) & 3u)
        return fail(c, RT_ERR_INVALID, "%s: float and int32 arrays must be 4-byte aligned", what);
    OverlapQuery q = {};
    q.q = queries; q.qs = stride; q.n = (uint32_t)n; q.offsets = prims ? offsets : nullptr; q.cap = cap; q.prims = prims; q.counts = counts; q.visits = visits;
    return QUERY_RUN(c, rt_overlap_launch(k.shape, st, c->treeDepth, c->dQueryFrame, make_dev_scene(c), q));
}

// Host offsets can be, and are, inspected: the staged prims array holds offsets[n] entries, or n * cap
int host_entries(RtContext *c, const char *what, int n, const int32_t *offsets, int cap, const int32_t *prims, size_t &entries) {
    entries = prims ? (size_t)n * (size_t)cap : 0;
    if (prims && offsets) {
        if (offsets[0] < 0) return fail(c, RT_ERR_INVALID, "%s: offsets[0] = %d", what, offsets[0]);
        for (int i = 0; i < n; ++i)
            if (offsets[i + 1] < offsets[i]) return fail(c, RT_ERR_INVALID, "%s: offsets descend at %d", what, i);
        entries = (size_t)offsets[n];
    }
    return RT_OK;
}

// The _host twin of `entry` (rt_query_boxes, rt_query_tris or rt_query_hulls): host pointers staged through the context's buffer
using OverlapEntry = int (*)(RtContext *, const float *, int, int, const int32_t *, int, int32_t *, int32_t *, int32_t *);
int overlap_host(RtContext *c, const char *what, const OverlapKind &k, OverlapEntry entry, const float *queries, int stride, int n, const int32_t *offsets, int cap,
                 int32_t *prims, int32_t *counts, int32_t *visits) {
    if (!c) return RT_ERR_INVALID;
    const int rc = overlap_args(c, what, k, queries, stride, n, offsets, cap, prims, counts);
    if (rc != RT_OK || n == 0) return rc;
    size_t entries = 0;
    const int er = host_entries(c, what, n, offsets, cap, prims, entries);
    if (er != RT_OK) return er;
    // staging layout: queries | offsets | prims | counts | visits | one spare word; the query array keeps its stride; prims goes in as well, for the entries
    // no list reaches.  An empty prims array has no staged address: the spare word stands in for it, and no list reaches that either
    const size_t N = (size_t)n;
    const int32_t spare = 0;
    const StageSeg segs[] = {{queries, ((N - 1) * stride + k.floats) * 4, false}, {offsets, prims && offsets ? (N + 1) * 4 : 0, false}, {prims, entries * 4, true, true},
                             {counts, counts ? N * 4 : 0, true}, {visits, visits ? N * 4 : 0, true}, {&spare, 4, false}};
    return staged(c, what, segs, [&](void *const *d) {
        return entry(c, (const float *)d[0], stride, n, (const int32_t *)d[1], cap, prims ? (int32_t *)(d[2] ? d[2] : d[5]) : nullptr, (int32_t *)d[3], (int32_t *)d[4]);
    });
}

// ---- marquee picking: the frusta behind rects of the frame, written into the caller's corners array by a kernel of their own, then
// the hull query on them, on the same stream and with no host wait
// What both entries check, before anything is enqueued or written: the camera, the depths and the rects, then what overlap_args checks of a hull query
// on `corners`
int pick_rects_args(RtContext *c, const char *what, const RtUniforms *u, const float *rects, int stride, int n, float tNear, float tFar, const float *corners,
                    const int32_t *offsets, int cap, const int32_t *prims, const int32_t *counts) {
    if (!u) return fail(c, RT_ERR_INVALID, "%s: null uniforms", what);
    if (!rthull::rect_args_ok(u, stride, tNear, tFar))
        return fail(c, RT_ERR_INVALID, "%s: resolution %g x %g, tNear %g, tFar %g, stride %d floats (a resolution above 0, tNear >= 0, tFar no NaN, at least 4: x0, y0, x1, y1)", what,
                    (double)u->resolution[0], (double)u->resolution[1], (double)tNear, (double)tFar, stride);
    if (n > 0 && (!rects || !corners)) return fail(c, RT_ERR_INVALID, "%s: null rect or corner array", what);
    if ((size_t)(n > 0 ? n - 1 : 0) * (size_t)stride + 4 > ((size_t)1 << 32)) return fail(c, RT_ERR_INVALID, "%s: the rect array exceeds 2^32 floats", what);
    return overlap_args(c, what, kHulls, corners, 24, n, offsets, cap, prims, counts);
}

}  // namespace

extern "C" {

// ---- ray queries: user rays through the frames' persistent traversal launch; reads the BVH, touches no frame state
int rt_trace_rays(RtContext *c, int kind, const float *origins, int originStride, const float *dirs, int dirStride, const float *tMax, float eps, float inf, int n,
                  RtHit *hits, float *normals, uint8_t *occluded) {
    if (!c) return RT_ERR_INVALID;
    const int rc = query_args(c, "rt_trace_rays", kind, 0, origins, originStride, dirs, dirStride, nullptr, tMax, n, hits, occluded, true);
    if (rc != RT_OK || n == 0) return rc;
    if (((uintptr_t)origins | (uintptr_t)dirs | (uintptr_t)tMax | (uintptr_t)normals) & 3u) return fail(c, RT_ERR_INVALID, "rt_trace_rays: float arrays must be 4-byte aligned");
    if (kind == RT_QUERY_CLOSEST && ((uintptr_t)hits & 15u)) return fail(c, RT_ERR_INVALID, "rt_trace_rays: hits must be 16-byte aligned (one 16-byte store per ray)");
    hipStream_t st = nullptr;
    const int br = query_begin(c, st);
    if (br != RT_OK) return br;
    const DevScene sc = make_dev_scene(c);
    const uint32_t built = rt_wave_trace_query(st, c->cus, c->treeDepth, c->dQueryFrame, sc, kind == RT_QUERY_ANY, origins, originStride, dirs, dirStride, tMax, eps, inf,
                                               (uint32_t)n, hits, normals, occluded, c->dQueryHeads);
    const int end = query_end(c, st);
    return end != RT_OK || built ? end : fail(c, RT_ERR_UNSUPPORTED, "rt_trace_rays: the library holds no k_trace build for the chosen options");
}

int rt_trace_rays_host(RtContext *c, int kind, const float *origins, int originStride, const float *dirs, int dirStride, const float *tMax, float eps, float inf, int n,
                       RtHit *hits, float *normals, uint8_t *occluded) {
    if (!c) return RT_ERR_INVALID;
    const int rc = query_args(c, "rt_trace_rays_host", kind, 0, origins, originStride, dirs, dirStride, nullptr, tMax, n, hits, occluded, true);
    if (rc != RT_OK || n == 0) return rc;
    // staging layout: origins | dirs | tMax | hits / occluded | normals; the ray arrays keep their strides
    const bool any = kind == RT_QUERY_ANY;
    const size_t N = (size_t)n;
    const StageSeg segs[] = {{origins, ((N - 1) * originStride + 3) * 4, false}, {dirs, ((N - 1) * dirStride + 3) * 4, false}, {tMax, tMax ? N * 4 : 0, false},
                             {any ? (void *)occluded : (void *)hits, any ? N : N * sizeof(RtHit), true}, {normals, (!any && normals) ? N * 12 : 0, true}};
    return staged(c, "rt_trace_rays_host", segs, [&](void *const *d) {
        return rt_trace_rays(c, kind, (const float *)d[0], originStride, (const float *)d[1], dirStride, (const float *)d[2], eps, inf, n,
                             any ? nullptr : (RtHit *)d[3], (float *)d[4], any ? (uint8_t *)d[3] : nullptr);
    });
}

int rt_trace_scene_rays(RtContext *c, const RtUniforms *u, int kind, int flags, const float *origins, int originStride, const float *dirs, int dirStride,
                        const float *tMax, int n, RtHit *hits, int32_t *objects, float *normals, float *points, uint8_t *occluded) {
    if (!c) return RT_ERR_INVALID;
    return scene_query(c, "rt_trace_scene_rays", u, kind, flags, origins, originStride, dirs, dirStride, nullptr, tMax, n, hits, objects, normals, points, occluded);
}

int rt_pick_pixels(RtContext *c, const RtUniforms *u, const int32_t *xy, int n, RtHit *hits, int32_t *objects, float *normals, float *points) {
    if (!c) return RT_ERR_INVALID;
    if (n > 0 && !xy) return fail(c, RT_ERR_INVALID, "rt_pick_pixels: null pixel array");
    return scene_query(c, "rt_pick_pixels", u, RT_QUERY_CLOSEST, 0, nullptr, 3, nullptr, 3, n > 0 ? xy : nullptr, nullptr, n, hits, objects, normals, points, nullptr);
}

int rt_trace_scene_rays_host(RtContext *c, const RtUniforms *u, int kind, int flags, const float *origins, int originStride, const float *dirs, int dirStride,
                             const float *tMax, int n, RtHit *hits, int32_t *objects, float *normals, float *points, uint8_t *occluded) {
    if (!c) return RT_ERR_INVALID;
    return scene_query_host(c, "rt_trace_scene_rays_host", u, kind, flags, origins, originStride, dirs, dirStride, nullptr, tMax, n, hits, objects, normals, points,
                            occluded);
}

int rt_pick_pixels_host(RtContext *c, const RtUniforms *u, const int32_t *xy, int n, RtHit *hits, int32_t *objects, float *normals, float *points) {
    if (!c) return RT_ERR_INVALID;
    if (n > 0 && !xy) return fail(c, RT_ERR_INVALID, "rt_pick_pixels_host: null pixel array");
    return scene_query_host(c, "rt_pick_pixels_host", u, RT_QUERY_CLOSEST, 0, nullptr, 3, nullptr, 3, n > 0 ? xy : nullptr, nullptr, n, hits, objects, normals,
                            points, nullptr);
}

// ---- multi-hit queries
int rt_trace_rays_multi(RtContext *c, const float *origins, int originStride, const float *dirs, int dirStride, const float *tMax, float eps, float inf, int n,
                        int maxHits, RtHit *hits, int32_t *counts) {
    if (!c) return RT_ERR_INVALID;
    int rc = multi_rays_args(c, "rt_trace_rays_multi", origins, originStride, dirs, dirStride, n, maxHits, hits, counts);
    if (rc != RT_OK || n == 0) return rc;
    rc = multi_aligned(c, "rt_trace_rays_multi", origins, dirs, tMax, maxHits ? hits : nullptr, counts);
    if (rc != RT_OK) return rc;
    MultiHitQuery q = {};
    q.o = origins; q.d = dirs; q.os = originStride; q.ds = dirStride; q.tm = tMax; q.n = (uint32_t)n; q.K = maxHits; q.eps = eps; q.inf = inf;
    q.hits = maxHits ? reinterpret_cast<float4 *>(hits) : nullptr; q.counts = counts;
    return multi_launch(c, true, q);
}

int rt_trace_rays_multi_host(RtContext *c, const float *origins, int originStride, const float *dirs, int dirStride, const float *tMax, float eps, float inf, int n,
                             int maxHits, RtHit *hits, int32_t *counts) {
    if (!c) return RT_ERR_INVALID;
    const int rc = multi_rays_args(c, "rt_trace_rays_multi_host", origins, originStride, dirs, dirStride, n, maxHits, hits, counts);
    if (rc != RT_OK || n == 0) return rc;
    // staging layout: origins | dirs | tMax | hits | counts; the ray arrays keep their strides
    const size_t N = (size_t)n;
    const StageSeg segs[] = {{origins, ((N - 1) * originStride + 3) * 4, false}, {dirs, ((N - 1) * dirStride + 3) * 4, false}, {tMax, tMax ? N * 4 : 0, false},
                             {hits, N * maxHits * sizeof(RtHit), true}, {counts, counts ? N * 4 : 0, true}};
    return staged(c, "rt_trace_rays_multi_host", segs, [&](void *const *d) {
        return rt_trace_rays_multi(c, (const float *)d[0], originStride, (const float *)d[1], dirStride, (const float *)d[2], eps, inf, n, maxHits, (RtHit *)d[3],
                                   (int32_t *)d[4]);
    });
}

int rt_pick_pixels_multi(RtContext *c, const RtUniforms *u, const int32_t *xy, int n, int maxHits, RtHit *hits, int32_t *counts) {
    if (!c) return RT_ERR_INVALID;
    bool mesh = false;
    int rc = multi_pick_args(c, "rt_pick_pixels_multi", u, xy, n, maxHits, hits, counts, mesh);
    if (rc != RT_OK || n == 0) return rc;
    rc = multi_aligned(c, "rt_pick_pixels_multi", xy, nullptr, nullptr, maxHits ? hits : nullptr, counts);
    if (rc != RT_OK) return rc;
    MultiHitQuery q = {};
    q.xy = xy; q.cam = u; q.os = q.ds = 3; q.n = (uint32_t)n; q.K = maxHits; q.eps = u->eps; q.inf = u->inf;
    q.hits = maxHits ? reinterpret_cast<float4 *>(hits) : nullptr; q.counts = counts;
    return multi_launch(c, mesh, q);
}

int rt_pick_pixels_multi_host(RtContext *c, const RtUniforms *u, const int32_t *xy, int n, int maxHits, RtHit *hits, int32_t *counts) {
    if (!c) return RT_ERR_INVALID;
    bool mesh = false;
    const int rc = multi_pick_args(c, "rt_pick_pixels_multi_host", u, xy, n, maxHits, hits, counts, mesh);
    if (rc != RT_OK || n == 0) return rc;
    const size_t N = (size_t)n;
    const StageSeg segs[] = {{xy, N * 8, false}, {hits, N * maxHits * sizeof(RtHit), true}, {counts, counts ? N * 4 : 0, true}};
    return staged(c, "rt_pick_pixels_multi_host", segs, [&](void *const *d) {
        return rt_pick_pixels_multi(c, u, (const int32_t *)d[0], n, maxHits, (RtHit *)d[1], (int32_t *)d[2]);
    });
}

// ---- nearest-point queries
int rt_query_nearest(RtContext *c, const float *points, int stride, const float *maxDist, int n, RtHit *hits, float *closest, int32_t *visits) {
    if (!c) return RT_ERR_INVALID;
    const int rc = nearest_args(c, "rt_query_nearest", points, stride, n, hits, true);
    if (rc != RT_OK || n == 0) return rc;
    if (((uintptr_t)points | (uintptr_t)maxDist | (uintptr_t)closest | (uintptr_t)visits) & 3u)
        return fail(c, RT_ERR_INVALID, "rt_query_nearest: float and int32 arrays must be 4-byte aligned");
    if ((uintptr_t)hits & 15u) return fail(c, RT_ERR_INVALID, "rt_query_nearest: hits must be 16-byte aligned (one 16-byte store per record)");
    NearestQuery q = {};
    q.p = points; q.ps = stride; q.md = maxDist; q.n = (uint32_t)n; q.hits = reinterpret_cast<float4 *>(hits); q.closest = closest; q.visits = visits;
    const char *e = getenv("RT_NEAREST_FAR_FIRST");   // (tests) the farther child first: the same answer by another visit order
    return QUERY_RUN(c, rt_nearest_launch(st, c->treeDepth, c->dQueryFrame, make_dev_scene(c), e && atoi(e) != 0, q));
}

int rt_query_nearest_host(RtContext *c, const float *points, int stride, const float *maxDist, int n, RtHit *hits, float *closest, int32_t *visits) {
    if (!c) return RT_ERR_INVALID;
    const int rc = nearest_args(c, "rt_query_nearest_host", points, stride, n, hits, true);
    if (rc != RT_OK || n == 0) return rc;
    // staging layout: points | maxDist | hits | closest | visits; the point array keeps its stride
    const size_t N = (size_t)n;
    const StageSeg segs[] = {{points, ((N - 1) * stride + 3) * 4, false}, {maxDist, maxDist ? N * 4 : 0, false}, {hits, N * sizeof(RtHit), true},
                             {closest, closest ? N * 12 : 0, true}, {visits, visits ? N * 4 : 0, true}};
    return staged(c, "rt_query_nearest_host", segs, [&](void *const *d) {
        return rt_query_nearest(c, (const float *)d[0], stride, (const float *)d[1], n, (RtHit *)d[2], (float *)d[3], (int32_t *)d[4]);
    });
}

// ---- proximity queries
int rt_query_nearest_multi(RtContext *c, const float *points, int stride, const float *maxDist, int n, int maxHits, RtHit *hits, int32_t *counts, float *closest,
                           int32_t *visits) {
    if (!c) return RT_ERR_INVALID;
    const int rc = nearest_multi_args(c, "rt_query_nearest_multi", points, stride, n, maxHits, hits, counts);
    if (rc != RT_OK || n == 0) return rc;
    if (((uintptr_t)points | (uintptr_t)maxDist | (uintptr_t)counts | (uintptr_t)closest | (uintptr_t)visits) & 3u)
        return fail(c, RT_ERR_INVALID, "rt_query_nearest_multi: float and int32 arrays must be 4-byte aligned");
    if (maxHits > 0 && ((uintptr_t)hits & 15u)) return fail(c, RT_ERR_INVALID, "rt_query_nearest_multi: hits must be 16-byte aligned (one 16-byte store per record)");
    NearestMultiQuery q = {};
    q.p = points; q.ps = stride; q.md = maxDist; q.n = (uint32_t)n; q.K = maxHits; q.hits = maxHits ? reinterpret_cast<float4 *>(hits) : nullptr; q.counts = counts;
    q.closest = maxHits ? closest : nullptr; q.visits = visits;
    const char *e = getenv("RT_NEAREST_FAR_FIRST");   // (tests) the farther child first: the same answer by another visit order
    return QUERY_RUN(c, rt_nearest_multi_launch(st, c->treeDepth, c->dQueryFrame, make_dev_scene(c), e && atoi(e) != 0, q));
}

int rt_query_nearest_multi_host(RtContext *c, const float *points, int stride, const float *maxDist, int n, int maxHits, RtHit *hits, int32_t *counts,
                                float *closest, int32_t *visits) {
    if (!c) return RT_ERR_INVALID;
    const int rc = nearest_multi_args(c, "rt_query_nearest_multi_host", points, stride, n, maxHits, hits, counts);
    if (rc != RT_OK || n == 0) return rc;
    // staging layout: points | maxDist | hits | counts | closest | visits; the point array keeps its stride
    const size_t N = (size_t)n, R = N * (size_t)maxHits;
    const StageSeg segs[] = {{points, ((N - 1) * stride + 3) * 4, false}, {maxDist, maxDist ? N * 4 : 0, false}, {hits, R * sizeof(RtHit), true},
                             {counts, counts ? N * 4 : 0, true}, {closest, closest ? R * 12 : 0, true}, {visits, visits ? N * 4 : 0, true}};
    return staged(c, "rt_query_nearest_multi_host", segs, [&](void *const *d) {
        return rt_query_nearest_multi(c, (const float *)d[0], stride, (const float *)d[1], n, maxHits, (RtHit *)d[2], (int32_t *)d[3], (float *)d[4], (int32_t *)d[5]);
    });
}

// ---- box queries
int rt_query_boxes(RtContext *c, const float *boxes, int stride, int n, const int32_t *offsets, int cap, int32_t *prims, int32_t *counts, int32_t *visits) {
    return overlap_query(c, "rt_query_boxes", kBoxes, boxes, stride, n, offsets, cap, prims, counts, visits);
}

int rt_query_boxes_host(RtContext *c, const float *boxes, int stride, int n, const int32_t *offsets, int cap, int32_t *prims, int32_t *counts, int32_t *visits) {
    return overlap_host(c, "rt_query_boxes_host", kBoxes, rt_query_boxes, boxes, stride, n, offsets, cap, prims, counts, visits);
}

// ---- triangle queries
int rt_query_tris(RtContext *c, const float *qtris, int stride, int n, const int32_t *offsets, int cap, int32_t *prims, int32_t *counts, int32_t *visits) {
    return overlap_query(c, "rt_query_tris", kTris, qtris, stride, n, offsets, cap, prims, counts, visits);
}

int rt_query_tris_host(RtContext *c, const float *qtris, int stride, int n, const int32_t *offsets, int cap, int32_t *prims, int32_t *counts, int32_t *visits) {
    return overlap_host(c, "rt_query_tris_host", kTris, rt_query_tris, qtris, stride, n, offsets, cap, prims, counts, visits);
}

// ---- hull queries
int rt_query_hulls(RtContext *c, const float *hulls, int stride, int n, const int32_t *offsets, int cap, int32_t *prims, int32_t *counts, int32_t *visits) {
    return overlap_query(c, "rt_query_hulls", kHulls, hulls, stride, n, offsets, cap, prims, counts, visits);
}

int rt_query_hulls_host(RtContext *c, const float *hulls, int stride, int n, const int32_t *offsets, int cap, int32_t *prims, int32_t *counts, int32_t *visits) {
    return overlap_host(c, "rt_query_hulls_host", kHulls, rt_query_hulls, hulls, stride, n, offsets, cap, prims, counts, visits);
}

int rt_pick_rects(RtContext *c, const RtUniforms *u, const float *rects, int stride, int n, float tNear, float tFar, float *corners, const int32_t *offsets, int cap,
                  int32_t *prims, int32_t *counts, int32_t *visits) {
    if (!c) return RT_ERR_INVALID;
    const int rc = pick_rects_args(c, "rt_pick_rects", u, rects, stride, n, tNear, tFar, corners, offsets, cap, prims, counts);
    if (rc != RT_OK || n == 0) return rc;
    if (((uintptr_t)rects | (uintptr_t)corners | (uintptr_t)offsets | (uintptr_t)prims | (uintptr_t)counts | (uintptr_t)visits) & 3u)
        return fail(c, RT_ERR_INVALID, "rt_pick_rects: float and int32 arrays must be 4-byte aligned");
    const rthull::RectCam cam = rthull::rect_cam(*u);
    OverlapQuery q = {};
    q.q = corners; q.qs = 24; q.n = (uint32_t)n; q.offsets = prims ? offsets : nullptr; q.cap = cap; q.prims = prims; q.counts = counts; q.visits = visits;
    return query_run(c, "rt_pick_rects", [&](hipStream_t st) {
        const DevScene sc = make_dev_scene(c);
        const hipError_t e = rt_rect_frusta_launch(st, c->dQueryFrame, sc, cam, rects, stride, (uint32_t)n, tNear, tFar, corners);
        return e != hipSuccess ? e : rt_overlap_launch(RT_OVERLAP_HULL, st, c->treeDepth, c->dQueryFrame, sc, q, true);   // (one prep launch per call)
    });
}

int rt_pick_rects_host(RtContext *c, const RtUniforms *u, const float *rects, int stride, int n, float tNear, float tFar, float *corners, const int32_t *offsets, int cap,
                       int32_t *prims, int32_t *counts, int32_t *visits) {
    if (!c) return RT_ERR_INVALID;
    const int rc = pick_rects_args(c, "rt_pick_rects_host", u, rects, stride, n, tNear, tFar, corners, offsets, cap, prims, counts);
    if (rc != RT_OK || n == 0) return rc;
    size_t entries = 0;
    const int er = host_entries(c, "rt_pick_rects_host", n, offsets, cap, prims, entries);
    if (er != RT_OK) return er;
    // staging layout: rects | corners | offsets | prims | counts | visits | one spare word, as overlap_host
    const size_t N = (size_t)n;
    const int32_t spare = 0;
    const StageSeg segs[] = {{rects, ((N - 1) * stride + 4) * 4, false}, {corners, N * 96, true}, {offsets, prims && offsets ? (N + 1) * 4 : 0, false},
                             {prims, entries * 4, true, true}, {counts, counts ? N * 4 : 0, true}, {visits, visits ? N * 4 : 0, true}, {&spare, 4, false}};
    return staged(c, "rt_pick_rects_host", segs, [&](void *const *d) {
        return rt_pick_rects(c, u, (const float *)d[0], stride, n, tNear, tFar, (float *)d[1], (const int32_t *)d[2], cap, prims ? (int32_t *)(d[3] ? d[3] : d[6]) : nullptr,
                             (int32_t *)d[4], (int32_t *)d[5]);
    });
}

}  // extern "C"
