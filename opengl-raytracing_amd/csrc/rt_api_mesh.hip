// rt_api_mesh.hip -- the dynamic-mesh part of the C ABI (include/rt_mi355.h): rt_bvh_layout and every rt_mesh_* entry point.
// Host code only: rt_mesh.hip and its siblings launch, this file checks arguments, orders the launches against the frame lanes and installs the scene.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rt_context.hpp"
#include "rt_mesh_uvs.hpp"
#include "rt_bvh_cost.hpp"
#include "rt_morph_pack.hpp"
#include "rt_normal_pack.hpp"
#include "rt_scene_pack.hpp"

using namespace rtd;
using namespace rtapi;

namespace {

// The two halves of the mesh path's event scheme around work enqueued on `st`, rt_stream()'s stream: what follows on `st` waits for
// everything already enqueued on every other lane ...
int mesh_after_lanes(RtContext *c, hipStream_t st) {
    for (int i = 0; i < c->nLanes; ++i) {
        if (c->lanes[i] == st) continue;
        HIP_TRY(c, hipEventRecord(c->evMeshLane[i], c->lanes[i]));
        HIP_TRY(c, hipStreamWaitEvent(st, c->evMeshLane[i], 0));
    }
    return RT_OK;
}
// ... and whatever another lane is given next waits for what has been enqueued on `st` so far.
int mesh_before_lanes(RtContext *c, hipStream_t st) {
    HIP_TRY(c, hipEventRecord(c->evMeshDone, st));
    for (int i = 0; i < c->nLanes; ++i)
        if (c->lanes[i] != st) HIP_TRY(c, hipStreamWaitEvent(c->lanes[i], c->evMeshDone, 0));
    return RT_OK;
}
// body(), which reads or writes what frames and queries on any lane read, between the two halves; a body that fails ends the call
template <class F> int between_lanes(RtContext *c, hipStream_t st, F &&body) {
    int rc = mesh_after_lanes(c, st);
    if (rc == RT_OK) rc = body();
    return rc == RT_OK ? mesh_before_lanes(c, st) : rc;
}

// body() may derive the order array of the current tree on `st` (rtl::mesh_order and whatever calls it).  If the array was not written before and is
// now, evMeshOrder is recorded behind it and meshOrderStream remembers where: a later reader on another stream -- frames rotate rt_stream() through
// the lanes -- waits for that launch by the event.  newTree: the body builds a new tree, whose order array no earlier call can have written.
// reads: the caller reads the array on `st`, and so is such a reader when the array was written before.  A body that fails ends the call.
template <class F> int with_order_event(RtContext *c, hipStream_t st, bool newTree, bool reads, F &&body) {
    const bool orderWas = !newTree && rtl::mesh_order_written(c->mesh);
    const int rc = body();
    if (rc != RT_OK) return rc;
    if (!orderWas && rtl::mesh_order_written(c->mesh)) { HIP_TRY(c, hipEventRecord(c->evMeshOrder, st)); c->meshOrderStream = st; }
    else if (orderWas && reads && c->meshOrderStream != st) HIP_TRY(c, hipStreamWaitEvent(st, c->evMeshOrder, 0));
    return RT_OK;
}

// The order array of the current tree, readable on `st`: derived there at the first call after a rebuild.
int mesh_order_on(RtContext *c, hipStream_t st, const char *who, const int **order) {
    return with_order_event(c, st, false, true, [&]() -> int {
        const char *err = nullptr;
        const int rc = rtl::mesh_order(c->mesh, st, order, &err);
        return rc == RT_OK ? RT_OK : fail(c, rc, "%s: %s", who, err ? err : "launch failed");
    });
}

// ---- the hit queries: per hit record of a closest-hit answer, an attribute of the mesh.  One routine serves the six
// device entry points and their *_host twins; a HitQuery is what tells them apart.
struct HitQuery {
    const char *entry;        // the device entry point: the name in a failed launch, also under the twin
    const char *needs;        // the arrays, as the "bad arguments" message lists them
    bool takesPoints;         // a second input, 12 bytes per hit
    int outputs, outBytes;    // output arrays (more than one: any may be null, not all) and their bytes per hit
    uintptr_t hitsMask;       // alignment of `hits` on the device: a kernel that loads whole records needs 16 bytes, the hit -> part map reads words
    const char *alignment;    // ... and the message behind it
    const void *(*enabled)(const rtl::Mesh *);   // null: the tree is all it takes
    const char *disabled;
    bool wantsOrder;
    int (*launch)(rtl::Mesh *, hipStream_t, const int *order, const void *hits, const float *points, int n, void *out0, void *out1, const char **err);
};

const HitQuery kHitParts = {
    "rt_mesh_hit_parts", "hits and one of parts / tris", false, 2, 4, 3u, "arrays must be 4-byte aligned", nullptr, nullptr, true,
    [](rtl::Mesh *m, hipStream_t st, const int *order, const void *hits, const float *, int n, void *parts, void *tris, const char **err) {
        return rtl::mesh_hit_parts(m, st, order, hits, n, (int32_t *)parts, (int32_t *)tris, err);
    }};
const HitQuery kHitPrevPoints = {
    "rt_mesh_hit_prev_points", "hits, points and prevPoints", true, 1, 12, 15u, "hits must be 16-byte aligned, points and prevPoints 4-byte aligned",
    [](const rtl::Mesh *m) -> const void * { return rtl::mesh_prev_tris(m); }, "motion is not enabled (rt_mesh_motion_enable first)", false,
    [](rtl::Mesh *m, hipStream_t st, const int *, const void *hits, const float *points, int n, void *prevPoints, void *, const char **err) {
        return rtl::mesh_hit_prev_points(m, st, hits, points, n, (float *)prevPoints, err);
    }};
const HitQuery kHitNormals = {
    "rt_mesh_hit_normals", "hits and normals", false, 1, 12, 15u, "hits must be 16-byte aligned, normals 4-byte aligned",
    [](const rtl::Mesh *m) -> const void * { return rtl::mesh_normal_rows(m); }, "normals are not enabled (rt_mesh_normals_enable first)", false,
    [](rtl::Mesh *m, hipStream_t st, const int *, const void *hits, const float *, int n, void *normals, void *, const char **err) {
        return rtl::mesh_hit_normals(m, st, hits, n, (float *)normals, err);
    }};
const HitQuery kHitColors = {
    "rt_mesh_hit_colors", "hits and colors", false, 1, 12, 15u, "hits must be 16-byte aligned, colors 4-byte aligned",
    [](const rtl::Mesh *m) -> const void * { return rtl::mesh_color_rows(m); }, "colours are not enabled (rt_mesh_colors_enable first)", false,
    [](rtl::Mesh *m, hipStream_t st, const int *, const void *hits, const float *, int n, void *colors, void *, const char **err) {
        return rtl::mesh_hit_blend(m, rtl::Corner::colors, st, hits, n, (float *)colors, err);
    }};
const HitQuery kHitUvs = {
    "rt_mesh_hit_uvs", "hits and uvs", false, 1, 8, 15u, "hits must be 16-byte aligned, uvs 4-byte aligned",
    [](const rtl::Mesh *m) -> const void * { return rtl::mesh_uv_rows(m); }, "UVs are not enabled (rt_mesh_uvs_enable first)", false,
    [](rtl::Mesh *m, hipStream_t st, const int *, const void *hits, const float *, int n, void *uvs, void *, const char **err) {
        return rtl::mesh_hit_blend(m, rtl::Corner::uvs, st, hits, n, (float *)uvs, err);
    }};
const HitQuery kHitTexels = {
    "rt_mesh_hit_texels", "hits and texels", false, 1, 12, 15u, "hits must be 16-byte aligned, texels 4-byte aligned",
    [](const rtl::Mesh *m) -> const void * { return rtl::mesh_uv_rows(m) ? (const void *)rtl::mesh_texture(m) : nullptr; },
    "UVs and a texture are needed (rt_mesh_uvs_enable and rt_mesh_texture_upload first)", false,
    [](rtl::Mesh *m, hipStream_t st, const int *, const void *hits, const float *, int n, void *texels, void *, const char **err) {
        return rtl::mesh_hit_texels(m, st, hits, n, (float *)texels, err);
    }};

// who: the entry point called.  host: its arrays are host memory, staged as hits | points | outputs around the device path (an output the caller
// leaves out still gets its room: the launch is the same).  Everything is checked before any device work, and n == 0 does none.
int mesh_hit_query(RtContext *c, const HitQuery &q, const char *who, bool host, const RtHit *hits, const float *points, int n, void *out0, void *out1) {
    if (!c) return RT_ERR_INVALID;
    if (n < 0 || (n > 0 && (!hits || (q.takesPoints && !points))) || (!out0 && !out1)) return fail(c, RT_ERR_INVALID, "%s: bad arguments (n = %d; %s are needed)", who, n, q.needs);
    if (!c->mesh || !rtl::mesh_has_tree(c->mesh)) return fail(c, RT_ERR_INVALID, "%s: no tree (rt_mesh_upload and rt_mesh_rebuild first)", who);
    if (q.enabled && !q.enabled(c->mesh)) return fail(c, RT_ERR_INVALID, "%s: %s", who, q.disabled);
    if (!host && (((uintptr_t)hits & q.hitsMask) || (((uintptr_t)points | (uintptr_t)out0 | (uintptr_t)out1) & 3u))) return fail(c, RT_ERR_INVALID, "%s: %s", who, q.alignment);
    if (n == 0) return RT_OK;
    auto onDevice = [&](const void *dHits, const float *dPoints, void *d0, void *d1) -> int {
        (void)hipSetDevice(c->cfg.device);
        hipStream_t st = api_stream(c);
        const int *order = nullptr;
        if (q.wantsOrder) {
            const int rc = mesh_order_on(c, st, q.entry, &order);
            if (rc != RT_OK) return rc;
        }
        const char *err = nullptr;
        const int rc = q.launch(c->mesh, st, order, dHits, dPoints, n, d0, d1, &err);
        return rc == RT_OK ? RT_OK : fail(c, rc, "%s: %s", q.entry, err ? err : "launch failed");
    };
    if (!host) return onDevice(hits, points, out0, out1);
    const size_t N = (size_t)n;
    const StageSeg segs[] = {{hits, N * sizeof(RtHit), false}, {points, q.takesPoints ? N * 12 : 0, false}, {out0, N * q.outBytes, true}, {out1, q.outputs > 1 ? N * q.outBytes : 0, true}};
    return staged(c, who, segs, [&](void *const *d) { return onDevice(d[0], (const float *)d[1], d[2], d[3]); });
}

// ---- the corner attributes a caller writes (colours 14.14, UVs 14.15): rt_mesh.hip gathers their rows inside every update; this file owns
// enabling, the ordering of the writes and of the gather alone.  One routine each serves rt_mesh_colors_* and rt_mesh_uvs_*; a CornerApi is what
// tells them apart.
struct CornerApi {
    rtl::Corner which;
    const char *enable, *accessor, *set, *refresh;   // the entry points
    const char *noun;                                // in the messages
    int floats;                                      // per vertex, as the host hands them over
    size_t stride;                                   // bytes per vertex on the device
    bool repack;                                     // ... where every vertex is four floats, the last one 0
    bool (*ok)(float);                               // what a component must be
    const char *needed;                              // ... and the message behind it
};
const CornerApi kColorsApi = {rtl::Corner::colors, "rt_mesh_colors_enable", "rt_mesh_colors", "rt_mesh_set_colors", "rt_mesh_colors_refresh", "colours", 3, 16, true,
                              [](float x) { return x >= 0.0f && x < INFINITY; }, "finite and >= 0 is needed"};
const CornerApi kUvsApi = {rtl::Corner::uvs, "rt_mesh_uvs_enable", "rt_mesh_uvs", "rt_mesh_set_uvs", "rt_mesh_uvs_refresh", "UVs", 2, 8, false,
                           [](float x) { return std::isfinite(x); }, "a finite value is needed"};

int corner_enable(RtContext *c, const CornerApi &a, int on) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "%s: no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)", a.enable);
    (void)hipSetDevice(c->cfg.device);
    HIP_TRY(c, sync_all(c));   // frames in flight read the array that is about to appear or go
    if (!on) { rtl::mesh_corner_release(c->mesh, a.which); return RT_OK; }
    if (rtl::mesh_corner_vertices(c->mesh, a.which)) return RT_OK;   // already enabled: the values and the rows stay as they are, nothing is allocated
    hipStream_t st = api_stream(c);   // rt_stream()
    const char *err = nullptr;
    int rc = RT_OK;
    // (a create that fails behind the order array's launch leaves the array written: the event is recorded either way; rt_mesh_normals_enable too)
    const int er = with_order_event(c, st, false, false, [&] { rc = rtl::mesh_corner_create(c->mesh, a.which, st, &err); return RT_OK; });
    if (er != RT_OK) return er;
    if (rc != RT_OK) return fail(c, rc, "%s: %s", a.enable, err ? err : "allocation failed");
    return RT_OK;
}

int corner_accessor(RtContext *c, const CornerApi &a, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes) return RT_ERR_INVALID;
    *devPtr = nullptr; *bytes = 0;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "%s: no mesh (rt_mesh_upload first)", a.accessor);
    if (!rtl::mesh_corner_vertices(c->mesh, a.which)) return fail(c, RT_ERR_INVALID, "%s: %s are not enabled (%s first)", a.accessor, a.noun, a.enable);
    *devPtr = rtl::mesh_corner_vertices(c->mesh, a.which);
    *bytes = (size_t)rtl::mesh_verts(c->mesh) * a.stride;
    return RT_OK;
}

int corner_set(RtContext *c, const CornerApi &a, const float *values, int first, int count) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh || !rtl::mesh_corner_vertices(c->mesh, a.which)) return fail(c, RT_ERR_INVALID, "%s: no %s (rt_mesh_upload and %s first)", a.set, a.noun, a.enable);
    const int n = rtl::mesh_verts(c->mesh);
    if (first < 0 || count < 0 || first > n || count > n - first) return fail(c, RT_ERR_INVALID, "%s: vertices %d .. %d of %d", a.set, first, first + count, n);
    if (count == 0) return RT_OK;
    if (!values) return fail(c, RT_ERR_INVALID, "%s: null %s", a.set, a.noun);
    const size_t F = (size_t)a.floats;
    for (size_t i = 0; i < (size_t)count * F; ++i)
        if (!a.ok(values[i])) return fail(c, RT_ERR_INVALID, "%s: component %zu of vertex %zu is %g (%s)", a.set, i % F, (size_t)first + i / F, (double)values[i], a.needed);
    return guarded(c, a.set, [&]() -> int {
        (void)hipSetDevice(c->cfg.device);
        hipStream_t st = api_stream(c);   // rt_stream()
        // The source is pageable host memory: the caller's array or, repacked, (r, g, b, 0) per vertex as the device holds them in a buffer of the call's
        // own.  Either may go when the call returns only because the HIP runtime finishes with pageable host memory -- stages it, or completes the copy
        // -- before hipMemcpyAsync returns; rt_mesh_set_bones leans on the same.  So the call is ordered on the stream like rt_mesh_set_bones, and like
        // it may spend the copy's time on the host.
        std::vector<float> v4;
        if (a.repack) {
            v4.resize((size_t)count * 4);
            for (size_t i = 0; i < (size_t)count; ++i) { v4[4 * i] = values[3 * i]; v4[4 * i + 1] = values[3 * i + 1]; v4[4 * i + 2] = values[3 * i + 2]; v4[4 * i + 3] = 0.0f; }
        }
        return between_lanes(c, st, [&]() -> int {   // a gather enqueued on another lane reads the vertex array
            char *dst = static_cast<char *>(rtl::mesh_corner_vertices(c->mesh, a.which)) + (size_t)first * a.stride;
            HIP_TRY(c, hipMemcpyAsync(dst, a.repack ? v4.data() : values, (size_t)count * a.stride, hipMemcpyHostToDevice, st));
            return RT_OK;
        });
    });
}

int corner_refresh(RtContext *c, const CornerApi &a) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "%s: no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)", a.refresh);
    if (!rtl::mesh_corner_vertices(c->mesh, a.which)) return fail(c, RT_ERR_INVALID, "%s: %s are not enabled (%s first)", a.refresh, a.noun, a.enable);
    if (!rtl::mesh_has_tree(c->mesh)) return fail(c, RT_ERR_INVALID, "%s: no rows to fill (rt_mesh_rebuild first)", a.refresh);
    (void)hipSetDevice(c->cfg.device);
    hipStream_t st = api_stream(c);   // rt_stream()
    // frames and queries on every lane read the rows they were enqueued with, and whatever a lane is given next sees the new ones
    return between_lanes(c, st, [&] {
        return with_order_event(c, st, false, false, [&]() -> int {
            const char *err = nullptr;
            const int rc = rtl::mesh_corner_refresh(c->mesh, a.which, st, &err);
            return rc == RT_OK ? RT_OK : fail(c, rc, "%s: %s", a.refresh, err ? err : "launch failed");
        });
    });
}

}  // namespace

extern "C" {

// ---- dynamic mesh: rt_mesh.hip builds, this file orders the rebuild against the lanes and installs its arrays
int rt_bvh_layout(int nTris, RtBvhLayout *out) {
    if (!out) return RT_ERR_INVALID;
    std::memset(out, 0, sizeof *out);
    return guarded(nullptr, "rt_bvh_layout", [&]() -> int {
        rtl::BvhLayout L;
        const int rc = rtl::bvh_layout(nTris, L);
        if (rc == RT_ERR_INVALID) return fail(nullptr, rc, "rt_bvh_layout: nTris = %d", nTris);
        if (rc != RT_OK) return fail(nullptr, rc, "rt_bvh_layout: %d triangles exceed the 2^28 leaf encoding or the 32-entry traversal stack", nTris);
        out->nTris = L.nTris; out->nNodes = L.nNodes; out->nInner = L.nInner; out->treeDepth = L.treeDepth;
        out->nWide4 = (int32_t)L.nWide4; out->nPairs = (int32_t)L.nPairs; out->anyStack = L.anyStack;
        out->quantised = rtl::want_quantised(rtl::pack_options_from_env(), L.nWide4, L.rootRef4) ? 1 : 0;
        out->bytesNodes2 = (uint64_t)std::max(L.nInner, 1) * 64;
        out->bytesNodes4 = out->quantised ? (uint64_t)L.nWide4 * 64 + (uint64_t)L.nLeaves * 32 : (uint64_t)L.nWide4 * 128;
        out->bytesPairs = (uint64_t)L.nPairs * 80;
        out->bytesTris = (uint64_t)L.nTris * 48;
        return RT_OK;
    });
}

static void mesh_quality_reset(RtContext *c) {
    for (auto &sl : c->meshQSlot) sl = RtContext::MeshQSlot{};
    c->meshQLatest = c->meshQBaseline = RtMeshQuality{};
    c->meshQHaveLatest = c->meshQHaveBaseline = false;
    c->meshQLatestTree = c->meshQBaselineTree = 0;
    c->meshQSkipped = c->meshQEnqueued = 0;
    c->meshQNewest = -1;
}

// rt_mesh_upload (partFirst == null: one part holding everything) and rt_mesh_upload_parts
static int mesh_upload(RtContext *c, const char *who, const float *positions, int nVerts, const uint32_t *indices, int nIdx, const int32_t *partFirst, int nParts) {
    if (!c) return RT_ERR_INVALID;
    if (nIdx < 0 || nVerts < 0 || (nIdx > 0 && (!positions || !indices || nVerts == 0))) return fail(c, RT_ERR_INVALID, "%s: bad arguments", who);
    if (nIdx % 3 != 0) return fail(c, RT_ERR_INVALID, "%s: %d indices are not a list of triangles", who, nIdx);
    for (int k = 0; k < nIdx; ++k)
        if (indices[k] >= (uint32_t)nVerts) return fail(c, RT_ERR_INVALID, "%s: index %d names vertex %u of %d", who, k, indices[k], nVerts);
    const int32_t one[2] = {0, nIdx / 3};
    if (!partFirst) { partFirst = one; nParts = 1; }
    if (nParts < 1 || nParts > RT_MAX_MESH_PARTS) return fail(c, RT_ERR_INVALID, "%s: %d parts (1 .. %d)", who, nParts, RT_MAX_MESH_PARTS);
    if (partFirst[0] != 0 || partFirst[nParts] != nIdx / 3)
        return fail(c, RT_ERR_INVALID, "%s: partFirst runs from %d to %d, the mesh from 0 to %d triangles", who, partFirst[0], partFirst[nParts], nIdx / 3);
    for (int p = 0; p < nParts; ++p)
        if (partFirst[p + 1] < partFirst[p]) return fail(c, RT_ERR_INVALID, "%s: partFirst decreases at part %d (%d after %d)", who, p, partFirst[p + 1], partFirst[p]);
    const rtl::PackOptions opt = rtl::pack_options_from_env();
    if (nIdx > 0) {
        if (opt.fused) return fail(c, RT_ERR_UNSUPPORTED, "%s: RT_FUSED records are not rebuilt on the device", who);
        if (opt.implicit) return fail(c, RT_ERR_UNSUPPORTED, "%s: RT_IMPLICIT records are not rebuilt on the device", who);
        if (opt.anyhitSah) return fail(c, RT_ERR_UNSUPPORTED, "%s: the RT_ANYHIT_TREE=sah tree is not rebuilt on the device", who);
        if (nIdx / 3 >= (1 << 28)) return fail(c, RT_ERR_UNSUPPORTED, "%s: %d triangles exceed the 2^28 leaf encoding", who, nIdx / 3);
    }
    const int rc = rt_upload_bvh(c, nullptr, 0, nullptr, 0);   // waits for the lanes, removes the scene and the previous mesh, forgets the bounce share
    if (rc != RT_OK || nIdx == 0) return rc;
    return guarded(c, who, [&]() -> int {
        rtl::BvhLayout L;
        const int lr = rtl::bvh_layout(nIdx / 3, L);
        if (lr != RT_OK) return fail(c, lr, "%s: %d triangles cannot be laid out", who, nIdx / 3);
        const char *err = nullptr;
        const int mr = rtl::mesh_create(positions, nVerts, indices, nIdx, partFirst, nParts, rtl::want_quantised(opt, L.nWide4, L.rootRef4), opt.sparseLeafBoxes, &c->mesh, &err);
        if (mr != RT_OK) { c->mesh = nullptr; return fail(c, mr, "%s: %s", who, err ? err : "layout failed"); }
        bool ok = hipEventCreateWithFlags(&c->evMeshDone, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&c->evMeshOrder, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; ok && i < c->nLanes; ++i) ok = hipEventCreateWithFlags(&c->evMeshLane[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) { release_mesh(c); return fail(c, RT_ERR_HIP, "%s: event creation failed", who); }
        c->meshRebuilds = c->meshHostSyncs = c->meshRefits = c->meshRefitsSinceRebuild = 0;
        mesh_quality_reset(c);
        return RT_OK;
    });
}

int rt_mesh_upload(RtContext *c, const float *positions, int nVerts, const uint32_t *indices, int nIdx) {
    return mesh_upload(c, "rt_mesh_upload", positions, nVerts, indices, nIdx, nullptr, 1);
}

int rt_mesh_upload_parts(RtContext *c, const float *positions, int nVerts, const uint32_t *indices, int nIdx, const int32_t *partFirst, int nParts) {
    if (!c) return RT_ERR_INVALID;
    if (!partFirst) return fail(c, RT_ERR_INVALID, "rt_mesh_upload_parts: null partFirst");
    return mesh_upload(c, "rt_mesh_upload_parts", positions, nVerts, indices, nIdx, partFirst, nParts);
}

int rt_mesh_parts(RtContext *c, int32_t *partFirst, int capacity, int *nParts) {
    if (!c || !nParts) return RT_ERR_INVALID;
    *nParts = 0;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_parts: no mesh (rt_mesh_upload first)");
    const int n = rtl::mesh_part_count(c->mesh);
    *nParts = n;
    if (!partFirst) return RT_OK;
    if (capacity < n + 1) return fail(c, RT_ERR_INVALID, "rt_mesh_parts: room for %d entries, the table has %d", capacity, n + 1);
    std::memcpy(partFirst, rtl::mesh_part_first(c->mesh), (size_t)(n + 1) * sizeof(int32_t));
    return RT_OK;
}

int rt_mesh_part_matrices(RtContext *c, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes) return RT_ERR_INVALID;
    *devPtr = nullptr; *bytes = 0;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_part_matrices: no mesh (rt_mesh_upload first)");
    *devPtr = rtl::mesh_part_matrices(c->mesh);
    *bytes = (size_t)rtl::mesh_part_count(c->mesh) * 64;
    return RT_OK;
}

int rt_mesh_set_part_matrices(RtContext *c, int first, int count, const float *M16s) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_set_part_matrices: no mesh (rt_mesh_upload first)");
    const int n = rtl::mesh_part_count(c->mesh);
    if (first < 0 || count < 0 || first > n || count > n - first) return fail(c, RT_ERR_INVALID, "rt_mesh_set_part_matrices: entries %d .. %d of a table of %d", first, first + count, n);
    if (count == 0) return RT_OK;
    if (!M16s) return fail(c, RT_ERR_INVALID, "rt_mesh_set_part_matrices: null matrices");
    (void)hipSetDevice(c->cfg.device);
    if (c->raster && rt_raster_order_after(c->raster, api_stream(c)) != RT_OK) return fail(c, RT_ERR_HIP, "rt_mesh_set_part_matrices: %s", rt_raster_error(c->raster));
    HIP_TRY(c, hipMemcpyAsync(rtl::mesh_part_matrices(c->mesh) + (size_t)first * 16, M16s, (size_t)count * 64, hipMemcpyHostToDevice, api_stream(c)));
    return RT_OK;
}

int rt_mesh_positions(RtContext *c, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes) return RT_ERR_INVALID;
    *devPtr = nullptr; *bytes = 0;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_positions: no mesh (rt_mesh_upload first)");
    *devPtr = rtl::mesh_positions(c->mesh);
    *bytes = (size_t)rtl::mesh_verts(c->mesh) * 12;
    return RT_OK;
}

int rt_mesh_set_positions(RtContext *c, const float *positions) {
    if (!c || !positions) return RT_ERR_INVALID;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_set_positions: no mesh (rt_mesh_upload first)");
    (void)hipSetDevice(c->cfg.device);
    if (c->raster && rt_raster_order_after(c->raster, api_stream(c)) != RT_OK) return fail(c, RT_ERR_HIP, "rt_mesh_set_positions: %s", rt_raster_error(c->raster));
    HIP_TRY(c, hipMemcpyAsync(rtl::mesh_positions(c->mesh), positions, (size_t)rtl::mesh_verts(c->mesh) * 12, hipMemcpyHostToDevice, api_stream(c)));
    return RT_OK;
}

// A rebuild or a refit: the device work of rt_mesh.hip between the two halves of the event scheme, then the scene installed (the same pointers and
// counts every time; what a refit can change is whether the quantised nodes could be built).
// parts: gather under the device matrix table instead of under M16.
static int mesh_update(RtContext *c, const float *M16, bool refit, bool parts = false, const char *caller = nullptr) {
    const char *who = caller ? caller : parts ? (refit ? "rt_mesh_refit_parts" : "rt_mesh_rebuild_parts") : (refit ? "rt_mesh_refit" : "rt_mesh_rebuild");
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "%s: no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)", who);
    if (refit && !rtl::mesh_has_tree(c->mesh)) return fail(c, RT_ERR_INVALID, "%s: no tree to keep (rt_mesh_rebuild first)", who);
    (void)hipSetDevice(c->cfg.device);
    static const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    hipStream_t st = api_stream(c);   // rt_stream()
    const char *err = nullptr;
    const float *gatherM = parts ? nullptr : (M16 ? M16 : kIdentity);   // null: the part-aware gather
    // every lane's frames and queries read the arrays that are about to be rewritten: the update waits for them, and whatever a lane is given next
    // waits for it.  Smooth normals and colours: the update derives the order array for itself, on `st`
    int rc = between_lanes(c, st, [&] {
        return with_order_event(c, st, !refit, false, [&]() -> int {
            const int ur = refit ? rtl::mesh_refit(c->mesh, st, gatherM, &err) : rtl::mesh_rebuild(c->mesh, st, gatherM, &err);
            return ur == RT_OK ? RT_OK : fail(c, ur, "%s: %s", who, err ? err : "launch failed");
        });
    });
    if (rc != RT_OK) return rc;
    const rtl::BvhLayout &L = rtl::mesh_layout(c->mesh);
    const rtl::MeshScene &sc = rtl::mesh_scene(c->mesh);
    bool okQ = sc.q4 != nullptr;
    if (sc.q4) {   // the host picks the any-hit kernel by whether the quantised nodes exist: the one allowed wait
        rc = rtl::mesh_quantised_ok(c->mesh, st, okQ, &err);
        ++c->meshHostSyncs;
        if (rc != RT_OK) return fail(c, rc, "%s: %s", who, err ? err : "status read failed");
    }
    // install: pointers and counts are those of the mesh, the same at every rebuild
    c->dWNodes = sc.wnodes; c->dWNodesW = sc.wnodesW; c->dW4 = sc.w4; c->dPairs = sc.pairs; c->dTris = sc.tris;
    c->dQ4 = okQ ? sc.q4 : nullptr; c->dLeafBox = okQ ? sc.leafBox : nullptr;
    c->leafBoxBytes = sc.leafBoxBytes; c->leafBoxMagic = sc.leafBoxMagic; c->nLeafBoxes = L.nLeaves;
    c->sceneFlags = (sc.q4 && !okQ) ? RT_SCENE_QNODES_REJECTED : 0;
    if (sc.q4 && !okQ && rtl::pack_options_from_env().verbose) fprintf(stderr, "[%s] quantised any-hit nodes rejected (exponent range): walking the exact 112-byte nodes\n", who);
    c->nNodes = L.nNodes; c->nTris = L.nTris; c->nInner = L.nInner; c->treeDepth = L.treeDepth;
    c->nWide4 = L.nWide4; c->nPairs = L.nPairs; c->nFused = 0;
    c->rootRef = L.rootRef; c->rootRefW = L.rootRefW; c->rootRef4 = L.rootRef4; c->anyStack = L.anyStack;
    c->dRootBox = sc.rootBox;
    c->sceneFromMesh = true;
    if (refit) { ++c->meshRefits; ++c->meshRefitsSinceRebuild; }
    else { ++c->meshRebuilds; c->meshRefitsSinceRebuild = 0; }
    if (rtl::mesh_prev_tris(c->mesh)) c->meshMotionDirty = true;
    return RT_OK;
}

int rt_mesh_rebuild(RtContext *c, const float *M16) { return mesh_update(c, M16, false); }
int rt_mesh_refit(RtContext *c, const float *M16) { return mesh_update(c, M16, true); }
int rt_mesh_rebuild_parts(RtContext *c) { return mesh_update(c, nullptr, false, true); }
int rt_mesh_refit_parts(RtContext *c) { return mesh_update(c, nullptr, true, true); }

// ---- previous pose: rt_mesh.hip moves it inside every update; this file owns enabling, the latch's ordering and the hit query
int rt_mesh_motion_enable(RtContext *c, int on) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_motion_enable: no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)");
    (void)hipSetDevice(c->cfg.device);
    HIP_TRY(c, sync_all(c));   // frames in flight read the array that is about to appear or go
    c->meshMotionDirty = false;
    if (!on) { rtl::mesh_motion_release(c->mesh); return RT_OK; }
    const char *err = nullptr;
    const int rc = rtl::mesh_motion_create(c->mesh, &err);
    if (rc != RT_OK) return fail(c, rc, "rt_mesh_motion_enable: %s", err ? err : "allocation failed");
    return RT_OK;
}

int rt_mesh_motion_latch(RtContext *c) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_motion_latch: no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)");
    if (!rtl::mesh_prev_tris(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_motion_latch: motion is not enabled (rt_mesh_motion_enable first)");
    if (!rtl::mesh_has_tree(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_motion_latch: no pose to keep (rt_mesh_rebuild first)");
    (void)hipSetDevice(c->cfg.device);
    hipStream_t st = api_stream(c);   // rt_stream()
    // frames and queries on every lane read the previous pose they were enqueued with, and whatever a lane is given next sees the latched one
    return between_lanes(c, st, [&]() -> int {
        const char *err = nullptr;
        const int rc = rtl::mesh_motion_latch(c->mesh, st, &err);
        if (rc != RT_OK) return fail(c, rc, "rt_mesh_motion_latch: %s", err ? err : "copy failed");
        c->meshMotionDirty = false;
        return RT_OK;
    });
}

int rt_mesh_hit_prev_points(RtContext *c, const RtHit *hits, const float *points, int n, float *prevPoints) {
    return mesh_hit_query(c, kHitPrevPoints, "rt_mesh_hit_prev_points", false, hits, points, n, prevPoints, nullptr);
}
int rt_mesh_hit_prev_points_host(RtContext *c, const RtHit *hits, const float *points, int n, float *prevPoints) {
    return mesh_hit_query(c, kHitPrevPoints, "rt_mesh_hit_prev_points_host", true, hits, points, n, prevPoints, nullptr);
}

// ---- smooth vertex normals: rt_normal_pack.cpp packs the adjacency, rt_mesh.hip recomputes the normals inside every update; this file
// owns enabling and the hit query
int rt_mesh_normals_enable(RtContext *c, int on) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_normals_enable: no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)");
    return guarded(c, "rt_mesh_normals_enable", [&]() -> int {
        (void)hipSetDevice(c->cfg.device);
        HIP_TRY(c, sync_all(c));   // frames in flight read the array that is about to appear or go
        if (!on) { rtl::mesh_corner_release(c->mesh, rtl::Corner::normals); return RT_OK; }
        const int nIdx = rtl::mesh_layout(c->mesh).nTris * 3, nVerts = rtl::mesh_verts(c->mesh);
        std::vector<uint32_t> idx((size_t)nIdx);
        HIP_TRY(c, hipMemcpy(idx.data(), rtl::mesh_indices(c->mesh), (size_t)nIdx * 4, hipMemcpyDeviceToHost));
        std::string perr;
        int rc = rtl::normal_validate(idx.data(), nIdx, nVerts, perr);
        rtl::NormalPlan plan;
        if (rc == RT_OK) rc = rtl::normal_plan(idx.data(), nIdx, nVerts, plan, perr);
        if (rc != RT_OK) return fail(c, rc, "rt_mesh_normals_enable: %s", perr.c_str());
        std::vector<int32_t> entries;
        rtl::normal_fill(plan, idx.data(), nIdx, entries);
        hipStream_t st = api_stream(c);   // rt_stream()
        const char *err = nullptr;
        // (recorded behind a create that failed as well: corner_enable)
        const int er = with_order_event(c, st, false, false, [&] { rc = rtl::mesh_normals_create(c->mesh, st, plan.sliceFirst.data(), entries.data(), plan.info, &err); return RT_OK; });
        if (er != RT_OK) return er;
        if (rc != RT_OK) return fail(c, rc, "rt_mesh_normals_enable: %s", err ? err : "allocation failed");
        return RT_OK;
    });
}

int rt_mesh_vertex_normals(RtContext *c, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes) return RT_ERR_INVALID;
    *devPtr = nullptr; *bytes = 0;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_vertex_normals: no mesh (rt_mesh_upload first)");
    if (!rtl::mesh_vertex_normals(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_vertex_normals: normals are not enabled (rt_mesh_normals_enable first)");
    *devPtr = const_cast<float4 *>(rtl::mesh_vertex_normals(c->mesh));
    *bytes = (size_t)rtl::mesh_verts(c->mesh) * 16;
    return RT_OK;
}

int rt_mesh_hit_normals(RtContext *c, const RtHit *hits, int n, float *normals) {
    return mesh_hit_query(c, kHitNormals, "rt_mesh_hit_normals", false, hits, nullptr, n, normals, nullptr);
}
int rt_mesh_hit_normals_host(RtContext *c, const RtHit *hits, int n, float *normals) {
    return mesh_hit_query(c, kHitNormals, "rt_mesh_hit_normals_host", true, hits, nullptr, n, normals, nullptr);
}

// ---- per-vertex colours
int rt_mesh_colors_enable(RtContext *c, int on) { return corner_enable(c, kColorsApi, on); }
int rt_mesh_colors(RtContext *c, void **devPtr, size_t *bytes) { return corner_accessor(c, kColorsApi, devPtr, bytes); }
int rt_mesh_set_colors(RtContext *c, const float *rgb3, int first, int count) { return corner_set(c, kColorsApi, rgb3, first, count); }
int rt_mesh_colors_refresh(RtContext *c) { return corner_refresh(c, kColorsApi); }
int rt_mesh_hit_colors(RtContext *c, const RtHit *hits, int n, float *colors) {
    return mesh_hit_query(c, kHitColors, "rt_mesh_hit_colors", false, hits, nullptr, n, colors, nullptr);
}
int rt_mesh_hit_colors_host(RtContext *c, const RtHit *hits, int n, float *colors) {
    return mesh_hit_query(c, kHitColors, "rt_mesh_hit_colors_host", true, hits, nullptr, n, colors, nullptr);
}

// ---- UVs and the albedo texture: beside the UVs' four calls this file owns the texture's upload and the two hit queries
int rt_mesh_uvs_enable(RtContext *c, int on) { return corner_enable(c, kUvsApi, on); }
int rt_mesh_uvs(RtContext *c, void **devPtr, size_t *bytes) { return corner_accessor(c, kUvsApi, devPtr, bytes); }
int rt_mesh_set_uvs(RtContext *c, const float *uv2, int first, int count) { return corner_set(c, kUvsApi, uv2, first, count); }
int rt_mesh_uvs_refresh(RtContext *c) { return corner_refresh(c, kUvsApi); }

int rt_mesh_texture_upload(RtContext *c, const uint8_t *rgba8, int W, int H, int flags) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_texture_upload: no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)");
    const bool release = !rgba8 && W == 0 && H == 0;
    if (!release) {
        if (W < 1 || H < 1 || W > RT_TEX_MAX_SIZE || H > RT_TEX_MAX_SIZE) return fail(c, RT_ERR_INVALID, "rt_mesh_texture_upload: %d x %d texels (1 .. %d each)", W, H, RT_TEX_MAX_SIZE);
        if ((uint32_t)flags & ~rtuv::kAllFlags) return fail(c, RT_ERR_INVALID, "rt_mesh_texture_upload: unknown flag bits 0x%x", (unsigned)flags & ~rtuv::kAllFlags);
        if (!rgba8) return fail(c, RT_ERR_INVALID, "rt_mesh_texture_upload: null texels");
    }
    return guarded(c, "rt_mesh_texture_upload", [&]() -> int {
        (void)hipSetDevice(c->cfg.device);
        HIP_TRY(c, sync_all(c));   // frames and queries in flight read the texels that are about to be replaced or go
        if (release) { rtl::mesh_texture_release(c->mesh); return RT_OK; }
        float table[256];
        if ((uint32_t)flags & rtuv::kSrgb) (void)rt_srgb_table(table);
        else for (int k = 0; k < 256; ++k) table[k] = rtuv::unorm8((uint8_t)k);
        const char *err = nullptr;
        const int rc = rtl::mesh_texture_create(c->mesh, rgba8, W, H, (uint32_t)flags, table, &err);
        return rc == RT_OK ? RT_OK : fail(c, rc, "rt_mesh_texture_upload: %s", err ? err : "allocation failed");
    });
}

int rt_mesh_texture(RtContext *c, void **devPtr, size_t *bytes, int *W, int *H) {
    if (!c || !devPtr || !bytes || !W || !H) return RT_ERR_INVALID;
    *devPtr = nullptr; *bytes = 0; *W = 0; *H = 0;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_texture: no mesh (rt_mesh_upload first)");
    const rtuv::Texture *t = rtl::mesh_texture(c->mesh);
    if (!t) return fail(c, RT_ERR_INVALID, "rt_mesh_texture: no texture (rt_mesh_texture_upload first)");
    *devPtr = const_cast<void *>(t->texels);
    *bytes = (size_t)t->W * (size_t)t->H * 4;
    *W = t->W; *H = t->H;
    return RT_OK;
}

int rt_mesh_hit_uvs(RtContext *c, const RtHit *hits, int n, float *uvs) {
    return mesh_hit_query(c, kHitUvs, "rt_mesh_hit_uvs", false, hits, nullptr, n, uvs, nullptr);
}
int rt_mesh_hit_uvs_host(RtContext *c, const RtHit *hits, int n, float *uvs) {
    return mesh_hit_query(c, kHitUvs, "rt_mesh_hit_uvs_host", true, hits, nullptr, n, uvs, nullptr);
}
int rt_mesh_hit_texels(RtContext *c, const RtHit *hits, int n, float *texels) {
    return mesh_hit_query(c, kHitTexels, "rt_mesh_hit_texels", false, hits, nullptr, n, texels, nullptr);
}
int rt_mesh_hit_texels_host(RtContext *c, const RtHit *hits, int n, float *texels) {
    return mesh_hit_query(c, kHitTexels, "rt_mesh_hit_texels_host", true, hits, nullptr, n, texels, nullptr);
}

// ---- skinning: rt_mesh_skin.hip rewrites the positions; this file validates the tables and orders the writes against every lane
int rt_mesh_skin_upload(RtContext *c, const float *rest, const uint16_t *boneIdx4, const float *weights4, int nBones) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_skin_upload: no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)");
    (void)hipSetDevice(c->cfg.device);
    if (nBones == 0) {
        HIP_TRY(c, sync_all(c));
        rtl::mesh_skin_release(c->mesh);
        return RT_OK;
    }
    if (nBones < 1 || nBones > RT_MAX_MESH_BONES) return fail(c, RT_ERR_INVALID, "rt_mesh_skin_upload: %d bones (1 .. %d)", nBones, RT_MAX_MESH_BONES);
    if (!boneIdx4 || !weights4) return fail(c, RT_ERR_INVALID, "rt_mesh_skin_upload: null %s", !boneIdx4 ? "boneIdx4" : "weights4");
    const size_t n = (size_t)rtl::mesh_verts(c->mesh) * RT_SKIN_INFLUENCES;
    for (size_t k = 0; k < n; ++k) {
        if ((int)boneIdx4[k] >= nBones)
            return fail(c, RT_ERR_INVALID, "rt_mesh_skin_upload: influence %zu of vertex %zu names bone %u of %d", k % RT_SKIN_INFLUENCES, k / RT_SKIN_INFLUENCES, (unsigned)boneIdx4[k], nBones);
        if (!std::isfinite(weights4[k]))
            return fail(c, RT_ERR_INVALID, "rt_mesh_skin_upload: weight %zu of vertex %zu is not finite", k % RT_SKIN_INFLUENCES, k / RT_SKIN_INFLUENCES);
    }
    return guarded(c, "rt_mesh_skin_upload", [&]() -> int {
        HIP_TRY(c, sync_all(c));   // a skin in flight reads the arrays that are replaced; the snapshot reads the positions as they stand
        const char *err = nullptr;
        const int rc = rtl::mesh_skin_create(c->mesh, rest, boneIdx4, weights4, nBones, &err);
        return rc == RT_OK ? RT_OK : fail(c, rc, "rt_mesh_skin_upload: %s", err ? err : "allocation failed");
    });
}

int rt_mesh_bones(RtContext *c, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes) return RT_ERR_INVALID;
    *devPtr = nullptr; *bytes = 0;
    if (!c->mesh || !rtl::mesh_bone_count(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_bones: no skin (rt_mesh_upload and rt_mesh_skin_upload first)");
    *devPtr = rtl::mesh_bones(c->mesh);
    *bytes = (size_t)rtl::mesh_bone_count(c->mesh) * 64;
    return RT_OK;
}

int rt_mesh_rest_positions(RtContext *c, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes) return RT_ERR_INVALID;
    *devPtr = nullptr; *bytes = 0;
    if (!c->mesh || !rtl::mesh_bone_count(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_rest_positions: no skin (rt_mesh_upload and rt_mesh_skin_upload first)");
    *devPtr = rtl::mesh_rest_positions(c->mesh);
    *bytes = (size_t)rtl::mesh_verts(c->mesh) * 12;
    return RT_OK;
}

int rt_mesh_set_bones(RtContext *c, int first, int count, const float *M16s) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh || !rtl::mesh_bone_count(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_set_bones: no skin (rt_mesh_upload and rt_mesh_skin_upload first)");
    const int n = rtl::mesh_bone_count(c->mesh);
    if (first < 0 || count < 0 || first > n || count > n - first) return fail(c, RT_ERR_INVALID, "rt_mesh_set_bones: entries %d .. %d of a table of %d", first, first + count, n);
    if (count == 0) return RT_OK;
    if (!M16s) return fail(c, RT_ERR_INVALID, "rt_mesh_set_bones: null matrices");
    (void)hipSetDevice(c->cfg.device);
    hipStream_t st = api_stream(c);   // rt_stream()
    return between_lanes(c, st, [&]() -> int {   // a skin enqueued on another lane reads the table
        HIP_TRY(c, hipMemcpyAsync(rtl::mesh_bones(c->mesh) + (size_t)first * 16, M16s, (size_t)count * 64, hipMemcpyHostToDevice, st));
        return RT_OK;
    });
}

int rt_mesh_skin(RtContext *c) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_skin: no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)");
    if (!rtl::mesh_bone_count(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_skin: no skin (rt_mesh_skin_upload first; rt_mesh_upload releases the skin)");
    (void)hipSetDevice(c->cfg.device);
    hipStream_t st = api_stream(c);   // rt_stream()
    // a position write: gathers, bone and rest writes and bound raster draws already enqueued on any lane come first, and updates, draws and table
    // writes a lane is given next see the new positions
    return between_lanes(c, st, [&]() -> int {
        if (c->raster && rt_raster_order_after(c->raster, st) != RT_OK) return fail(c, RT_ERR_HIP, "rt_mesh_skin: %s", rt_raster_error(c->raster));
        const char *err = nullptr;
        const int rc = rtl::mesh_skin(c->mesh, st, &err);
        return rc == RT_OK ? RT_OK : fail(c, rc, "rt_mesh_skin: %s", err ? err : "launch failed");
    });
}

// ---- morph targets: rt_morph_pack.cpp checks and packs the targets, rt_mesh_morph.hip blends them; this file orders the writes
int rt_mesh_morph_upload(RtContext *c, const float *base, const int32_t *targetFirst, const uint32_t *vertIdx, const float *deltas, int nTargets) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_morph_upload: no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)");
    (void)hipSetDevice(c->cfg.device);
    if (nTargets == 0) {
        HIP_TRY(c, sync_all(c));
        rtl::mesh_morph_release(c->mesh);
        return RT_OK;
    }
    return guarded(c, "rt_mesh_morph_upload", [&]() -> int {
        const int nVerts = rtl::mesh_verts(c->mesh);
        std::string msg;
        int rc = rtl::morph_validate(nVerts, targetFirst, vertIdx, deltas, nTargets, msg);
        if (rc != RT_OK) return fail(c, rc, "rt_mesh_morph_upload: %s", msg.c_str());
        rtl::MorphPlan plan;
        rc = rtl::morph_plan(nVerts, targetFirst, vertIdx, nTargets, plan, msg);
        if (rc != RT_OK) return fail(c, rc, "rt_mesh_morph_upload: %s", msg.c_str());
        std::vector<rtl::MorphRecord> records;
        rtl::morph_fill(plan, targetFirst, vertIdx, deltas, records);
        HIP_TRY(c, sync_all(c));   // a morph in flight reads the arrays that are replaced; the snapshot reads its source as it stands
        const char *err = nullptr;
        rc = rtl::mesh_morph_create(c->mesh, base, plan.sliceFirst.data(), records.data(), plan.info, &err);
        return rc == RT_OK ? RT_OK : fail(c, rc, "rt_mesh_morph_upload: %s", err ? err : "allocation failed");
    });
}

int rt_mesh_morph_base(RtContext *c, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes) return RT_ERR_INVALID;
    *devPtr = nullptr; *bytes = 0;
    if (!c->mesh || !rtl::mesh_morph_target_count(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_morph_base: no morph (rt_mesh_upload and rt_mesh_morph_upload first)");
    *devPtr = rtl::mesh_morph_base(c->mesh);
    *bytes = (size_t)rtl::mesh_verts(c->mesh) * 12;
    return RT_OK;
}

int rt_mesh_morph_weights(RtContext *c, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes) return RT_ERR_INVALID;
    *devPtr = nullptr; *bytes = 0;
    if (!c->mesh || !rtl::mesh_morph_target_count(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_morph_weights: no morph (rt_mesh_upload and rt_mesh_morph_upload first)");
    *devPtr = rtl::mesh_morph_weights(c->mesh);
    *bytes = (size_t)rtl::mesh_morph_target_count(c->mesh) * 4;
    return RT_OK;
}

int rt_mesh_set_morph_weights(RtContext *c, int first, int count, const float *weights) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh || !rtl::mesh_morph_target_count(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_set_morph_weights: no morph (rt_mesh_upload and rt_mesh_morph_upload first)");
    const int n = rtl::mesh_morph_target_count(c->mesh);
    if (first < 0 || count < 0 || first > n || count > n - first) return fail(c, RT_ERR_INVALID, "rt_mesh_set_morph_weights: entries %d .. %d of a table of %d", first, first + count, n);
    if (count == 0) return RT_OK;
    if (!weights) return fail(c, RT_ERR_INVALID, "rt_mesh_set_morph_weights: null weights");
    (void)hipSetDevice(c->cfg.device);
    hipStream_t st = api_stream(c);   // rt_stream()
    return between_lanes(c, st, [&]() -> int {   // a morph enqueued on another lane reads the table
        HIP_TRY(c, hipMemcpyAsync(rtl::mesh_morph_weights(c->mesh) + first, weights, (size_t)count * 4, hipMemcpyHostToDevice, st));
        return RT_OK;
    });
}

int rt_mesh_morph(RtContext *c, int dst) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_morph: no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)");
    if (!rtl::mesh_morph_target_count(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_morph: no morph (rt_mesh_morph_upload first; rt_mesh_upload releases the morph)");
    if (dst != RT_MORPH_TO_POSITIONS && dst != RT_MORPH_TO_REST) return fail(c, RT_ERR_INVALID, "rt_mesh_morph: destination %d", dst);
    if (dst == RT_MORPH_TO_REST && !rtl::mesh_bone_count(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_morph: no rest array to write (rt_mesh_skin_upload first)");
    (void)hipSetDevice(c->cfg.device);
    hipStream_t st = api_stream(c);   // rt_stream()
    // gathers, skins, weight and base writes already enqueued on any lane come first, and for a position write the bound raster draws as well; skins,
    // updates, draws and table writes a lane is given next see what was written
    return between_lanes(c, st, [&]() -> int {
        if (dst == RT_MORPH_TO_POSITIONS && c->raster && rt_raster_order_after(c->raster, st) != RT_OK) return fail(c, RT_ERR_HIP, "rt_mesh_morph: %s", rt_raster_error(c->raster));
        const char *err = nullptr;
        const int rc = rtl::mesh_morph(c->mesh, st, dst == RT_MORPH_TO_REST, &err);
        return rc == RT_OK ? RT_OK : fail(c, rc, "rt_mesh_morph: %s", err ? err : "launch failed");
    });
}

int rt_mesh_morph_info(RtContext *c, RtMorphInfo *out) {
    if (!c || !out) return RT_ERR_INVALID;
    std::memset(out, 0, sizeof *out);
    if (!c->mesh || !rtl::mesh_morph_target_count(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_morph_info: no morph (rt_mesh_upload and rt_mesh_morph_upload first)");
    *out = rtl::mesh_morph_info(c->mesh);
    return RT_OK;
}

// ---- tree quality
static inline float key2f(uint32_t s) { const uint32_t u = (s & 0x80000000u) ? (s & 0x7fffffffu) : ~s; float f; std::memcpy(&f, &u, 4); return f; }

// Collects what has arrived, without waiting: an arrived slot's integers become a record (rt_bvh_cost's own expressions) and the slot is free again.
static void mesh_quality_harvest(RtContext *c) {
    const rtl::BvhLayout &L = rtl::mesh_layout(c->mesh);
    for (int i = 0; i < rtl::kQualityRing; ++i) {
        RtContext::MeshQSlot &sl = c->meshQSlot[i];
        if (!sl.inFlight || hipEventQuery(rtl::mesh_quality_event(c->mesh, i)) != hipSuccess) continue;
        sl.inFlight = false;
        const rtl::QualityRecord r = *rtl::mesh_quality_record(c->mesh, i);
        RtMeshQuality q = {};
        RtBvhCost &k = q.cost;
        k.nInner = L.nInner; k.nLeaves = (int32_t)L.nLeaves;
        const double A = rtcost::half_area(key2f(r.rootKeys[3]) - key2f(r.rootKeys[0]), key2f(r.rootKeys[4]) - key2f(r.rootKeys[1]), key2f(r.rootKeys[5]) - key2f(r.rootKeys[2]));
        k.rootArea = A;
        if (A == 0.0) k.degenerate = 1;
        else {
            k.rootExp = rtcost::root_exp(A);
            k.innerQ = r.innerQ; k.leafQ = r.leafQ;
            k.inner = rtcost::from_sum(k.innerQ, k.rootExp, A);
            k.leaf = rtcost::from_sum(k.leafQ, k.rootExp, A);
            k.cost = k.inner + k.leaf;
        }
        q.update = sl.update; q.refitsSinceRebuild = sl.refits;
        if (!c->meshQHaveLatest || q.update >= c->meshQLatest.update) { c->meshQLatest = q; c->meshQLatestTree = sl.tree; c->meshQHaveLatest = true; }
        if (sl.refits == 0 && (!c->meshQHaveBaseline || sl.tree >= c->meshQBaselineTree)) { c->meshQBaseline = q; c->meshQBaselineTree = sl.tree; c->meshQHaveBaseline = true; }
    }
}

static int mesh_measure(RtContext *c, const char *who) {
    (void)hipSetDevice(c->cfg.device);
    mesh_quality_harvest(c);
    int slot = -1;
    for (int i = 0; i < rtl::kQualityRing && slot < 0; ++i) if (!c->meshQSlot[i].inFlight) slot = i;
    if (slot < 0) { ++c->meshQSkipped; return RT_OK; }
    const char *err = nullptr;
    const int rc = rtl::mesh_measure(c->mesh, api_stream(c), slot, &err);
    if (rc != RT_OK) return fail(c, rc, "%s: %s", who, err ? err : "launch failed");
    RtContext::MeshQSlot &sl = c->meshQSlot[slot];
    sl.inFlight = true; sl.update = c->meshRebuilds + c->meshRefits; sl.tree = c->meshRebuilds; sl.refits = (int32_t)c->meshRefitsSinceRebuild;
    c->meshQNewest = slot;
    ++c->meshQEnqueued;
    return RT_OK;
}

int rt_mesh_measure(RtContext *c) {
    if (!c) return RT_ERR_INVALID;
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_measure: no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)");
    if (!rtl::mesh_has_tree(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_measure: no tree to measure (rt_mesh_rebuild first)");
    return mesh_measure(c, "rt_mesh_measure");
}

int rt_mesh_quality(RtContext *c, int which, int wait, RtMeshQuality *out) {
    if (!c || !out) return RT_ERR_INVALID;
    std::memset(out, 0, sizeof *out);
    if (which != RT_MESH_QUALITY_LATEST && which != RT_MESH_QUALITY_BASELINE) return fail(c, RT_ERR_INVALID, "rt_mesh_quality: which = %d", which);
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_quality: no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)");
    (void)hipSetDevice(c->cfg.device);
    if (wait && c->meshQNewest >= 0 && c->meshQSlot[c->meshQNewest].inFlight) HIP_TRY(c, hipEventSynchronize(rtl::mesh_quality_event(c->mesh, c->meshQNewest)));
    mesh_quality_harvest(c);
    if (which == RT_MESH_QUALITY_LATEST) {
        if (!c->meshQHaveLatest) return fail(c, RT_ERR_STATE, "rt_mesh_quality: no measurement has arrived yet");
        *out = c->meshQLatest;
    } else {
        if (!c->meshQHaveBaseline || c->meshQBaselineTree != c->meshRebuilds)
            return fail(c, RT_ERR_STATE, "rt_mesh_quality: no measurement of the current tree as its rebuild left it has arrived");
        *out = c->meshQBaseline;
    }
    out->skipped = (int32_t)c->meshQSkipped;
    return RT_OK;
}

int rt_mesh_update(RtContext *c, int mode, const float *M16, float rebuildAbove, int *action) {
    if (!c) return RT_ERR_INVALID;
    if (mode != RT_MESH_UPDATE_SINGLE && mode != RT_MESH_UPDATE_PARTS) return fail(c, RT_ERR_INVALID, "rt_mesh_update: mode = %d", mode);
    if (mode == RT_MESH_UPDATE_PARTS && M16) return fail(c, RT_ERR_INVALID, "rt_mesh_update: RT_MESH_UPDATE_PARTS gathers under the matrix table, M16 must be NULL");
    if (!(rebuildAbove >= 1.0f)) return fail(c, RT_ERR_INVALID, "rt_mesh_update: rebuildAbove = %g (a ratio of costs, at least 1)", (double)rebuildAbove);
    if (!c->mesh) return fail(c, RT_ERR_INVALID, "rt_mesh_update: no mesh (rt_mesh_upload first; rt_upload_bvh releases the mesh)");
    (void)hipSetDevice(c->cfg.device);
    bool rebuild = true;
    if (rtl::mesh_has_tree(c->mesh)) {
        mesh_quality_harvest(c);
        const bool haveBase = c->meshQHaveBaseline && c->meshQBaselineTree == c->meshRebuilds;
        bool baseInFlight = false;
        for (const auto &sl : c->meshQSlot) baseInFlight = baseInFlight || (sl.inFlight && sl.tree == c->meshRebuilds && sl.refits == 0);
        if (haveBase) {
            // a record of the current tree is at least as new as its baseline; one of an older tree cannot be newer
            const RtMeshQuality &latest = (c->meshQHaveLatest && c->meshQLatestTree == c->meshRebuilds) ? c->meshQLatest : c->meshQBaseline;
            if (c->meshQBaseline.cost.degenerate || latest.cost.degenerate) rebuild = false;
            else rebuild = latest.cost.cost > (double)rebuildAbove * c->meshQBaseline.cost.cost;
        } else rebuild = !baseInFlight;
    }
    const int rc = mesh_update(c, M16, !rebuild, mode == RT_MESH_UPDATE_PARTS, "rt_mesh_update");
    if (rc != RT_OK) return rc;
    if (action) *action = rebuild ? RT_MESH_DID_REBUILD : RT_MESH_DID_REFIT;
    return mesh_measure(c, "rt_mesh_update");
}

int rt_mesh_refit_count(RtContext *c, uint64_t *total, uint64_t *sinceRebuild) {
    if (!c || (!total && !sinceRebuild)) return RT_ERR_INVALID;
    if (total) *total = c->mesh ? c->meshRefits : 0;
    if (sinceRebuild) *sinceRebuild = c->mesh ? c->meshRefitsSinceRebuild : 0;
    return RT_OK;
}

int rt_mesh_order_device(RtContext *c, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes) return RT_ERR_INVALID;
    *devPtr = nullptr; *bytes = 0;
    if (!c->mesh || !rtl::mesh_has_tree(c->mesh)) return fail(c, RT_ERR_INVALID, "rt_mesh_order: no tree (rt_mesh_upload and rt_mesh_rebuild first)");
    (void)hipSetDevice(c->cfg.device);
    const int *order = nullptr;
    const int rc = mesh_order_on(c, api_stream(c), "rt_mesh_order", &order);
    if (rc != RT_OK) return rc;
    *devPtr = const_cast<int *>(order);
    *bytes = (size_t)rtl::mesh_layout(c->mesh).nTris * 4;
    return RT_OK;
}

int rt_mesh_hit_parts(RtContext *c, const RtHit *hits, int n, int32_t *parts, int32_t *tris) {
    return mesh_hit_query(c, kHitParts, "rt_mesh_hit_parts", false, hits, nullptr, n, parts, tris);
}
int rt_mesh_hit_parts_host(RtContext *c, const RtHit *hits, int n, int32_t *parts, int32_t *tris) {
    return mesh_hit_query(c, kHitParts, "rt_mesh_hit_parts_host", true, hits, nullptr, n, parts, tris);
}

int rt_mesh_order(RtContext *c, int32_t *order) {
    if (!c || !order) return RT_ERR_INVALID;
    void *d = nullptr;
    size_t bytes = 0;
    const int rc = rt_mesh_order_device(c, &d, &bytes);
    if (rc != RT_OK) return rc;
    hipStream_t st = api_stream(c);
    HIP_TRY(c, hipMemcpyAsync(order, d, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return RT_OK;
}

int rt_get_mesh_info(RtContext *c, RtMeshInfo *out) {
    if (!c || !out) return RT_ERR_INVALID;
    std::memset(out, 0, sizeof *out);
    if (!c->mesh) return RT_OK;
    out->nVerts = rtl::mesh_verts(c->mesh); out->nTris = rtl::mesh_layout(c->mesh).nTris;
    out->rebuilds = c->meshRebuilds; out->allocations = rtl::mesh_allocations(c->mesh); out->hostSyncs = c->meshHostSyncs;
    out->scratchBytes = rtl::mesh_scratch_bytes(c->mesh); out->sceneBytes = rtl::mesh_scene_bytes(c->mesh);
    return RT_OK;
}

}  // extern "C"
