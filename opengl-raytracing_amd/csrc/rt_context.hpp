// rt_context.hpp -- private to the C ABI's translation units (rt_api.hip and rt_api_*.hip): the context, how a call fails, and the
// helpers more than one of them needs.  Everything here is host code and has internal names: the exported rt_* set is include/rt_mi355.h's alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rt_mi355.h"
#include "rt_frame.hpp"
#include "rt_mesh.hpp"
#include "rt_wave.hpp"

#define RT_MAX_LANES 8
struct StageEvent { int stage; hipEvent_t a, b; };

struct RtContext {
    RtDeviceConfig cfg{};
    // Frames in flight: frame f runs on lane f % nLanes (own stream, frame descriptor, ray-queue arenas, COLOR0 buffer), so
    // up to nLanes consecutive frames overlap everywhere except at the temporal resolve.  stream == lanes[0]: every
    // non-frame operation runs there after a sync of all lanes.
    int nLanes = 3;
    bool serialFrames = false;          // RT_LANES=1: a frame starts when its predecessor has finished
    hipStream_t lanes[RT_MAX_LANES] = {};
    hipStream_t stream = nullptr;
    hipStream_t lastStream = nullptr;    // stream of the most recent frame (gather / assemble are ordered behind it)
    hipEvent_t evDone[RT_MAX_LANES] = {};   // the frame on lane i has written its targets
    std::string err;
    // scene
    float4 *dWNodes = nullptr, *dW4 = nullptr, *dTris = nullptr, *dWNodesW = nullptr, *dPairs = nullptr;
    float4 *dQ4 = nullptr, *dLeafBox = nullptr;   // RT_QNODES: quantised any-hit nodes + the leaves' exact boxes
    float4 *dWF = nullptr;           // fused closest-hit records (round 5), null when the tree's boxes are not the unions of their children's
    float4 *dIN4 = nullptr, *dIQ4 = nullptr, *dILeafBox = nullptr;   // ... and the any-hit walk's four-wide records, exact (96 B) and quantised (48 B + the leaves' exact boxes by ordinal)
    float4 *dIN2 = nullptr, *dIPairs = nullptr;   // implicit records (round 5): 48-byte two-child records without references + the pair records in leaf order; null unless every leaf sits at depth implD
    int implD = 0, implR = 0;
    size_t nFused = 0;
    int sceneFlags = 0;              // RT_SCENE_* bits of RtSceneInfo.flags
    int rootRefW = 0;
    void *dHistAll[RT_MAX_LANES] = {};      // tile-parallel + moving camera: every rank's COLOR0 block of the frame a lane rendered
    bool histExchanged[RT_MAX_LANES] = {};
    uchar4 *dEnv = nullptr;
    int envSize = 0;
    int nNodes = 0, nTris = 0, nInner = 0, rootRef = 0, rootRef4 = 0, treeDepth = 0;
    size_t nWide4 = 0, nPairs = 0;   // records in dW4 / dPairs
    size_t nLeafBoxes = 0;           // leaves with an exact box in dLeafBox (quantised any-hit nodes)
    uint32_t leafBoxMagic = 0;       // dLeafBox index of a leaf = (first pair record * magic) >> 32 (0: = first)
    int anyStack = 0;                // stack entries of the any-hit walk (0: from the binary depth)
    float rootMin[3] = {0, 0, 0}, rootMax[3] = {0, 0, 0};
    size_t leafBoxBytes = 0;         // bytes of dLeafBox
    // dynamic mesh: its arrays belong to `mesh`; once a rebuild has installed them the scene pointers above alias them (sceneFromMesh)
    rtl::Mesh *mesh = nullptr;
    bool sceneFromMesh = false;
    float *dRootBox = nullptr;       // sceneFromMesh: node 0's box on the device -- the host does not know it (rootMin / rootMax above are not used then)
    hipEvent_t evMeshLane[RT_MAX_LANES] = {}, evMeshDone = nullptr;   // a rebuild waits for every lane / every lane waits for the rebuild
    hipEvent_t evMeshOrder = nullptr;      // the order array of the current tree has been written, on meshOrderStream
    hipStream_t meshOrderStream = nullptr;
    uint64_t meshRebuilds = 0, meshHostSyncs = 0, meshRefits = 0, meshRefitsSinceRebuild = 0;
    bool meshMotionDirty = false;          // previous pose: an update since the last latch, for rt_render_ray's own frame state
    // tree quality: which result slots of the mesh are in flight and what they measure; the arrived records the policy reads
    struct MeshQSlot { bool inFlight = false; uint64_t update = 0, tree = 0; int32_t refits = 0; } meshQSlot[rtl::kQualityRing];
    RtMeshQuality meshQLatest = {}, meshQBaseline = {};
    bool meshQHaveLatest = false, meshQHaveBaseline = false;
    uint64_t meshQLatestTree = 0, meshQBaselineTree = 0;   // RtMeshInfo.rebuilds when the measured tree was built
    uint64_t meshQSkipped = 0, meshQEnqueued = 0;
    int meshQNewest = -1;                                  // slot of the newest enqueued measurement
    // frame state
    rtd::FrameGeom g{};
    bool sized = false;
    uint2 *dColor[RT_MAX_LANES] = {};   // COLOR0 ring: frame f writes [f % nLanes], reads [(f-1) % nLanes]
    // motion / position / normal are ringed like COLOR0: a gather (or any other reader) of frame f's targets runs on lane f's
    // stream and must not see frame f+1's stores, which run on another stream
    uint32_t *dMotion[RT_MAX_LANES] = {};
    uint2 *dGPos[RT_MAX_LANES] = {}, *dGNrm[RT_MAX_LANES] = {};
    size_t nSlots = 0;
    int frameIndex = 0, writeIdx = 0;     // include/render/accum.h:125-138
    bool haveFrameState = false;
    float prevVP[16];
    rtd::DevFrame *dFrame[RT_MAX_LANES] = {};
    unsigned long long *dCounters = nullptr;
    void *dStaging = nullptr;
    size_t stagingBytes = 0;
    RtWave *wave[RT_MAX_LANES] = {};
    RtArenaPool *arenaPool = nullptr;   // ray-queue arenas shared by the lanes' wavefront pipelines
    RtHybrid *hybrid[RT_MAX_LANES] = {};   // EXTENSION: staged hybrid pipeline, created on first use
    RtRaster *raster = nullptr;            // raster preview (rt_raster.hip): mesh slots + its own buffers, created on first use
    int cus = 256;
    uint32_t debugBuilds = 0;   // RT_BUILD_* bits of the rt_debug_trace kind 2 - 4 launches since the last rt_debug_builds reset
    // rt_trace_rays scratch, allocated on the first query: the query's frame descriptor (uEPS / uINF / scene, written on the stream) and its
    // cursor words.  Queries share it, so a query on another stream than the previous one waits for that one's event first.
    rtd::DevFrame *dQueryFrame = nullptr;
    uint32_t *dQueryHeads = nullptr;
    hipEvent_t queryDone = nullptr;
    hipStream_t queryStream = nullptr;   // stream of the last query (null: none yet)
    int giBounces = 1;   // EXTENSION, rt_set_extension
    int envFilter = 0;   // rt_set_extension: cube-map filter model (0 exact fp32 weights, 1 coordinates rounded to 1/256 texel)
    // tile-parallel exchange owned by the library (rt_api_exchange.hip): RCCL communicator + per-lane gather buffers on the gathering rank
    void *comm = nullptr;                               // ncclComm_t
    void *dGathered[RT_MAX_LANES][4] = {};              // [lane][target]: worldSize blocks, rank-major
    void *dAssembled[RT_MAX_LANES][4] = {};             // [lane][target]: row-major frame of halfs
    int gatheredLane[4] = {-1, -1, -1, -1};             // lane whose frame rt_gather_frame(which) gathered last
    // timing
    bool timing = false;
    std::vector<StageEvent> pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> freeEvents;
    uint64_t gathers = 0, gatherBytes = 0, historyExchanges = 0;   // rt_comm_info
    double stageMs[RT_MAX_STAGES] = {0};
    uint64_t stageLaunches[RT_MAX_STAGES] = {0};
    int timedFrames = 0;
};

namespace rtapi {

inline thread_local std::string g_createError;   // rt_last_error(NULL): what a call without a context refused

inline int fail(RtContext *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_createError = buf;
    return code;
}
// No C++ exception crosses the C ABI: std::bad_alloc etc. from the host-side repacking become status codes.
template <class F> int guarded(RtContext *c, const char *what, F &&body) {
    try { return body(); }
    catch (const std::bad_alloc &) { return fail(c, RT_ERR_IO, "%s: out of host memory", what); }
    catch (...) { return fail(c, RT_ERR_INVALID, "%s: unexpected exception", what); }
}
inline hipError_t sync_all(RtContext *c) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < c->nLanes; ++i)
        if (c->lanes[i]) { hipError_t ei = hipStreamSynchronize(c->lanes[i]); if (e == hipSuccess) e = ei; }
    return e;
}
#define HIP_TRY(c, expr)                                                                                  \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return fail((c), RT_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// rt_stream()'s stream: the one the most recent frame was enqueued on
inline hipStream_t api_stream(const RtContext *c) { return c->lastStream ? c->lastStream : c->stream; }

inline int last_lane(const RtContext *c) { return (c->writeIdx + c->nLanes - 1) % c->nLanes; }   // lane of the frame rendered last
// Target `which` (RT_TARGET_*) of the frame a lane rendered and its channels; null / 0 for an unknown target.
inline void *lane_target(RtContext *c, int lane, int which, int &ch) {
    switch (which) {
        case RT_TARGET_COLOR: ch = 4; return c->dColor[lane];
        case RT_TARGET_MOTION: ch = 2; return c->dMotion[lane];
        case RT_TARGET_GPOS: ch = 4; return c->dGPos[lane];
        case RT_TARGET_GNRM: ch = 4; return c->dGNrm[lane];
        default: ch = 0; return nullptr;
    }
}
inline void *target_ptr(RtContext *c, int which, int &ch) { return lane_target(c, last_lane(c), which, ch); }

// rt_api.hip: the frame geometry of a w x h framebuffer on rank `rank` of `world` (rt_resize), for a batch of one ...
rtd::FrameGeom make_frame_geom(int w, int h, int rank, int world);
// ... and k_frame_root_box on `st`: a scene a device rebuild installed has its root box on the device only, the descriptor at `fr` takes it from there
void launch_frame_root_box(hipStream_t st, rtd::DevFrame *fr);

// The per-lane tallies of the wavefront pipelines as one sum: fn is rt_wave_traced or one of its kin (rt_wave.hpp), v the K words it hands out.
template <int K, class F> int sum_over_lanes(RtContext *c, const char *what, F fn, int reset, unsigned long long (&v)[K]) {
    for (int k = 0; k < K; ++k) v[k] = 0;
    for (int i = 0; i < c->nLanes; ++i) {
        unsigned long long t[K];
        const int rc = fn(c->wave[i], c->lanes[i], t, reset != 0);
        if (rc != RT_OK) return fail(c, rc, "%s: %s", what, rt_wave_error(c->wave[i]));
        for (int k = 0; k < K; ++k) v[k] += t[k];
    }
    return RT_OK;
}

inline rtd::DevScene make_dev_scene(const RtContext *c) {
    rtd::DevScene s;
    s.wnodes = c->dWNodes;
    s.w4 = c->dW4;
    s.q4 = c->dQ4;
    s.leafBox = c->dLeafBox;
    s.leafBoxMagic = c->leafBoxMagic;
    s.wnodesW = c->dWNodesW;
    s.wF = c->dWF;
    s.iN2 = c->dIN2; s.iPairs = c->dIPairs; s.implD = c->implD; s.implR = c->implR;
    s.iN4 = c->dIN4; s.iQ4 = c->dIQ4; s.iLeafBox = c->dILeafBox;
    s.pairs = c->dPairs;
    s.rootRefW = c->rootRefW;
    s.tris = c->dTris;
    s.env = c->dEnv;
    s.envSize = c->envSize;
    s.envFilter = c->envFilter;
    s.rootRef = c->rootRef;
    s.rootRef4 = c->rootRef4;
    s.hasBVH = (c->nNodes > 0 && c->nTris > 0) ? 1 : 0;
    s.anyStack = c->anyStack;
    std::memcpy(s.rootMin, c->rootMin, 12);
    std::memcpy(s.rootMax, c->rootMax, 12);
    s.rootBox = c->sceneFromMesh ? c->dRootBox : nullptr;
    return s;
}

// The one list of what makes up the BVH scene: afterwards the context describes the empty scene.  owned: the arrays are the context's and are freed
// (false: they alias the dynamic mesh's and are only forgotten).  Callers have synchronised.
inline void clear_scene(RtContext *c, bool owned) {
    float4 **arrays[] = {&c->dWNodes, &c->dWNodesW, &c->dW4, &c->dQ4, &c->dLeafBox, &c->dWF, &c->dIN2, &c->dIPairs, &c->dIN4, &c->dIQ4, &c->dILeafBox, &c->dPairs, &c->dTris};
    for (float4 **p : arrays) { if (owned && *p) (void)hipFree(*p); *p = nullptr; }
    c->nNodes = c->nTris = c->nInner = c->treeDepth = 0;
    c->nWide4 = c->nPairs = c->nFused = c->nLeafBoxes = c->leafBoxBytes = 0;
    c->rootRef = c->rootRefW = c->rootRef4 = c->anyStack = 0;
    c->implD = c->implR = 0;
    c->leafBoxMagic = 0;
    c->sceneFlags = 0;
    for (int a = 0; a < 3; ++a) c->rootMin[a] = c->rootMax[a] = 0.0f;
}

// Lets go of the dynamic mesh; a scene its rebuild installed goes with it (the scene pointers alias the mesh's arrays).  Callers have synchronised.
inline void release_mesh(RtContext *c) {
    if (c->sceneFromMesh) {
        clear_scene(c, false);
        c->sceneFromMesh = false;
        c->dRootBox = nullptr;
    }
    rtl::mesh_destroy(c->mesh);
    c->mesh = nullptr;
    c->meshMotionDirty = false;
    for (int i = 0; i < RT_MAX_LANES; ++i) { if (c->evMeshLane[i]) (void)hipEventDestroy(c->evMeshLane[i]); c->evMeshLane[i] = nullptr; }
    if (c->evMeshDone) (void)hipEventDestroy(c->evMeshDone);
    c->evMeshDone = nullptr;
    if (c->evMeshOrder) (void)hipEventDestroy(c->evMeshOrder);
    c->evMeshOrder = nullptr; c->meshOrderStream = nullptr;
}

inline int ensure_staging(RtContext *c, size_t bytes) {
    if (c->stagingBytes >= bytes) return RT_OK;
    if (c->dStaging) (void)hipFree(c->dStaging);
    c->dStaging = nullptr; c->stagingBytes = 0;
    HIP_TRY(c, hipMalloc(&c->dStaging, bytes));
    c->stagingBytes = bytes;
    return RT_OK;
}

// ---- host arrays through the context's staging buffer: the one protocol of every *_host entry point.
// A segment is one array of the call: `bytes` of it lie at a 16-byte-aligned offset of the buffer, in the order given (bytes == 0: the array is not
// part of this call and its device address is null).  Inputs are copied in from `host`; outputs are copied out to it, unless it is null -- the
// device entry still gets the room.
struct StageSeg { const void *host; size_t bytes; bool out; bool in = false; };   // in: an output the device writes in part -- copied in first, so the rest survives

// sync_all and ensure_staging (the buffer may be replaced: nothing may be in flight), copies in on rt_stream()'s stream, body(device addresses) -- the
// device entry point --, copies out, one wait.  A refused body leaves nothing in flight either.
template <size_t K, class F> int staged(RtContext *c, const char *what, const StageSeg (&segs)[K], F &&body) {
    return guarded(c, what, [&]() -> int {
        (void)hipSetDevice(c->cfg.device);
        size_t off[K], total = 0;
        for (size_t k = 0; k < K; ++k) { off[k] = total; total += (segs[k].bytes + 15) / 16 * 16; }
        HIP_TRY(c, sync_all(c));
        const int sr = ensure_staging(c, total);
        if (sr != RT_OK) return sr;
        char *base = (char *)c->dStaging;
        hipStream_t st = api_stream(c);
        void *dev[K];
        for (size_t k = 0; k < K; ++k) {
            dev[k] = segs[k].bytes ? base + off[k] : nullptr;
            if (segs[k].bytes && (!segs[k].out || segs[k].in)) HIP_TRY(c, hipMemcpyAsync(dev[k], segs[k].host, segs[k].bytes, hipMemcpyHostToDevice, st));
        }
        const int qr = body(dev);
        if (qr != RT_OK) { (void)sync_all(c); return qr; }
        for (size_t k = 0; k < K; ++k)
            if (segs[k].bytes && segs[k].out && segs[k].host) HIP_TRY(c, hipMemcpyAsync(const_cast<void *>(segs[k].host), dev[k], segs[k].bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        return RT_OK;
    });
}

}  // namespace rtapi
