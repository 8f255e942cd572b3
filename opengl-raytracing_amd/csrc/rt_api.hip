// rt_api.hip -- C ABI of librt_mi355.so (include/rt_mi355.h): context, uploads, frame loop, readback, present, raster wrappers; the rest is in rt_api_*.hip.
//
// The context owns one HIP stream and all device memory.  There is no CPU rendering path: without
// a usable HIP device rt_create fails with RT_ERR_NO_DEVICE and nothing else can be called.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "rt_context.hpp"
#include "rt_scene_pack.hpp"

using namespace rtd;
using namespace rtapi;

constexpr int kDefaultArenas = 2;   // ray-queue arenas shared by the frame lanes (rt_wave.hpp RtArenaPool; measured in profiles/r04_experiments.txt)

static const char *kStageNames[RT_MAX_STAGES] = {"mega",     "primary", "trace_primary",   "post_primary", "gen_direct", "trace_shadow",
                                                 "trace_gi", "gen_gi",  "resolve",         "combine",      "assemble",   "present",
                                                 "gather", "trace_ao"};   // gather: the whole of rt_gather_frame on its stream (copy / send / recv / un-tiling; "assemble" lies inside it)

// ------------------------------------------------------------------------------------------------
namespace {

__global__ void k_untile(const void *src, void *dst, FrameGeom g, int channels, int toF32) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.W * g.H) return;
    int x = i % g.W, y = i / g.W;
    int s = slot_of_pixel(g, x, y);
    const uint16_t *in = (const uint16_t *)src + (size_t)(s < 0 ? 0 : s) * channels;
    for (int c = 0; c < channels; ++c) {
        uint16_t h = (s < 0) ? (uint16_t)0 : in[c];
        if (toF32) ((float *)dst)[(size_t)i * channels + c] = f16_bits_to_f32(h);
        else ((uint16_t *)dst)[(size_t)i * channels + c] = h;
    }
}

// Row-major frame of halfs -> this rank's tile-major slots (inverse of k_untile).
__global__ void k_tile(const void *src, void *dst, FrameGeom g, int channels) {
    int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= g.nLocalTiles * 256) return;
    int x, y;
    if (!pixel_of_slot(g, slot >> 8, slot & 255, x, y)) return;
    const uint16_t *in = (const uint16_t *)src + ((size_t)y * g.W + x) * channels;
    uint16_t *out = (uint16_t *)dst + (size_t)slot * channels;
    for (int c = 0; c < channels; ++c) out[c] = in[c];
}

// A scene a device rebuild installed: the frame descriptor the host copied carries no root box; take it from the device.
__global__ void k_frame_root_box(DevFrame *fr) {
    if (threadIdx.x == 0) scene_take_root_box(fr->sc);
}

void free_targets(RtContext *c) {
    for (int i = 0; i < RT_MAX_LANES; ++i) {
        for (void *p : {(void *)c->dColor[i], c->dHistAll[i], (void *)c->dMotion[i], (void *)c->dGPos[i], (void *)c->dGNrm[i]}) if (p) (void)hipFree(p);
        c->dColor[i] = c->dGPos[i] = c->dGNrm[i] = nullptr; c->dMotion[i] = nullptr; c->dHistAll[i] = nullptr; c->histExchanged[i] = false;
        for (int w = 0; w < 4; ++w) {
            if (c->dGathered[i][w]) (void)hipFree(c->dGathered[i][w]);
            if (c->dAssembled[i][w]) (void)hipFree(c->dAssembled[i][w]);
            c->dGathered[i][w] = c->dAssembled[i][w] = nullptr;
        }
    }
    for (int w = 0; w < 4; ++w) c->gatheredLane[w] = -1;
    c->sized = false;
}

// One scene array to the device (an empty one stays null)
template <class T> int upload(RtContext *c, float4 **dst, const std::vector<T> &v) {
    if (v.empty()) return RT_OK;
    HIP_TRY(c, hipMalloc(dst, v.size() * sizeof(T)));
    HIP_TRY(c, hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return RT_OK;
}

// A read-back through the context's staging buffer: nothing in flight, the buffer of `bytes`, launch() into it on c->stream, the copy out to dst, one wait
template <class F> int read_back_via_staging(RtContext *c, size_t bytes, void *dst, F &&launch) {
    HIP_TRY(c, sync_all(c));
    int rc = ensure_staging(c, bytes);
    if (rc == RT_OK) rc = launch();
    if (rc != RT_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(dst, c->dStaging, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_all(c));
    return RT_OK;
}

// Stage "present" into the staging buffer and out to dst; blockSlots: launch_present's, the block size of gathered targets (0: this context's own)
int present_to(RtContext *c, const RtPresentParams &p, const void *color, const void *motion, const void *gpos, const void *gnrm, int blockSlots, uint8_t *dst) {
    return read_back_via_staging(c, (size_t)c->g.W * c->g.H * 4, dst, [&]() -> int {
        rt_stage_begin(c, 11);
        HIP_TRY(c, rtl::launch_present(c->stream, c->g, (const uint2 *)color, (const uint32_t *)motion, (const uint2 *)gpos, (const uint2 *)gnrm, p,
                                       (uint32_t *)c->dStaging, blockSlots));
        rt_stage_end(c, 11, 1);
        return RT_OK;
    });
}

// The raster preview's wrappers: body(the rasteriser, created first if `create` and absent) and, where it refuses, its error as the context's
template <class F> int with_raster(RtContext *c, bool create, F &&body) {
    (void)hipSetDevice(c->cfg.device);
    if (create && !c->raster) c->raster = rt_raster_create();
    const int rc = body(c->raster);
    return rc == RT_OK ? RT_OK : fail(c, rc, "%s", rt_raster_error(c->raster));
}

}  // namespace

FrameGeom rtapi::make_frame_geom(int w, int h, int rank, int world) {
    FrameGeom g;
    g.W = w; g.H = h;
    g.tilesX = (w + RT_TILE_DIM - 1) / RT_TILE_DIM;
    g.tilesY = (h + RT_TILE_DIM - 1) / RT_TILE_DIM;
    g.nTiles = g.tilesX * g.tilesY;
    g.rank = rank; g.world = world;
    g.nLocalTiles = (g.nTiles - g.rank + g.world - 1) / g.world;
    if (g.nLocalTiles < 0) g.nLocalTiles = 0;
    g.batch = 1;
    frame_geom_set_reciprocals(g);
    return g;
}
void rtapi::launch_frame_root_box(hipStream_t st, DevFrame *fr) { hipLaunchKernelGGL(k_frame_root_box, dim3(1), dim3(64), 0, st, fr); }

// ------------------------------------------------------------------------------------------------
// stage timing helpers (used by rt_wave.hip through RtStageTimer)
void rt_stage_begin(RtContext *c, int stage, hipStream_t on) {
    if (!c->timing) return;
    StageEvent ev;
    ev.stage = stage;
    if (!c->freeEvents.empty()) { ev.a = c->freeEvents.back().first; ev.b = c->freeEvents.back().second; c->freeEvents.pop_back(); }
    else { (void)hipEventCreate(&ev.a); (void)hipEventCreate(&ev.b); }
    (void)hipEventRecord(ev.a, on ? on : c->stream);
    c->pending.push_back(ev);
}
void rt_stage_end(RtContext *c, int stage, int launches, hipStream_t on) {
    if (!c->timing) return;
    for (size_t i = c->pending.size(); i-- > 0;)
        if (c->pending[i].stage == stage) { (void)hipEventRecord(c->pending[i].b, on ? on : c->stream); break; }
    c->stageLaunches[stage] += (uint64_t)launches;
}
// Long timed runs: fold the events that have completed into the totals so that the pending list stays short (no host sync).
static void harvest_stage_events(RtContext *c) {
    if (c->pending.size() < 1024) return;
    size_t done = 0;
    while (done < c->pending.size() && hipEventQuery(c->pending[done].b) == hipSuccess) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->pending[done].a, c->pending[done].b) == hipSuccess) c->stageMs[c->pending[done].stage] += ms;
        c->freeEvents.emplace_back(c->pending[done].a, c->pending[done].b);
        ++done;
    }
    c->pending.erase(c->pending.begin(), c->pending.begin() + (std::ptrdiff_t)done);
}
static void resolve_stage_events(RtContext *c) {
    (void)sync_all(c);
    for (auto &ev : c->pending) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) c->stageMs[ev.stage] += ms;
        c->freeEvents.emplace_back(ev.a, ev.b);
    }
    c->pending.clear();
}

extern "C" {

const char *rt_stage_name(int stage) { return (stage >= 0 && stage < RT_MAX_STAGES) ? kStageNames[stage] : ""; }

const char *rt_last_error(const RtContext *ctx) { return ctx ? ctx->err.c_str() : g_createError.c_str(); }

int rt_create(const RtDeviceConfig *cfg, RtContext **out) {
    if (!cfg || !out) return fail(nullptr, RT_ERR_INVALID, "rt_create: null argument");
    *out = nullptr;
    if (cfg->worldSize < 1 || cfg->rank < 0 || cfg->rank >= cfg->worldSize) return fail(nullptr, RT_ERR_INVALID, "rt_create: bad rank/worldSize");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, RT_ERR_NO_DEVICE, "rt_create: no HIP device (%s); this library has no CPU path", hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, RT_ERR_INVALID, "rt_create: device %d of %d", cfg->device, ndev);
    e = hipSetDevice(cfg->device);
    if (e != hipSuccess) return fail(nullptr, RT_ERR_NO_DEVICE, "hipSetDevice: %s", hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, cfg->device);
    if (e != hipSuccess) return fail(nullptr, RT_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, RT_ERR_UNSUPPORTED, "rt_create: device is %s, this library carries gfx950 code only", prop.gcnArchName);
    RtContext *c = new RtContext();
    c->cfg = *cfg;
    // measured on MI355X (1080p / 4 spp): whole frame on one GPU 3.0 / 2.48 / 2.44 / 2.58 ms with 1 / 2 / 3 / 4 lanes; one rank of
    // eight (1/8 of the tiles, latency-bound stages) 0.92 / 0.64 / 0.56 / 0.51 ms
    // round 3, batches of eight frames with 75 % persistent grids: 1.76 / 1.75 ms per frame with 3 / 4 lanes
    c->nLanes = 4;
    if (const char *e = getenv("RT_LANES")) c->nLanes = std::max(1, std::min(RT_MAX_LANES, atoi(e)));
    // RT_LANES=1 = one frame (launch set) in flight.  The COLOR0 ring still needs two buffers -- with one, a moving frame's reprojection would read
    // history texels its own resolve is overwriting (rt_taa.glsl:128 reads the previous frame at arbitrary pixels) -- so it is two lanes whose
    // frames wait for their predecessor from the first kernel on.
    if (c->nLanes == 1) { c->nLanes = 2; c->serialFrames = true; }
    bool ok = hipMalloc(&c->dCounters, 16 * sizeof(unsigned long long)) == hipSuccess;
    // EXPERIMENT RT_CU_SPLIT=k (rt_wave.hip): the lanes' own streams -- the traversal launches -- keep 8 - k eighths of the CUs
    uint32_t cuMask[8];
    bool masked = false;
    if (const char *e = getenv("RT_CU_SPLIT")) {
        const int k = std::max(1, std::min(7, atoi(e)));
        for (int i = 0; i < 8; ++i) { uint32_t m = 0; for (int b = 0; b < 32; ++b) if (((i * 32 + b) & 7) >= k) m |= 1u << b; cuMask[i] = m; }
        masked = true;
    }
    for (int i = 0; ok && i < c->nLanes; ++i)
        ok = (masked ? hipExtStreamCreateWithCUMask(&c->lanes[i], 8, cuMask) : hipStreamCreateWithFlags(&c->lanes[i], hipStreamNonBlocking)) == hipSuccess &&
             hipMalloc(&c->dFrame[i], sizeof(DevFrame)) == hipSuccess && hipEventCreateWithFlags(&c->evDone[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        rt_destroy(c);
        return fail(nullptr, RT_ERR_HIP, "rt_create: stream/alloc failed");
    }
    c->stream = c->lanes[0];
    (void)hipMemset(c->dCounters, 0, 16 * sizeof(unsigned long long));
    c->cus = prop.multiProcessorCount;
    // ray-queue arenas: RT_ARENAS of them shared by the lanes (default below; = lanes: one each, as in rounds 1-3)
    int arenas = std::min(c->nLanes, kDefaultArenas);
    if (const char *e = getenv("RT_ARENAS")) arenas = std::max(1, std::min(atoi(e), c->nLanes));
    c->arenaPool = rt_arena_pool_create(arenas);
    for (int i = 0; i < c->nLanes; ++i) c->wave[i] = rt_wave_create(prop.multiProcessorCount, c->arenaPool, i);
    c->lastStream = c->stream;
    int rc = rt_upload_env(c, nullptr, 0, 0);   // dummy cube map like Application::initState (application.cpp:281)
    if (rc != RT_OK) { g_createError = c->err; rt_destroy(c); return rc; }
    *out = c;
    return RT_OK;
}

void rt_destroy(RtContext *c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    (void)sync_all(c);
    (void)rt_comm_destroy(c);
    release_mesh(c);
    free_targets(c);
    for (int i = 0; i < RT_MAX_LANES; ++i) { if (c->hybrid[i]) rt_hybrid_destroy(c->hybrid[i]); if (c->wave[i]) rt_wave_destroy(c->wave[i]); if (c->dFrame[i]) (void)hipFree(c->dFrame[i]); if (c->evDone[i]) (void)hipEventDestroy(c->evDone[i]); }
    rt_raster_destroy(c->raster);
    if (c->dQueryFrame) (void)hipFree(c->dQueryFrame);
    if (c->dQueryHeads) (void)hipFree(c->dQueryHeads);
    if (c->queryDone) (void)hipEventDestroy(c->queryDone);
    rt_arena_pool_destroy(c->arenaPool);
    for (int i = 0; i < RT_MAX_LANES; ++i) if (c->lanes[i]) (void)hipStreamDestroy(c->lanes[i]);   // c->stream is lanes[0]
    clear_scene(c, true);
    if (c->dEnv) (void)hipFree(c->dEnv);
    if (c->dCounters) (void)hipFree(c->dCounters);
    if (c->dStaging) (void)hipFree(c->dStaging);
    for (auto &ev : c->pending) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    for (auto &p : c->freeEvents) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    delete c;
}

// The record forms are packed on the host (rt_scene_pack.cpp); this uploads them and, after the last upload has succeeded, commits the
// context's fields in one block.  A failed upload leaves the empty scene behind.
int rt_upload_bvh(RtContext *c, const float *nodes12, int nNodes, const float *tris12, int nTris) {
    if (!c) return RT_ERR_INVALID;
    if (nNodes < 0 || nTris < 0 || (nNodes > 0 && !nodes12) || (nTris > 0 && !tris12)) return fail(c, RT_ERR_INVALID, "rt_upload_bvh: bad arguments");
    return guarded(c, "rt_upload_bvh", [&]() -> int {
        (void)hipSetDevice(c->cfg.device);
        HIP_TRY(c, sync_all(c));
        release_mesh(c);   // an upload takes the scene over from the dynamic mesh
        clear_scene(c, true);
        for (int i = 0; i < RT_MAX_LANES; ++i) { rt_wave_forget_share(c->wave[i]); rt_wave_set_probe_tree(c->wave[i], true); }   // a new scene: its share of bounce hits is not known
        if (nNodes == 0 || nTris == 0) return RT_OK;
        rtl::PackedScene s;
        std::string err;
        int rc = rtl::pack_scene(nodes12, nNodes, tris12, nTris, rtl::pack_options_from_env(), s, err);
        if (rc != RT_OK) return fail(c, rc, "%s", err.c_str());
        auto up = [&](float4 **dst, const auto &v) { if (rc == RT_OK) rc = upload(c, dst, v); };
        // (the optional arrays first, then nodes, pairs and triangles: the order of allocation the upload has always had)
        up(&c->dQ4, s.q4); up(&c->dLeafBox, s.leafBox);
        up(&c->dIN2, s.iN2); up(&c->dIPairs, s.iPairs); up(&c->dIN4, s.iN4); up(&c->dIQ4, s.iQ4); up(&c->dILeafBox, s.iLeafBox);
        up(&c->dWF, s.wF);
        up(&c->dWNodes, s.wn); up(&c->dW4, s.w4); up(&c->dWNodesW, s.wnW); up(&c->dPairs, s.pairs);
        if (rc == RT_OK) rc = [&]() -> int {
            // 8 triangles of zero padding: the traversal kernels load triangle records in groups without a bounds branch
            HIP_TRY(c, hipMalloc(&c->dTris, (size_t)(nTris + 8) * 12 * sizeof(float)));
            HIP_TRY(c, hipMemset(c->dTris, 0, (size_t)(nTris + 8) * 12 * sizeof(float)));
            HIP_TRY(c, hipMemcpy(c->dTris, tris12, (size_t)nTris * 12 * sizeof(float), hipMemcpyHostToDevice));
            return RT_OK;
        }();
        if (rc != RT_OK) { clear_scene(c, true); return rc; }
        c->nNodes = nNodes; c->nTris = nTris; c->nInner = s.nInner; c->treeDepth = s.depth;
        c->nWide4 = s.w4.size() / 32; c->nPairs = s.pairs.size() / 20 - 8; c->nFused = s.wF.size() / 32;
        c->rootRef = s.rootRef; c->rootRefW = s.rootRefW; c->rootRef4 = s.rootRef4; c->anyStack = s.anyStack;
        c->leafBoxMagic = s.leafBoxMagic; c->nLeafBoxes = s.nLeafBoxes; c->leafBoxBytes = s.leafBox.size() * 4;
        c->implD = s.implD; c->implR = s.implR;
        c->sceneFlags = s.flags;
        std::memcpy(c->rootMin, s.rootMin, 12);
        std::memcpy(c->rootMax, s.rootMax, 12);
        if (!s.collapsed4) for (int i = 0; i < RT_MAX_LANES; ++i) rt_wave_set_probe_tree(c->wave[i], false);
        return RT_OK;
    });
}

int rt_build_bvh_gpu(RtContext *c, const float *tris9, int nTris, float *nodes12, float *tris12) {
    if (!c) return RT_ERR_INVALID;
    const char *err = nullptr;
    const int rc = rtl::build_bvh_gpu(c->cfg.device, tris9, nTris, nodes12, tris12, &err);
    if (rc < 0) return fail(c, rc, "rt_build_bvh_gpu: %s", err ? err : "bad arguments");
    return rc;
}

int rt_upload_env(RtContext *c, const uint8_t *faces, int faceSize, int channels) {
    if (!c) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    static const uint8_t dummy[6 * 4] = {128, 128, 255, 255, 128, 128, 255, 255, 128, 128, 255, 255,
                                         128, 128, 255, 255, 128, 128, 255, 255, 128, 128, 255, 255};   // cubemap.cpp:13
    if (!faces) { faces = dummy; faceSize = 1; channels = 4; }
    if (faceSize <= 0 || (channels != 3 && channels != 4)) return fail(c, RT_ERR_INVALID, "rt_upload_env: faceSize=%d channels=%d", faceSize, channels);
    return guarded(c, "rt_upload_env", [&]() -> int {
    const size_t texels = (size_t)6 * faceSize * faceSize;
    std::vector<uint8_t> rgba(texels * 4);
    for (size_t i = 0; i < texels; ++i) {
        rgba[i * 4 + 0] = faces[i * channels + 0];
        rgba[i * 4 + 1] = faces[i * channels + 1];
        rgba[i * 4 + 2] = faces[i * channels + 2];
        rgba[i * 4 + 3] = (channels == 4) ? faces[i * channels + 3] : (uint8_t)255;
    }
    HIP_TRY(c, sync_all(c));
    if (c->dEnv) (void)hipFree(c->dEnv);
    c->dEnv = nullptr;
    HIP_TRY(c, hipMalloc(&c->dEnv, texels * 4));
    HIP_TRY(c, hipMemcpy(c->dEnv, rgba.data(), texels * 4, hipMemcpyHostToDevice));
    c->envSize = faceSize;
    return RT_OK;
    });
}

int rt_resize(RtContext *c, int w, int h) {
    if (!c) return RT_ERR_INVALID;
    if (w <= 0 || h <= 0) return fail(c, RT_ERR_INVALID, "rt_resize: %dx%d", w, h);
    (void)hipSetDevice(c->cfg.device);
    HIP_TRY(c, sync_all(c));
    free_targets(c);
    const FrameGeom g = make_frame_geom(w, h, c->cfg.rank, c->cfg.worldSize);
    c->g = g;
    // every rank allocates the padded size so gather blocks are equal
    const size_t maxLocal = (size_t)(g.nTiles + g.world - 1) / g.world;
    c->nSlots = std::max<size_t>(maxLocal, 1) * RT_TILE_PIXELS;
    for (int i = 0; i < c->nLanes; ++i) HIP_TRY(c, hipMalloc(&c->dColor[i], c->nSlots * 8));
    for (int i = 0; i < c->nLanes; ++i) {
        HIP_TRY(c, hipMalloc(&c->dMotion[i], c->nSlots * 4));
        HIP_TRY(c, hipMalloc(&c->dGPos[i], c->nSlots * 8));
        HIP_TRY(c, hipMalloc(&c->dGNrm[i], c->nSlots * 8));
    }
    c->sized = true;
    c->haveFrameState = false;
    for (int i = 0; i < RT_MAX_LANES; ++i) rt_wave_forget_share(c->wave[i]);   // the share of bounce hits belongs to the old frame
    return rt_reset_accum(c);
}

int rt_reset_accum(RtContext *c) {
    if (!c) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_reset_accum before rt_resize");
    (void)hipSetDevice(c->cfg.device);
    HIP_TRY(c, sync_all(c));
    c->frameIndex = 0;
    c->writeIdx = 0;
    for (int i = 0; i < RT_MAX_LANES; ++i) c->histExchanged[i] = false;
    for (int i = 0; i < c->nLanes; ++i) HIP_TRY(c, hipMemsetAsync(c->dColor[i], 0, c->nSlots * 8, c->stream));
    for (int i = 0; i < c->nLanes; ++i) {
        HIP_TRY(c, hipMemsetAsync(c->dMotion[i], 0, c->nSlots * 4, c->stream));
        HIP_TRY(c, hipMemsetAsync(c->dGPos[i], 0, c->nSlots * 8, c->stream));
        HIP_TRY(c, hipMemsetAsync(c->dGNrm[i], 0, c->nSlots * 8, c->stream));
    }
    for (int w = 0; w < 4; ++w) c->gatheredLane[w] = -1;
    return RT_OK;
}

int rt_frame_index(const RtContext *c) { return c ? c->frameIndex : RT_ERR_INVALID; }

// One set of launches for `batch` consecutive frames (batch == 1: the plain frame).  jitterK: uJitter of the batch's frames.
static int render_frames_impl(RtContext *c, const RtUniforms *uIn, int batch, const float (*jitterK)[2]) {
    if (!c || !uIn) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_render_frame before rt_resize");
    (void)hipSetDevice(c->cfg.device);
    if (c->timing) harvest_stage_events(c);
    DevFrame fr;
    fr.u = *uIn;
    fr.u.frameIndex = c->frameIndex;
    if ((int)fr.u.resolution[0] != c->g.W || (int)fr.u.resolution[1] != c->g.H)
        return fail(c, RT_ERR_INVALID, "rt_render_frame: uResolution %gx%g != framebuffer %dx%d", fr.u.resolution[0], fr.u.resolution[1], c->g.W, c->g.H);
    if ((fr.u.useBVH == 1 || fr.u.useBVH == RT_SCENE_HYBRID) && fr.u.nodeCount > 0 && fr.u.triCount > 0 && (c->nNodes == 0 || fr.u.nodeCount > c->nNodes || fr.u.triCount > c->nTris))
        return fail(c, RT_ERR_STATE, "rt_render_frame: uniforms name %d nodes / %d tris, uploaded %d / %d", fr.u.nodeCount, fr.u.triCount, c->nNodes, c->nTris);
    if (fr.u.useEnvMap == 1 && !c->dEnv) return fail(c, RT_ERR_STATE, "rt_render_frame: uUseEnvMap without an environment");
    // Lane = frame index mod nLanes = index of the COLOR0 buffer this frame writes: consecutive frames rotate over the lanes'
    // streams and overlap everywhere except at the temporal resolve (the only read of the previous frame), and every later
    // reader of a COLOR0 buffer (gather, assemble) is stream-ordered before the next writer of the same buffer.
    const int lane = c->writeIdx, prevLane = last_lane(c);
    const bool needAll = fr.u.cameraMoved == 1 && c->g.world > 1 && fr.u.enableTAA == 1 && c->frameIndex > 0;
    if (needAll && !(c->dHistAll[prevLane] && c->histExchanged[prevLane]))
        return fail(c, RT_ERR_STATE, "rt_render_frame: cameraMoved on a tile-parallel context: reprojection reads other ranks' history -- all-gather the "
                                     "previous frame's COLOR0 blocks into rt_history_exchange_buffer() and call rt_history_exchanged() first");
    fr.sc = make_dev_scene(c);
    if (!(fr.u.nodeCount > 0 && fr.u.triCount > 0)) fr.sc.hasBVH = 0;
    fr.g = c->g;
    fr.g.batch = batch;
    frame_geom_set_reciprocals(fr.g);   // (the largest local tile index grows with the batch)
    for (int k = 0; k < RT_MAX_BATCH; ++k) {   // cpOffset's ld2(uFrameIndex) of the batch's frames: the device's own function, evaluated here once per frame
        const int fi = c->frameIndex + (k < batch ? k : 0);
        fr.ld2K[k][0] = halton(fi + 1, 2); fr.ld2K[k][1] = halton(fi + 1, 3);
    }
    for (int k = 0; k < RT_MAX_BATCH; ++k) { fr.jitterK[k][0] = jitterK ? jitterK[k < batch ? k : 0][0] : fr.u.jitter[0]; fr.jitterK[k][1] = jitterK ? jitterK[k < batch ? k : 0][1] : fr.u.jitter[1]; }
    fr.giBounces = c->giBounces;
    // object motion: primary hits of the dynamic mesh's own scene; the hybrid scene keeps the reference's motion
    fr.prevTris = (c->mesh && c->sceneFromMesh && fr.u.useBVH == 1) ? rtl::mesh_prev_tris(c->mesh) : nullptr;
    // smooth normals: mesh hits of the dynamic mesh's own scene; the hybrid scene keeps the face normal
    fr.nrmRows = (c->mesh && c->sceneFromMesh && fr.u.useBVH == 1) ? rtl::mesh_normal_rows(c->mesh) : nullptr;
    // per-vertex colours: mesh hits of the dynamic mesh's own scene; the hybrid scene keeps the constant albedo
    fr.colRows = (c->mesh && c->sceneFromMesh && fr.u.useBVH == 1) ? rtl::mesh_color_rows(c->mesh) : nullptr;
    // UVs and the albedo texture: mesh hits of the dynamic mesh's own scene, and only with both the UVs and a texture
    if (c->mesh && c->sceneFromMesh && fr.u.useBVH == 1 && rtl::mesh_uv_rows(c->mesh) && rtl::mesh_texture(c->mesh)) {
        fr.uvRows = rtl::mesh_uv_rows(c->mesh);
        fr.tex = *rtl::mesh_texture(c->mesh);
    }
    hipStream_t st = c->lanes[lane];
    if (c->serialFrames) HIP_TRY(c, hipStreamWaitEvent(st, c->evDone[prevLane], 0));
    // the albedo texture: the caller may have written the texels on rt_stream()'s stream, the previous frame's lane; this frame reads
    // them as they stand behind that write
    if (fr.uvRows && api_stream(c) != st) {
        HIP_TRY(c, hipEventRecord(c->evMeshDone, api_stream(c)));
        HIP_TRY(c, hipStreamWaitEvent(st, c->evMeshDone, 0));
    }
    const bool count = c->cfg.countWork != 0;
    int pipeline = c->cfg.pipeline;
    if (pipeline == RT_PIPELINE_AUTO) pipeline = (fr.u.useBVH == 1 && fr.sc.hasBVH && !count) ? RT_PIPELINE_WAVEFRONT : RT_PIPELINE_MEGAKERNEL;
    if (pipeline == RT_PIPELINE_WAVEFRONT && !(fr.u.useBVH == 1)) pipeline = RT_PIPELINE_MEGAKERNEL;   // analytic scene: pure ALU, megakernel only
    // beam cull: BVH frames of the wavefront pipeline; the lane says whether this launch set is culled and where its flags lie
    const bool cacheResident = (size_t)c->nInner * 64 + c->nWide4 * 128 + c->nPairs * 80 < ((size_t)32 << 20);   // the BVH arrays fit the 32 MB of L2
    if (pipeline == RT_PIPELINE_WAVEFRONT && !count) fr.tileDead = rt_wave_beam_flags(c->wave[lane], st, fr, std::max(c->treeDepth, 1), cacheResident);
    HIP_TRY(c, hipMemcpyAsync(c->dFrame[lane], &fr, sizeof(fr), hipMemcpyHostToDevice, st));
    if (fr.sc.rootBox) launch_frame_root_box(st, c->dFrame[lane]);
    Targets tg;
    tg.color = c->dColor[c->writeIdx];
    tg.prev = c->dColor[prevLane];
    tg.prevAll = needAll ? (const uint2 *)c->dHistAll[prevLane] : nullptr;
    tg.blockSlots = (int)c->nSlots;
    c->histExchanged[lane] = false;   // this lane's exchange buffer belongs to the frame that is about to be rendered
    tg.motion = c->dMotion[lane]; tg.gpos = c->dGPos[lane]; tg.gnrm = c->dGNrm[lane];
    if (batch > 1 && pipeline != RT_PIPELINE_WAVEFRONT) return fail(c, RT_ERR_STATE, "internal: a frame batch reached the megakernel");
    // EXTENSION: the hybrid scene in stages (rt_hybrid.hip) unless the megakernel was asked for; same frames bit for bit
    const bool staged = c->cfg.pipeline != RT_PIPELINE_MEGAKERNEL && fr.u.useBVH == RT_SCENE_HYBRID && fr.sc.hasBVH && !count;
    if (staged) {
        if (!c->hybrid[0]) c->hybrid[0] = rt_hybrid_create(c->cus);   // one arena for all lanes: the passes synchronise with the host anyway
        int rc = rt_hybrid_render(c->hybrid[0], c, st, c->dFrame[lane], fr, tg, std::max(c->treeDepth, 1), c->nLanes > 1 ? c->evDone[prevLane] : nullptr);
        if (rc != RT_OK) return fail(c, rc, "staged hybrid pipeline: %s", rt_hybrid_error(c->hybrid[0]));
    } else if (pipeline == RT_PIPELINE_WAVEFRONT) {
        int rc = rt_wave_render(c->wave[lane], c, st, c->dFrame[lane], fr, tg, c->dCounters, count, std::max(c->treeDepth, 1), c->nLanes > 1 ? c->evDone[prevLane] : nullptr,
                                cacheResident);
        if (rc != RT_OK) return fail(c, rc, "wavefront pipeline: %s", rt_wave_error(c->wave[lane]));
    } else {
        if (c->nLanes > 1) HIP_TRY(c, hipStreamWaitEvent(st, c->evDone[prevLane], 0));   // the megakernel reads the history from its first instruction on
        rt_stage_begin(c, 0, st);
        HIP_TRY(c, rtl::launch_mega(st, c->dFrame[lane], tg, c->dCounters, count, std::max(c->treeDepth, 1), c->g.nLocalTiles));
        rt_stage_end(c, 0, 1, st);
    }
    HIP_TRY(c, hipEventRecord(c->evDone[lane], st));
    c->lastStream = st;
    if (c->timing) c->timedFrames += batch;
    c->frameIndex += batch;          // Accum::swapAfterFrame, include/render/accum.h:125-128
    c->writeIdx = (c->writeIdx + 1) % c->nLanes;
    // rt_stream() is this lane from here on: device writes to the dynamic mesh that the caller orders on it must find a raster call that read the
    // mesh on another lane finished.  Nothing is enqueued unless such a call is in flight; the frame itself does not wait.
    if (c->raster && rt_raster_order_after(c->raster, st) != RT_OK) return fail(c, RT_ERR_HIP, "%s", rt_raster_error(c->raster));
    return RT_OK;
}

int rt_render_frame(RtContext *c, const RtUniforms *uIn) { return render_frames_impl(c, uIn, 1, nullptr); }

// K consecutive frames of a static camera in ONE set of launches ("batch several frames per gather ... when the camera is
// static").  The frames of such a sequence differ only in uFrameIndex and uJitter; the only thing frame f+1 needs from frame f is the
// accumulation history at its own pixel (rt_taa.glsl:86-105), which the resolve kernel chains in registers.  What a tile-parallel
// rank gains: each launch carries K times the work, so the fixed cost of the persistent traversal launches (ramp-up, tail of the
// longest rays) and of nine launches per frame is paid once per K frames -- measured per rank at world = 8: 0.40 -> 0.27 ms per frame
// at K = 4.  Results are bit-identical to K calls of rt_render_frame; the four targets afterwards are those of the LAST frame.
int rt_render_frames(RtContext *c, const RtUniforms *us, int count) {
    if (!c || !us || count < 1) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_render_frames before rt_resize");
    // A run of frames shares one set of launches only if every frame of it would take the wavefront pipeline (decided per run from
    // its first frame: the uniform blocks of a run agree in everything but jitter, so they agree in useBVH / nodeCount / triCount) and
    // if the resolve of frame k > 0 is sure to take the still branch of resolveTAA (rt_taa.glsl:86-105), whose history is the pixel's
    // own texel and is chained in registers.  With uTaaStillThresh <= 0 the test `length(motion) < thresh` fails even for zero motion
    // and the reprojection branch would read the texture from BEFORE the batch: such frames go one by one.
    auto batchable = [&](const RtUniforms &u) {
        return c->cfg.pipeline != RT_PIPELINE_MEGAKERNEL && c->cfg.countWork == 0 && u.useBVH == 1 && c->nNodes > 0 && u.nodeCount > 0 && u.triCount > 0 &&
               u.cameraMoved == 0 && (u.enableTAA == 0 || u.taaStillThresh > 0.0f);
    };
    // uniform blocks of a batch must agree in everything but frameIndex (ignored anyway) and jitter
    auto same_but_jitter = [](const RtUniforms &a, const RtUniforms &b) {
        RtUniforms x = a, y = b;
        x.frameIndex = y.frameIndex = 0;
        x.jitter[0] = y.jitter[0] = x.jitter[1] = y.jitter[1] = 0.0f;
        return std::memcmp(&x, &y, sizeof x) == 0;
    };
    int done = 0;
    while (done < count) {
        int k = 1;
        if (batchable(us[done]))
            while (k < RT_MAX_BATCH && done + k < count && same_but_jitter(us[done], us[done + k])) ++k;
        float jit[RT_MAX_BATCH][2] = {};
        for (int q = 0; q < k; ++q) { jit[q][0] = us[done + q].jitter[0]; jit[q][1] = us[done + q].jitter[1]; }
        int rc = render_frames_impl(c, &us[done], k, jit);
        if (rc != RT_OK) return rc;
        done += k;
    }
    return RT_OK;
}

int rt_render_ray(RtContext *c, const RtRenderParams *params, const RtCamera *cam, int useBVH, int showMotion, const float *currView,
                  const float *currProj) {
    if (!c || !params || !cam) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_render_ray before rt_resize");
    float V[16], P[16], VP[16];
    if (currView) std::memcpy(V, currView, 64); else rt_camera_view(cam, V);
    if (currProj) std::memcpy(P, currProj, 64); else rt_camera_proj(cam, P);
    rt_mat4_mul(P, V, VP);                                   // FrameState::beginFrame, frame_state.h:68-73
    if (!c->haveFrameState) { std::memcpy(c->prevVP, VP, 64); c->haveFrameState = true; }   // application.cpp:316-319
    // previous pose: the mesh moved since the last latch -- the frame is a moved one whatever the camera did, and takes the pose with it
    const bool meshMoved = c->mesh && c->meshMotionDirty && rtl::mesh_prev_tris(c->mesh);
    const int moved = (rt_camera_moved(VP, c->prevVP) || meshMoved) ? 1 : 0;        // application.cpp:387-395
    RtUniforms u;
    rt_make_uniforms(params, cam, V, VP, c->prevVP, c->g.W, c->g.H, c->frameIndex, moved, useBVH, showMotion, c->nNodes, c->nTris,
                     c->dEnv != nullptr, &u);
    int rc = rt_render_frame(c, &u);
    if (rc != RT_OK) return rc;
    std::memcpy(c->prevVP, VP, 64);                          // FrameState::endFrame, frame_state.h:81-84
    return meshMoved ? rt_mesh_motion_latch(c) : RT_OK;
}

int rt_set_extension(RtContext *c, const RtExtension *ext) {
    if (!c || !ext) return RT_ERR_INVALID;
    if (ext->giBounces < 1 || ext->giBounces > 8) return fail(c, RT_ERR_INVALID, "rt_set_extension: giBounces = %d (1..8)", ext->giBounces);
    if (ext->envFilter != 0 && ext->envFilter != 1) return fail(c, RT_ERR_INVALID, "rt_set_extension: envFilter = %d (0 or 1)", ext->envFilter);
    c->giBounces = ext->giBounces;
    c->envFilter = ext->envFilter;
    return RT_OK;
}

// `count` consecutive rt_render_ray calls with the same camera and parameters, handed to rt_render_frames as one sequence (so an
// accumulating static camera is rendered in batches).  Frame state (prev / curr view-projection) is kept exactly as rt_render_ray does.
int rt_render_ray_frames(RtContext *c, const RtRenderParams *params, const RtCamera *cam, int useBVH, int showMotion, int count) {
    if (!c || !params || !cam || count < 1) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_render_ray_frames before rt_resize");
    return guarded(c, "rt_render_ray_frames", [&]() -> int {
        float V[16], P[16], VP[16];
        rt_camera_view(cam, V);
        rt_camera_proj(cam, P);
        rt_mat4_mul(P, V, VP);
        if (!c->haveFrameState) { std::memcpy(c->prevVP, VP, 64); c->haveFrameState = true; }
        std::vector<RtUniforms> us((size_t)count);
        float prev[16];
        std::memcpy(prev, c->prevVP, 64);
        // previous pose: as rt_render_ray -- the first frame is a moved one and latches, the rest are batched behind it
        const bool meshMoved = c->mesh && c->meshMotionDirty && rtl::mesh_prev_tris(c->mesh);
        for (int i = 0; i < count; ++i) {
            const int moved = (rt_camera_moved(VP, prev) || (meshMoved && i == 0)) ? 1 : 0;
            rt_make_uniforms(params, cam, V, VP, prev, c->g.W, c->g.H, c->frameIndex + i, moved, useBVH, showMotion, c->nNodes, c->nTris, c->dEnv != nullptr,
                             &us[(size_t)i]);
            std::memcpy(prev, VP, 64);
        }
        const int first = c->frameIndex;
        int rc = RT_OK;
        if (meshMoved) {
            rc = rt_render_frame(c, &us[0]);
            if (rc == RT_OK) rc = rt_mesh_motion_latch(c);
            if (rc == RT_OK && count > 1) rc = rt_render_frames(c, us.data() + 1, count - 1);
        } else rc = rt_render_frames(c, us.data(), count);
        // FrameState::endFrame (frame_state.h:81-84) runs after every rendered frame: if the sequence failed part-way, the frames
        // that did render have advanced frameIndex and the camera state must follow them, exactly as with rt_render_ray per frame
        if (rc == RT_OK || c->frameIndex != first) std::memcpy(c->prevVP, VP, 64);
        return rc;
    });
}

int rt_synchronize(RtContext *c) {
    if (!c) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    HIP_TRY(c, sync_all(c));
    return RT_OK;
}

int rt_read_target(RtContext *c, int which, void *dst, int fmt) {
    if (!c || !dst) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_read_target before rt_resize");
    (void)hipSetDevice(c->cfg.device);
    int ch;
    void *src = target_ptr(c, which, ch);
    if (!src || (fmt != RT_FORMAT_F16 && fmt != RT_FORMAT_F32)) return fail(c, RT_ERR_INVALID, "rt_read_target: which=%d format=%d", which, fmt);
    const size_t n = (size_t)c->g.W * c->g.H, bytes = n * ch * (fmt == RT_FORMAT_F32 ? 4 : 2);
    return read_back_via_staging(c, bytes, dst, [&]() -> int {
        hipLaunchKernelGGL(k_untile, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, src, c->dStaging, c->g, ch, fmt == RT_FORMAT_F32 ? 1 : 0);
        HIP_TRY(c, hipGetLastError());
        return RT_OK;
    });
}

int rt_write_target(RtContext *c, int which, const void *srcHost, int fmt) {
    if (!c || !srcHost) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_write_target before rt_resize");
    (void)hipSetDevice(c->cfg.device);
    int ch;
    void *dstT = target_ptr(c, which, ch);
    if (!dstT || fmt != RT_FORMAT_F16) return fail(c, RT_ERR_INVALID, "rt_write_target: which=%d format=%d (RT_FORMAT_F16 only)", which, fmt);
    const size_t bytes = (size_t)c->g.W * c->g.H * ch * 2;
    HIP_TRY(c, sync_all(c));
    int rc = ensure_staging(c, bytes);
    if (rc != RT_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->dStaging, srcHost, bytes, hipMemcpyHostToDevice, c->stream));
    const unsigned nSlots = (unsigned)c->g.nLocalTiles * 256u;
    hipLaunchKernelGGL(k_tile, dim3((nSlots + 255) / 256), dim3(256), 0, c->stream, (const void *)c->dStaging, dstT, c->g, ch);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sync_all(c));
    return RT_OK;
}

int rt_present(RtContext *c, const RtPresentParams *p, uint8_t *dst) {
    if (!c || !p || !dst) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_present before rt_resize");
    if (c->g.world > 1) return fail(c, RT_ERR_UNSUPPORTED, "rt_present: the 7x7 filter reads other ranks' tiles; gather the four targets and use rt_present_gathered");
    if ((int)p->resolution[0] != c->g.W || (int)p->resolution[1] != c->g.H) return fail(c, RT_ERR_INVALID, "rt_present: uResolution != framebuffer");
    (void)hipSetDevice(c->cfg.device);
    const int l = last_lane(c);
    return present_to(c, *p, c->dColor[l], c->dMotion[l], c->dGPos[l], c->dGNrm[l], 0, dst);
}

int rt_present_gathered(RtContext *c, const RtPresentParams *p, const void *color, const void *motion, const void *gpos, const void *gnrm, uint8_t *dst) {
    if (!c || !p || !color || !motion || !gpos || !gnrm || !dst) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_present_gathered before rt_resize");
    if ((int)p->resolution[0] != c->g.W || (int)p->resolution[1] != c->g.H) return fail(c, RT_ERR_INVALID, "rt_present_gathered: uResolution != framebuffer");
    (void)hipSetDevice(c->cfg.device);
    return present_to(c, *p, color, motion, gpos, gnrm, (int)c->nSlots, dst);
}

// ---- raster preview (renderRaster): the work is in rt_raster.hip; its buffers are its own, no ray target or frame state is touched
int rt_raster_mesh(RtContext *c, int slot, const float *positions, int nVerts, const uint32_t *indices, int nIdx) {
    if (!c) return RT_ERR_INVALID;
    return with_raster(c, true, [&](RtRaster *r) { return rt_raster_set_mesh(r, slot, positions, nVerts, indices, nIdx); });
}

int rt_render_raster(RtContext *c, const RtRasterDraw *draws, int nDraws, const float *view16, const float *proj16) {
    if (!c) return RT_ERR_INVALID;
    if (nDraws < 0 || (nDraws > 0 && !draws) || !view16 || !proj16) return fail(c, RT_ERR_INVALID, "rt_render_raster: bad arguments");
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_render_raster before rt_resize");
    if (c->g.world > 1) return fail(c, RT_ERR_UNSUPPORTED, "rt_render_raster: tile-parallel contexts (worldSize %d) do not rasterise; use a single-rank context", c->g.world);
    hipStream_t st = api_stream(c);   // rt_stream()
    // the dynamic mesh as it is now (a binding follows a later rt_mesh_upload): its arrays, and mesh_update's per-lane events for the other lanes.  Whoever
    // releases the mesh has waited for every lane, and this call runs on one, so no array is freed under it.
    RtRasterDynamic dyn = {};
    if (c->mesh) {
        dyn.pos = rtl::mesh_positions(c->mesh); dyn.idx = rtl::mesh_indices(c->mesh); dyn.partOf = rtl::mesh_part_of(c->mesh); dyn.partM = rtl::mesh_part_matrices(c->mesh);
        dyn.nTris = rtl::mesh_layout(c->mesh).nTris; dyn.nParts = rtl::mesh_part_count(c->mesh);
        for (int i = 0; i < c->nLanes; ++i)
            if (c->lanes[i] != st) { dyn.others[dyn.nOthers] = c->lanes[i]; dyn.evOther[dyn.nOthers] = c->evMeshLane[i]; ++dyn.nOthers; }
    }
    return with_raster(c, true, [&](RtRaster *r) { return rt_raster_render(r, st, c->g.W, c->g.H, draws, nDraws, view16, proj16, c->mesh ? &dyn : nullptr); });
}

int rt_raster_mesh_dynamic(RtContext *c, int slot, int mode) {
    if (!c) return RT_ERR_INVALID;
    return with_raster(c, true, [&](RtRaster *r) { return rt_raster_bind_dynamic(r, slot, mode); });
}

int rt_raster_part_colors(RtContext *c, int slot, const float *rgb, int nParts) {
    if (!c) return RT_ERR_INVALID;
    return with_raster(c, true, [&](RtRaster *r) { return rt_raster_set_part_colors(r, slot, rgb, nParts); });
}

int rt_raster_targets(RtContext *c, void **rgba8, void **primId, void **depth24, size_t *bytesEach) {
    if (!c) return RT_ERR_INVALID;
    for (void **p : {rgba8, primId, depth24}) if (p) *p = nullptr;
    if (bytesEach) *bytesEach = 0;
    if (!c->raster) return fail(c, RT_ERR_STATE, "rt_raster_targets before rt_render_raster");
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_raster_targets before rt_resize");
    const int rc = rt_raster_buffers(c->raster, c->g.W, c->g.H, rgba8, primId, depth24, bytesEach);
    return rc == RT_OK ? RT_OK : fail(c, rc, "%s", rt_raster_error(c->raster));
}

int rt_read_raster(RtContext *c, uint8_t *rgba8, uint32_t *primId, uint32_t *depth24) {
    if (!c) return RT_ERR_INVALID;
    if (!c->raster) return fail(c, RT_ERR_STATE, "rt_read_raster before rt_render_raster");
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_read_raster before rt_resize");
    return with_raster(c, false, [&](RtRaster *r) { return rt_raster_read(r, c->g.W, c->g.H, rgba8, primId, depth24); });
}

int rt_get_raster_stats(RtContext *c, RtRasterStats *out) {
    if (!c || !out) return RT_ERR_INVALID;
    return with_raster(c, false, [&](RtRaster *r) { return rt_raster_stats(r, out); });
}

int rt_stream(RtContext *c, void **s) {
    if (!c || !s) return RT_ERR_INVALID;
    *s = (void *)api_stream(c);   // the stream the most recent frame was enqueued on
    return RT_OK;
}

int rt_get_counters(RtContext *c, RtCounters *out) {
    if (!c || !out) return RT_ERR_INVALID;
    if (!c->cfg.countWork) return fail(c, RT_ERR_STATE, "rt_get_counters: context created without countWork");
    (void)hipSetDevice(c->cfg.device);
    unsigned long long v[16];
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(v, c->dCounters, sizeof v, hipMemcpyDeviceToHost));
    out->raysClosest = v[0]; out->raysShadow = v[1]; out->raysAnalytic = v[2]; out->nodeFetch = v[3];
    out->triFetch = v[4]; out->envLookup = v[5]; out->hitPixels = v[6];
    out->fetchPrimary = v[7]; out->fetchShadow = v[8]; out->fetchAO = v[9];
    return RT_OK;
}
int rt_reset_counters(RtContext *c) {
    if (!c) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    // frames still in flight on ANY lane add their atomics until they finish: drain all lanes, then clear synchronously
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemset(c->dCounters, 0, 16 * sizeof(unsigned long long)));
    return RT_OK;
}

int rt_get_scene_info(const RtContext *c, RtSceneInfo *out) {
    if (!c || !out) return RT_ERR_INVALID;
    std::memset(out, 0, sizeof *out);
    out->nNodes = c->nNodes; out->nTris = c->nTris; out->nInner = c->nInner; out->treeDepth = c->treeDepth;
    if (c->nNodes == 0) return RT_OK;
    out->nWide4 = (int32_t)c->nWide4; out->nPairs = (int32_t)c->nPairs;
    out->bytesNodes2 = (uint64_t)std::max(c->nInner, 1) * 64;
    out->bytesNodes4 = c->dQ4 ? (uint64_t)c->nWide4 * 64 + (uint64_t)c->nLeafBoxes * 32 : (uint64_t)c->nWide4 * 128;   // the any-hit launches walk the quantised nodes when they exist
    out->bytesPairs = (uint64_t)c->nPairs * 80;
    out->bytesTris = (uint64_t)c->nTris * 48;
    out->nFused = (int32_t)c->nFused;
    out->flags = c->sceneFlags | (c->dIN2 ? RT_SCENE_IMPLICIT : 0);
    out->implicitDepth = c->implD;
    return RT_OK;
}

int rt_get_memory_info(RtContext *c, RtMemoryInfo *out) {
    if (!c || !out) return RT_ERR_INVALID;
    std::memset(out, 0, sizeof *out);
    (void)hipSetDevice(c->cfg.device);
    out->queueArenaBytes = rt_arena_pool_bytes(c->arenaPool);
    out->queueArenas = rt_arena_pool_count(c->arenaPool);
    out->lanes = c->nLanes;
    for (int i = 0; i < c->nLanes; ++i) { out->frameArrayBytes += rt_wave_frame_bytes(c->wave[i]); out->hybridArenaBytes += rt_hybrid_arena_bytes(c->hybrid[i]); }
    size_t fr = 0, tot = 0;
    HIP_TRY(c, hipMemGetInfo(&fr, &tot));
    out->deviceFreeBytes = fr; out->deviceTotalBytes = tot;
    return RT_OK;
}

int rt_get_traced_rays(RtContext *c, RtTracedRays *out, int reset) {
    if (!c || !out) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    unsigned long long v[16];
    (void)sync_all(c);
    const int rc = sum_over_lanes(c, "rt_get_traced_rays", rt_wave_traced, reset, v);
    if (rc != RT_OK) return rc;
    out->candidatePixels = v[0]; out->hitPixels = v[1]; out->primary = v[2]; out->shadow = v[3]; out->bounce = v[4];
    out->bounceShadow = v[5]; out->frames = v[6];
    out->gatherLoadsPrimary = v[8]; out->gatherLoadsShadow = v[9]; out->gatherLoadsBounce = v[10];
    out->mergedLoadsPrimary = v[11]; out->mergedLoadsShadow = v[12]; out->mergedLoadsBounce = v[13];
    out->ao = v[7]; out->gatherLoadsAO = v[14];
    return RT_OK;
}

int rt_enable_stage_timing(RtContext *c, int enable) {
    if (!c) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    resolve_stage_events(c);
    c->timing = enable != 0;
    std::memset(c->stageMs, 0, sizeof c->stageMs);
    std::memset(c->stageLaunches, 0, sizeof c->stageLaunches);
    c->timedFrames = 0;
    return RT_OK;
}
int rt_get_stage_times(RtContext *c, RtStageTimes *out) {
    if (!c || !out) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    resolve_stage_events(c);
    out->nStages = RT_MAX_STAGES;
    out->frames = c->timedFrames;
    for (int i = 0; i < RT_MAX_STAGES; ++i) { out->ms[i] = c->stageMs[i]; out->launches[i] = c->stageLaunches[i]; }
    return RT_OK;
}

}  // extern "C"
