// rt_api.hip -- C ABI of librt_mi355.so (include/rt_mi355.h): context, uploads, frame loop, readback.
//
// The context owns one HIP stream and all device memory.  There is no CPU rendering path: without
// a usable HIP device rt_create fails with RT_ERR_NO_DEVICE and nothing else can be called.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: RCCL is bound at run time (rccl_api below), single-GPU users never load it

#include "rt_context.hpp"
#include "rt_scene_pack.hpp"
#include "rt_wave_plan.hpp"

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

// Gathered blocks (rank-major, blockBytes each, tile-major inside) -> row-major frame of halfs.
__global__ void k_assemble(const void *gathered, void *dst, FrameGeom g, int channels, size_t blockBytes) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.W * g.H) return;
    int x = i % g.W, y = i / g.W;
    int tx = x >> 4, ty = y >> 4;
    int t = tile_index(g, tx, ty);
    int owner = t % g.world, local = t / g.world;
    int lx = x & 15, ly = y & 15;
    int q = (lx >> 3) | ((ly >> 3) << 1);
    size_t slot = (size_t)local * 256 + q * 64 + (ly & 7) * 8 + (lx & 7);
    const uint16_t *in = (const uint16_t *)((const char *)gathered + (size_t)owner * blockBytes) + slot * channels;
    uint16_t *out = (uint16_t *)dst + (size_t)i * channels;
    for (int c = 0; c < channels; ++c) out[c] = in[c];
}

__global__ void k_debug_eval(int op, const float *a, const float *b, const float *c, uint32_t *out, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = a[i], y = b ? b[i] : 0.0f, z = c ? c[i] : 0.0f;
    float s, co;
    uint32_t r = 0;
    switch (op) {
        case 0: sincosr(x, s, co); r = f2u(s); break;
        case 1: sincosr(x, s, co); r = f2u(co); break;
        case 2: r = f2u(exp2r(x)); break;
        case 3: r = f2u(log2r(x)); break;
        case 4: r = f2u(powr(x, y)); break;
        case 5: r = f32_to_f16_bits(x); break;
        case 6: r = rand_bits(x, y, (int)z); break;
        case 7: r = f2u(x / y); break;
        case 8: r = f2u(__builtin_sqrtf(x)); break;
        case 9: r = f2u(1.0f / __builtin_sqrtf(x)); break;
        case 10: r = f2u(texel_unorm8((uint8_t)(int)x)); break;
        case 11: r = f2u(halton((int)x, (int)y)); break;
        case 12: case 13: {   // a, b, c hold integers as bit patterns here: thread index, live hits, spp
            int sm; uint32_t j;
            sample_and_hit(f2u(x), f2u(y), (int)f2u(z), sm, j);
            r = op == 12 ? (uint32_t)sm : j;
            break;
        }
        default: break;
    }
    out[i] = r;
}

// rt_debug_disk_unlit: diskUnlit(hp, N) beside what it stands for -- diskSample, the production code, for the four samples of `seeds` (pixel, frame) seeds.
// flags bit 0: diskUnlit; bit 1: some sample had geom != 0 (NaN counts).  maxDot: the largest dot(N, s.L) as diskSample / shadeLambertPhong compute it.
__global__ __launch_bounds__(256) void k_debug_disk_unlit(RtUniforms u, const float *hp, const float *nrm, int n, int seeds, uint8_t *flags, float *maxDot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 p = ld3(hp + (size_t)i * 3), N = ld3(nrm + (size_t)i * 3);
    Frag F;
    F.u = &u; F.sc = nullptr;
    V3 lt, lb;
    lightFrame(lt, lb);
    bool lit = false;
    float md = -__builtin_inff();
    for (int k = 0; k < seeds; ++k) {
        F.fcx = (float)((k * 73 + i) % 1920) + 0.5f; F.fcy = (float)((k * 151 + i * 7) % 1080) + 0.5f;
        F.frameIndex = k;
        const V2 rot = cpOffset(F.fcx, F.fcy, F.frameIndex);
        for (int j = 0; j < 4; ++j) {
            const DiskSample s = diskSample(F, p, N, k * 4 + (i & 3), j, rot, lt, lb);
            lit = lit || !(s.geom == 0.0f);
            md = fmaxr(md, dot(N, s.L));
        }
    }
    flags[i] = (uint8_t)((diskUnlit(p, N) ? 1 : 0) | (lit ? 2 : 0));
    maxDot[i] = md;
}

// A scene a device rebuild installed: the frame descriptor the host copied carries no root box; take it from the device.
__global__ void k_frame_root_box(DevFrame *fr) {
    if (threadIdx.x == 0) scene_take_root_box(fr->sc);
}

__global__ __launch_bounds__(256) void k_debug_trace(DevScene sc, int kind, const float *o, const float *d, const float *tMax, float eps,
                                                     float inf, float *out7, int n) {
    __shared__ StackEntry stack[4 * 32 * 64];
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    StackEntry *stk = &stack[(threadIdx.x >> 6) * 32 * 64 + (threadIdx.x & 63)];
    if (i >= n) return;
    scene_take_root_box(sc);
    Work w;
    work_zero(w);
    V3 ro = ld3(o + (size_t)i * 3), rd = ld3(d + (size_t)i * 3);
    float *out = out7 + (size_t)i * 7;
    if (kind == 0) {
        float t;
        int tri;
        bool hit = bvh_closest<false>(sc, ro, rd, eps, inf, stk, t, tri, w);
        out[0] = hit ? t : inf;
        if (hit) {
            V3 p = ro + rd * t, nn = tri_normal(sc, tri);
            out[1] = p.x; out[2] = p.y; out[3] = p.z; out[4] = nn.x; out[5] = nn.y; out[6] = nn.z;
        } else {
            for (int k = 1; k < 7; ++k) out[k] = 0.0f;
        }
    } else {
        out[0] = bvh_anyhit<false>(sc, ro, rd, eps, tMax[i], stk, w) ? 1.0f : 0.0f;
        for (int k = 1; k < 7; ++k) out[k] = 0.0f;
    }
}

void free_gather_buffers(RtContext *c) {
    for (int l = 0; l < RT_MAX_LANES; ++l)
        for (int w = 0; w < 4; ++w) {
            if (c->dGathered[l][w]) (void)hipFree(c->dGathered[l][w]);
            if (c->dAssembled[l][w]) (void)hipFree(c->dAssembled[l][w]);
            c->dGathered[l][w] = c->dAssembled[l][w] = nullptr;
        }
    for (int w = 0; w < 4; ++w) c->gatheredLane[w] = -1;
}

void free_targets(RtContext *c) {
    for (int i = 0; i < RT_MAX_LANES; ++i) { if (c->dColor[i]) (void)hipFree(c->dColor[i]); c->dColor[i] = nullptr; }
    for (int i = 0; i < RT_MAX_LANES; ++i) { if (c->dHistAll[i]) (void)hipFree(c->dHistAll[i]); c->dHistAll[i] = nullptr; c->histExchanged[i] = false; }
    for (int i = 0; i < RT_MAX_LANES; ++i) {
        if (c->dMotion[i]) (void)hipFree(c->dMotion[i]);
        if (c->dGPos[i]) (void)hipFree(c->dGPos[i]);
        if (c->dGNrm[i]) (void)hipFree(c->dGNrm[i]);
        c->dMotion[i] = nullptr; c->dGPos[i] = c->dGNrm[i] = nullptr;
    }
    free_gather_buffers(c);
    c->sized = false;
}

void free_scene(RtContext *c) { clear_scene(c, true); }

// One scene array to the device (an empty one stays null)
template <class T> int upload(RtContext *c, float4 **dst, const std::vector<T> &v) {
    if (v.empty()) return RT_OK;
    HIP_TRY(c, hipMalloc(dst, v.size() * sizeof(T)));
    HIP_TRY(c, hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return RT_OK;
}

int last_lane(const RtContext *c) { return (c->writeIdx + c->nLanes - 1) % c->nLanes; }   // lane of the frame rendered last
void *target_ptr(RtContext *c, int which, int &channels) {
    const int l = last_lane(c);
    switch (which) {
        case RT_TARGET_COLOR: channels = 4; return c->dColor[l];
        case RT_TARGET_MOTION: channels = 2; return c->dMotion[l];
        case RT_TARGET_GPOS: channels = 4; return c->dGPos[l];
        case RT_TARGET_GNRM: channels = 4; return c->dGNrm[l];
        default: channels = 0; return nullptr;
    }
}

}  // namespace

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
    free_scene(c);
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
        free_scene(c);
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
        if (rc != RT_OK) { free_scene(c); return rc; }
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

int rt_debug_read_scene(RtContext *c, int which, void *dst, size_t capacity, size_t *bytes) {
    if (!c || !bytes) return RT_ERR_INVALID;
    *bytes = 0;
    const void *src = nullptr;
    size_t n = 0;
    const bool have = c->nNodes > 0 && c->nTris > 0;
    const size_t implNodes = ((size_t)1 << c->implD) - 1;   // slots of the implicit node arrays; the leaves are one more
    switch (which) {
        case RT_SCENE_ARRAY_TRIS: src = c->dTris; n = (size_t)(c->nTris + 8) * 48; break;
        case RT_SCENE_ARRAY_PAIRS: src = c->dPairs; n = (c->nPairs + 8) * 80; break;
        case RT_SCENE_ARRAY_NODES2: src = c->dWNodes; n = (size_t)std::max(c->nInner, 1) * 64; break;
        case RT_SCENE_ARRAY_NODES2W: src = c->dWNodesW; n = (size_t)std::max(c->nInner, 1) * 64; break;
        case RT_SCENE_ARRAY_NODES4: src = c->dW4; n = c->nWide4 * 128; break;
        case RT_SCENE_ARRAY_QNODES4: src = c->dQ4; n = c->nWide4 * 64; break;
        case RT_SCENE_ARRAY_LEAFBOX: src = c->dLeafBox; n = c->leafBoxBytes; break;
        case RT_SCENE_ARRAY_FUSED: src = c->dWF; n = c->nFused * 128; break;
        case RT_SCENE_ARRAY_IMPL_NODES2: src = c->dIN2; n = implNodes * 48; break;
        case RT_SCENE_ARRAY_IMPL_PAIRS: src = c->dIPairs; n = ((implNodes + 1) * (size_t)c->implR + 8) * 80; break;
        case RT_SCENE_ARRAY_IMPL_NODES4: src = c->dIN4; n = implNodes * 96; break;
        case RT_SCENE_ARRAY_IMPL_QNODES4: src = c->dIQ4; n = implNodes * 48; break;
        case RT_SCENE_ARRAY_IMPL_LEAFBOX: src = c->dILeafBox; n = (implNodes + 1) * 32; break;
        case RT_SCENE_ARRAY_PREV_TRIS: src = (c->mesh && c->sceneFromMesh) ? rtl::mesh_prev_tris(c->mesh) : nullptr; n = (size_t)c->nTris * 48; break;
        case RT_SCENE_ARRAY_NORMAL_ROWS: src = (c->mesh && c->sceneFromMesh) ? rtl::mesh_normal_rows(c->mesh) : nullptr; n = (size_t)c->nTris * 48; break;
        case RT_SCENE_ARRAY_COLOR_ROWS: src = (c->mesh && c->sceneFromMesh) ? rtl::mesh_color_rows(c->mesh) : nullptr; n = (size_t)c->nTris * 48; break;
        case RT_SCENE_ARRAY_UV_ROWS: src = (c->mesh && c->sceneFromMesh) ? rtl::mesh_uv_rows(c->mesh) : nullptr; n = (size_t)c->nTris * 32; break;
        default: return fail(c, RT_ERR_INVALID, "rt_debug_read_scene: array %d", which);
    }
    if (!have || !src) return RT_OK;
    *bytes = n;
    if (!dst) return RT_OK;
    if (capacity < n) return fail(c, RT_ERR_INVALID, "rt_debug_read_scene: array %d has %zu bytes, room for %zu", which, n, capacity);
    (void)hipSetDevice(c->cfg.device);
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_debug_pack_scene(const float *nodes12, int nNodes, const float *tris12, int nTris, const RtPackOptions *opt, int which, void *dst, size_t capacity,
                        size_t *bytes) {
    if (!bytes || !nodes12 || !tris12 || nNodes <= 0 || nTris <= 0) return RT_ERR_INVALID;
    *bytes = 0;
    return guarded(nullptr, "rt_debug_pack_scene", [&]() -> int {
        rtl::PackOptions o = rtl::pack_options_from_env();
        if (opt) { o.qnodes = opt->qnodes; o.fused = opt->fused != 0; o.implicit = opt->implicit != 0; o.anyhitSah = opt->anyhitSah != 0; o.sparseLeafBoxes = opt->sparseLeafBoxes != 0; }
        rtl::PackedScene s;
        std::string err;
        const int rc = rtl::pack_scene(nodes12, nNodes, tris12, nTris, o, s, err);
        if (rc != RT_OK) return fail(nullptr, rc, "%s", err.c_str());
        std::vector<float> tris;
        const void *src = nullptr;
        size_t n = 0;
        auto of = [&](const auto &v) { src = v.data(); n = v.size() * 4; };
        switch (which) {
            case RT_SCENE_ARRAY_TRIS: tris.assign(tris12, tris12 + (size_t)nTris * 12); tris.resize((size_t)(nTris + 8) * 12, 0.0f); of(tris); break;
            case RT_SCENE_ARRAY_PAIRS: of(s.pairs); break;
            case RT_SCENE_ARRAY_NODES2: of(s.wn); break;
            case RT_SCENE_ARRAY_NODES2W: of(s.wnW); break;
            case RT_SCENE_ARRAY_NODES4: of(s.w4); break;
            case RT_SCENE_ARRAY_QNODES4: of(s.q4); break;
            case RT_SCENE_ARRAY_LEAFBOX: of(s.leafBox); break;
            case RT_SCENE_ARRAY_FUSED: of(s.wF); break;
            case RT_SCENE_ARRAY_IMPL_NODES2: of(s.iN2); break;
            case RT_SCENE_ARRAY_IMPL_PAIRS: of(s.iPairs); break;
            case RT_SCENE_ARRAY_IMPL_NODES4: of(s.iN4); break;
            case RT_SCENE_ARRAY_IMPL_QNODES4: of(s.iQ4); break;
            case RT_SCENE_ARRAY_IMPL_LEAFBOX: of(s.iLeafBox); break;
            case RT_SCENE_ARRAY_PACK_INFO: {
                static_assert(sizeof(RtPackInfo) % 4 == 0, "RtPackInfo is handed out as words");
                RtPackInfo info = {};
                info.nNodes = nNodes; info.nTris = nTris; info.nInner = s.nInner; info.treeDepth = s.depth;
                info.nWide4 = (int32_t)(s.w4.size() / 32); info.nPairs = (int32_t)(s.pairs.size() / 20 - 8); info.nFused = (int32_t)(s.wF.size() / 32);
                info.flags = s.flags | (s.iN2.empty() ? 0 : RT_SCENE_IMPLICIT); info.implicitDepth = s.implD; info.implicitRecords = s.implR;
                info.rootRef = s.rootRef; info.rootRefW = s.rootRefW; info.rootRef4 = s.rootRef4; info.anyStack = s.anyStack;
                info.leafBoxMagic = s.leafBoxMagic; info.nLeafBoxes = (int32_t)s.nLeafBoxes; info.collapsed4 = s.collapsed4 ? 1 : 0;
                std::memcpy(info.rootMin, s.rootMin, 12); std::memcpy(info.rootMax, s.rootMax, 12);
                tris.resize(sizeof info / 4);
                std::memcpy(tris.data(), &info, sizeof info);
                of(tris);
                break;
            }
            default: return fail(nullptr, RT_ERR_INVALID, "rt_debug_pack_scene: array %d", which);
        }
        *bytes = n;
        if (!dst) return RT_OK;
        if (capacity < n) return fail(nullptr, RT_ERR_INVALID, "rt_debug_pack_scene: array %d has %zu bytes, room for %zu", which, n, capacity);
        if (n) std::memcpy(dst, src, n);
        return RT_OK;
    });
}

int rt_debug_wave_plan(uint64_t slots, int spp, int aoRays, const RtWaveOptions *opt, int64_t hits, double share, RtWavePlan *out) {
    if (!out || slots == 0 || slots % 256 != 0 || spp < 1 || aoRays < 0 || !(share >= 0.0)) return RT_ERR_INVALID;
    return guarded(nullptr, "rt_debug_wave_plan", [&]() -> int {
        const rtl::WavePlan p = rtl::wave_plan((size_t)slots, spp, aoRays, opt ? *opt : rtl::wave_options_from_env());
        if (p.tooLarge) return fail(nullptr, RT_ERR_UNSUPPORTED, "%s", rtl::kTooLargeMessage);
        rtl::wave_plan_describe(p, hits, share, *out);
        return RT_OK;
    });
}

// The frame geometry of a w x h framebuffer on rank `rank` of `world` (rt_resize), for a batch of one.
static FrameGeom make_frame_geom(int w, int h, int rank, int world) {
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

int rt_debug_texel_unorm8(float *out256) {
    if (!out256) return RT_ERR_INVALID;
    for (int c = 0; c < 256; ++c) out256[c] = texel_unorm8((uint8_t)c);
    return RT_OK;
}
int rt_debug_halton_pairs(int frame0, int count, float *out) {
    if (!out || count < 0 || frame0 < 0) return RT_ERR_INVALID;
    for (int i = 0; i < count; ++i) { out[2 * i] = halton(frame0 + i + 1, 2); out[2 * i + 1] = halton(frame0 + i + 1, 3); }
    return RT_OK;
}
uint32_t rt_debug_div_reciprocal(uint32_t d, uint64_t nMax) { return div_reciprocal(d, nMax); }
int rt_debug_div_by(uint32_t d, uint32_t rcp, const uint32_t *n, size_t count, uint32_t *q, uint32_t *r) {
    if (d == 0 || !n || !q || !r) return RT_ERR_INVALID;
    for (size_t i = 0; i < count; ++i) { q[i] = div_by(n[i], d, rcp); r[i] = n[i] - q[i] * d; }
    return RT_OK;
}
int rt_debug_frame_geom(int w, int h, int rank, int world, int batch, int useReciprocals, RtFrameGeomInfo *out, int32_t *xy) {
    if (!out || w <= 0 || h <= 0 || world < 1 || rank < 0 || rank >= world || batch < 1 || batch > RT_MAX_BATCH) return RT_ERR_INVALID;
    FrameGeom g = make_frame_geom(w, h, rank, world);
    g.batch = batch;
    frame_geom_set_reciprocals(g);
    if (!useReciprocals) g.rcpLocalTiles = g.rcpTilesX = g.rcpWorld = 0;
    out->tilesX = g.tilesX; out->tilesY = g.tilesY; out->nTiles = g.nTiles; out->nLocalTiles = g.nLocalTiles;
    out->rcpLocalTiles = g.rcpLocalTiles; out->rcpTilesX = g.rcpTilesX; out->rcpWorld = g.rcpWorld;
    if (xy)
        for (int lt = 0; lt < g.nLocalTiles * batch; ++lt)
            for (int tid = 0; tid < 256; ++tid) {
                int x, y;
                int32_t *o = xy + ((size_t)lt * 256 + tid) * 3;
                if (pixel_of_slot(g, lt, tid, x, y)) { o[0] = x; o[1] = y; o[2] = sub_frame_of_tile(g, lt); }
                else o[0] = o[1] = o[2] = -1;
            }
    return RT_OK;
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
    const int prevLaneX = (c->writeIdx + c->nLanes - 1) % c->nLanes;
    const bool needAll = fr.u.cameraMoved == 1 && c->g.world > 1 && fr.u.enableTAA == 1 && c->frameIndex > 0;
    if (needAll && !(c->dHistAll[prevLaneX] && c->histExchanged[prevLaneX]))
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
    // Lane = frame index mod nLanes = index of the COLOR0 buffer this frame writes: consecutive frames rotate over the lanes'
    // streams and overlap everywhere except at the temporal resolve (the only read of the previous frame), and every later
    // reader of a COLOR0 buffer (gather, assemble) is stream-ordered before the next writer of the same buffer.
    const int lane = c->writeIdx, prevLane = (c->writeIdx + c->nLanes - 1) % c->nLanes;
    hipStream_t st = c->lanes[lane];
    if (c->serialFrames) HIP_TRY(c, hipStreamWaitEvent(st, c->evDone[prevLane], 0));
    // the albedo texture: the caller may have written the texels on rt_stream()'s stream, the previous frame's lane; this frame reads
    // them as they stand behind that write
    if (fr.uvRows && api_stream(c) != st) {
        HIP_TRY(c, hipEventRecord(c->evMeshDone, api_stream(c)));
        HIP_TRY(c, hipStreamWaitEvent(st, c->evMeshDone, 0));
    }
    HIP_TRY(c, hipMemcpyAsync(c->dFrame[lane], &fr, sizeof(fr), hipMemcpyHostToDevice, st));
    if (fr.sc.rootBox) hipLaunchKernelGGL(k_frame_root_box, dim3(1), dim3(64), 0, st, c->dFrame[lane]);
    Targets tg;
    tg.color = c->dColor[c->writeIdx];
    tg.prev = c->dColor[prevLane];
    tg.prevAll = needAll ? (const uint2 *)c->dHistAll[prevLane] : nullptr;
    tg.blockSlots = (int)c->nSlots;
    c->histExchanged[lane] = false;   // this lane's exchange buffer belongs to the frame that is about to be rendered
    tg.motion = c->dMotion[lane]; tg.gpos = c->dGPos[lane]; tg.gnrm = c->dGNrm[lane];
    const bool count = c->cfg.countWork != 0;
    int pipeline = c->cfg.pipeline;
    if (pipeline == RT_PIPELINE_AUTO) pipeline = (fr.u.useBVH == 1 && fr.sc.hasBVH && !count) ? RT_PIPELINE_WAVEFRONT : RT_PIPELINE_MEGAKERNEL;
    if (pipeline == RT_PIPELINE_WAVEFRONT && !(fr.u.useBVH == 1)) pipeline = RT_PIPELINE_MEGAKERNEL;   // analytic scene: pure ALU, megakernel only
    if (batch > 1 && pipeline != RT_PIPELINE_WAVEFRONT) return fail(c, RT_ERR_STATE, "internal: a frame batch reached the megakernel");
    // EXTENSION: the hybrid scene in stages (rt_hybrid.hip) unless the megakernel was asked for; same frames bit for bit
    const bool staged = c->cfg.pipeline != RT_PIPELINE_MEGAKERNEL && fr.u.useBVH == RT_SCENE_HYBRID && fr.sc.hasBVH && !count;
    if (staged) {
        if (!c->hybrid[0]) c->hybrid[0] = rt_hybrid_create(c->cus);   // one arena for all lanes: the passes synchronise with the host anyway
        int rc = rt_hybrid_render(c->hybrid[0], c, st, c->dFrame[lane], fr, tg, std::max(c->treeDepth, 1), c->nLanes > 1 ? c->evDone[prevLane] : nullptr);
        if (rc != RT_OK) return fail(c, rc, "staged hybrid pipeline: %s", rt_hybrid_error(c->hybrid[0]));
    } else if (pipeline == RT_PIPELINE_WAVEFRONT) {
        int rc = rt_wave_render(c->wave[lane], c, st, c->dFrame[lane], fr, tg, c->dCounters, count, std::max(c->treeDepth, 1), c->nLanes > 1 ? c->evDone[prevLane] : nullptr,
                                (size_t)c->nInner * 64 + c->nWide4 * 128 + c->nPairs * 80 < ((size_t)32 << 20));
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
    HIP_TRY(c, sync_all(c));
    int rc = ensure_staging(c, bytes);
    if (rc != RT_OK) return rc;
    hipLaunchKernelGGL(k_untile, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, src, c->dStaging, c->g, ch, fmt == RT_FORMAT_F32 ? 1 : 0);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(dst, c->dStaging, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_all(c));
    return RT_OK;
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
    const size_t bytes = (size_t)c->g.W * c->g.H * 4;
    HIP_TRY(c, sync_all(c));
    int rc = ensure_staging(c, bytes);
    if (rc != RT_OK) return rc;
    rt_stage_begin(c, 11);
    HIP_TRY(c, rtl::launch_present(c->stream, c->g, c->dColor[last_lane(c)], c->dMotion[last_lane(c)], c->dGPos[last_lane(c)], c->dGNrm[last_lane(c)], *p, (uint32_t *)c->dStaging));
    rt_stage_end(c, 11, 1);
    HIP_TRY(c, hipMemcpyAsync(dst, c->dStaging, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_all(c));
    return RT_OK;
}

int rt_present_gathered(RtContext *c, const RtPresentParams *p, const void *color, const void *motion, const void *gpos, const void *gnrm, uint8_t *dst) {
    if (!c || !p || !color || !motion || !gpos || !gnrm || !dst) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_present_gathered before rt_resize");
    if ((int)p->resolution[0] != c->g.W || (int)p->resolution[1] != c->g.H) return fail(c, RT_ERR_INVALID, "rt_present_gathered: uResolution != framebuffer");
    (void)hipSetDevice(c->cfg.device);
    const size_t bytes = (size_t)c->g.W * c->g.H * 4;
    HIP_TRY(c, sync_all(c));
    int rc = ensure_staging(c, bytes);
    if (rc != RT_OK) return rc;
    rt_stage_begin(c, 11);
    HIP_TRY(c, rtl::launch_present(c->stream, c->g, (const uint2 *)color, (const uint32_t *)motion, (const uint2 *)gpos, (const uint2 *)gnrm, *p,
                                   (uint32_t *)c->dStaging, (int)c->nSlots));
    rt_stage_end(c, 11, 1);
    HIP_TRY(c, hipMemcpyAsync(dst, c->dStaging, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_all(c));
    return RT_OK;
}

int rt_history_exchange_buffer(RtContext *c, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_history_exchange_buffer before rt_resize");
    (void)hipSetDevice(c->cfg.device);
    const int lane = (c->writeIdx + c->nLanes - 1) % c->nLanes;   // the frame rendered last
    const size_t n = (size_t)c->g.world * c->nSlots * 8;
    if (!c->dHistAll[lane]) HIP_TRY(c, hipMalloc(&c->dHistAll[lane], n));
    *devPtr = c->dHistAll[lane];
    *bytes = n;
    return RT_OK;
}
int rt_history_exchanged(RtContext *c) {
    if (!c) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_history_exchanged before rt_resize");
    (void)hipSetDevice(c->cfg.device);
    const int lane = (c->writeIdx + c->nLanes - 1) % c->nLanes;
    if (!c->dHistAll[lane]) return fail(c, RT_ERR_STATE, "rt_history_exchanged without rt_history_exchange_buffer");
    // the next frame's resolve waits on this event: it now also covers the all-gather the caller enqueued on rt_stream()
    HIP_TRY(c, hipEventRecord(c->evDone[lane], c->lanes[lane]));
    c->histExchanged[lane] = true;
    return RT_OK;
}

int rt_local_target(RtContext *c, int which, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_local_target before rt_resize");
    int ch;
    void *p = target_ptr(c, which, ch);
    if (!p) return fail(c, RT_ERR_INVALID, "rt_local_target: which=%d", which);
    *devPtr = p;
    *bytes = c->nSlots * ch * 2;
    return RT_OK;
}
int rt_gather_block_bytes(const RtContext *c, int which, size_t *bytes) {
    if (!c || !bytes || !c->sized) return RT_ERR_INVALID;
    const int ch = (which == RT_TARGET_MOTION) ? 2 : 4;
    *bytes = c->nSlots * ch * 2;
    return RT_OK;
}
int rt_assemble_gathered(RtContext *c, int which, const void *gatheredDev, void *dstDev) {
    if (!c || !gatheredDev || !dstDev) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_assemble_gathered before rt_resize");
    (void)hipSetDevice(c->cfg.device);
    const int ch = (which == RT_TARGET_MOTION) ? 2 : 4;
    const size_t n = (size_t)c->g.W * c->g.H;
    hipStream_t st = api_stream(c);   // behind the gather the caller enqueued on rt_stream()
    rt_stage_begin(c, 10, st);
    hipLaunchKernelGGL(k_assemble, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, gatheredDev, dstDev, c->g, ch, c->nSlots * ch * 2);
    rt_stage_end(c, 10, 1, st);
    HIP_TRY(c, hipGetLastError());
    return RT_OK;
}
// ---- raster preview (renderRaster): the work is in rt_raster.hip; its buffers are its own, no ray target or frame state is touched
int rt_raster_mesh(RtContext *c, int slot, const float *positions, int nVerts, const uint32_t *indices, int nIdx) {
    if (!c) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    if (!c->raster) c->raster = rt_raster_create();
    const int rc = rt_raster_set_mesh(c->raster, slot, positions, nVerts, indices, nIdx);
    return rc == RT_OK ? RT_OK : fail(c, rc, "%s", rt_raster_error(c->raster));
}

int rt_render_raster(RtContext *c, const RtRasterDraw *draws, int nDraws, const float *view16, const float *proj16) {
    if (!c) return RT_ERR_INVALID;
    if (nDraws < 0 || (nDraws > 0 && !draws) || !view16 || !proj16) return fail(c, RT_ERR_INVALID, "rt_render_raster: bad arguments");
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_render_raster before rt_resize");
    if (c->g.world > 1) return fail(c, RT_ERR_UNSUPPORTED, "rt_render_raster: tile-parallel contexts (worldSize %d) do not rasterise; use a single-rank context", c->g.world);
    (void)hipSetDevice(c->cfg.device);
    if (!c->raster) c->raster = rt_raster_create();
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
    const int rc = rt_raster_render(c->raster, st, c->g.W, c->g.H, draws, nDraws, view16, proj16, c->mesh ? &dyn : nullptr);
    return rc == RT_OK ? RT_OK : fail(c, rc, "%s", rt_raster_error(c->raster));
}

int rt_raster_mesh_dynamic(RtContext *c, int slot, int mode) {
    if (!c) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    if (!c->raster) c->raster = rt_raster_create();
    const int rc = rt_raster_bind_dynamic(c->raster, slot, mode);
    return rc == RT_OK ? RT_OK : fail(c, rc, "%s", rt_raster_error(c->raster));
}

int rt_raster_part_colors(RtContext *c, int slot, const float *rgb, int nParts) {
    if (!c) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    if (!c->raster) c->raster = rt_raster_create();
    const int rc = rt_raster_set_part_colors(c->raster, slot, rgb, nParts);
    return rc == RT_OK ? RT_OK : fail(c, rc, "%s", rt_raster_error(c->raster));
}

int rt_raster_targets(RtContext *c, void **rgba8, void **primId, void **depth24, size_t *bytesEach) {
    if (!c) return RT_ERR_INVALID;
    if (rgba8) *rgba8 = nullptr;
    if (primId) *primId = nullptr;
    if (depth24) *depth24 = nullptr;
    if (bytesEach) *bytesEach = 0;
    if (!c->raster) return fail(c, RT_ERR_STATE, "rt_raster_targets before rt_render_raster");
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_raster_targets before rt_resize");
    const int rc = rt_raster_buffers(c->raster, c->g.W, c->g.H, rgba8, primId, depth24, bytesEach);
    return rc == RT_OK ? RT_OK : fail(c, rc, "%s", rt_raster_error(c->raster));
}

int rt_read_raster(RtContext *c, uint8_t *rgba8, uint32_t *primId, uint32_t *depth24) {
    if (!c) return RT_ERR_INVALID;
    if (!c->raster) return fail(c, RT_ERR_STATE, "rt_read_raster before rt_render_raster");
    (void)hipSetDevice(c->cfg.device);
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_read_raster before rt_resize");
    const int rc = rt_raster_read(c->raster, c->g.W, c->g.H, rgba8, primId, depth24);
    return rc == RT_OK ? RT_OK : fail(c, rc, "%s", rt_raster_error(c->raster));
}

int rt_debug_raster_bin_capacity(RtContext *c, uint64_t pairs) {
    if (!c) return RT_ERR_INVALID;
    if (pairs > ((uint64_t)1 << 31)) return fail(c, RT_ERR_INVALID, "rt_debug_raster_bin_capacity: %llu pairs (at most 2^31)", (unsigned long long)pairs);
    if (!c->raster) c->raster = rt_raster_create();
    rt_raster_force_bin_capacity(c->raster, (size_t)pairs);
    return RT_OK;
}

int rt_get_raster_stats(RtContext *c, RtRasterStats *out) {
    if (!c || !out) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    const int rc = rt_raster_stats(c->raster, out);
    return rc == RT_OK ? RT_OK : fail(c, rc, "%s", rt_raster_error(c->raster));
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
    unsigned long long v[16] = {0};
    (void)sync_all(c);
    for (int i = 0; i < c->nLanes; ++i) {
        unsigned long long t[16];
        int rc = rt_wave_traced(c->wave[i], c->lanes[i], t, reset != 0);
        if (rc != RT_OK) return fail(c, rc, "rt_get_traced_rays: %s", rt_wave_error(c->wave[i]));
        for (int k = 0; k < 16; ++k) v[k] += t[k];
    }
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

int rt_debug_eval(RtContext *c, int op, const float *a, const float *b, const float *cc, uint32_t *out, int n) {
    if (!c || !a || !out || n <= 0) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    float *da = nullptr, *db = nullptr, *dc = nullptr;
    uint32_t *dout = nullptr;
    const size_t bytes = (size_t)n * 4;
    HIP_TRY(c, hipMalloc(&da, bytes));
    HIP_TRY(c, hipMalloc(&dout, bytes));
    HIP_TRY(c, hipMemcpy(da, a, bytes, hipMemcpyHostToDevice));
    if (b) { HIP_TRY(c, hipMalloc(&db, bytes)); HIP_TRY(c, hipMemcpy(db, b, bytes, hipMemcpyHostToDevice)); }
    if (cc) { HIP_TRY(c, hipMalloc(&dc, bytes)); HIP_TRY(c, hipMemcpy(dc, cc, bytes, hipMemcpyHostToDevice)); }
    hipLaunchKernelGGL(k_debug_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, op, da, db, dc, dout, n);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    (void)hipFree(da); (void)hipFree(dout);
    if (db) (void)hipFree(db);
    if (dc) (void)hipFree(dc);
    return RT_OK;
}

// kinds 2 / 3: the same rays through the wavefront pipeline's traversal kernels (k_trace, as the frames launch it); kind 4: any-hit rays four at a time
// through the packet kernel (k_trace_packets), ray r of packet p = input ray 4 p + r stored at [r * n / 4 + p] as PacketSrc reads it
static int debug_trace_wave(RtContext *c, int kind, const float *origins, const float *dirs, const float *tMax, float eps, float inf, float *out7, int n) {
    if (c->nNodes <= 0 || c->nTris <= 0) return fail(c, RT_ERR_INVALID, "rt_debug_trace: no BVH uploaded");
    const bool any = kind != 2, packets = kind == 4;
    const size_t P = (size_t)n / 4;
    auto at = [&](int i) { return packets ? (size_t)(i % 4) * P + (size_t)(i / 4) : (size_t)i; };   // device address of input ray i
    std::vector<float> o4((size_t)n * 4, 0.0f), d4((size_t)n * 4, 0.0f), tm((size_t)n, inf);
    for (int i = 0; i < n; ++i) {
        const size_t a = at(i);
        std::memcpy(&o4[a * 4], origins + (size_t)i * 3, 12);
        std::memcpy(&d4[a * 4], dirs + (size_t)i * 3, 12);
        if (any) tm[a] = tMax[i];
    }
    std::vector<unsigned char> hostBytes(sizeof(DevFrame), 0);
    DevFrame *host = reinterpret_cast<DevFrame *>(hostBytes.data());
    host->u.eps = eps; host->u.inf = inf;
    host->sc = make_dev_scene(c);
    host->giBounces = 1;
    float4 *dO = nullptr, *dD = nullptr;
    float *dT = nullptr, *dOutT = nullptr;
    int *dTri = nullptr;
    uint8_t *dOcc = nullptr;
    uint32_t *dCnt = nullptr, *dHeads = nullptr;
    DevFrame *dF = nullptr;
    auto freeAll = [&]() { for (void *p : {(void *)dO, (void *)dD, (void *)dT, (void *)dOutT, (void *)dTri, (void *)dOcc, (void *)dCnt, (void *)dHeads, (void *)dF}) if (p) (void)hipFree(p); };
    bool ok = hipMalloc(&dO, (size_t)n * 16) == hipSuccess && hipMalloc(&dD, (size_t)n * 16) == hipSuccess && hipMalloc(&dT, (size_t)n * 4) == hipSuccess &&
              hipMalloc(&dOutT, (size_t)n * 4) == hipSuccess && hipMalloc(&dTri, (size_t)n * 4) == hipSuccess && hipMalloc(&dOcc, (size_t)n) == hipSuccess &&
              hipMalloc(&dCnt, 4) == hipSuccess && hipMalloc(&dHeads, rt_wave_head_words() * 4) == hipSuccess && hipMalloc(&dF, sizeof(DevFrame)) == hipSuccess;
    const uint32_t un = (uint32_t)n, live = packets ? (uint32_t)P : un;   // queue entries: rays, or packets
    ok = ok && hipMemcpy(dO, o4.data(), (size_t)n * 16, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dD, d4.data(), (size_t)n * 16, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(dT, tm.data(), (size_t)n * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dCnt, &live, 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemset(dHeads, 0, rt_wave_head_words() * 4) == hipSuccess &&   // (dOcc: cleared by the wave entries on the launch's stream; dTri: every ray stores one)
         hipMemcpy(dF, host, sizeof(DevFrame), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { freeAll(); return fail(c, RT_ERR_HIP, "rt_debug_trace: allocation / upload failed"); }
    if (host->sc.rootBox) hipLaunchKernelGGL(k_frame_root_box, dim3(1), dim3(64), 0, c->stream, dF);
    const uint32_t built = packets ? rt_wave_debug_packets(c->stream, c->cus, c->treeDepth, dF, host->sc, dO, dD, dT, dCnt, (uint32_t)P, dOcc, dHeads)
                                   : rt_wave_debug_trace(c->stream, c->cus, c->treeDepth, dF, host->sc, any, dO, dD, dT, dCnt, un, dOutT, dTri, dOcc, dHeads);
    if (!built) { (void)sync_all(c); freeAll(); return fail(c, RT_ERR_UNSUPPORTED, "rt_debug_trace: the library holds no k_trace build for the chosen options"); }
    c->debugBuilds |= built;
    std::vector<float> t((size_t)n);
    std::vector<int> tri((size_t)n);
    std::vector<uint8_t> occ((size_t)n);
    ok = hipGetLastError() == hipSuccess && sync_all(c) == hipSuccess && hipMemcpy(t.data(), dOutT, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(tri.data(), dTri, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(occ.data(), dOcc, (size_t)n, hipMemcpyDeviceToHost) == hipSuccess;
    freeAll();
    if (!ok) return fail(c, RT_ERR_HIP, "rt_debug_trace: launch failed");
    for (int i = 0; i < n; ++i) {
        float *out = out7 + (size_t)i * 7;
        for (int k = 0; k < 7; ++k) out[k] = 0.0f;
        if (any) out[0] = occ[at(i)] ? 1.0f : 0.0f;
        else { out[0] = tri[(size_t)i] >= 0 ? t[(size_t)i] : inf; out[1] = (float)tri[(size_t)i]; }   // closest: t and the triangle's index in the reference order
    }
    return RT_OK;
}

int rt_debug_trace(RtContext *c, int kind, const float *origins, const float *dirs, const float *tMax, float eps, float inf, float *out7, int n) {
    if (!c || !origins || !dirs || !out7 || n <= 0 || ((kind == 1 || kind >= 3) && !tMax) || kind < 0 || kind > 4 || (kind == 4 && n % 4 != 0)) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    if (kind >= 2) return guarded(c, "rt_debug_trace", [&]() -> int { return debug_trace_wave(c, kind, origins, dirs, tMax, eps, inf, out7, n); });
    float *dO = nullptr, *dD = nullptr, *dT = nullptr, *dOut = nullptr;
    HIP_TRY(c, hipMalloc(&dO, (size_t)n * 12));
    HIP_TRY(c, hipMalloc(&dD, (size_t)n * 12));
    HIP_TRY(c, hipMalloc(&dT, (size_t)n * 4));
    HIP_TRY(c, hipMalloc(&dOut, (size_t)n * 28));
    HIP_TRY(c, hipMemcpy(dO, origins, (size_t)n * 12, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(dD, dirs, (size_t)n * 12, hipMemcpyHostToDevice));
    if (tMax) HIP_TRY(c, hipMemcpy(dT, tMax, (size_t)n * 4, hipMemcpyHostToDevice));
    DevScene sc = make_dev_scene(c);
    hipLaunchKernelGGL(k_debug_trace, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, sc, kind, dO, dD, dT, eps, inf, dOut, n);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(out7, dOut, (size_t)n * 28, hipMemcpyDeviceToHost));
    (void)hipFree(dO); (void)hipFree(dD); (void)hipFree(dT); (void)hipFree(dOut);
    return RT_OK;
}

// ---- ray queries: user rays through the frames' persistent traversal launch; reads the BVH, touches no frame state
static int query_args(RtContext *c, const char *what, int kind, const float *origins, int originStride, const float *dirs, int dirStride, const float *tMax, int n,
                      const RtHit *hits, const uint8_t *occluded) {
    if (kind != RT_QUERY_CLOSEST && kind != RT_QUERY_ANY) return fail(c, RT_ERR_INVALID, "%s: kind %d (RT_QUERY_CLOSEST or RT_QUERY_ANY)", what, kind);
    if (n < 0) return fail(c, RT_ERR_INVALID, "%s: n = %d", what, n);
    if (originStride < 3 || dirStride < 3) return fail(c, RT_ERR_INVALID, "%s: strides %d / %d floats (at least 3)", what, originStride, dirStride);
    if (n > 0 && (!origins || !dirs)) return fail(c, RT_ERR_INVALID, "%s: null ray arrays", what);
    if (kind == RT_QUERY_ANY && !tMax) return fail(c, RT_ERR_INVALID, "%s: any-hit queries need tMax", what);
    if (n > 0 && kind == RT_QUERY_CLOSEST && !hits) return fail(c, RT_ERR_INVALID, "%s: closest-hit queries need hits", what);
    if (n > 0 && kind == RT_QUERY_ANY && !occluded) return fail(c, RT_ERR_INVALID, "%s: any-hit queries need occluded", what);
    if ((size_t)(n > 0 ? n - 1 : 0) * (size_t)std::max(originStride, dirStride) + 3 > ((size_t)1 << 32))
        return fail(c, RT_ERR_INVALID, "%s: the ray arrays exceed 2^32 floats", what);
    if (c->nNodes <= 0 || c->nTris <= 0) return fail(c, RT_ERR_STATE, "%s: no BVH uploaded", what);
    return RT_OK;
}

// The query scratch (allocated on the first query) and rt_stream()'s stream, which first waits for the previous query if that ran on another stream
static int query_begin(RtContext *c, hipStream_t &st) {
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
static int query_end(RtContext *c, hipStream_t st) {
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->queryDone, st));
    c->queryStream = st;
    return RT_OK;
}

int rt_trace_rays(RtContext *c, int kind, const float *origins, int originStride, const float *dirs, int dirStride, const float *tMax, float eps, float inf, int n,
                  RtHit *hits, float *normals, uint8_t *occluded) {
    if (!c) return RT_ERR_INVALID;
    const int rc = query_args(c, "rt_trace_rays", kind, origins, originStride, dirs, dirStride, tMax, n, hits, occluded);
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
    const int rc = query_args(c, "rt_trace_rays_host", kind, origins, originStride, dirs, dirStride, tMax, n, hits, occluded);
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

// ---- scene queries and pixel picking: the analytic leg (rt_scene_query.hip) into the caller's outputs, then the mesh leg through the frames'
// persistent traversal launch (SceneSrc).  Shares rt_trace_rays' scratch; touches no frame state.
// xy != null: pixel rays (rt_pick_pixels), else origins / dirs.  Checks everything before any device work; `mesh` = the scene has a mesh leg.
static int scene_query_args(RtContext *c, const char *what, const RtUniforms *u, int kind, int flags, const float *origins, int originStride, const float *dirs,
                            int dirStride, const int32_t *xy, const float *tMax, int n, const RtHit *hits, const uint8_t *occluded, bool &mesh) {
    if (!u) return fail(c, RT_ERR_INVALID, "%s: null uniforms", what);
    if (kind != RT_QUERY_CLOSEST && kind != RT_QUERY_ANY) return fail(c, RT_ERR_INVALID, "%s: kind %d (RT_QUERY_CLOSEST or RT_QUERY_ANY)", what, kind);
    if (flags & ~(RT_QUERY_SKIP_GLASS | RT_QUERY_SKIP_MARKER)) return fail(c, RT_ERR_INVALID, "%s: flags 0x%x (RT_QUERY_SKIP_*)", what, flags);
    if (n < 0) return fail(c, RT_ERR_INVALID, "%s: n = %d", what, n);
    if (xy) {
        if ((size_t)n * 2 > ((size_t)1 << 32)) return fail(c, RT_ERR_INVALID, "%s: the pixel array exceeds 2^32 entries", what);
    } else {
        if (originStride < 3 || dirStride < 3) return fail(c, RT_ERR_INVALID, "%s: strides %d / %d floats (at least 3)", what, originStride, dirStride);
        if (n > 0 && (!origins || !dirs)) return fail(c, RT_ERR_INVALID, "%s: null ray arrays", what);
        if ((size_t)(n > 0 ? n - 1 : 0) * (size_t)std::max(originStride, dirStride) + 3 > ((size_t)1 << 32))
            return fail(c, RT_ERR_INVALID, "%s: the ray arrays exceed 2^32 floats", what);
    }
    if (kind == RT_QUERY_ANY && !tMax) return fail(c, RT_ERR_INVALID, "%s: any-hit queries need tMax", what);
    if (n > 0 && kind == RT_QUERY_CLOSEST && !hits) return fail(c, RT_ERR_INVALID, "%s: closest-hit queries need hits", what);
    if (n > 0 && kind == RT_QUERY_ANY && !occluded) return fail(c, RT_ERR_INVALID, "%s: any-hit queries need occluded", what);
    // the mesh as render_frames_impl sees it
    const bool meshMode = u->useBVH == 1 || u->useBVH == RT_SCENE_HYBRID;
    mesh = meshMode && u->nodeCount > 0 && u->triCount > 0;
    if (mesh && (c->nNodes == 0 || u->nodeCount > c->nNodes || u->triCount > c->nTris))
        return fail(c, RT_ERR_STATE, "%s: uniforms name %d nodes / %d tris, uploaded %d / %d", what, u->nodeCount, u->triCount, c->nNodes, c->nTris);
    return RT_OK;
}

static int scene_query(RtContext *c, const char *what, const RtUniforms *u, int kind, int flags, const float *origins, int originStride, const float *dirs, int dirStride,
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

// host arrays: staged through the context's buffer (origins | dirs | xy | tMax | hits / occluded | objects | normals | points; the ray arrays keep their
// strides), then synchronised
static int scene_query_host(RtContext *c, const char *what, const RtUniforms *u, int kind, int flags, const float *origins, int originStride, const float *dirs,
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

int rt_debug_bounce_probe(RtContext *c, RtBounceProbe *out, int reset) {
    if (!c || !out) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    unsigned long long v[4] = {0, 0, 0, 0};
    for (int i = 0; i < c->nLanes; ++i) {
        unsigned long long t[4];
        int rc = rt_wave_bounce_probe(c->wave[i], c->lanes[i], t, reset != 0);
        if (rc != RT_OK) return fail(c, rc, "rt_debug_bounce_probe: %s", rt_wave_error(c->wave[i]));
        for (int k = 0; k < 4; ++k) v[k] += t[k];
    }
    out->probed = v[0]; out->retraced = v[1]; out->probeLaunches = v[2]; out->closestLaunches = v[3];
    return RT_OK;
}

int rt_debug_disk_skip(RtContext *c, RtDiskSkip *out, int reset) {
    if (!c || !out) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    unsigned long long v[10] = {};
    for (int i = 0; i < c->nLanes; ++i) {
        unsigned long long t[10];
        int rc = rt_wave_disk_skip(c->wave[i], c->lanes[i], t, reset != 0);
        if (rc != RT_OK) return fail(c, rc, "rt_debug_disk_skip: %s", rt_wave_error(c->wave[i]));
        for (int k = 0; k < 10; ++k) v[k] += t[k];
    }
    out->directPairs = v[0]; out->directUnlit = v[1]; out->directSkipped = v[2]; out->directWaves = v[3]; out->directWavesSkipped = v[4];
    out->giPairs = v[5]; out->giUnlit = v[6]; out->giSkipped = v[7]; out->giWaves = v[8]; out->giWavesSkipped = v[9];
    return RT_OK;
}

int rt_debug_gi_list(RtContext *c, RtGiList *out, int reset) {
    if (!c || !out) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    unsigned long long v[4] = {0, 0, 0, 0};
    for (int i = 0; i < c->nLanes; ++i) {
        unsigned long long t[4];
        int rc = rt_wave_gi_list(c->wave[i], c->lanes[i], t, reset != 0);
        if (rc != RT_OK) return fail(c, rc, "rt_debug_gi_list: %s", rt_wave_error(c->wave[i]));
        for (int k = 0; k < 4; ++k) v[k] += t[k];
    }
    out->visited = v[0]; out->shaded = v[1]; out->listedLaunches = v[2]; out->pairLaunches = v[3];
    return RT_OK;
}

int rt_debug_disk_unlit(RtContext *c, const RtUniforms *u, const float *hp, const float *normals, int n, int seeds, uint8_t *flags, float *maxDot) {
    if (!c || !u || !hp || !normals || !flags || !maxDot || n <= 0 || seeds <= 0) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    float *dP = nullptr, *dN = nullptr, *dM = nullptr;
    uint8_t *dF = nullptr;
    auto freeAll = [&]() { for (void *p : {(void *)dP, (void *)dN, (void *)dM, (void *)dF}) if (p) (void)hipFree(p); };
    const size_t b3 = (size_t)n * 12;
    bool ok = hipMalloc(&dP, b3) == hipSuccess && hipMalloc(&dN, b3) == hipSuccess && hipMalloc(&dM, (size_t)n * 4) == hipSuccess && hipMalloc(&dF, (size_t)n) == hipSuccess &&
              hipMemcpy(dP, hp, b3, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dN, normals, b3, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { freeAll(); return fail(c, RT_ERR_HIP, "rt_debug_disk_unlit: allocation / upload failed"); }
    hipLaunchKernelGGL(k_debug_disk_unlit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, *u, dP, dN, n, seeds, dF, dM);
    ok = hipGetLastError() == hipSuccess && sync_all(c) == hipSuccess && hipMemcpy(flags, dF, (size_t)n, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(maxDot, dM, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    freeAll();
    if (!ok) return fail(c, RT_ERR_HIP, "rt_debug_disk_unlit: launch failed");
    return RT_OK;
}

int rt_debug_builds(RtContext *c, uint32_t *out, int reset) {
    if (!c || !out) return RT_ERR_INVALID;
    uint32_t b = c->debugBuilds;
    for (int i = 0; i < RT_MAX_LANES; ++i) b |= rt_wave_builds(c->wave[i], reset != 0);
    if (reset) c->debugBuilds = 0;
    *out = b;
    return RT_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Tile-parallel exchange over RCCL, owned by the library.  librccl is half a gigabyte and only multi-GPU
// runs need it, so it is bound on first use: an already loaded copy (e.g. the one a PyTorch wheel brought into the process) is
// reused by SONAME, otherwise librccl.so.1 is loaded from the ROCm installation.
namespace {
struct RcclApi {
    decltype(&ncclGetUniqueId) getUniqueId = nullptr;
    decltype(&ncclCommInitRank) commInitRank = nullptr;
    decltype(&ncclCommDestroy) commDestroy = nullptr;
    decltype(&ncclGroupStart) groupStart = nullptr;
    decltype(&ncclGroupEnd) groupEnd = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclAllGather) allGather = nullptr;
    decltype(&ncclGetErrorString) errorString = nullptr;
    decltype(&ncclCommCount) commCount = nullptr;          // optional (rt_comm_info)
    decltype(&ncclCommUserRank) commUserRank = nullptr;
    std::string err;
    bool ok = false;
};
static void rccl_bind(RcclApi &a);
RcclApi &rccl_api() {
    static RcclApi a;
    static std::once_flag once;              // contexts on different threads may reach their first rt_comm_* call together
    std::call_once(once, [] { rccl_bind(a); });
    return a;
}
static void rccl_bind(RcclApi &a) {
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) { const char *e = dlerror(); a.err = std::string("librccl.so.1 could not be loaded: ") + (e ? e : "?"); return; }
#define RT_BIND(field, name) do { a.field = (decltype(a.field))dlsym(h, #name); if (!a.field) { a.err = "librccl lacks " #name; return; } } while (0)
    RT_BIND(getUniqueId, ncclGetUniqueId); RT_BIND(commInitRank, ncclCommInitRank); RT_BIND(commDestroy, ncclCommDestroy);
    RT_BIND(groupStart, ncclGroupStart); RT_BIND(groupEnd, ncclGroupEnd); RT_BIND(send, ncclSend); RT_BIND(recv, ncclRecv);
    RT_BIND(allGather, ncclAllGather); RT_BIND(errorString, ncclGetErrorString);
#undef RT_BIND
    a.commCount = (decltype(a.commCount))dlsym(h, "ncclCommCount");
    a.commUserRank = (decltype(a.commUserRank))dlsym(h, "ncclCommUserRank");
    a.ok = true;
}
#define NCCL_TRY(c, expr)                                                                                           \
    do {                                                                                                            \
        ncclResult_t r_ = (expr);                                                                                   \
        if (r_ != ncclSuccess) return fail((c), RT_ERR_HIP, "%s failed: %s", #expr, rccl_api().errorString(r_));     \
    } while (0)
void *lane_target(RtContext *c, int lane, int which, int &ch) {
    switch (which) {
        case RT_TARGET_COLOR: ch = 4; return c->dColor[lane];
        case RT_TARGET_MOTION: ch = 2; return c->dMotion[lane];
        case RT_TARGET_GPOS: ch = 4; return c->dGPos[lane];
        case RT_TARGET_GNRM: ch = 4; return c->dGNrm[lane];
        default: ch = 0; return nullptr;
    }
}
}  // namespace

extern "C" {

int rt_comm_unique_id(void *id, size_t bytes) {
    if (!id || bytes < RT_COMM_ID_BYTES) return fail(nullptr, RT_ERR_INVALID, "rt_comm_unique_id: need %d bytes", RT_COMM_ID_BYTES);
    RcclApi &a = rccl_api();
    if (!a.ok) return fail(nullptr, RT_ERR_UNSUPPORTED, "rt_comm_unique_id: %s", a.err.c_str());
    static_assert(sizeof(ncclUniqueId) == RT_COMM_ID_BYTES, "RT_COMM_ID_BYTES");
    ncclUniqueId u;
    ncclResult_t r = a.getUniqueId(&u);
    if (r != ncclSuccess) return fail(nullptr, RT_ERR_HIP, "ncclGetUniqueId: %s", a.errorString(r));
    std::memcpy(id, &u, sizeof u);
    return RT_OK;
}

int rt_comm_init(RtContext *c, const void *id, size_t bytes) {
    if (!c || !id || bytes < RT_COMM_ID_BYTES) return RT_ERR_INVALID;
    if (c->comm) return fail(c, RT_ERR_STATE, "rt_comm_init: the context already has a communicator");
    RcclApi &a = rccl_api();
    if (!a.ok) return fail(c, RT_ERR_UNSUPPORTED, "rt_comm_init: %s", a.err.c_str());
    (void)hipSetDevice(c->cfg.device);
    HIP_TRY(c, sync_all(c));
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    ncclComm_t comm = nullptr;
    NCCL_TRY(c, a.commInitRank(&comm, c->cfg.worldSize, u, c->cfg.rank));   // collective over all ranks of the frame
    c->comm = (void *)comm;
    // the gathering rank's COLOR0 buffers for every frame lane now, not inside the frame loop (a first-gather hipMalloc would otherwise land in
    // whatever is being timed; the other targets are gathered for a present only and keep allocating on first use)
    if (c->sized && c->g.rank == 0) {
        const size_t block = c->nSlots * 8;
        for (int l = 0; l < c->nLanes; ++l) {
            if (!c->dGathered[l][RT_TARGET_COLOR]) HIP_TRY(c, hipMalloc(&c->dGathered[l][RT_TARGET_COLOR], block * (size_t)c->g.world));
            if (!c->dAssembled[l][RT_TARGET_COLOR]) HIP_TRY(c, hipMalloc(&c->dAssembled[l][RT_TARGET_COLOR], (size_t)c->g.W * c->g.H * 8));
        }
    }
    return RT_OK;
}

int rt_comm_destroy(RtContext *c) {
    if (!c) return RT_ERR_INVALID;
    if (!c->comm) return RT_OK;
    (void)hipSetDevice(c->cfg.device);
    (void)sync_all(c);
    ncclResult_t r = rccl_api().commDestroy((ncclComm_t)c->comm);
    c->comm = nullptr;
    if (r != ncclSuccess) return fail(c, RT_ERR_HIP, "ncclCommDestroy: %s", rccl_api().errorString(r));
    return RT_OK;
}

// One exchange per gathered frame: every rank sends the block of its tiles to rank 0 -- grouped point-to-point
// transfers, so the root's inbound xGMI links run in parallel and nothing is reduced -- and rank 0 un-tiles the blocks into a
// row-major frame.  Everything is enqueued on the lane (stream) of the frame rendered last and uses that lane's own buffers, so
// gathers of consecutive frames overlap like the frames themselves and never share a buffer.
int rt_gather_frame(RtContext *c, int which) {
    if (!c) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_gather_frame before rt_resize");
    if (c->frameIndex == 0) return fail(c, RT_ERR_STATE, "rt_gather_frame before the first frame");
    if (c->g.world > 1 && !c->comm) return fail(c, RT_ERR_STATE, "rt_gather_frame on a tile-parallel context without rt_comm_init");
    (void)hipSetDevice(c->cfg.device);
    const int lane = last_lane(c);
    int ch;
    void *local = lane_target(c, lane, which, ch);
    if (!local) return fail(c, RT_ERR_INVALID, "rt_gather_frame: which=%d", which);
    const size_t block = c->nSlots * (size_t)ch * 2;
    hipStream_t st = c->lanes[lane];
    const bool root = c->g.rank == 0;
    if (root) {
        if (!c->dGathered[lane][which]) HIP_TRY(c, hipMalloc(&c->dGathered[lane][which], block * (size_t)c->g.world));
        if (!c->dAssembled[lane][which]) HIP_TRY(c, hipMalloc(&c->dAssembled[lane][which], (size_t)c->g.W * c->g.H * ch * 2));
    }
    // stage "gather": from the point the lane's stream reaches the exchange (its frame is done) to the end of the un-tiling on the root / of
    // the send on the others -- on the root this is what the first 8-GPU run needs to see next to the ranks' frame times (bench.py)
    struct GatherSpan {
        RtContext *c; hipStream_t st;
        GatherSpan(RtContext *c_, hipStream_t s_) : c(c_), st(s_) { rt_stage_begin(c, 12, st); }
        ~GatherSpan() { rt_stage_end(c, 12, 1, st); }
    } span(c, st);
    c->gathers++;
    c->gatherBytes += root ? block * (size_t)(c->g.world - 1) : block;
    if (root) HIP_TRY(c, hipMemcpyAsync(c->dGathered[lane][which], local, block, hipMemcpyDeviceToDevice, st));
    if (c->g.world > 1) {
        RcclApi &a = rccl_api();
        ncclComm_t comm = (ncclComm_t)c->comm;
        NCCL_TRY(c, a.groupStart());
        // a failing send / recv must not leave the communicator inside an open group (later collectives and ncclCommDestroy would
        // hang): close the group first, then report the first error
        ncclResult_t r1 = ncclSuccess;
        if (root) {
            for (int r = 1; r < c->g.world && r1 == ncclSuccess; ++r)
                r1 = a.recv((char *)c->dGathered[lane][which] + (size_t)r * block, block, ncclUint8, r, comm, st);
        } else {
            r1 = a.send(local, block, ncclUint8, 0, comm, st);
        }
        const ncclResult_t r2 = a.groupEnd();
        if (r1 != ncclSuccess) return fail(c, RT_ERR_HIP, "ncclSend/ncclRecv failed: %s", a.errorString(r1));
        if (r2 != ncclSuccess) return fail(c, RT_ERR_HIP, "ncclGroupEnd failed: %s", a.errorString(r2));
    }
    if (root) {
        const size_t n = (size_t)c->g.W * c->g.H;
        rt_stage_begin(c, 10, st);
        hipLaunchKernelGGL(k_assemble, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const void *)c->dGathered[lane][which],
                           c->dAssembled[lane][which], c->g, ch, block);
        rt_stage_end(c, 10, 1, st);
        HIP_TRY(c, hipGetLastError());
    }
    c->gatheredLane[which] = lane;
    return RT_OK;
}

int rt_gathered_frame(RtContext *c, int which, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes || which < 0 || which > 3) return RT_ERR_INVALID;
    if (c->g.rank != 0) return fail(c, RT_ERR_STATE, "rt_gathered_frame: only rank 0 holds the gathered frame");
    const int lane = c->gatheredLane[which];
    if (lane < 0 || !c->dAssembled[lane][which]) return fail(c, RT_ERR_STATE, "rt_gathered_frame: no rt_gather_frame(%d) since the last reset", which);
    *devPtr = c->dAssembled[lane][which];
    *bytes = (size_t)c->g.W * c->g.H * (which == RT_TARGET_MOTION ? 2 : 4) * 2;
    return RT_OK;
}

int rt_read_gathered(RtContext *c, int which, void *dstHalfs) {
    if (!c || !dstHalfs) return RT_ERR_INVALID;
    void *p;
    size_t n;
    int rc = rt_gathered_frame(c, which, &p, &n);
    if (rc != RT_OK) return rc;
    (void)hipSetDevice(c->cfg.device);
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(dstHalfs, p, n, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_present_last_gathered(RtContext *c, const RtPresentParams *p, uint8_t *dst) {
    if (!c || !p || !dst) return RT_ERR_INVALID;
    if (c->g.rank != 0) return fail(c, RT_ERR_STATE, "rt_present_last_gathered: only rank 0 holds the gathered targets");
    const int lane = c->gatheredLane[0];
    for (int w = 0; w < 4; ++w)
        if (c->gatheredLane[w] < 0 || c->gatheredLane[w] != lane || !c->dGathered[lane][w])
            return fail(c, RT_ERR_STATE, "rt_present_last_gathered: gather all four targets of the same frame first (rt_gather_frame 0..3)");
    return rt_present_gathered(c, p, c->dGathered[lane][0], c->dGathered[lane][1], c->dGathered[lane][2], c->dGathered[lane][3], dst);
}

// Moving camera on a tile-parallel frame: every rank needs the whole previous COLOR0 (rt_taa.glsl:116-179 reads it at arbitrary
// pixels) -> one all-gather of the ranks' blocks into this lane's exchange buffer, then the event the next frame's resolve waits on.
int rt_exchange_history(RtContext *c) {
    if (!c) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_exchange_history before rt_resize");
    if (c->g.world > 1 && !c->comm) return fail(c, RT_ERR_STATE, "rt_exchange_history on a tile-parallel context without rt_comm_init");
    void *buf;
    size_t bytes;
    int rc = rt_history_exchange_buffer(c, &buf, &bytes);
    if (rc != RT_OK) return rc;
    const int lane = last_lane(c);
    const size_t block = c->nSlots * 8;
    if (c->g.world > 1) NCCL_TRY(c, rccl_api().allGather(c->dColor[lane], buf, block, ncclUint8, (ncclComm_t)c->comm, c->lanes[lane]));
    else HIP_TRY(c, hipMemcpyAsync(buf, c->dColor[lane], block, hipMemcpyDeviceToDevice, c->lanes[lane]));
    c->historyExchanges++;
    return rt_history_exchanged(c);
}

int rt_comm_info(RtContext *c, RtCommInfo *out) {
    if (!c || !out) return RT_ERR_INVALID;
    out->commWorld = out->commRank = -1;
    out->rank = c->cfg.rank; out->worldSize = c->cfg.worldSize;
    out->gathers = c->gathers; out->gatherBytes = c->gatherBytes; out->historyExchanges = c->historyExchanges;
    if (c->comm) {
        RcclApi &a = rccl_api();
        int v = -1;
        if (a.commCount && a.commCount((ncclComm_t)c->comm, &v) == ncclSuccess) out->commWorld = v;
        v = -1;
        if (a.commUserRank && a.commUserRank((ncclComm_t)c->comm, &v) == ncclSuccess) out->commRank = v;
    }
    return RT_OK;
}

}  // extern "C"
