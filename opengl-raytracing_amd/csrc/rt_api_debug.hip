// rt_api_debug.hip -- the rt_debug_* part of the C ABI (include/rt_mi355.h): what the tests ask of the library beyond rendering.  Device
// functions evaluated one by one (k_debug_eval, k_debug_disk_unlit), rays through the traversal code outside a frame (k_debug_trace and the wave
// entries), the lane-summed probes, the scene arrays as uploaded and as packed, and host arithmetic that needs no context.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "rt_batch_order.hpp"
#include "rt_context.hpp"
#include "rt_scene_pack.hpp"
#include "rt_wave_plan.hpp"

using namespace rtd;
using namespace rtapi;

namespace {

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

// The device buffers of one debug call: freed when the call returns, whichever way it does.  After a failed get the later ones do nothing, so a call
// asks for all its buffers and then looks at status() once.
struct DevBufs {
    void *p[9] = {};   // (the most a call needs: debug_trace_wave)
    int n = 0;
    hipError_t err = hipSuccess;   // of the first get that failed
    DevBufs() = default; DevBufs(const DevBufs &) = delete;
    ~DevBufs() { for (int i = 0; i < n; ++i) (void)hipFree(p[i]); }
    // `bytes` of device memory, filled from `src` when there is one
    template <class T> T *get(size_t bytes, const void *src = nullptr) {
        if (err == hipSuccess) err = n < 9 ? hipMalloc(&p[n], bytes) : hipErrorOutOfMemory;
        if (err != hipSuccess) return nullptr;
        T *d = (T *)p[n++];
        if (src) err = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
        return d;
    }
    hipError_t status() const { return err; }
};

// kinds 2 / 3: the same rays through the wavefront pipeline's traversal kernels (k_trace, as the frames launch it); kind 4: any-hit rays four at a time
// through the packet kernel (k_trace_packets), ray r of packet p = input ray 4 p + r stored at [r * n / 4 + p] as PacketSrc reads it
int debug_trace_wave(RtContext *c, int kind, const float *origins, const float *dirs, const float *tMax, float eps, float inf, float *out7, int n) {
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
    const uint32_t un = (uint32_t)n, live = packets ? (uint32_t)P : un;   // queue entries: rays, or packets
    DevBufs bufs;
    float4 *dO = bufs.get<float4>((size_t)n * 16, o4.data()), *dD = bufs.get<float4>((size_t)n * 16, d4.data());
    float *dT = bufs.get<float>((size_t)n * 4, tm.data()), *dOutT = bufs.get<float>((size_t)n * 4);
    int *dTri = bufs.get<int>((size_t)n * 4);         // (every ray stores one)
    uint8_t *dOcc = bufs.get<uint8_t>((size_t)n);     // (cleared by the wave entries on the launch's stream)
    uint32_t *dCnt = bufs.get<uint32_t>(4, &live), *dHeads = bufs.get<uint32_t>(rt_wave_head_words() * 4);
    DevFrame *dF = bufs.get<DevFrame>(sizeof(DevFrame), host);
    if (bufs.status() != hipSuccess || hipMemset(dHeads, 0, rt_wave_head_words() * 4) != hipSuccess) return fail(c, RT_ERR_HIP, "rt_debug_trace: allocation / upload failed");
    if (host->sc.rootBox) launch_frame_root_box(c->stream, dF);
    const uint32_t built = packets ? rt_wave_debug_packets(c->stream, c->cus, c->treeDepth, dF, host->sc, dO, dD, dT, dCnt, (uint32_t)P, dOcc, dHeads)
                                   : rt_wave_debug_trace(c->stream, c->cus, c->treeDepth, dF, host->sc, any, dO, dD, dT, dCnt, un, dOutT, dTri, dOcc, dHeads);
    if (!built) { (void)sync_all(c); return fail(c, RT_ERR_UNSUPPORTED, "rt_debug_trace: the library holds no k_trace build for the chosen options"); }
    c->debugBuilds |= built;
    std::vector<float> t((size_t)n);
    std::vector<int> tri((size_t)n);
    std::vector<uint8_t> occ((size_t)n);
    if (hipGetLastError() != hipSuccess || sync_all(c) != hipSuccess || hipMemcpy(t.data(), dOutT, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(tri.data(), dTri, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(occ.data(), dOcc, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(c, RT_ERR_HIP, "rt_debug_trace: launch failed");
    for (int i = 0; i < n; ++i) {
        float *out = out7 + (size_t)i * 7;
        for (int k = 0; k < 7; ++k) out[k] = 0.0f;
        if (any) out[0] = occ[at(i)] ? 1.0f : 0.0f;
        else { out[0] = tri[(size_t)i] >= 0 ? t[(size_t)i] : inf; out[1] = (float)tri[(size_t)i]; }   // closest: t and the triangle's index in the reference order
    }
    return RT_OK;
}

// The three probes: each record (rt_mi355.h) is the words rt_wave_*'s entry hands out, in their order, summed over the lanes
template <class T, class F> int lane_sum_record(RtContext *c, const char *what, F fn, T *out, int reset) {
    static_assert(sizeof(T) % sizeof(uint64_t) == 0 && sizeof(uint64_t) == sizeof(unsigned long long), "a record of 64-bit counts");
    if (!c || !out) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    unsigned long long v[sizeof(T) / sizeof(uint64_t)];
    const int rc = sum_over_lanes(c, what, fn, reset, v);
    if (rc == RT_OK) std::memcpy(out, v, sizeof v);
    return rc;
}

}  // namespace

extern "C" {

int rt_debug_eval(RtContext *c, int op, const float *a, const float *b, const float *cc, uint32_t *out, int n) {
    if (!c || !a || !out || n <= 0) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    const size_t bytes = (size_t)n * 4;
    DevBufs bufs;
    float *da = bufs.get<float>(bytes, a), *db = b ? bufs.get<float>(bytes, b) : nullptr, *dc = cc ? bufs.get<float>(bytes, cc) : nullptr;
    uint32_t *dout = bufs.get<uint32_t>(bytes);
    HIP_TRY(c, bufs.status());
    hipLaunchKernelGGL(k_debug_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, op, da, db, dc, dout, n);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_debug_trace(RtContext *c, int kind, const float *origins, const float *dirs, const float *tMax, float eps, float inf, float *out7, int n) {
    if (!c || !origins || !dirs || !out7 || n <= 0 || ((kind == 1 || kind >= 3) && !tMax) || kind < 0 || kind > 4 || (kind == 4 && n % 4 != 0)) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    if (kind >= 2) return guarded(c, "rt_debug_trace", [&]() -> int { return debug_trace_wave(c, kind, origins, dirs, tMax, eps, inf, out7, n); });
    DevBufs bufs;
    float *dO = bufs.get<float>((size_t)n * 12, origins), *dD = bufs.get<float>((size_t)n * 12, dirs), *dT = bufs.get<float>((size_t)n * 4, tMax),
          *dOut = bufs.get<float>((size_t)n * 28);
    HIP_TRY(c, bufs.status());
    DevScene sc = make_dev_scene(c);
    hipLaunchKernelGGL(k_debug_trace, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, sc, kind, dO, dD, dT, eps, inf, dOut, n);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(out7, dOut, (size_t)n * 28, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_debug_disk_unlit(RtContext *c, const RtUniforms *u, const float *hp, const float *normals, int n, int seeds, uint8_t *flags, float *maxDot) {
    if (!c || !u || !hp || !normals || !flags || !maxDot || n <= 0 || seeds <= 0) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    DevBufs bufs;
    float *dP = bufs.get<float>((size_t)n * 12, hp), *dN = bufs.get<float>((size_t)n * 12, normals), *dM = bufs.get<float>((size_t)n * 4);
    uint8_t *dF = bufs.get<uint8_t>((size_t)n);
    if (bufs.status() != hipSuccess) return fail(c, RT_ERR_HIP, "rt_debug_disk_unlit: allocation / upload failed");
    hipLaunchKernelGGL(k_debug_disk_unlit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, *u, dP, dN, n, seeds, dF, dM);
    if (hipGetLastError() != hipSuccess || sync_all(c) != hipSuccess || hipMemcpy(flags, dF, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(maxDot, dM, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(c, RT_ERR_HIP, "rt_debug_disk_unlit: launch failed");
    return RT_OK;
}

int rt_debug_bounce_probe(RtContext *c, RtBounceProbe *out, int reset) { return lane_sum_record(c, "rt_debug_bounce_probe", rt_wave_bounce_probe, out, reset); }
int rt_debug_disk_skip(RtContext *c, RtDiskSkip *out, int reset) { return lane_sum_record(c, "rt_debug_disk_skip", rt_wave_disk_skip, out, reset); }
int rt_debug_gi_list(RtContext *c, RtGiList *out, int reset) { return lane_sum_record(c, "rt_debug_gi_list", rt_wave_gi_list, out, reset); }
int rt_debug_light_masks(RtContext *c, RtLightMasks *out, int reset) { return lane_sum_record(c, "rt_debug_light_masks", rt_wave_light_masks, out, reset); }
int rt_debug_beam_cull_stats(RtContext *c, RtBeamCullStats *out, int reset) { return lane_sum_record(c, "rt_debug_beam_cull_stats", rt_wave_beam_cull, out, reset); }
// the flags of the lane that rendered last
int rt_debug_beam_cull_flags(RtContext *c, uint8_t *out, int nLocalTiles) {
    if (!c || !out || nLocalTiles <= 0) return RT_ERR_INVALID;
    (void)hipSetDevice(c->cfg.device);
    const int lane = last_lane(c);
    const int rc = rt_wave_beam_read(c->wave[lane], c->lanes[lane], out, (size_t)nLocalTiles);
    return rc == RT_OK ? RT_OK : fail(c, rc, "rt_debug_beam_cull_flags: %s", rt_wave_error(c->wave[lane]));
}

int rt_debug_builds(RtContext *c, uint32_t *out, int reset) {
    if (!c || !out) return RT_ERR_INVALID;
    uint32_t b = c->debugBuilds;
    for (int i = 0; i < RT_MAX_LANES; ++i) b |= rt_wave_builds(c->wave[i], reset != 0);
    if (reset) c->debugBuilds = 0;
    *out = b;
    return RT_OK;
}

int rt_debug_raster_bin_capacity(RtContext *c, uint64_t pairs) {
    if (!c) return RT_ERR_INVALID;
    if (pairs > ((uint64_t)1 << 31)) return fail(c, RT_ERR_INVALID, "rt_debug_raster_bin_capacity: %llu pairs (at most 2^31)", (unsigned long long)pairs);
    if (!c->raster) c->raster = rt_raster_create();
    rt_raster_force_bin_capacity(c->raster, (size_t)pairs);
    return RT_OK;
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

// ---- host arithmetic the device code shares (rt_frame.hpp, rt_device_math.hpp): no context, no device
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

int rt_debug_batch_tiles(int batch, int nLocalTiles, int32_t *out) {
    if (!out || batch < 1 || batch > RT_MAX_BATCH || nLocalTiles < 0) return RT_ERR_INVALID;
    for (int v = 0; v < batch * nLocalTiles; ++v) out[v] = batch_tile_of_virtual(v, batch, nLocalTiles);
    return RT_OK;
}
int rt_debug_batch_order(const uint64_t *ballots, int n, int waves, uint32_t *out) {
    if (!ballots || !out || n < 1 || n > 32 || waves < 1) return RT_ERR_INVALID;
    const unsigned long long *m = reinterpret_cast<const unsigned long long *>(ballots);
    uint32_t waveBase = 0;   // the items of lower waves (InterleavedAppend::commit)
    for (int w = 0; w < waves; ++w) {
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t start = waveBase + interleaved_lane_start(m + w, waves, n, lane), bits = interleaved_lane_bits(m + w, waves, n, lane);
            for (int k = 0; k < n; ++k) out[((size_t)k * waves + w) * 64 + lane] = (bits >> k) & 1u ? interleaved_index(start, bits, k) : 0xffffffffu;
        }
        for (int k = 0; k < n; ++k) waveBase += (uint32_t)__builtin_popcountll(m[(size_t)k * waves + w]);
    }
    return RT_OK;
}
}  // extern "C"
