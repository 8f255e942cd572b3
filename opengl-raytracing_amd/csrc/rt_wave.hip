// rt_wave.hip -- wavefront pipeline for BVH scenes (the production path on MI355X).
//
// One frame of rt.frag in BVH mode is cut into stages so that every traversal runs in a dedicated,
// register-lean persistent kernel and all shading runs in dense ALU kernels:
//
//   primary        thread = pixel.  Ray generation + slab test against the root box.  Pixels whose
//                  ray misses the scene box (the vast majority when the mesh is small on screen)
//                  are finished here: sky x SPP, TAA resolve, 4 target stores.  The rest are
//                  compacted (wave ballot, one atomic per wave) into the candidate list.
//   trace_primary  persistent closest-hit traversal over the candidates (ray rebuilt from the pixel).
//   post_primary   thread = candidate.  Misses are finished like above; hits are compacted into
//                  the hit list {slot, t, triangle}.
//   gen_direct     thread = (hit, sample).  Runs the reference's shading code with a tracer that
//                  only RECORDS rays: 4 disk + sun + point shadow rays, the GI bounce ray, and
//                  (sample 0) the AO rays.  Queues are slot-major: all "sun" rays of a chunk are
//                  contiguous, so neighbouring lanes trace near-identical rays.
//   trace_shadow   persistent any-hit traversal (direct shadows + AO as any-hit with tMax < radius)
//   trace_gi       persistent closest-hit traversal of the bounce rays
//   gen_gi         thread = (hit, sample): shadow rays at the bounce hit
//   trace_gi_shadow
//   combine        thread = hit: the reference's shading code again, now with a tracer that READS
//                  the recorded visibilities / hits, in the reference's evaluation order (so the
//                  sums are bit-identical to the megakernel and the oracle); TAA; stores.
//
// Persistent traversal ("ray scheduler"): a fixed grid of waves pulls rays from a global cursor.
// When enough lanes of a wave have finished their ray (ballot + popcount), exactly those lanes
// fetch new rays with ONE atomic for the wave and restart, so divergent ray lengths do not leave
// the SIMD half empty.  Each lane's traversal stack is in LDS (stack[e*64 + lane], 8-byte entries:
// deferred child + its entry distance).
#include "rt_wave.hpp"

#include <cstdio>
#include <string>

#include "../../include/rt_mi355.h"
#include "rt_wave_plan.hpp"

#pragma clang fp contract(off)

using namespace rtd;

#include "rt_wave_stages.hpp"   // and through it rt_trace.hpp, rt_trace_src.hpp, rt_wave_buf.hpp: this unit's device code (file map)

// -------------------------------------------------------------------------------------------------
constexpr int kMinLaunches = 256;   // trace launches per frame (1 + 3 per chunk) the cursor table starts with; grown on demand

#ifndef RT_MAX_LANES
#define RT_MAX_LANES 8
#endif
struct RtArenaPool {
    int n = 0;
    void *mem[RT_MAX_LANES] = {};
    size_t bytes[RT_MAX_LANES] = {};
    double q2Frac = 0.0;                       // largest share of (hit, sample) pairs whose bounce ray hit, over the launch sets of all lanes so far (read back with the NEXT
                                               // launch set's hit count: no extra synchronisation); 0: nothing known yet.  Forgotten by rt_upload_bvh, rt_resize and an spp change
    int q2SPP = 0;                             // samples per pixel q2Frac was measured at
    size_t maxCh[RT_MAX_LANES] = {};           // most hits an arena has been sized for
    hipEvent_t freeEv[RT_MAX_LANES] = {};      // recorded behind the last kernel of the batch that used the arena last
    hipStream_t lastUser[RT_MAX_LANES] = {};   // (a later batch on the same stream is ordered behind it anyway)
};
RtArenaPool *rt_arena_pool_create(int arenas) {
    RtArenaPool *p = new RtArenaPool();
    p->n = std::max(1, std::min(arenas, (int)RT_MAX_LANES));
    for (int i = 0; i < RT_MAX_LANES; ++i) (void)hipEventCreateWithFlags(&p->freeEv[i], hipEventDisableTiming);
    return p;
}
void rt_arena_pool_destroy(RtArenaPool *p) {
    if (!p) return;
    for (int i = 0; i < RT_MAX_LANES; ++i) { if (p->mem[i]) (void)hipFree(p->mem[i]); if (p->freeEv[i]) (void)hipEventDestroy(p->freeEv[i]); }
    delete p;
}
int rt_arena_pool_count(const RtArenaPool *p) { int c = 0; for (int i = 0; p && i < RT_MAX_LANES; ++i) c += p->mem[i] ? 1 : 0; return c; }
size_t rt_arena_pool_bytes(const RtArenaPool *p) { size_t b = 0; for (int i = 0; p && i < RT_MAX_LANES; ++i) b += p->bytes[i]; return b; }

struct RtWave {
    std::string err;
    RtArenaPool *pool = nullptr;   // the context's ray arenas (rt_api.hip)
    int arena = 0;                 // index into pool: lane % n for a launch set of one chunk, the lane itself for a set of several (wave_settle_chunks)
    int lane = 0;
    int cus = 256;
    rtl::WaveOptions opt = rtl::wave_default_options();   // the options of the environment, read ONCE: at rt_wave_create (rt_wave_plan.cpp)
    TraceTune tune = tune_from_env();   // chunk 0 = run length chosen in the kernel from the queue size
    // allocations
    size_t slotsCap = 0;      // per-frame arrays sized for this many pixel slots
    int prevChunks = 0, prevSPP = 1;   // chunks / spp of this lane's previous launch set: its hit count and bounce-hit counts are copied to hostHits[1], [2..] before the counters are cleared
    void *frameArena = nullptr, *chunkArena = nullptr, *resultArena = nullptr;   // chunkArena: the pool's arena this launch set uses
    size_t resultBytes = 0;   // per-lane traversal results (what k_combine reads)
    uint32_t *counts = nullptr, *heads = nullptr;
    int launchCap = 0, chunkCap = 0;     // trace launches `heads` holds cursors for / chunks `counts` holds bounce counters for
    unsigned long long *acc = nullptr;   // traced-ray tallies accumulated over frames
    unsigned long long *stats = nullptr; // RT_TRACE_STATS=1: 4 stages x 8 diagnostic sums
    uint32_t *hostHits = nullptr;        // pinned: the hit count of a batch that needs more than one chunk (read back once per batch)
    hipStream_t shadeStream = nullptr;   // RT_CU_SPLIT: the shading kernels' stream (a CU-masked one), else null
    hipEvent_t hopEv = nullptr;
    uint32_t builds = 0;                 // RT_BUILD_* bits of the traversal builds launched since the last rt_wave_builds reset
    bool noKernel = false;               // a trace launch found no kernel for the build it chose and launched nothing (wave_built): the stage fails
    bool probeTree = true;               // the any-hit tree is the collapse of the binary one (rt_upload_bvh): false under RT_ANYHIT_TREE=sah
    unsigned long long *probeAcc = nullptr;   // device, monotonic: [0] bounce rays the probe walked [1] rays it re-traced closest-hit
    unsigned long long probeLaunches = 0, closestLaunches = 0;   // bounce launches (chunks) with / without the probe
    unsigned long long probeBase[4] = {};     // rt_wave_bounce_probe's reset: the values above at that time
    unsigned long long *diskAcc = nullptr;    // device: rt_wave_disk_skip's ten sums (disk_stat_add); the generators count only once the entry was called
    bool diskStatOn = false;
    unsigned long long *giListAcc = nullptr;  // device: rt_wave_gi_list's two sums (gi_list_stat_add); counted only once the entry was called
    bool giListOn = false;
    unsigned long long listedLaunches = 0, pairLaunches = 0, giListBase[2] = {0, 0};   // host: bounce-hit generator launches over the hit list / over every pair
    unsigned long long tracedProbeBase = 0;   // rt_wave_traced's reset: probeAcc[0] at that time (probed rays count as bounce rays there)
    // light-slot liveness masks: the lane's own words, grown with the chunk arrays; queue 1's first, queue 2's behind them
    int lightMasks = rtl::light_masks_from_env();   // 0 none, 1 queue 1, 2 both queues
    int batchInterleave = rtl::batch_interleave_from_env();   // RT_BATCH_INTERLEAVE: a batch's candidates pixel-major, the frames of a pixel side by side (k_primary_interleaved); 0: frame-major (k_primary)
    unsigned long long *liveMem = nullptr;
    size_t liveWords = 0;
    unsigned long long *maskAcc = nullptr;    // device: rt_wave_light_masks' sums -- [0] set bits of queue 1 [1] of queue 2 (k_count_live) [2] mask words scanned [3] masked
    bool maskStatOn = false;                  // refill passes (k_trace); counted only once the entry was called
    unsigned long long maskWordsLast[2] = {0, 0};   // mask words of the last chunk: queue 1, queue 2
    // beam cull: the lane's own flags, one byte per local spatial tile, grown with the frame
    int beamCull = rtl::beam_cull_from_env();   // RT_BEAM_CULL: -1 auto (launch sets of two or more frames), 1 single frames too, 0 never
    uint8_t *beamDead = nullptr;
    size_t beamCap = 0, beamLast = 0;           // tiles the flags hold room for / tiles of the last culled launch set (0: none yet)
    unsigned long long *beamAcc = nullptr;      // device: rt_wave_beam_cull's four sums (k_beam_cull); counted only once the entry was called
    bool beamStatOn = false;
};

RtWave *rt_wave_create(int cus, RtArenaPool *pool, int lane) {
    RtWave *w = new RtWave();
    w->cus = cus > 0 ? cus : 256;
    w->pool = pool;
    w->lane = lane;
    w->arena = lane % pool->n;
    w->opt = rtl::wave_options_from_env();
    if (w->opt.skipTraversalSet) w->tune.skipTraversal = w->opt.skipTraversal;
    (void)hipEventCreateWithFlags(&w->hopEv, hipEventDisableTiming);
    if (w->opt.cuSplit) {
        const int k = w->opt.cuSplit;
        uint32_t mask[8];
        for (int i = 0; i < 8; ++i) { uint32_t m = 0; for (int b = 0; b < 32; ++b) if (((i * 32 + b) & 7) < k) m |= 1u << b; mask[i] = m; }
        if (hipExtStreamCreateWithCUMask(&w->shadeStream, 8, mask) != hipSuccess) w->shadeStream = nullptr;
    }
    // EXPERIMENT RT_SHADE_PRIORITY=p: the shading kernels on a second stream of queue priority p (-1 high, 1 low; no CU mask), the traversal launches on the lane's own
    else if (w->opt.shadePrioritySet) {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        const int p = std::max(greatest, std::min(least, (int)w->opt.shadePriority));
        if (hipStreamCreateWithPriority(&w->shadeStream, hipStreamNonBlocking, p) != hipSuccess) w->shadeStream = nullptr;
    }
    return w;
}
void rt_wave_destroy(RtWave *w) {
    if (!w) return;
    if (w->shadeStream) (void)hipStreamDestroy(w->shadeStream);
    if (w->hopEv) (void)hipEventDestroy(w->hopEv);
    for (void *p : std::initializer_list<void *>{w->frameArena, w->resultArena, w->counts, w->heads, w->acc, w->probeAcc, w->diskAcc, w->giListAcc, w->stats, w->liveMem, w->maskAcc, w->beamDead, w->beamAcc})
        if (p) (void)hipFree(p);
    if (w->hostHits) (void)hipHostFree(w->hostHits);
    delete w;
}
const char *rt_wave_error(const RtWave *w) { return w->err.c_str(); }
size_t rt_wave_frame_bytes(const RtWave *w) { return w ? rtl::arena_bytes(rtl::frame_arena(w->slotsCap)) + w->resultBytes : 0; }   // (the planner's totals, tests/test_gpu_wave_plan.py; the liveness words, 8 B each: rt_wave_light_masks)

#define W_TRY(expr)                                                                   \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) { w->err = std::string(#expr) + ": " + hipGetErrorString(e_); return RT_ERR_HIP; } \
    } while (0)
#define W_STEP(expr)                      \
    do {                                  \
        const int rc_ = (expr);           \
        if (rc_ != RT_OK) return rc_;     \
    } while (0)

// ---- one launch set (a frame, or a batch of frames) on its way through the steps of rt_wave_render
struct LaunchSet {
    RtWave *w;
    RtContext *ctx;
    hipStream_t st, ss;        // the lane's stream: traversal launches; the shading kernels' stream (== st unless RT_CU_SPLIT / RT_SHADE_PRIORITY)
    const DevFrame *dFrame;
    const DevFrame *host;      // host copy of *dFrame
    Targets tg;
    int treeDepth;
    rtl::WavePlan plan;
    WaveBuf wb;
    size_t CH;                 // hits per chunk
    int nChunks;
    int giCopied;              // bounce-hit counters of the lane's previous launch set on their way to hostHits[2..]
    int gridPct, gridPctPrimary;
    unsigned long long *S;     // RT_TRACE_STATS / RT_TRACE_TIMING sums, or null
    bool probe;                // this set's bounce rays are walked any-hit first
    unsigned retraceBlocks, listedBlocks;
};

static_assert(sizeof(HitRec) == rtl::kHitRecBytes, "the planner's frame arena holds HitRec records");

static double &wave_share(RtWave *w) { return w->pool->q2Frac; }   // (live: updated behind a set's hit-count read-back, before a large set sizes its arena)

// a trace launch's RT_BUILD_* bits into the lane's record; 0: launch_trace holds no kernel for the build it chose and launched nothing
const char *const kNoKernelMessage = "traversal launch: the library holds no k_trace build for the chosen options";
static void wave_built(RtWave *w, uint32_t built) { w->builds |= built; if (!built) w->noKernel = true; }

static hipError_t wave_hop(RtWave *w, hipStream_t from, hipStream_t to) {
    if (from == to) return hipSuccess;
    hipError_t e = hipEventRecord(w->hopEv, from);
    return e != hipSuccess ? e : hipStreamWaitEvent(to, w->hopEv, 0);
}
// One timed stage on `on` -- the shading stream L.ss or the traversal stream L.st: `on` waits for what the lane's stream holds, and the lane's stream for the stage.
// EXPERIMENT (RT_CU_SPLIT=k): the shading kernels run on a second stream restricted to k eighths of the CUs, the traversal
// launches -- the lane's own stream, created with the complementary mask in rt_api.hip -- on the rest.  ss == st when the experiment is off.
template <class Launch>
static int wave_stage(LaunchSet &L, int stage, hipStream_t on, Launch launch) {
    RtWave *w = L.w;
    W_TRY(wave_hop(w, L.st, on));
    rt_stage_begin(L.ctx, stage, on);
    launch();
    rt_stage_end(L.ctx, stage, 1, on);
    if (w->noKernel) { w->noKernel = false; w->err = kNoKernelMessage; return RT_ERR_UNSUPPORTED; }
    W_TRY(wave_hop(w, on, L.st));
    return RT_OK;
}
// the sharded cursors of trace launch k of chunk c -- 0: the any-hit launch, 1: the bounce rays, 2: the probe's re-trace, 3: the AO packets ([0] of the table: the primary rays)
static uint32_t *wave_cursor(const WaveBuf &wb, int c, int k) { return &wb.heads[(size_t)(1 + c * 4 + k) * kHeadWords]; }
// a trace launch of the set: its cursors, where its rays and gather loads are tallied, and -- RT_TRACE_STATS / RT_TRACE_TIMING -- the first of its sixteen sums in L.S
static TraceLaunch wave_trace(const LaunchSet &L, int gridPct, uint32_t *head, const TraceTune &tune, unsigned long long *tally, unsigned long long *gatherLoads, int statsAt = -1) {
    return TraceLaunch{L.st, L.w->cus, gridPct, L.treeDepth, L.dFrame, L.host->sc, head, tune, tally, gatherLoads, (L.S && statsAt >= 0) ? L.S + statsAt : nullptr};
}

// Ray sources, here and where a launch builds its own in place, start from a value-initialised object (`QueueSrc q{};`): a field that is not named is zero -- nLive / n
// among them, which prepare() fills on the device -- and none reaches a launch indeterminate.
// shadow queue 1 as the any-hit launch reads it: whole, or -- the AO rays went as packets -- from behind its A AO slots
static MaskedQueueSrc wave_shadow_queue1(const LaunchSet &L, uint32_t c0, bool pkAO) {
    const WaveBuf &wb = L.wb;
    const int A = L.plan.ao;
    const size_t skip = pkAO ? (size_t)A * L.CH : 0;   // (packets: the A AO slots are answered already)
    MaskedQueueSrc q{};
    q.live = wb.shLive; q.maskStat = (wb.shLive && L.w->maskStatOn) ? L.w->maskAcc + 2 : nullptr;
    q.o = wb.shO; q.d = wb.shD + skip; q.tm = wb.shT; q.org = wb.aoOrg; q.orgStride = 0; q.liveCount = &wb.counts[1]; q.c0 = c0; q.cap = wb.CH; q.stride = wb.CH; q.outOcc = wb.occ1 + skip;
    q.slots = (uint32_t)(L.plan.S1 - (pkAO ? A : 0));
    q.denseSlots = pkAO ? 0u : (uint32_t)A;
    return q;
}

// step 1 -- lane bookkeeping: the tallies, the share of bounce hits (it belongs to one spp; rt_upload_bvh / rt_resize forget it too), the per-frame arena
static int wave_begin(LaunchSet &L) {
    RtWave *w = L.w;
    const int SPP = L.plan.spp;
    if (!w->acc) { W_TRY(hipMalloc(&w->acc, 16 * sizeof(unsigned long long))); W_TRY(hipMemsetAsync(w->acc, 0, 16 * sizeof(unsigned long long), L.st)); }
    if (!w->probeAcc) { W_TRY(hipMalloc(&w->probeAcc, 2 * sizeof(unsigned long long))); W_TRY(hipMemsetAsync(w->probeAcc, 0, 2 * sizeof(unsigned long long), L.st)); }
    if (w->pool->q2SPP != SPP) { w->pool->q2Frac = 0.0; w->pool->q2SPP = SPP; }
    if (w->prevSPP != SPP) w->prevChunks = 0;   // this lane's previous launch set ran at another spp: its bounce counts are not read
    if (w->slotsCap < L.plan.slots) {
        if (w->frameArena) (void)hipFree(w->frameArena);
        w->frameArena = nullptr;
        W_TRY(hipMalloc(&w->frameArena, rtl::arena_bytes(rtl::frame_arena(L.plan.slots))));
        w->slotsCap = L.plan.slots;
    }
    return RT_OK;
}

// step 3 -- arrays that hold `ch` hits (grown, never shrunk; `room`: allocate for that many when growing, so that a batch with a few more hits fits too).
// predict: shadow queue 2 from the share of bounce hits (a deferred set behind its read-back), else the worst case.
static int wave_grow_arenas(LaunchSet &L, size_t ch, size_t room, bool predict) {
    RtWave *w = L.w;
    const rtl::WavePlan &plan = L.plan;
    room = std::max(room, ch);
    if (w->resultBytes < plan.result_bytes(ch)) {
        if (w->resultArena) { W_TRY(hipStreamSynchronize(L.st)); (void)hipFree(w->resultArena); }
        w->resultArena = nullptr;
        w->resultBytes = 0;
        W_TRY(hipMalloc(&w->resultArena, plan.result_bytes(room)));
        w->resultBytes = plan.result_bytes(room);
    }
    // a shared arena: grown once its current user is done with it
    RtArenaPool &P = *w->pool;
    const int a = w->arena;
    const double share = wave_share(w);
    auto arena_bytes = [&](size_t n) { return plan.ray_bytes(n, predict, share); };
    // (grown when too small; given back ONCE it is more than 1.6 x what a launch set asks for now that the share of bounce hits is known: the worst-case
    // allocation of the first launch sets.  Either way behind the arena's current user.)
    // The new size is for the LARGEST launch set the arena has held, not for this one: bench.py's five-frame warm-up batch once shrank an arena that the
    // seven-frame batches of the timed region then had to grow again (a device-wide synchronisation and a multi-gigabyte hipMalloc inside a 34 ms region:
    // 1.65 -> 1.81 ms per step).
    room = std::max(room, P.maxCh[a]);
    if (P.bytes[a] < arena_bytes(ch) || (plan.opt.q2Predict && predict && share > 0.0 && P.bytes[a] > arena_bytes(room) + arena_bytes(room) / 2 + arena_bytes(room) / 10)) {
        if (P.lastUser[a]) W_TRY(hipEventSynchronize(P.freeEv[a]));
        if (P.mem[a]) (void)hipFree(P.mem[a]);
        P.mem[a] = nullptr; P.bytes[a] = 0;
        W_TRY(hipMalloc(&P.mem[a], arena_bytes(room)));
        P.bytes[a] = arena_bytes(room);
    }
    P.maxCh[a] = room;
    w->chunkArena = P.mem[a];
    return RT_OK;
}

// the WaveBuf pointers of an arena, from the list its bytes came from
static void wave_point_frame_arrays(LaunchSet &L) {
    void *p[rtl::WA_COUNT] = {};
    rtl::arena_carve(rtl::frame_arena(L.plan.slots), L.w->frameArena, p);
    WaveBuf &wb = L.wb;
    wb.cand = (uint32_t *)p[rtl::WA_CAND]; wb.primT = (float *)p[rtl::WA_PRIMT]; wb.primTri = (int *)p[rtl::WA_PRIMTRI]; wb.hits = (HitRec *)p[rtl::WA_HITS];
    wb.pendC = (float4 *)p[rtl::WA_PENDC]; wb.pendPos = (uint2 *)p[rtl::WA_PENDPOS]; wb.pendNrm = (uint2 *)p[rtl::WA_PENDNRM]; wb.pendMy = (float *)p[rtl::WA_PENDMY];
}
static void wave_point_chunk_arrays(LaunchSet &L, size_t ch, bool predict) {
    const size_t n2 = L.plan.q2_entries(ch, predict, wave_share(L.w));
    void *p[rtl::WA_COUNT] = {};
    rtl::arena_carve(L.plan.ray_arena(ch, n2), L.w->chunkArena, p);
    rtl::arena_carve(L.plan.result_arena(ch), L.w->resultArena, p);
    WaveBuf &wb = L.wb;
    wb.shO = (float4 *)p[rtl::WA_SHO]; wb.shD = (float4 *)p[rtl::WA_SHD]; wb.shT = (float *)p[rtl::WA_SHT]; wb.aoOrg = (float4 *)p[rtl::WA_AOORG];
    wb.giD = (float4 *)p[rtl::WA_GID]; wb.giOrg = (float4 *)p[rtl::WA_GIORG];
    wb.sh2O = (float4 *)p[rtl::WA_SH2O]; wb.sh2D = (float4 *)p[rtl::WA_SH2D]; wb.sh2T = (float *)p[rtl::WA_SH2T];
    wb.q2Stride = (uint32_t)n2;
    wb.occ1 = (uint8_t *)p[rtl::WA_OCC1]; wb.giT = (float *)p[rtl::WA_GIT]; wb.giTri = (int *)p[rtl::WA_GITRI];
    wb.occ2 = (uint8_t *)p[rtl::WA_OCC2]; wb.occOvf = (uint8_t *)p[rtl::WA_OCCOVF];
    wb.giPos = (int *)p[rtl::WA_GIPOS]; wb.giPerm = (int *)p[rtl::WA_GIPERM]; wb.giHit = (uint32_t *)p[rtl::WA_GIHIT];   // (giPerm: null unless RT_BIN_GI)
    wb.CH = (uint32_t)ch;
}

// The liveness words of the chunk arrays just pointed: L1 * CH bits for the light slots of queue 1 and -- RT_LIGHT_MASKS=2 -- 6 * q2Stride for
// queue 2, one word more each.
// The lane's own allocation (grown, never shrunk, behind the lane's stream), beside the planned arenas and outside their layout.  RT_LIGHT_MASKS=0: none.
static int wave_light_masks(LaunchSet &L) {
    RtWave *w = L.w;
    if (!w->lightMasks) return RT_OK;
    const size_t w1 = rtl::align_up(((size_t)L.plan.L1 * L.wb.CH + 63) / 64 + 1, 32), w2 = w->lightMasks >= 2 ? rtl::align_up(((size_t)6 * L.wb.q2Stride + 63) / 64 + 1, 32) : 0;
    if (w->liveWords < w1 + w2) {
        if (w->liveMem) { W_TRY(hipStreamSynchronize(L.st)); (void)hipFree(w->liveMem); }
        w->liveMem = nullptr;
        w->liveWords = 0;
        W_TRY(hipMalloc(&w->liveMem, (w1 + w2) * sizeof(unsigned long long)));
        w->liveWords = w1 + w2;
    }
    L.wb.shLive = w->liveMem;
    L.wb.sh2Live = w2 ? w->liveMem + w1 : nullptr;
    w->maskWordsLast[0] = w1; w->maskWordsLast[1] = w2;
    return RT_OK;
}
// rt_debug_light_masks: the set bits of both mask arrays, counted behind the chunk's generators
static __global__ __launch_bounds__(256) void k_count_live(const unsigned long long *live, size_t words1, size_t words2, unsigned long long *sums) {
    unsigned long long n1 = 0, n2 = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words1 + words2; i += (size_t)gridDim.x * 256) {
        const unsigned long long c = (unsigned long long)__popcll(live[i]);
        if (i < words1) n1 += c; else n2 += c;
    }
    for (int off = 32; off > 0; off >>= 1) { n1 += __shfl_down(n1, off, 64); n2 += __shfl_down(n2, off, 64); }
    if ((threadIdx.x & 63) == 0) { if (n1) atomicAdd(&sums[0], n1); if (n2) atomicAdd(&sums[1], n2); }
}

// step 4 -- cursor table (one set of sharded cursors per trace launch) and per-chunk bounce counters: grown when a small queue budget
// cuts the frame into more chunks than seen so far (4K / 16 spp at RT_QUEUE_BUDGET_MB=128 is 491 chunks).  Both arrays are
// only touched by this lane's stream, which is drained first.
static int wave_cursor_table(LaunchSet &L) {
    RtWave *w = L.w;
    const int nChunks = L.nChunks;
    if (1 + nChunks * 4 > w->launchCap || nChunks > w->chunkCap) {
        W_TRY(hipStreamSynchronize(L.st));
        if (w->counts) (void)hipFree(w->counts);
        if (w->heads) (void)hipFree(w->heads);
        w->counts = w->heads = nullptr;
        w->launchCap = w->chunkCap = 0;
        w->prevChunks = 0;
        const int lc = std::max(kMinLaunches, 1 + nChunks * 4), cc = std::max(4096, nChunks);
        W_TRY(hipMalloc(&w->counts, (size_t)(64 + 2 * cc) * sizeof(uint32_t)));   // [64 + c]: bounce hits of chunk c, [64 + cc + c]: its probe's hit list length
        W_TRY(hipMalloc(&w->heads, (size_t)lc * kHeadWords * sizeof(uint32_t)));
        w->launchCap = lc; w->chunkCap = cc;
    }
    L.wb.counts = w->counts; L.wb.heads = w->heads;

    // the bounce-hit counts of this lane's PREVIOUS launch set, before they are cleared: read on the host behind this set's own hit-count read-back (no extra
    // synchronisation) -- what the capacity of shadow queue 2 is predicted from
    if (!w->hostHits) W_TRY(hipHostMalloc((void **)&w->hostHits, 64 * sizeof(uint32_t)));
    L.giCopied = std::min(w->prevChunks, 60);
    if (L.giCopied > 0) {
        W_TRY(hipMemcpyAsync(w->hostHits + 1, w->counts + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, L.st));
        W_TRY(hipMemcpyAsync(w->hostHits + 2, w->counts + 64, (size_t)L.giCopied * sizeof(uint32_t), hipMemcpyDeviceToHost, L.st));
    }
    W_TRY(hipMemsetAsync(w->counts, 0, (size_t)(64 + w->chunkCap + nChunks) * sizeof(uint32_t), L.st));
    W_TRY(hipMemsetAsync(w->heads, 0, (size_t)(1 + nChunks * 4) * kHeadWords * sizeof(uint32_t), L.st));
    return RT_OK;
}

// step 5 -- the primary stages: candidates, their closest hits, the hit list
static int wave_primary(LaunchSet &L, unsigned tiles) {
    RtWave *w = L.w;
    const WaveBuf &wb = L.wb;
    const bool interleave = w->batchInterleave && L.host->g.batch > 1;   // a single frame keeps k_primary: nothing to put side by side
    W_STEP(wave_stage(L, ST_PRIMARY, L.ss, [&] {
        // the beam cull (rt_wave_beam_flags chose it for this set): the tiles' flags in front of the kernel that reads them, one wave per local spatial tile
        if (L.host->tileDead) hipLaunchKernelGGL(k_beam_cull, dim3(((unsigned)std::max(L.host->g.nLocalTiles, 0) + 3u) / 4u), dim3(256), 0, L.ss, L.dFrame, const_cast<uint8_t *>(L.host->tileDead), w->beamStatOn ? w->beamAcc : nullptr);
        hipLaunchKernelGGL(interleave ? k_primary_interleaved : k_primary, dim3((tiles + kAppendBatch - 1) / kAppendBatch), dim3(256), 0, L.ss, L.dFrame, L.tg, wb);
    }));
    W_STEP(wave_stage(L, ST_TRACE_PRIMARY, L.st, [&] {
        PrimarySrc ps{};
        ps.fr = L.dFrame; ps.cand = wb.cand; ps.count = &wb.counts[0]; ps.outT = wb.primT; ps.outTri = wb.primTri;
        TraceTune tuneP = w->tune;   // primary rays: their cost varies strongly across the screen, so shorter runs than the queue launches (128 - 256, see k_trace)
        tuneP.chunkMax = 256;
        if (w->opt.chunkPrimarySet) tuneP.chunk = w->opt.chunkPrimary;
        wave_built(w, launch_trace<PrimarySrc, false>(wave_trace(L, L.gridPctPrimary, &wb.heads[0], tuneP, w->acc + 2, w->acc + 8, 0), ps));
    }));
    W_STEP(wave_stage(L, ST_POST_PRIMARY, L.ss, [&] { hipLaunchKernelGGL(k_post_primary, dim3((tiles + kAppendBatch - 1) / kAppendBatch), dim3(256), 0, L.ss, L.dFrame, L.tg, wb); }));
    return RT_OK;
}

// step 6 -- More than one chunk: the number of chunks that hold hits is known only on the device.  Launching the chunk loop for the upper
// bound (rounds 1-2) costs little time -- the kernels of an empty chunk return at once -- but fills the launch statistics with
// empty launches (bench.py's batches of eight 1080p frames: 5 launch sets, 2 of them with rays).  Such a batch is tens of
// milliseconds of work, so the hit count is read back once (this lane's stream only; the other lanes keep the GPU busy) and
// the hits are dealt over equal chunks.  A single-chunk frame -- every frame-by-frame BASELINE configuration -- never syncs.
static int wave_settle_chunks(LaunchSet &L) {
    RtWave *w = L.w;
    const rtl::WavePlan &plan = L.plan;
    if (!(plan.deferred || L.nChunks > 1) || w->opt.chunksFromSlots) return RT_OK;
    W_TRY(hipMemcpyAsync(w->hostHits, &w->counts[1], sizeof(uint32_t), hipMemcpyDeviceToHost, L.st));
    W_TRY(hipStreamSynchronize(L.st));
    const size_t hits = *w->hostHits;
    if (L.giCopied > 0 && w->hostHits[1] > 0) {     // the previous launch set of this lane: what share of its (hit, sample) pairs had a bounce hit
        unsigned long long bounced = 0;
        for (int i = 0; i < L.giCopied; ++i) bounced += w->hostHits[2 + i];
        double &frac = wave_share(w);
        frac = std::max(frac, std::max(1e-9, (double)bounced / ((double)w->hostHits[1] * (double)std::max(w->prevSPP, 1))));
    }
    const rtl::ChunkSplit split = plan.split(hits);
    L.nChunks = split.nChunks;
    L.CH = split.ch;
    // a set of several chunks keeps its arena for the whole chunk loop -- shared by two lanes that would serialise the lanes (4 spp -> 16 spp, 4K and
    // the 1 M-triangle scene lost 3 % that way) -- so it takes the lane's OWN arena; one-chunk sets (every frame-by-frame configuration, bench.py's
    // batches) share lane % n
    if (plan.deferred) w->arena = L.nChunks > 1 ? w->lane : w->lane % w->pool->n;   // (not deferred: chosen and allocated before k_primary)
    if (plan.deferred && L.nChunks > 0) W_STEP(wave_grow_arenas(L, L.CH, split.room, true));
    if (L.nChunks > 0) { wave_point_chunk_arrays(L, L.CH, plan.deferred); W_STEP(wave_light_masks(L)); }
    return RT_OK;
}

// step 7a -- shade the hits of chunk c: the light and AO rays into shadow queue 1, the bounce rays into theirs; with RT_PACKET_AO the AO rays are traced here,
// one packet per hit (k_trace_packets), and the any-hit launch then starts behind the A AO slots of queue 1 (wave_shadow_queue1).
static int wave_chunk_direct(LaunchSet &L, int c, uint32_t c0, bool pkAO) {
    RtWave *w = L.w;
    const WaveBuf &wb = L.wb;
    const unsigned gridHS = (unsigned)((L.CH * (size_t)L.plan.spp + 255) / 256);
    // the chunk's liveness bits start clear: on the lane's stream, behind the any-hit launch of the chunk before and of the lane's previous launch set
    if (wb.shLive) W_TRY(hipMemsetAsync(wb.shLive, 0, (size_t)(w->maskWordsLast[0] + w->maskWordsLast[1]) * sizeof(unsigned long long), L.st));
    W_STEP(wave_stage(L, ST_GEN_DIRECT, L.ss, [&] { hipLaunchKernelGGL(L.host->nrmRows ? k_gen_direct_smooth : k_gen_direct, dim3(gridHS), dim3(256), 0, L.ss, L.dFrame, wb, c0, w->diskStatOn ? w->diskAcc : nullptr); }));
    if (pkAO) W_STEP(wave_stage(L, ST_TRACE_AO, L.st, [&] {
        PacketSrc pk{};   // the A dense AO slots in front of shadow queue 1
        pk.d = wb.shD; pk.org = wb.aoOrg; pk.occ = wb.occ1; pk.liveCount = &wb.counts[1]; pk.c0 = c0; pk.cap = wb.CH; pk.stride = wb.CH; pk.A = L.plan.ao;
        wave_built(w, launch_packets(wave_trace(L, L.gridPct, wave_cursor(wb, c, 3), w->tune, w->acc + 7, w->acc + 14), pk));
    }));
    return RT_OK;
}

// step 7b -- the bounce rays of chunk c: traced (any-hit first behind a probe), then shaded where they hit -- six shadow rays per bounce hit into queue 2
static int wave_chunk_bounce(LaunchSet &L, int c, uint32_t c0) {
    RtWave *w = L.w;
    const WaveBuf &wb = L.wb;
    const int SPP = L.plan.spp;
    const unsigned gridHS = (unsigned)((L.CH * (size_t)SPP + 255) / 256);
    uint32_t *const listCount = &wb.counts[64 + w->chunkCap + c];
    QueueSrc qg{};   // the bounce queue: SPP dense slots, the origin per hit (RT_BIN_GI: per record)
    qg.d = wb.giD; qg.org = wb.giOrg; qg.orgStride = wb.giPerm ? wb.CH : 0u; qg.liveCount = &wb.counts[1]; qg.c0 = c0; qg.cap = wb.CH; qg.stride = wb.CH; qg.slots = (uint32_t)SPP; qg.denseSlots = (uint32_t)SPP;
    qg.outT = wb.giT; qg.outTri = wb.giTri;
    W_STEP(wave_stage(L, ST_TRACE_GI, L.st, [&] {
        if (L.probe) {
            // any-hit walk of every bounce ray (misses answered in place, hits listed), then the closest-hit walk of the listed ones
            BounceProbeSrc pb{};
            pb.q = qg; pb.hitters = wb.giHit; pb.hitCount = listCount; pb.inf = L.host->u.inf;
            wave_built(w, launch_trace<BounceProbeSrc, true>(wave_trace(L, L.gridPct, wave_cursor(wb, c, 1), w->tune, w->probeAcc + 0, w->acc + 10, 32), pb));
            w->builds |= (uint32_t)RT_BUILD_BOUNCE_PROBE << RT_BUILD_ANY_SHIFT;
            IndexedDenseSrc rq{};
            rq.idx = wb.giHit; rq.count = listCount; rq.org = wb.giOrg; rq.d = wb.giD; rq.stride = wb.CH; rq.orgStride = qg.orgStride; rq.outT = wb.giT; rq.outTri = wb.giTri;
            TraceLaunch retrace = wave_trace(L, L.gridPct, wave_cursor(wb, c, 2), w->tune, w->probeAcc + 1, w->acc + 10);
            retrace.maxBlocks = L.retraceBlocks;
            wave_built(w, launch_trace<IndexedDenseSrc, false>(retrace, rq));
            w->probeLaunches++;
        } else {
            wave_built(w, launch_trace<QueueSrc, false>(wave_trace(L, L.gridPct, wave_cursor(wb, c, 1), w->tune, w->acc + 4, w->acc + 10, 32), qg));
            w->closestLaunches++;
        }
    }));
    return wave_stage(L, ST_GEN_GI, L.ss, [&] {
        // behind a probe the generator walks the probe's hit list (k_gen_gi_listed); RT_BIN_GI's permuted queue and sets without a probe visit every pair
        const bool listed = L.probe && !wb.giPerm;
        const uint32_t *hitList = listed ? wb.giHit : nullptr, *hitCount = listed ? listCount : nullptr;
        unsigned long long *listStat = w->giListOn ? w->giListAcc : nullptr;
        if (listed) {
            hipLaunchKernelGGL(L.host->nrmRows ? k_gen_gi_listed_smooth : k_gen_gi_listed, dim3(L.listedBlocks), dim3(256), 0, L.ss, L.dFrame, wb, c0, hitList, hitCount, &wb.counts[64 + c], w->diskStatOn ? w->diskAcc : nullptr, listStat);
            w->listedLaunches++;
        } else {
            hipLaunchKernelGGL(L.host->nrmRows ? k_gen_gi_smooth : k_gen_gi, dim3(gridHS), dim3(256), 0, L.ss, L.dFrame, wb, c0, &wb.counts[64 + c], w->diskStatOn ? w->diskAcc : nullptr, listStat);
            w->pairLaunches++;
        }
        if (wb.q2Stride < wb.CH * (uint32_t)SPP)   // a predicted capacity: the pairs beyond it (normally none) trace their rays in place
            hipLaunchKernelGGL(L.host->nrmRows ? k_gen_gi_overflow_smooth : k_gen_gi_overflow, dim3(std::min<unsigned>(gridHS, (unsigned)w->cus * 4u)), dim3(256), (size_t)256 * std::max(L.treeDepth, 4) * 8, L.ss, L.dFrame, wb, c0, &wb.counts[64 + c], std::max(L.treeDepth, 4), hitList, hitCount);
    });
}

// step 7 -- one chunk: generate, bounce, shadows, combine
static int wave_chunk(LaunchSet &L, int c) {
    RtWave *w = L.w;
    const WaveBuf &wb = L.wb;
    const uint32_t c0 = (uint32_t)((size_t)c * L.CH);
    const bool pkAO = w->opt.packetAO && L.plan.ao > 0;
    W_STEP(wave_chunk_direct(L, c, c0, pkAO));
    const MaskedQueueSrc q1 = wave_shadow_queue1(L, c0, pkAO);
    const TraceLaunch shadows = wave_trace(L, L.gridPct, wave_cursor(wb, c, 0), w->tune, w->acc + 3, w->acc + 9, 16);
    // rt_debug_light_masks: the bits the generators set, counted before the launch that reads them
    auto count_live = [&] { if (wb.shLive && w->maskStatOn) hipLaunchKernelGGL(k_count_live, dim3(256), dim3(256), 0, L.st, wb.shLive, (size_t)w->maskWordsLast[0], (size_t)w->maskWordsLast[1], w->maskAcc); };
    if (L.host->u.enableGI == 1) {
        // bounce rays first, then ONE any-hit launch over both shadow queues
        W_STEP(wave_chunk_bounce(L, c, c0));
        count_live();
        DualQueueSrc qq{};
        qq.a = q1;   // b: shadow queue 2, six slots, the entries compacted over the chunk's bounce hits
        qq.b.live = wb.sh2Live; qq.b.maskStat = q1.maskStat;
        qq.b.o = wb.sh2O; qq.b.d = wb.sh2D; qq.b.tm = wb.sh2T; qq.b.liveCount = &wb.counts[64 + c]; qq.b.c0 = 0; qq.b.cap = wb.q2Stride; qq.b.stride = wb.q2Stride; qq.b.slots = 6u; qq.b.outOcc = wb.occ2;
        W_STEP(wave_stage(L, ST_TRACE_SHADOW, L.st, [&] { wave_built(w, launch_trace<DualQueueSrc, true>(shadows, qq)); }));
    } else {
        count_live();
        W_STEP(wave_stage(L, ST_TRACE_SHADOW, L.st, [&] { wave_built(w, launch_trace<MaskedQueueSrc, true>(shadows, q1)); }));
    }
    // the last traversal launch of the batch is queued: the shared ray arena may go to the next batch (k_combine reads the lane's own result arrays)
    if (c == L.nChunks - 1) { W_TRY(hipEventRecord(w->pool->freeEv[w->arena], L.st)); w->pool->lastUser[w->arena] = L.st; }
    const unsigned gridH = (unsigned)((L.CH + 255) / 256);
    return wave_stage(L, ST_COMBINE, L.ss, [&] { hipLaunchKernelGGL(L.host->uvRows ? (L.host->nrmRows ? k_combine_smooth_tex : k_combine_tex) : L.host->colRows ? (L.host->nrmRows ? k_combine_smooth_color : k_combine_color) : (L.host->nrmRows ? k_combine_smooth : k_combine), dim3(gridH), dim3(256), 0, L.ss, L.dFrame, L.tg, wb, c0); });
}

// The steps of a launch set: lane bookkeeping, plan, arenas, cursor table, primary stages, chunks settled, chunk by chunk, tally and resolve.
int rt_wave_render(RtWave *w, RtContext *ctx, hipStream_t st, const DevFrame *dFrame, const DevFrame &host, Targets tg,
                   unsigned long long *, bool count, int treeDepth, hipEvent_t evPrevDone, bool cacheResident) {
    if (count) { w->err = "work counters are produced by the megakernel pipeline (RT_PIPELINE_MEGAKERNEL)"; return RT_ERR_UNSUPPORTED; }
    const RtUniforms &u = host.u;
    const int batch = std::max(host.g.batch, 1);
    const size_t nSlots = (size_t)std::max(host.g.nLocalTiles, 1) * 256 * (size_t)batch;   // pixel slots of all frames of the batch
    LaunchSet L{};
    L.w = w; L.ctx = ctx; L.st = st; L.ss = w->shadeStream ? w->shadeStream : st; L.dFrame = dFrame; L.host = &host; L.tg = tg; L.treeDepth = treeDepth;
    const rtl::WavePlan &plan = L.plan = rtl::wave_plan(nSlots, u.spp, u.enableAO == 1 ? u.aoSamples : 0, w->opt);
    const int SPP = plan.spp;
    W_STEP(wave_begin(L));
    if (plan.tooLarge) { w->err = rtl::kTooLargeMessage; return RT_ERR_UNSUPPORTED; }
    L.CH = plan.chBudget;
    L.nChunks = plan.chunks_upper_bound();   // upper bound (every pixel slot a hit); cut down to the hit count by wave_settle_chunks
    wave_point_frame_arrays(L);
    if (!plan.deferred) {   // (deferred: the chunk arrays stay null until they are carved behind k_post_primary)
        w->arena = L.nChunks > 1 ? w->lane : w->lane % w->pool->n;
        W_STEP(wave_grow_arenas(L, L.CH, L.CH, false));
        wave_point_chunk_arrays(L, L.CH, false);
        W_STEP(wave_light_masks(L));
    }
    L.wb.CH = (uint32_t)L.CH; L.wb.A = plan.ao; L.wb.SPP = SPP;
    W_STEP(wave_cursor_table(L));
    // Persistent grids smaller than what fits, for the two queue launches of a cache-resident scene: they run near the vector L1's access
    // rate (0.81 accesses per clock and CU, PMC), which four and a half workgroups per CU sustain as well as six, and the
    // registers left free let the shading kernels of the other frame lanes run beside them instead of waiting for a persistent grid to
    // drain (kernel timeline, profiles/r03_timeline.txt: k_combine in flight 78 % of the time for 8 % of the work).  One GPU, batches of
    // eight frames: 1.83 -> 1.76 ms per frame.  Not for the primary launch (latency-bound: 0.24 -> 0.27 ms at 75 %) and not for a
    // scene that misses L2 (1 M triangles: any-hit launch 15.2 -> 16.1 ms at 75 % -- it needs every wave to cover the fabric's latency).
    // A tile-parallel rank traces 1/n of the rays and overlaps four batches: half-size grids (one rank of 8: 0.47 -> 0.43 ms/frame).
    L.gridPct = w->opt.gridPct ? w->opt.gridPct : (host.g.world > 1 ? 50 : (cacheResident ? 75 : 100));
    L.gridPctPrimary = w->opt.gridPctPrimary ? w->opt.gridPctPrimary : (host.g.world > 1 ? L.gridPct : 100);
    if ((w->opt.traceStatsSet || w->opt.traceTimingSet) && !w->stats) { W_TRY(hipMalloc(&w->stats, 64 * sizeof(unsigned long long))); W_TRY(hipMemset(w->stats, 0, 64 * sizeof(unsigned long long))); }
    L.S = w->stats;
    const unsigned tilesFrame = (unsigned)std::max(host.g.nLocalTiles, 0);
    const unsigned tiles = tilesFrame * (unsigned)batch;
    if (tiles == 0) return RT_OK;
    W_STEP(wave_primary(L, tiles));
    W_STEP(wave_settle_chunks(L));
    const double share = wave_share(w);
    L.probe = u.enableGI == 1 && w->probeTree && rtl::wave_probe_on(w->opt, share);
    // the re-trace launch: a grid for about twice the expected hits (a persistent grid for ~1 % of the rays would mostly ramp up and drain)
    L.retraceBlocks = share > 0.0 ? (unsigned)std::max(32.0, std::min(1e6, 2.0 * share * (double)L.CH * SPP / 2048.0)) : 0u;
    // k_gen_gi_listed: one thread per listed hit for about twice the expected hits, between 32 workgroups and eight per CU; the grid strides over whatever the list holds
    L.listedBlocks = (unsigned)std::max(32.0, std::min((double)w->cus * 8.0, share > 0.0 ? 2.0 * share * (double)L.CH * SPP / 256.0 : (double)w->cus * 4.0));
    // shared arena: everything from here to the last combine reads or writes it
    if (L.nChunks > 0 && w->pool->lastUser[w->arena] && w->pool->lastUser[w->arena] != st) W_TRY(hipStreamWaitEvent(st, w->pool->freeEv[w->arena], 0));
    for (int c = 0; c < L.nChunks; ++c) W_STEP(wave_chunk(L, c));
    // step 8 -- tally, and the temporal resolve: the one stage that needs the previous frame's COLOR0 (and must not overtake its target stores)
    w->prevChunks = (u.enableGI == 1) ? L.nChunks : 0;
    w->prevSPP = SPP;
    hipLaunchKernelGGL(k_accum_tally, dim3(1), dim3(64), 0, st, w->counts, w->acc, batch);
    if (evPrevDone) W_TRY(hipStreamWaitEvent(st, evPrevDone, 0));
    rt_stage_begin(ctx, ST_RESOLVE, st);
    hipLaunchKernelGGL(k_resolve, dim3(tilesFrame), dim3(256), 0, st, dFrame, tg, L.wb);
    rt_stage_end(ctx, ST_RESOLVE, 1, st);
    W_TRY(hipGetLastError());
    return RT_OK;
}

// Closest-hit traversal of the rays listed in idx[0 .. *count) (queue addresses into o / d; results to outT / outTri at the same address) with the
// persistent kernel of this pipeline, for rt_hybrid.hip.  `heads`: kHeadWords zeroed cursor words.
uint32_t rt_wave_trace_closest_indexed(hipStream_t st, int cus, int treeDepth, const DevFrame *dFrame, const DevScene &hostScene, const uint32_t *idx,
                                   const uint32_t *count, const float4 *o, const float4 *d, float *outT, int *outTri, uint32_t *heads) {
    IndexedSrc q{};
    q.idx = idx; q.count = count; q.o = o; q.d = d; q.outT = outT; q.outTri = outTri;
    return launch_trace<IndexedSrc, false>(TraceLaunch{st, cus, 100, treeDepth, dFrame, hostScene, heads, default_tune()}, q);
}
uint32_t rt_wave_trace_closest_compact(hipStream_t st, int cus, int treeDepth, const DevFrame *dFrame, const DevScene &hostScene, const float4 *o, const float4 *d,
                                   const uint32_t *dst, const uint32_t *count, const uint32_t *flags, uint32_t cap, float *outT, int *outTri, uint32_t *heads, uint32_t capOut) {
    CompactSrc q{};
    q.o = o; q.d = d; q.dst = dst; q.count = count; q.flags = flags; q.cap = cap; q.capOut = capOut; q.outT = outT; q.outTri = outTri;
    return launch_trace<CompactSrc, false>(TraceLaunch{st, cus, 100, treeDepth, dFrame, hostScene, heads, default_tune()}, q);
}
// Diagnostics (rt_debug_trace kinds 2 / 3): n arbitrary rays through the PRODUCTION traversal kernels -- a one-slot queue of n entries, closest-hit or any-hit
// launch as the frames use it (persistent grid, refill scheduler, the any-hit node form rt_upload_bvh chose, the build the environment selects: tune_from_env)
// -- so that the kernels can be tested ray by ray.  Returns the RT_BUILD_* bits of the build launched.
uint32_t rt_wave_debug_trace(hipStream_t st, int cus, int treeDepth, const DevFrame *dFrame, const DevScene &hostScene, bool any, const float4 *o, const float4 *d,
                             const float *tm, const uint32_t *liveCount, uint32_t n, float *outT, int *outTri, uint8_t *outOcc, uint32_t *heads) {
    QueueSrc q{};
    q.o = o; q.d = d; q.tm = tm; q.liveCount = liveCount; q.c0 = 0; q.cap = n; q.stride = n; q.slots = 1; q.outT = outT; q.outTri = outTri; q.outOcc = outOcc;
    // QueueSrc stores occlusions only: "not occluded" goes in first, on the launch's stream (an empty slot, tm < 0, keeps it)
    if (any) (void)hipMemsetAsync(outOcc, 0, n, st);
    return launch_trace_kind(any, TraceLaunch{st, cus, 100, treeDepth, dFrame, hostScene, heads, tune_from_env()}, q);
}
// rt_debug_trace kind 4: nPackets packets of four any-hit rays through k_trace_packets, in the layout of PacketSrc with A = 4 AO slots: ray r of packet p at
// [r * nPackets + p] (*liveCount = nPackets).  A packet leaves from the origin of its ray 0; tm < 0 marks an empty slot (its occ entry keeps the 0 written here first).
uint32_t rt_wave_debug_packets(hipStream_t st, int cus, int treeDepth, const DevFrame *dFrame, const DevScene &hostScene, const float4 *o, const float4 *d,
                               const float *tm, const uint32_t *liveCount, uint32_t nPackets, uint8_t *outOcc, uint32_t *heads) {
    PacketSrc pk{};
    (void)hipMemsetAsync(outOcc, 0, (size_t)nPackets * 4, st);   // what an empty slot reads
    pk.o = o; pk.d = d; pk.tm = tm; pk.occ = outOcc; pk.liveCount = liveCount; pk.c0 = 0; pk.cap = nPackets; pk.stride = nPackets; pk.A = 4;
    return launch_packets(TraceLaunch{st, cus, 100, treeDepth, dFrame, hostScene, heads, tune_from_env()}, pk);
}
// rt_trace_rays: n user rays through the production traversal launch of the environment's build (tune_from_env), the node form
// rt_upload_bvh chose, a persistent grid of at most the waves n rays occupy.  dFrame / heads: the context's query scratch (one query at a time).
uint32_t rt_wave_trace_query(hipStream_t st, int cus, int treeDepth, DevFrame *dFrame, const DevScene &hostScene, bool any, const float *o, int os, const float *d,
                             int ds, const float *tm, float eps, float inf, uint32_t n, void *hits, float *normals, uint8_t *occ, uint32_t *heads) {
    QuerySrc q{};
    q.o = o; q.d = d; q.tm = tm; q.os = (uint32_t)os; q.ds = (uint32_t)ds; q.n = n; q.inf = inf; q.tris = hostScene.tris;
    q.hits = any ? nullptr : reinterpret_cast<float4 *>(hits); q.normals = any ? nullptr : normals; q.occ = any ? occ : nullptr;
    hipLaunchKernelGGL(k_query_prep, dim3(1), dim3(256), 0, st, dFrame, hostScene, eps, inf, heads);
    TraceLaunch t{st, cus, 100, treeDepth, dFrame, hostScene, heads, tune_from_env()};
    t.maxBlocks = (unsigned)((n + 255u) / 256u);
    return launch_trace_kind(any, t, q);
}
// rt_trace_scene_rays / rt_pick_pixels: the mesh leg, after rt_scene_query_analytic wrote dFrame, heads and every ray's first answer
uint32_t rt_wave_trace_scene(hipStream_t st, int cus, int treeDepth, const DevFrame *dFrame, const DevScene &hostScene, bool hybrid, const SceneRays &r, float inf,
                             uint32_t *heads) {
    SceneSrc q{};
    q.o = r.o; q.d = r.d; q.xy = r.xy; q.cam = &dFrame->u; q.tm = r.tm; q.os = (uint32_t)r.os; q.ds = (uint32_t)r.ds; q.n = r.n; q.inf = inf; q.hybrid = hybrid;
    q.tris = hostScene.tris; q.hits = r.hits; q.objects = r.objects; q.normals = r.normals; q.points = r.points; q.occ = r.occ;
    TraceLaunch t{st, cus, 100, treeDepth, dFrame, hostScene, heads, tune_from_env()};
    t.maxBlocks = (unsigned)((r.n + 255u) / 256u);
    return launch_trace_kind(!r.hits, t, q);
}
uint32_t rt_wave_builds(RtWave *w, bool reset) {
    if (!w) return 0;
    const uint32_t b = w->builds;
    if (reset) w->builds = 0;
    return b;
}
size_t rt_wave_head_words() { return kHeadWords; }

int rt_wave_traced(RtWave *w, hipStream_t st, unsigned long long *out8, bool reset) {   // 16 words, see rt_wave.hpp
    for (int i = 0; i < 16; ++i) out8[i] = 0;
    if (!w->acc) return RT_OK;
    W_TRY(hipStreamSynchronize(st));
    W_TRY(hipMemcpy(out8, w->acc, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (w->probeAcc) {   // bounce rays the probe walked count as bounce rays, once (their re-traced hits do not count again)
        unsigned long long pa[2];
        W_TRY(hipMemcpy(pa, w->probeAcc, sizeof pa, hipMemcpyDeviceToHost));
        out8[4] += pa[0] - w->tracedProbeBase;
        if (reset) w->tracedProbeBase = pa[0];
    }
    if (w->stats) {
        unsigned long long v[64];
        W_TRY(hipMemcpy(v, w->stats, sizeof v, hipMemcpyDeviceToHost));
        static const char *nm[4] = {"primary", "shadow", "bounce", "bounce_shadow"};
        if (w->opt.traceTimingSet && w->opt.traceTiming) {
            // RT_TRACE_TIMING=1 (k_trace<.., TIMING>): sums over all waves of the launches since the last reset
            for (int k = 0; k < 3; ++k) {
                const unsigned long long *q = v + k * 16;
                if (!q[0] && !q[4]) continue;
                const double it = (double)std::max<unsigned long long>(q[0], 1), lf = (double)std::max<unsigned long long>(q[4], 1), rf = (double)std::max<unsigned long long>(q[6], 1);
                fprintf(stderr, "[trace timing] %-8s wave lifetime %.4g cycles | inner iterations %.4g: to load issue %.0f + loads in flight %.0f + after arrival %.0f cycles each (%.2f / %.2f / %.2f of the "
                                "lifetime) | leaf phases %.4g: %.0f cycles each (%.2f) | refill rounds %.4g: %.0f cycles each (%.2f)\n",
                        nm[k], (double)q[8], it, q[1] / it, q[2] / it, q[3] / it, (double)q[1] / (double)std::max<unsigned long long>(q[8], 1), (double)q[2] / (double)std::max<unsigned long long>(q[8], 1),
                        (double)q[3] / (double)std::max<unsigned long long>(q[8], 1), lf, q[5] / lf, (double)q[5] / (double)std::max<unsigned long long>(q[8], 1), rf, q[7] / rf,
                        (double)q[7] / (double)std::max<unsigned long long>(q[8], 1));
            }
            if (reset) W_TRY(hipMemset(w->stats, 0, sizeof v));
            if (reset) W_TRY(hipMemset(w->acc, 0, 16 * sizeof(unsigned long long)));
            return RT_OK;
        }
        const bool quiet = w->opt.traceStatsSet && w->opt.traceStats >= 2;   // RT_TRACE_STATS=2: collect (rt_get_traced_rays' mergedLoads*), do not print
        for (int k = 0; k < 4; ++k) {
            const unsigned long long *q = v + k * 16;
            double rays = (double)std::max<unsigned long long>(out8[2 + k], 1);
            if (!quiet) fprintf(stderr, "[trace stats] %-13s rays %.3g | per ray: inner %.1f leaf %.1f tri %.1f | inner-phase lane util %.2f (%.3g wave-iters, %.0f cyc each) "
                            "leaf-phase util %.2f (%.3g, %.0f cyc each) | refills %.3g (%.0f cyc each) | gather loads per ray %.0f, merged within lane quads %.0f (nodes %.0f + triangles %.0f), merged wave-wide %.0f (%.0f + %.0f)\n",
                    nm[k], rays, q[0] / rays, q[1] / rays, q[2] / rays, q[3] ? q[4] / (64.0 * q[3]) : 0.0, (double)q[3], q[3] ? (double)q[8] / q[3] : 0.0,
                    q[5] ? q[6] / (64.0 * q[5]) : 0.0, (double)q[5], q[5] ? (double)q[9] / q[5] : 0.0, (double)q[7], q[7] ? (double)q[10] / q[7] : 0.0,
                    k < 3 ? out8[8 + k] / rays : 0.0, (q[12] + q[13]) / rays, q[12] / rays, q[13] / rays, (q[14] + q[15]) / rays, q[14] / rays, q[15] / rays);
            if (k < 3) out8[11 + k] = q[12] + q[13];   // k: 0 primary, 1 shadow (+ bounce-shadow: one launch), 2 bounce
        }
        if (reset) W_TRY(hipMemset(w->stats, 0, sizeof v));
    }
    if (reset) W_TRY(hipMemset(w->acc, 0, 16 * sizeof(unsigned long long)));
    return RT_OK;
}

int rt_wave_bounce_probe(RtWave *w, hipStream_t st, unsigned long long *out4, bool reset) {
    for (int i = 0; i < 4; ++i) out4[i] = 0;
    if (!w) return RT_OK;
    unsigned long long v[4] = {0, 0, w->probeLaunches, w->closestLaunches};
    if (w->probeAcc) {
        W_TRY(hipStreamSynchronize(st));
        W_TRY(hipMemcpy(v, w->probeAcc, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < 4; ++i) { out4[i] = v[i] - w->probeBase[i]; if (reset) w->probeBase[i] = v[i]; }
    return RT_OK;
}

// Read-back of n sums the generators add to once an entry has asked for them: synchronise, allocate and zero at the first call, copy out, zero again on request
static int wave_read_sums(RtWave *w, hipStream_t st, unsigned long long *&sums, size_t n, unsigned long long *out, bool reset) {
    W_TRY(hipStreamSynchronize(st));
    if (!sums) { W_TRY(hipMalloc(&sums, n * sizeof(unsigned long long))); W_TRY(hipMemset(sums, 0, n * sizeof(unsigned long long))); }
    W_TRY(hipMemcpy(out, sums, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (reset) W_TRY(hipMemset(sums, 0, n * sizeof(unsigned long long)));
    return RT_OK;
}

int rt_wave_disk_skip(RtWave *w, hipStream_t st, unsigned long long *out10, bool reset) {
    for (int i = 0; i < 10; ++i) out10[i] = 0;
    if (!w) return RT_OK;
    W_STEP(wave_read_sums(w, st, w->diskAcc, 10, out10, reset));
    w->diskStatOn = true;
    return RT_OK;
}

int rt_wave_gi_list(RtWave *w, hipStream_t st, unsigned long long *out4, bool reset) {
    for (int i = 0; i < 4; ++i) out4[i] = 0;
    if (!w) return RT_OK;
    W_STEP(wave_read_sums(w, st, w->giListAcc, 2, out4, reset));
    const unsigned long long l[2] = {w->listedLaunches, w->pairLaunches};
    for (int i = 0; i < 2; ++i) { out4[2 + i] = l[i] - w->giListBase[i]; if (reset) w->giListBase[i] = l[i]; }
    w->giListOn = true;
    return RT_OK;
}

int rt_wave_light_masks(RtWave *w, hipStream_t st, unsigned long long *out6, bool reset) {
    for (int i = 0; i < 6; ++i) out6[i] = 0;
    if (!w) return RT_OK;
    W_STEP(wave_read_sums(w, st, w->maskAcc, 4, out6, reset));
    if (w->lightMasks) { out6[4] = w->maskWordsLast[0]; out6[5] = w->maskWordsLast[1]; }
    w->maskStatOn = true;
    return RT_OK;
}

// The beam cull: whether the launch set `host` describes is culled, and where its flags go.  Culled: a BVH frame whose primary launch walks the
// two-child records k_beam_cull walks (not the fused or implicit forms: their tests are the same floats, but nothing has checked the cull against them), in a launch
// set of two or more frames over a scene that fits L2 (cacheResident, as rt_wave_render takes it), or any launch set under RT_BEAM_CULL=1.  The flags are the lane's own, grown behind the lane's stream.  null: no cull, or no memory for it.
const uint8_t *rt_wave_beam_flags(RtWave *w, hipStream_t st, const DevFrame &host, int treeDepth, bool cacheResident) {
    if (!w) return nullptr;
    w->beamLast = 0;   // (rt_wave_beam_read: the flags of an earlier set are not this set's)
    // auto: not for a tree that misses L2 -- the walk's record loads then cost what the (cheap) culled rays saved and more: 1 M triangles 16.955 -> 16.990 ms per frame
    if (w->beamCull == 0 || (w->beamCull < 0 && (host.g.batch < 2 || !cacheResident))) return nullptr;
    if (!host.sc.hasBVH || !host.sc.wnodesW || host.g.nLocalTiles <= 0) return nullptr;
    for (bool stats : {false, true})
        if (rtl::trace_build(false, w->tune, trace_forms(host.sc), treeDepth, stats).nodes != rtl::TN_WNODESW) return nullptr;
    const size_t need = (size_t)host.g.nLocalTiles;
    if (w->beamCap < need) {
        if (w->beamDead) { if (hipStreamSynchronize(st) != hipSuccess) return nullptr; (void)hipFree(w->beamDead); }
        w->beamDead = nullptr;
        w->beamCap = 0;
        if (hipMalloc(&w->beamDead, need) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        w->beamCap = need;
    }
    w->beamLast = need;
    return w->beamDead;
}
int rt_wave_beam_cull(RtWave *w, hipStream_t st, unsigned long long *out4, bool reset) {
    for (int i = 0; i < 4; ++i) out4[i] = 0;
    if (!w) return RT_OK;
    W_STEP(wave_read_sums(w, st, w->beamAcc, 4, out4, reset));
    w->beamStatOn = true;
    return RT_OK;
}
int rt_wave_beam_read(RtWave *w, hipStream_t st, uint8_t *out, size_t n) {
    if (!w || !w->beamDead || w->beamLast == 0 || n != w->beamLast) { if (w) w->err = "no culled launch set of that many tiles"; return RT_ERR_STATE; }
    W_TRY(hipStreamSynchronize(st));
    W_TRY(hipMemcpy(out, w->beamDead, n, hipMemcpyDeviceToHost));
    return RT_OK;
}

void rt_wave_forget_share(RtWave *w) {
    if (!w) return;
    w->pool->q2Frac = 0.0;
    w->prevChunks = 0;   // the bounce counts of the launch set in flight belong to the old scene / frame size: not read
}

void rt_wave_set_probe_tree(RtWave *w, bool collapsed) { if (w) w->probeTree = collapsed; }
