// rt_trace.hpp -- persistent traversal ("ray scheduler", see rt_wave.hip): the closest- / any-hit kernel k_trace and its builds, the AO packet kernel, and the
// launches that size their persistent grids.
// Part of the rt_wave.hip translation unit: included by it alone, behind its `#pragma clang fp contract(off)` and `using namespace rtd;`.
#pragma once
#include <algorithm>
#include <map>
#include <tuple>
#include <utility>

#include "rt_trace_build.hpp"
#include "rt_trace_src.hpp"

using rtl::TraceTune;   // the scheduler's tunables and the switches of the environment: plain C++ (rt_trace_build.hpp), and k_trace's argument
using rtl::default_tune;
using rtl::tune_from_env;

namespace {
// hipcc sinks loads into the branches that first use them (e.g. a triangle's v0 behind the determinant test), which turns
// one gather round trip into two or three dependent ones.  pin() makes a loaded record "used" right after the loads were
// issued, so the whole group is in flight together.
RT_DEV void pin(float4 &v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }
// The traversal kernels pin whole 128-bit registers tuples: with four 32-bit constraints the register allocator is free to move the
// components apart from the tuple the load wrote, and did (19 v_mov per 4-wide node visit, about a tenth of the step's vector instructions --
// and these launches are bound by vector-instruction issue).
typedef float v4f __attribute__((ext_vector_type(4)));
RT_DEV void pin(v4f &v) { asm volatile("" : "+v"(v)); }

// ---- quad-cooperative record fetch (round 4; microbenchmark tools/gather2.hip) ------------------------------------
// The four lanes of a quad fetch ONE 64-byte record per instruction -- lane q piece q of the record quad-lane k stands on, k = 0..3 -- so a
// quad's load touches one line instead of four; a 4x4 transpose inside the quad (two butterfly stages of v_cndmask_b32_dpp: the select and the
// cross-lane read in one instruction, 32 per record set) then gives every lane the four pieces of ITS record.  Arithmetic and visit order are
// untouched.  All 64 lanes must be enabled where this runs (DPP reads of disabled lanes return the old destination).
template <int CTRL> RT_DEV int quad_bcast_i(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true); }
// one dword of a butterfly stage: a = keepA ? x : partner(y), b = keepB ? y : partner(x).  `a` is written while x, y are still read
// (early clobber); `b` is written by the last instruction and may reuse an input's register, so a stage needs one spare register, not eight.
// (the s_nop 1 sits INSIDE the block: a DPP source written by a VALU instruction needs two wait states, the assembler does not insert them in inline asm, and
// between two asm statements the compiler may place a copy for an operand -- ADVICE r04.  The s_mov that follows is a third instruction in between.)
#define RT_QT_PAIR(PERM, X, Y, A, B)                                                                                               \
    asm volatile("s_nop 1\n\ts_mov_b64 vcc, %[ka]\n\tv_cndmask_b32_dpp %[a], %[y], %[x], vcc quad_perm:" PERM " row_mask:0xf bank_mask:0xf\n\t" \
                 "s_mov_b64 vcc, %[kb]\n\tv_cndmask_b32_dpp %[b], %[x], %[y], vcc quad_perm:" PERM " row_mask:0xf bank_mask:0xf"      \
                 : [a] "=&v"(A), [b] "=v"(B) : [x] "v"(X), [y] "v"(Y), [ka] "s"(keepA), [kb] "s"(keepB) : "vcc")
RT_DEV void quad_transpose(v4f &r0, v4f &r1, v4f &r2, v4f &r3) {
    // in: r[k] of quad-lane q = piece q of record k; out: r[j] of quad-lane q = piece j of record q
    v4f a0, a1, a2, a3;
    {
        const unsigned long long keepA = 0x5555555555555555ull, keepB = 0xAAAAAAAAAAAAAAAAull;   // lane bit 0 clear / set
        RT_QT_PAIR("[1,0,3,2]", r0.x, r1.x, a0.x, a1.x); RT_QT_PAIR("[1,0,3,2]", r0.y, r1.y, a0.y, a1.y);
        RT_QT_PAIR("[1,0,3,2]", r0.z, r1.z, a0.z, a1.z); RT_QT_PAIR("[1,0,3,2]", r0.w, r1.w, a0.w, a1.w);
        RT_QT_PAIR("[1,0,3,2]", r2.x, r3.x, a2.x, a3.x); RT_QT_PAIR("[1,0,3,2]", r2.y, r3.y, a2.y, a3.y);
        RT_QT_PAIR("[1,0,3,2]", r2.z, r3.z, a2.z, a3.z); RT_QT_PAIR("[1,0,3,2]", r2.w, r3.w, a2.w, a3.w);
    }
    {
        const unsigned long long keepA = 0x3333333333333333ull, keepB = 0xCCCCCCCCCCCCCCCCull;   // lane bit 1 clear / set
        RT_QT_PAIR("[2,3,0,1]", a0.x, a2.x, r0.x, r2.x); RT_QT_PAIR("[2,3,0,1]", a0.y, a2.y, r0.y, r2.y);
        RT_QT_PAIR("[2,3,0,1]", a0.z, a2.z, r0.z, r2.z); RT_QT_PAIR("[2,3,0,1]", a0.w, a2.w, r0.w, r2.w);
        RT_QT_PAIR("[2,3,0,1]", a1.x, a3.x, r1.x, r3.x); RT_QT_PAIR("[2,3,0,1]", a1.y, a3.y, r1.y, r3.y);
        RT_QT_PAIR("[2,3,0,1]", a1.z, a3.z, r1.z, r3.z); RT_QT_PAIR("[2,3,0,1]", a1.w, a3.w, r1.w, r3.w);
    }
}

// lane position of the n-th (0-based) set bit of m (n < popcount(m)): binary search over popcounts
RT_DEV uint32_t nth_set(unsigned long long m, uint32_t n) {
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t w = 32u; w; w >>= 1) {
        const uint32_t c = (uint32_t)__popcll((m >> pos) & ((1ull << w) - 1ull));
        if (n >= c) { n -= c; pos += w; }
    }
    return pos;
}

// Diagnostic build only: how many cache accesses the lanes that call this together cost the vector L1 when each reads the record `key`.
// The texture addresser takes a wave's 16-byte lane-loads four adjacent lanes at a time and merges lanes of such a quad that read
// the same bytes (tools/gather.hip mode 6 under rocprofv3 --pmc: four adjacent lanes on one record = 0.25 accesses per lane-load);
// lanes further apart are not merged (the kernels' PMC access counts are 2-3 x their wave-wide distinct-record counts).
//   -> number of (quad, record) pairs = lanes whose key differs from every lower active lane of their quad.
RT_DEV uint32_t wave_distinct(uint32_t key) {   // distinct keys among the calling lanes
    unsigned long long m = __ballot(1);
    uint32_t n = 0;
    while (m) {
        const uint32_t k = (uint32_t)__shfl((int)key, __ffsll((long long)m) - 1, 64);
        m &= ~__ballot(key == k);
        n++;
    }
    return n;
}
RT_DEV uint32_t quad_distinct(uint32_t key) {
    const unsigned long long am = __ballot(1);
    const uint32_t lane = threadIdx.x & 63u, q0 = lane & ~3u;
    bool first = true;
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j) {
        const uint32_t kj = (uint32_t)__shfl((int)key, (int)(q0 + j), 64);
        if (j < (lane & 3u) && ((am >> (q0 + j)) & 1ull) && kj == key) first = false;
    }
    return (uint32_t)__popcll(__ballot(first));
}


// The slab test of rt_bvh.glsl:124-134 in two halves, so that the per-axis values of two child boxes can be merged into their parent's (k_trace, FUSE):
// slab_parts + slab_eval are slab() operation for operation.
struct SlabP { float sx, sy, sz, bx, by, bz; };
RT_DEV SlabP slab_parts(V3 ro, V3 rdInv, V3 bmin, V3 bmax) {
    const V3 t0 = (bmin - ro) * rdInv, t1 = (bmax - ro) * rdInv;
    SlabP p;
    p.sx = fminr(t0.x, t1.x); p.sy = fminr(t0.y, t1.y); p.sz = fminr(t0.z, t1.z);
    p.bx = fmaxr(t0.x, t1.x); p.by = fmaxr(t0.y, t1.y); p.bz = fmaxr(t0.z, t1.z);
    return p;
}
RT_DEV bool slab_eval(const SlabP &p, float &tminOut) {
    const float tmin = fmaxr(fmaxr(p.sx, p.sy), fmaxr(p.sz, 0.0f));
    const float tmax = fminr(fminr(p.bx, p.by), p.bz);
    tminOut = tmin;
    return tmax >= tmin;
}
// the parts of the box min(a.min, b.min) .. max(a.max, b.max): (x - ro) * rdInv is monotone in x, so the union's near / far plane distances are the smaller / larger
// of the two boxes' (v_min / v_max drop the NaN of 0 * inf and of an absent child's NaN box exactly as the direct evaluation does: tests/test_fused_nodes.py)
RT_DEV SlabP slab_union(const SlabP &a, const SlabP &b) {
    SlabP p;
    p.sx = fminr(a.sx, b.sx); p.sy = fminr(a.sy, b.sy); p.sz = fminr(a.sz, b.sz);
    p.bx = fmaxr(a.bx, b.bx); p.by = fmaxr(a.by, b.by); p.bz = fmaxr(a.bz, b.bz);
    return p;
}

template <bool ANY> struct StackOf { typedef StackEntry type; };          // closest: {deferred child, its entry distance}
template <> struct StackOf<true> { typedef uint32_t type; };              // any-hit: the pop-time cull never fires (tMax is constant)

// Per-lane traversal stacks live in dynamic LDS sized for THIS tree (stackEntries per lane): the resident workgroups per CU -- and
// with them the memory-level parallelism of these latency-bound loops -- follow from the scene's depth instead of from a few
// compiled-in sizes (1 M triangles, depth 18: 4 / 5 workgroups per CU for closest- / any-hit instead of 3 / 4 with 24- and 36-entry stacks).
extern __shared__ __align__(16) unsigned char rt_dyn_lds[];
// Register budget: the closest-hit launches run five workgroups per CU (their 8-byte stack entries fill the LDS first), so their kernels may use
// up to 96 VGPRs (five waves per SIMD) but not more; the diagnostic builds are unconstrained.
#ifndef RT_ANYHIT_WAVES
#define RT_ANYHIT_WAVES 7   // any-hit launches: 72 VGPRs, seven waves per SIMD (with the exact stack size of rt_upload_bvh seven workgroups fit a CU's LDS)
#endif
#ifndef RT_IMPL_ANYHIT_WAVES
#define RT_IMPL_ANYHIT_WAVES 6   // the implicit any-hit build at six waves per SIMD: at seven (72 VGPRs) it spills 32 B per lane into its inner loop (experiment 9)
#endif
// A k_trace build is named by its RT_BUILD_* bits (include/rt_mi355.h), unshifted and without RT_BUILD_LAUNCHED: OPT.  The waves per SIMD a build is held to:
constexpr int trace_waves(bool any, uint32_t opt) {
    const bool stats = (opt & RT_BUILD_STATS) != 0, leafb2 = (opt & RT_BUILD_LEAFB4) == 0;
    return (!stats && !any) ? 5 : (((opt & (RT_BUILD_NEAR | RT_BUILD_QN2)) != 0 || ((opt & RT_BUILD_IMPL) != 0 && RT_IMPL_ANYHIT_WAVES == 6)) ? 6 : (any && !stats && leafb2 ? RT_ANYHIT_WAVES : 1));
}
template <class Src, bool ANY, uint32_t OPT>
__global__ __launch_bounds__(256, trace_waves(ANY, OPT)) void k_trace(const DevFrame *__restrict__ fr, const float4 *__restrict__ wnodes, const float4 *__restrict__ tris, Src src,
                                                uint32_t *head, unsigned long long *tally, unsigned long long *gatherLoads, TraceTune tune,
                                                int stackEntries, unsigned long long *stats = nullptr, const float4 *__restrict__ leafBox = nullptr) {
    constexpr int LEAFB = (OPT & RT_BUILD_LEAFB4) ? 4 : 2, QN = (OPT & RT_BUILD_QN1) ? 1 : ((OPT & RT_BUILD_QN2) ? 2 : 0);
    constexpr bool STATS = (OPT & RT_BUILD_STATS) != 0, COOP = (OPT & RT_BUILD_COOP) != 0, NEAR = (OPT & RT_BUILD_NEAR) != 0, FUSE = (OPT & RT_BUILD_FUSE) != 0,
                   IMPL = (OPT & RT_BUILD_IMPL) != 0, TIMING = (OPT & RT_BUILD_TIMING) != 0;
    // STATS (diagnostic build only, RT_TRACE_STATS=1): [0] inner-node visits [1] leaf visits [2] triangle tests [3] inner-phase wave
    // iterations [4] active lanes summed over them [5] leaf-phase wave iterations [6] lanes with a leaf summed [7] refill rounds
    unsigned long long st_[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // [14] / [15]: the same with wave-wide merging (distinct records per wave step)   // [8] cycles in inner steps [9] in leaf phases [10] in refills [11] wave lifetime
    // [12] / [13] node / triangle gather loads after merging: adjacent lanes (a quad) that stand on the same record read the same 16-byte
    // pieces, which the vector L1 serves as one access (quad_distinct above) -- (quad, record) pairs per wave step x loads per record
    const unsigned long long tStart_ = (STATS || TIMING) ? clock64() : 0ull;
    // TIMING (RT_TRACE_TIMING=1, diagnostic build of the PRODUCTION kernels -- same registers and occupancy, nothing of the STATS build's counting): where a wave's cycles
    // go, from s_memtime stamps kept in scalar registers: [0] inner-phase iterations [1] cycles from the top of an iteration to the issue of its loads [2] from there to
    // their arrival (an explicit s_waitcnt vmcnt(0)) [3] from there to the end of the iteration [4] leaf phases [5] cycles in them [6] refill rounds [7] cycles in them
    // [8] wave lifetime
    unsigned long long tm_[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tA_ = 0, tB_ = 0, tC_ = 0;
    auto stamp_loads = [&]() {
        if constexpr (TIMING) { tB_ = clock64(); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); tC_ = clock64(); }
    };
    typedef typename StackOf<ANY>::type Entry;
    Entry *stk = reinterpret_cast<Entry *>(rt_dyn_lds) + (threadIdx.x >> 6) * stackEntries * 64 + (threadIdx.x & 63);
    DevScene sc = fr->sc;   // private copy: scene constants stay in SGPRs instead of being re-read per step
    sc.tris = tris;         // kernel-argument copies: known-global pointers (global_load, not flat_load)
    const float4 *__restrict__ nodes = wnodes;   // 2-wide records for closest-hit, 4-wide records for any-hit
    const float eps = fr->u.eps, inf = fr->u.inf;
    src.prepare();
    const uint32_t n = src.size();
    const uint32_t lane = threadIdx.x & 63;
    // run length: RT_CHUNK, else about a third of a wave's share of the queue, in [128, 384] rays (measured on MI355X, 1080p / 4 spp:
    // whole frame 2.42 / 2.26 / 2.18 / 2.20 ms with runs of 64 / 128 / 256 / 512; one rank of eight 0.51 / 0.48 / 0.52 / 0.55; round 3, batches
    // of eight frames, 1.83 / 1.78 / 1.79 ms per frame with runs of at most 256 / 384 / 512)
    // round 4 (seven-wave any-hit kernels, larger grids): at most 768 -- 1.669 against 1.678 / 1.695 / 1.70 ms per frame with runs of at most 512 / 384 / 1024
    // primary launch (chunkMax 256): runs of 64 candidates = one 8x8 pixel block were right for single frames traced alone (rounds 1-3); with batches of
    // frames and four launch sets in flight 256 are: 1.613 against 1.640 ms per frame, frame by frame 1.805 against 1.825, one rank of eight 0.225 against 0.230
    const uint32_t runLen = tune.chunk > 0 ? (uint32_t)max(tune.chunk, 8)
                                           : min((uint32_t)tune.chunkMax, max(128u, ((n / (3u * 4u * gridDim.x) + 63u) / 64u) * 64u));

    // per-lane ray state
    V3 ro = mk3(0.0f), rd = mk3(0.0f), rdInv = mk3(0.0f);
    float tBest = 0.0f;          // closest: best t so far; any: tMax
    int triBest = -1;
    int ref = 0, sp = 0;
    int leaf = 0;                // any-hit only: one postponed leaf (0 = none; leaf refs are negative)
    uint32_t rayId = 0;
    bool active = false;
    bool exhausted = (n == 0);
    uint32_t traced = 0;
    uint32_t gathers = 0;        // 16-byte gather loads this lane issued for nodes and triangles (the L1 gather roofline's unit)
    uint32_t runNext = 0, runEnd = 0;   // wave-uniform: the part of the current run not handed out yet
    const uint32_t shard = (blockIdx.x * 4u + (threadIdx.x >> 6)) % kShards;   // home shard of this wave
    bool homeDry = false;
    // Guided run lengths (RT_GUIDED=1 / 2, measured option of round 4, off): the rays dealt LAST go out in short runs -- `lateRays` (about an eighth of the
    // queue, a multiple of runLen) in runs of runLen / 8 (at least 64) -- so that the launch does not end with a few waves still working through a long run
    // each.  Alone the bounce launch gains 2 %; with four launch sets in flight, which fill each other's tails anyway, the frame is 1-2 % slower
    // (profiles/r04_experiments.txt 13).  Dealing order d = 0 .. nRuns - 1: the nEarly long runs first, then the short ones.
    const bool guided = tune.guided == 1 || (tune.guided == 2 && !ANY);   // 2: closest-hit launches only
    const uint32_t shortLen = guided ? max(64u, runLen / 8u) : runLen;
    const uint32_t lateRays = (guided && n > 16u * runLen) ? (n / 8u / runLen) * runLen : 0u;
    const uint32_t nEarly = (n - lateRays + runLen - 1u) / runLen;
    const uint32_t nRuns = nEarly + (lateRays + shortLen - 1u) / shortLen;

    // pop the next subtree of this lane's ray, or retire the ray
    auto pop_or_finish = [&]() {
        bool found = false;
        while (sp > 0) {
            sp--;
            if constexpr (ANY) {
                const int r = (int)stk[sp * 64];
                if (r < 0 && leaf == 0) { leaf = r; continue; }   // leaves wait in `leaf`; keep looking for an inner node
                ref = r;                                          // an inner node, or a second leaf (the lane then waits)
                found = true;
                break;
            } else {
                StackEntry e = stk[sp * 64];
                if (u2f(e.y) > tBest) continue;   // rt_bvh.glsl:208 cull
                ref = (int)e.x;
                found = true;
                break;
            }
        }
        if (!found) {
            if constexpr (ANY) {
                ref = RT_NO_CHILD;
                if (leaf == 0) { src.store_any(rayId, false); active = false; }   // else: the postponed leaf is all that is left
            } else {
                src.store_closest(rayId, triBest >= 0 ? tBest : inf, triBest);
                active = false;
            }
        }
    };

    for (;;) {
        // ---- scheduler: idle lanes take the next rays of this wave's current run (`runLen` consecutive rays: same ray
        // type, neighbouring pixels).  Runs are dealt by kShards cursors, each on its own 128-byte line: shard s owns
        // runs s, s+kShards, ...; a wave draws from its home shard and steals round-robin once that is dry.  (One shared
        // cursor word sustains only ~88 M atomics/s on MI355X -- per-refill, then per-run atomics on a single word
        // bounded earlier versions of this kernel; a purely static deal leaves the bounce-ray tail unbalanced.)
        // quadRefill: only quads of four adjacent lanes that are idle together take new rays, four consecutive ones: the vector L1 merges
        // the loads of adjacent lanes that stand on the same record (quad_distinct), and rays dealt together walk the top of the tree together
        auto whole_quads = [&](unsigned long long m) {
            if (!tune.quadRefill) return m;
            unsigned long long q = m & (m >> 1) & (m >> 2) & (m >> 3) & 0x1111111111111111ull;
            return q | (q << 1) | (q << 2) | (q << 3);
        };
        unsigned long long idleMask = whole_quads(__ballot(!active));
        int nIdle = __popcll(idleMask);
        if (!exhausted && nIdle >= tune.refillMin) {
            const unsigned long long tR_ = (STATS || TIMING) ? clock64() : 0ull;
            if (STATS && lane == 0) st_[7]++;
            if (runNext >= runEnd) {
                // shard s owns runs s, s + kShards, ...: k = 0 .. runsOf(s)-1
                auto runsOf = [&](uint32_t sh) { return sh < nRuns ? (nRuns - sh + kShards - 1u) / kShards : 0u; };
                uint32_t k = 0, from = shard;
                bool got = false;
                if (!homeDry) {                       // live phase: one atomic per run on the home shard
                    if (lane == 0) k = atomicAdd(&head[shard * kShardStride], 1u);
                    k = __shfl(k, 0, 64);
                    got = k < runsOf(shard);
                    homeDry = !got;
                }
                while (!got) {                        // stealing / drain: ONE 64-lane probe of all cursors, then one atomic
                    const uint32_t cur = __hip_atomic_load(&head[lane * kShardStride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    unsigned long long open = __ballot(cur < runsOf(lane));
                    if (open == 0ull) break;
                    // first open shard at or after the home shard (rotate so that waves spread over the open shards)
                    const unsigned long long rot = (open >> shard) | (shard ? (open << (64u - shard)) : 0ull);
                    from = (shard + (uint32_t)__ffsll((long long)rot) - 1u) % kShards;
                    if (lane == 0) k = atomicAdd(&head[from * kShardStride], 1u);
                    k = __shfl(k, 0, 64);
                    got = k < runsOf(from);           // lost a race for the last run of that shard: probe again
                }
                if (!got) { exhausted = true; continue; }
                // any-hit queues are dealt from their END (round 4): the expensive rays -- bounce-hit shadow rays, then the disk / sun / point slots -- sit behind
                // the cheap AO slots, and a launch that starts with its longest work ends with short runs instead of a tail of long ones
                const uint32_t dIdx = k * kShards + from;           // place in the dealing order
                const bool late = dIdx >= nEarly;
                const uint32_t len = late ? shortLen : runLen;
                const uint32_t span = late ? lateRays : n - lateRays;   // rays of the region this run belongs to
                const uint32_t off = (late ? dIdx - nEarly : dIdx) * len;   // offset inside the region, in dealing order
                const uint32_t cnt = min(len, span - off);
                if (ANY && tune.reverse) {                          // region layout: [late | early], each dealt from its end
                    const uint32_t top = late ? lateRays : n;
                    runEnd = top - off;
                    runNext = runEnd - cnt;
                } else {                                            // [early | late], each dealt from its beginning
                    runNext = (late ? n - lateRays : 0u) + off;
                    runEnd = runNext + cnt;
                }
            }
            // Deal the run's LIVE rays to the idle lanes, one 64-slot window per pass: every lane probes one slot's liveness word
            // (coalesced), the live slots go to the idle lanes in order and dead slots cost nothing further.  (Before, a refill
            // handed out `idle lanes` consecutive slots dead or alive and went round again: with 55 % of the shadow queue's slots
            // dead, three rounds -- each a full scheduler iteration -- to fill half a wave.)
            // a lane starts on the ray it was given (record in ro / rd, any-hit limit tMax)
            auto start_ray = [&](float tMax, uint32_t token) {
                rayId = token;
                traced++;
                rdInv = mk3(1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z);
                tBest = (ANY || QueryTMax<Src>::value) ? tMax : inf;
                triBest = -1;
                sp = 0;
                leaf = 0;
                ref = ANY ? sc.rootRef4 : sc.rootRefW;
                if (ANY && ref < 0) { leaf = ref; ref = RT_NO_CHILD; }   // single-leaf tree
                float tmin;
                bool in = sc.hasBVH && !tune.skipTraversal && slab(ro, rdInv, ld3(sc.rootMin), ld3(sc.rootMax), tmin) && !(tmin > tBest);
                if (in) active = true;
                else if (ANY) src.store_any(token, false);
                else src.store_closest(token, inf, -1);
            };
            unsigned long long idleLeft = idleMask;
            while (idleLeft != 0ull && runNext < runEnd) {
                uint32_t window = min(64u, runEnd - runNext);
                if constexpr (MaskedSrc<Src>::value) {
                    // Light-slot liveness masks: behind the dense slots a slot's liveness is one bit.  The lanes read the mask words of the run's
                    // next segment -- the slots left that share a queue slot: consecutive bits -- in one coalesced load; the i-th idle lane gets the i-th set
                    // bit, across all words of the segment, with no further memory access; the takers then read tMax and record together.  Two round trips per
                    // refill pass, however many dead slots lie in between, instead of two per 64-slot window.
                    if (src.masked()) {
                        const uint32_t dEnd = src.dense_end();
                        if (runNext >= dEnd && runNext < src.masked_end()) {
                            MaskSeg sg = src.segment(runNext, runEnd);
                            const uint32_t sh = sg.bit & 63u;
                            sg.len = min(sg.len, 4096u - sh);                         // one word per lane (RT_CHUNK allows longer runs: the rest is the next pass's)
                            const uint32_t endBit = sh + sg.len, nW = (endBit + 63u) >> 6;
                            unsigned long long word = 0ull;
                            if (lane < nW) word = sg.live[(sg.bit >> 6) + lane];
                            if (lane == 0u) word &= ~0ull << sh;                      // bits in front of the segment and behind it: other runs, the next slot
                            if (lane == nW - 1u && (endBit & 63u) != 0u) word &= ~0ull >> (64u - (endBit & 63u));
                            const uint32_t nIdleL = (uint32_t)__popcll(idleLeft);
                            const uint32_t rank = (uint32_t)__popcll(idleLeft & ((1ull << lane) - 1ull));
                            const bool idleMe = ((idleLeft >> lane) & 1ull) != 0ull;
                            bool takes = false;
                            unsigned long long mineW = 0ull;                          // the word this lane's slot is in, its place in the segment, the slot's rank in it
                            uint32_t mineAt = 0u, mineN = 0u;
                            uint32_t taken = 0u, stop = endBit;                       // live slots handed out so far; first bit of the segment that is NOT used up
                            for (uint32_t w = 0; w < nW; ++w) {
                                const unsigned long long mw = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(word >> 32), (int)w) << 32) |
                                                              (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)word, (int)w);
                                const uint32_t c = (uint32_t)__popcll(mw);
                                if (c == 0u) continue;
                                if (idleMe && rank >= taken && rank - taken < c) { takes = true; mineW = mw; mineAt = w * 64u; mineN = rank - taken; }
                                if (taken + c > nIdleL) { stop = w * 64u + nth_set(mw, nIdleL - taken); break; }   // more live slots than idle lanes: the rest stays
                                taken += c;
                            }
                            if (takes) {
                                uint32_t token;
                                const float tMax = src.take_live(sg.a + (mineAt + nth_set(mineW, mineN) - sh), ro, rd, token);
                                start_ray(tMax, token);
                            }
                            if (lane == 0u) if (unsigned long long *ms = src.mask_stat()) { atomicAdd(&ms[0], (unsigned long long)nW); atomicAdd(&ms[1], 1ull); }
                            runNext += stop - sh;
                            idleLeft = whole_quads(__ballot(!active));               // root misses may draw again
                            continue;
                        }
                        if (runNext < dEnd) window = min(window, dEnd - runNext);   // the dense slots in front are probed as ever, but not beyond them: a dead light slot has no tMax word
                    }
                }
                if (tune.denseTake && src.dense(runNext, runNext + window)) {
                    // dense slots: no probe -- the i-th idle lane reads the i-th entry left, liveness word and record in ONE round trip
                    const uint32_t nIdleL = (uint32_t)__popcll(idleLeft);
                    const uint32_t nTake = min(window, nIdleL);
                    const uint32_t rank = (uint32_t)__popcll(idleLeft & ((1ull << lane) - 1ull));
                    if (((idleLeft >> lane) & 1ull) && rank < nTake) {
                        uint32_t token;
                        const float tMax = src.probe_take(runNext + rank, ro, rd, token);
                        if (!(tMax < 0.0f)) start_ray(tMax, token);
                    }
                    runNext += nTake;
                    idleLeft = whole_quads(__ballot(!active));
                    continue;
                }
                float t = -1.0f;
                typename Src::Payload pl{};
                if (lane < window) t = src.probe(runNext + lane, pl);
                const unsigned long long liveMask = __ballot(lane < window && !(t < 0.0f));
                const uint32_t nLiveW = (uint32_t)__popcll(liveMask), nIdleL = (uint32_t)__popcll(idleLeft);
                const uint32_t nTake = min(nLiveW, nIdleL);
                const uint32_t rank = (uint32_t)__popcll(idleLeft & ((1ull << lane) - 1ull));
                const bool takes = ((idleLeft >> lane) & 1ull) && rank < nTake;
                const uint32_t e = takes ? nth_set(liveMask, rank) : lane;      // window entry this lane takes
                const float tMax = __shfl(t, (int)e, 64);
                const typename Src::Payload mine = Src::route(pl, (int)e);
                if (takes) {
                    uint32_t token;
                    src.take(runNext + e, mine, ro, rd, token);
                    start_ray(tMax, token);
                }
                // all live slots taken: the window is used up; else everything before the first live slot left over
                runNext += nLiveW <= nIdleL ? window : nth_set(liveMask, nTake);
                idleLeft = whole_quads(__ballot(!active));                     // root misses may draw again
            }
            if (STATS && lane == 0) st_[10] += clock64() - tR_;
            if constexpr (TIMING) { tm_[6]++; tm_[7] += clock64() - tR_; }
            continue;   // lanes that drew a dead slot or a root miss may draw again
        }
        if (__ballot(active) == 0ull) {
            if (exhausted) break;
            continue;
        }
        // ---- phase 1: walk inner nodes until (almost) every live lane holds a leaf
        for (;;) {
            const bool searching = active && (uint32_t)ref < (uint32_t)RT_NO_CHILD;   // an inner node in hand
            const unsigned long long sm = __ballot(searching);
            if (sm == 0ull) break;
            if (__popcll(sm) < tune.minSearch && __ballot(active && (ANY ? leaf != 0 : ref < 0)) != 0ull) break;   // keep the leaf phase dense
            const unsigned long long tI_ = STATS ? clock64() : 0ull;
            if constexpr (TIMING) { tA_ = clock64(); tB_ = tC_ = 0; }
            if (STATS && lane == 0) { st_[3]++; st_[4] += (unsigned long long)__popcll(sm); }
            // COOP (closest-hit, RT_COOP=1): the quad fetches its searching lanes' records together, then transposes (see quad_transpose)
            v4f ca = {0, 0, 0, 0}, cb = ca, cc = ca, cd = ca;
            if constexpr (COOP && !ANY) {
                const uint32_t q = lane & 3u;
                const int me = searching ? ref : -1;
                const int i0 = quad_bcast_i<0x00>(me), i1 = quad_bcast_i<0x55>(me), i2 = quad_bcast_i<0xAA>(me), i3 = quad_bcast_i<0xFF>(me);
                const v4f *nv = reinterpret_cast<const v4f *>(nodes) + q;
                if (i0 >= 0) ca = nv[(size_t)i0 * 4];
                if (i1 >= 0) cb = nv[(size_t)i1 * 4];
                if (i2 >= 0) cc = nv[(size_t)i2 * 4];
                if (i3 >= 0) cd = nv[(size_t)i3 * 4];
                pin(ca); pin(cb); pin(cc); pin(cd);
                quad_transpose(ca, cb, cc, cd);
            }
            if (searching) {
                if (STATS) { st_[0]++; const uint32_t dk = quad_distinct((uint32_t)ref), dw = wave_distinct((uint32_t)ref); if (lane == (uint32_t)(__ffsll((long long)sm) - 1)) { st_[12] += dk * (ANY ? 7u : (IMPL ? 3u : 4u)); st_[14] += dw * (ANY ? 7u : (IMPL ? 3u : 4u)); } }
                gathers += ANY ? (QN ? 4u : 7u) : 4u;
                if constexpr (ANY) {
                    int r0, r1, r2, r3;
                    float t0, t1, t2, t3;
                    bool h0, h1, h2, h3;
                    // IMPL (RT_IMPLICIT=1, trees whose leaves sit at one depth D): `ref` = depth << 24 | path of an even-depth node; its children are (d + 2, 4p + j) -- leaves
                    // -(4p + j + 1) when d + 2 == D, the two leaves -(2p + j + 1) when d + 1 == D -- so the record carries no references: six loads instead of seven
                    // (quantised: three instead of four), at the node's pre-order position
                    uint32_t dN = 0, pN = 0, atN = 0;
                    auto impl_refs = [&]() {
                        const uint32_t D = (uint32_t)sc.implD;
                        if (dN + 1u == D) { r0 = -(int)(2u * pN + 1u); r1 = -(int)(2u * pN + 2u); r2 = RT_NO_CHILD; r3 = RT_NO_CHILD; }
                        else if (dN + 2u == D) { r0 = -(int)(4u * pN + 1u); r1 = -(int)(4u * pN + 2u); r2 = -(int)(4u * pN + 3u); r3 = -(int)(4u * pN + 4u); }
                        else { const int b = (int)(((dN + 2u) << 24) | (4u * pN)); r0 = b; r1 = b + 1; r2 = b + 2; r3 = b + 3; }
                    };
                    if constexpr (IMPL) {
                        dN = (uint32_t)ref >> 24; pN = (uint32_t)ref & 0x00ffffffu;
                        atN = dN - (uint32_t)__popc(pN) + (pN << ((uint32_t)sc.implD - dN));
                        gathers -= 1u;      // (one load fewer than counted above)
                    }
                    if constexpr (QN) {
                        // RT_QNODES: 64-byte node, child boxes as bytes on the node's own grid (rt_upload_bvh): box = fmaf(byte, 2^e, origin) per component,
                        // checked at upload to contain the child's box; then the slab test of the exact kernel on the decoded floats
                        const v4f *ndv = IMPL ? reinterpret_cast<const v4f *>(nodes) + (size_t)atN * 3 : reinterpret_cast<const v4f *>(nodes + (size_t)ref * 4);
                        v4f p0 = ndv[0], p1 = ndv[1], p2 = ndv[2], p3 = {0, 0, 0, 0};
                        if constexpr (!IMPL) p3 = ndv[3];
                        pin(p0); pin(p1); pin(p2); pin(p3);
                        if constexpr (IMPL) impl_refs();
                        else { r0 = (int)f2u(p3.x); r1 = (int)f2u(p3.y); r2 = (int)f2u(p3.z); r3 = (int)f2u(p3.w); }
                        const uint32_t ex = f2u(p0.w);
                        const float sx = u2f((ex & 0xffu) << 23), sy = u2f(((ex >> 8) & 0xffu) << 23), sz = u2f(((ex >> 16) & 0xffu) << 23);
                        const uint32_t lx = f2u(p1.x), ly = f2u(p1.y), lz = f2u(p1.z), hx = f2u(p1.w), hy = f2u(p2.x), hz = f2u(p2.y);
                        auto box = [&](int k, float &t) {
                            const V3 lo = mk3(__builtin_fmaf((float)((lx >> (8 * k)) & 0xffu), sx, p0.x), __builtin_fmaf((float)((ly >> (8 * k)) & 0xffu), sy, p0.y),
                                              __builtin_fmaf((float)((lz >> (8 * k)) & 0xffu), sz, p0.z));
                            const V3 hi = mk3(__builtin_fmaf((float)((hx >> (8 * k)) & 0xffu), sx, p0.x), __builtin_fmaf((float)((hy >> (8 * k)) & 0xffu), sy, p0.y),
                                              __builtin_fmaf((float)((hz >> (8 * k)) & 0xffu), sz, p0.z));
                            return slab(ro, rdInv, lo, hi, t) && t <= tBest;
                        };
                        h0 = box(0, t0) && r0 != RT_NO_CHILD;
                        h1 = box(1, t1) && r1 != RT_NO_CHILD;
                        h2 = box(2, t2) && r2 != RT_NO_CHILD;
                        h3 = box(3, t3) && r3 != RT_NO_CHILD;
                    } else {
                    // 4-wide node: up to four grandchild boxes per 128-byte record, order irrelevant for any-hit
                    // component-wise: [min.x x4][min.y x4][min.z x4][max.x x4][max.y x4][max.z x4][ref x4] = 7 loads, 8th piece unused
                    const v4f *ndv = IMPL ? reinterpret_cast<const v4f *>(nodes) + (size_t)atN * 6 : reinterpret_cast<const v4f *>(nodes + (size_t)ref * 8);
                    v4f q0 = ndv[0], q1 = ndv[1], q2 = ndv[2], q3 = ndv[3], q4 = ndv[4], q5 = ndv[5], q6 = {0, 0, 0, 0};
                    if constexpr (!IMPL) q6 = ndv[6];
                    pin(q0); pin(q1); pin(q2); pin(q3); pin(q4); pin(q5); pin(q6);
                    stamp_loads();
                    if constexpr (IMPL) impl_refs();
                    else { r0 = (int)f2u(q6.x); r1 = (int)f2u(q6.y); r2 = (int)f2u(q6.z); r3 = (int)f2u(q6.w); }
                    h0 = slab(ro, rdInv, mk3(q0.x, q1.x, q2.x), mk3(q3.x, q4.x, q5.x), t0) && t0 <= tBest;
                    h1 = slab(ro, rdInv, mk3(q0.y, q1.y, q2.y), mk3(q3.y, q4.y, q5.y), t1) && t1 <= tBest;
                    // absent children carry NaN boxes: with v_min/v_max NaN semantics their slab test is false, so all
                    // loads are issued up front and the four tests are branch-free (no dependent "is there a child" round trip)
                    h2 = slab(ro, rdInv, mk3(q0.z, q1.z, q2.z), mk3(q3.z, q4.z, q5.z), t2) && t2 <= tBest;
                    h3 = slab(ro, rdInv, mk3(q0.w, q1.w, q2.w), mk3(q3.w, q4.w, q5.w), t3) && t3 <= tBest;
                    }
                    // Any-hit order is free, so leaves are postponed: the first leaf met goes to `leaf`, the lane goes on with an
                    // inner child (or pops one), and leaves are tested in the leaf phase when (nearly) every lane holds one --
                    // both phases run with more lanes busy than when a lane stops at its first leaf.
                    int nxt = RT_NO_CHILD;
                    auto take = [&](bool h, int r) {
                        if (!h) return;
                        if (r < 0 && leaf == 0) { leaf = r; return; }
                        if (nxt == RT_NO_CHILD) { nxt = r; return; }
                        if (r >= 0 && nxt < 0) { const int t = nxt; nxt = r; r = t; }   // go on with the inner node, defer the leaf
                        stk[sp * 64] = (uint32_t)r;
                        sp++;
                    };
                    if constexpr (NEAR) {
                        // RT_NEAR_FIRST=1 (experiment, round 4): go on with the NEAREST inner child that was hit instead of the first in record order -- an
                        // occluded ray then tends to meet its occluder sooner; the answer (an OR over leaves) does not depend on the order
                        float kb = h0 && r0 >= 0 ? t0 : 3.0e38f;
                        int ib = 0;
                        const float k1 = h1 && r1 >= 0 ? t1 : 3.0e38f, k2 = h2 && r2 >= 0 ? t2 : 3.0e38f, k3 = h3 && r3 >= 0 ? t3 : 3.0e38f;
                        if (k1 < kb) { kb = k1; ib = 1; }
                        if (k2 < kb) { kb = k2; ib = 2; }
                        if (k3 < kb) { kb = k3; ib = 3; }
                        if (ib == 1) { const bool th = h0; h0 = h1; h1 = th; const int tr_ = r0; r0 = r1; r1 = tr_; }
                        if (ib == 2) { const bool th = h0; h0 = h2; h2 = th; const int tr_ = r0; r0 = r2; r2 = tr_; }
                        if (ib == 3) { const bool th = h0; h0 = h3; h3 = th; const int tr_ = r0; r0 = r3; r3 = tr_; }
                        // (a leaf child in position 0 goes to `leaf` or the stack as before: `take` prefers inner nodes for nxt)
                    }
                    take(h0, r0); take(h1, r1); take(h2, r2); take(h3, r3);
                    if (nxt == RT_NO_CHILD) pop_or_finish();
                    else ref = nxt;
                } else if constexpr (IMPL) {
                    // Implicit records (round 5, rt_upload_bvh): every leaf at depth D, so a node is (depth d, path p), `ref` = d << 24 | p, its children (d + 1, 2p)
                    // and (d + 1, 2p + 1), a leaf the reference -(p + 1); the record -- the two child boxes, 48 bytes, THREE loads instead of four -- sits at the
                    // node's pre-order position.  Boxes, tests, order and stack contents are those of the 64-byte records below.
                    const uint32_t dN = (uint32_t)ref >> 24, pN = (uint32_t)ref & 0x00ffffffu;
                    const uint32_t at = dN - (uint32_t)__popc(pN) + (pN << ((uint32_t)sc.implD - dN));
                    const v4f *ndv = reinterpret_cast<const v4f *>(nodes) + (size_t)at * 3;
                    v4f a = ndv[0], b = ndv[1], c = ndv[2];
                    pin(a); pin(b); pin(c);
                    stamp_loads();
                    gathers -= 1u;                                              // (4 were counted above)
                    float tL, tR;
                    const bool hitL = slab(ro, rdInv, mk3(a.x, a.y, a.z), mk3(a.w, b.x, b.y), tL) && tL <= tBest;
                    const bool hitR = slab(ro, rdInv, mk3(b.z, b.w, c.x), mk3(c.y, c.z, c.w), tR) && tR <= tBest;
                    const bool lastLevel = dN + 1u == (uint32_t)sc.implD;
                    const int refL = lastLevel ? -(int)(2u * pN + 1u) : (int)(((dN + 1u) << 24) | (2u * pN));
                    const int refR = lastLevel ? -(int)(2u * pN + 2u) : (int)(((dN + 1u) << 24) | (2u * pN + 1u));
                    if (hitL && hitR) {
                        const bool leftFirst = tL < tR;
                        StackEntry e;
                        e.x = (uint32_t)(leftFirst ? refR : refL);
                        e.y = f2u(leftFirst ? tR : tL);
                        stk[sp * 64] = e;
                        sp++;
                        ref = leftFirst ? refL : refR;
                    } else if (hitL || hitR) {
                        ref = hitL ? refL : refR;
                    } else pop_or_finish();
                } else if constexpr (FUSE) {
                    // Fused records (round 5, rt_upload_bvh): `ref` names a hub N -- an even-level inner node whose 128-byte record holds the 64-byte records of its
                    // two children A and B -- or, with kPair set, ONE of those children (a far child the step at N deferred).  A full step is the reference's step
                    // at N (rt_bvh.glsl:226-239: both child boxes, near one first, far one deferred with its entry distance) followed at once by its step at the
                    // near child X, from one round trip of eight loads; a pair step is the step at the deferred child alone (four loads).  The boxes of A and B are
                    // the unions of their children's (checked at upload), so their slab values are merged from the grandchildren's: same floats, same decisions,
                    // same visiting order as the two-wide walk below -- the stack holds what it would hold (one entry per binary level).
                    constexpr uint32_t kPair = 0x40000000u, kHalfB = 0x20000000u, kIdx = 0x1fffffffu;
                    const uint32_t code = (uint32_t)ref;
                    const bool pairStep = (code & kPair) != 0u;
                    const uint32_t hub = code & kIdx;
                    const v4f *ndv = reinterpret_cast<const v4f *>(nodes + (size_t)hub * 8) + ((pairStep && (code & kHalfB)) ? 4 : 0);
                    v4f x0 = ndv[0], x1 = ndv[1], x2 = ndv[2], x3 = ndv[3];     // the half the walk goes into (full step: A, swapped below when B is nearer)
                    v4f y0 = {0, 0, 0, 0}, y1 = y0, y2 = y0, y3 = y0;
                    if (!pairStep) { y0 = ndv[4]; y1 = ndv[5]; y2 = ndv[6]; y3 = ndv[7]; }
                    pin(x0); pin(x1); pin(x2); pin(x3); pin(y0); pin(y1); pin(y2); pin(y3);
                    gathers += pairStep ? 0u : 4u;      // (4 were counted above)
                    SlabP pX1 = slab_parts(ro, rdInv, mk3(x0.x, x0.y, x0.z), mk3(x1.x, x1.y, x1.z));
                    SlabP pX2 = slab_parts(ro, rdInv, mk3(x2.x, x2.y, x2.z), mk3(x3.x, x3.y, x3.z));
                    int g1 = (int)f2u(x0.w), g2 = (int)f2u(x1.w);              // X's children (g2 == RT_NO_CHILD: X is a leaf, g1 its reference)
                    bool enter = true;
                    if (!pairStep) {
                        const SlabP pY1 = slab_parts(ro, rdInv, mk3(y0.x, y0.y, y0.z), mk3(y1.x, y1.y, y1.z));
                        const SlabP pY2 = slab_parts(ro, rdInv, mk3(y2.x, y2.y, y2.z), mk3(y3.x, y3.y, y3.z));
                        float tA, tB;
                        const bool hitA = slab_eval(slab_union(pX1, pX2), tA) && tA <= tBest;
                        const bool hitB = slab_eval(slab_union(pY1, pY2), tB) && tB <= tBest;
                        const bool goB = hitB && !(hitA && tA < tB);           // both hit: leftFirst = tA < tB (rt_bvh.glsl:232)
                        enter = hitA || hitB;
                        if (hitA && hitB) {                                     // defer the far child: a leaf as itself, an inner node as (hub, half)
                            const int f1 = goB ? g1 : (int)f2u(y0.w), f2 = goB ? g2 : (int)f2u(y1.w);
                            StackEntry e;
                            e.x = f2 == RT_NO_CHILD ? (uint32_t)f1 : (kPair | (goB ? 0u : kHalfB) | hub);
                            e.y = f2u(goB ? tA : tB);
                            stk[sp * 64] = e;
                            sp++;
                        }
                        if (goB) { pX1 = pY1; pX2 = pY2; g1 = (int)f2u(y0.w); g2 = (int)f2u(y1.w); }
                    }
                    if (!enter) pop_or_finish();
                    else if (g2 == RT_NO_CHILD) ref = g1;                       // the near child is a leaf: the leaf phase takes it
                    else {                                                      // the reference's step at the near child X
                        float t1, t2;
                        const bool h1 = slab_eval(pX1, t1) && t1 <= tBest;
                        const bool h2 = slab_eval(pX2, t2) && t2 <= tBest;
                        if (h1 && h2) {
                            const bool leftFirst = t1 < t2;
                            StackEntry e;
                            e.x = (uint32_t)(leftFirst ? g2 : g1);
                            e.y = f2u(leftFirst ? t2 : t1);
                            stk[sp * 64] = e;
                            sp++;
                            ref = leftFirst ? g1 : g2;
                        } else if (h1 || h2) {
                            ref = h1 ? g1 : g2;
                        } else pop_or_finish();
                    }
                } else {
                    const float4 *nd = nodes + (size_t)ref * 4;
                    const v4f *ndv = reinterpret_cast<const v4f *>(nd);
                    v4f a, b, c, d;
                    if constexpr (COOP) { a = ca; b = cb; c = cc; d = cd; }
                    else { a = ndv[0]; b = ndv[1]; c = ndv[2]; d = ndv[3]; pin(a); pin(b); pin(c); pin(d); stamp_loads(); }
                    float tL, tR;
                    bool hitL = slab(ro, rdInv, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), tL) && tL <= tBest;
                    bool hitR = slab(ro, rdInv, mk3(c.x, c.y, c.z), mk3(d.x, d.y, d.z), tR) && tR <= tBest;
                    int refL = (int)f2u(a.w), refR = (int)f2u(b.w);
                    if (hitL && hitR) {
                        bool leftFirst = tL < tR;
                        StackEntry e;
                        e.x = (uint32_t)(leftFirst ? refR : refL);
                        e.y = f2u(leftFirst ? tR : tL);
                        stk[sp * 64] = e;
                        sp++;
                        ref = leftFirst ? refL : refR;
                    } else if (hitL || hitR) {
                        ref = hitL ? refL : refR;
                    } else pop_or_finish();
                }
            }
            if (STATS) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); if (lane == 0) st_[8] += clock64() - tI_; }
            if constexpr (TIMING) { const unsigned long long tD = clock64(); tm_[0]++; if (tB_) { tm_[1] += tB_ - tA_; tm_[2] += tC_ - tB_; tm_[3] += tD - tC_; } }
        }
        // ---- phase 2: leaves
        const unsigned long long tL_ = (STATS || TIMING) ? clock64() : 0ull;
        const int leafNow = ANY ? leaf : ref;   // any-hit: the postponed leaf; closest: the leaf the walk stopped at
        if (STATS) { unsigned long long lm = __ballot(active && leafNow < 0); if (lane == 0 && lm) { st_[5]++; st_[6] += (unsigned long long)__popcll(lm); } }
        if (active && leafNow < 0) {
            if (STATS) st_[1]++;
            int v = -leafNow - 1;
            int first = v >> 3, count = (v & 7) + 1;   // first: pair record, count: triangles
            if constexpr (IMPL) { first = v * sc.implR; count = 2; }   // implicit records: leaf v owns the records from v * R on; its count arrives with the first of them (below)
            bool done = false;
            // RT_QNODES: the leaf's exact box (the test the 112-byte node makes in the parent) -- fetched together with the first triangle group, tested after it
            bool boxOK = true;
            v4f lb0 = {0, 0, 0, 0}, lb1 = lb0;
            if constexpr (QN) {
                const uint32_t at = IMPL ? (uint32_t)v : (sc.leafBoxMagic ? __umulhi((uint32_t)first, sc.leafBoxMagic) : (uint32_t)first);   // implicit records: the leaf's ordinal
                const v4f *lb = reinterpret_cast<const v4f *>(leafBox) + (size_t)at * 2;
                lb0 = lb[0]; lb1 = lb[1];
                gathers += 2u;
            }
            auto gate = [&]() {
                if constexpr (QN) {
                    pin(lb0); pin(lb1);
                    float tb;
                    boxOK = slab(ro, rdInv, mk3(lb0.x, lb0.y, lb0.z), mk3(lb0.w, lb1.x, lb1.y), tb) && tb <= tBest;
                }
            };
            // Two triangles of a leaf share one 80-byte record (5 gather loads instead of 6).  Records of a leaf are contiguous:
            // fetch LEAFB/2 of them at a time so that the gather round trips of one group overlap (the array is padded, so no
            // bounds branch); test in leaf order.
            // LEAFB == 4 (closest-hit launches, round 4): groups of FOUR triangles (two records, 10 loads in flight) while at least four are left,
            // then pairs, then the odd tail -- a 5-triangle leaf is two dependent round trips instead of three.  The closest-hit launches are held
            // to five workgroups per CU by their LDS stacks, so the 96 registers of this form cost them no occupancy (the any-hit launch would
            // drop from six to five waves per SIMD: it keeps LEAFB == 2).
            auto group = [&](auto npc, int i) {
                constexpr int NPG = decltype(npc)::value;
                const float4 *t = sc.tris + (size_t)(first + (i >> 1)) * 5;
                gathers += 5u * NPG;
                if (STATS) { const unsigned long long am = __ballot(1); const uint32_t dk = quad_distinct((uint32_t)(first + (i >> 1))), dw = wave_distinct((uint32_t)(first + (i >> 1))); if (lane == (uint32_t)(__ffsll((long long)am) - 1)) { st_[13] += dk * 5u * NPG; st_[15] += dw * 5u * NPG; } }
                const v4f *tv = reinterpret_cast<const v4f *>(t);
                v4f rec[NPG][5];
#pragma unroll
                for (int k = 0; k < NPG; ++k) { rec[k][0] = tv[k * 5 + 0]; rec[k][1] = tv[k * 5 + 1]; rec[k][2] = tv[k * 5 + 2]; rec[k][3] = tv[k * 5 + 3]; rec[k][4] = tv[k * 5 + 4]; }
#pragma unroll
                for (int k = 0; k < NPG; ++k) { pin(rec[k][0]); pin(rec[k][1]); pin(rec[k][2]); pin(rec[k][3]); pin(rec[k][4]); }
                if (QN && i == 0) gate();
#pragma unroll
                for (int k = 0; k < 2 * NPG; ++k) {
                    const v4f &r0 = rec[k >> 1][0], &r1 = rec[k >> 1][1], &r2 = rec[k >> 1][2], &r3 = rec[k >> 1][3], &r4 = rec[k >> 1][4];
                    const V3 v0 = (k & 1) ? mk3(r2.y, r2.z, r2.w) : mk3(r0.x, r0.y, r0.z);
                    const V3 e1 = (k & 1) ? mk3(r3.x, r3.y, r3.z) : mk3(r0.w, r1.x, r1.y);
                    const V3 e2 = (k & 1) ? mk3(r3.w, r4.x, r4.y) : mk3(r1.z, r1.w, r2.x);
                    float tt;
                    if (STATS && !done) st_[2]++;
                    if (!done && boxOK && tri_hit(ro, rd, v0, e1, e2, eps, tBest, tt)) {
                        if (ANY) done = true;
                        else { tBest = tt; triBest = (int)f2u(r4.z) + (k & 1); }
                    }
                }
            };
            int i = 0;
            if constexpr (IMPL) {
                // first record of the leaf: one or two triangles and, in its spare word, the leaf's triangle count
                const v4f *tv = reinterpret_cast<const v4f *>(sc.tris + (size_t)first * 5);
                gathers += 5u;
                v4f r0 = tv[0], r1 = tv[1], r2 = tv[2], r3 = tv[3], r4 = tv[4];
                pin(r0); pin(r1); pin(r2); pin(r3); pin(r4);
                count = (int)f2u(r4.w);
                if (STATS) st_[2] += (unsigned long long)min(count, 2);
                if (QN) gate();                            // quantised nodes: the leaf's exact box, fetched with this record, decides whether its triangles count
                float tt;
                if (boxOK && tri_hit(ro, rd, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), eps, tBest, tt)) {
                    if (ANY) done = true;
                    else { tBest = tt; triBest = (int)f2u(r4.z); }
                }
                if (boxOK && !done && count >= 2 && tri_hit(ro, rd, mk3(r2.y, r2.z, r2.w), mk3(r3.x, r3.y, r3.z), mk3(r3.w, r4.x, r4.y), eps, tBest, tt)) {
                    if (ANY) done = true;
                    else { tBest = tt; triBest = (int)f2u(r4.z) + 1; }
                }
                i = 2;
                if (count == 1) count = 2;                 // (nothing left: keeps the odd-tail test below from firing for a one-triangle leaf)
            }
            if constexpr (LEAFB >= 4) for (; i + 4 <= count && !done; i += 4) group(std::integral_constant<int, 2>{}, i);
            for (; i + 2 <= count && !done && boxOK; i += 2) group(std::integral_constant<int, 1>{}, i);
            // ... then the odd last triangle of the leaf: its record holds ONE triangle, whose nine floats (and, for closest-hit rays, its
            // index, repeated in the otherwise unused tenth float) sit in the first three 16-byte pieces: 3 gather loads instead of 5
            // (every leaf of the bench mesh has 5 triangles: 13 loads per leaf visit instead of 15).
            if ((count & 1) && !done && boxOK) {
                const float4 *t = sc.tris + (size_t)(first + (count >> 1)) * 5;
                gathers += 3u;
                if (STATS) { const unsigned long long am = __ballot(1); const uint32_t dk = quad_distinct((uint32_t)(first + (count >> 1))), dw = wave_distinct((uint32_t)(first + (count >> 1))); if (lane == (uint32_t)(__ffsll((long long)am) - 1)) { st_[13] += dk * 3u; st_[15] += dw * 3u; } st_[2]++; }
                const v4f *tv = reinterpret_cast<const v4f *>(t);
                v4f r0 = tv[0], r1 = tv[1], r2 = tv[2];
                pin(r0); pin(r1); pin(r2);
                if (QN && count == 1) gate();
                float tt;
                if (boxOK && tri_hit(ro, rd, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), eps, tBest, tt)) {
                    if (ANY) done = true;
                    else { tBest = tt; triBest = (int)f2u(r2.y); }
                }
            }
            if (ANY && done) {
                src.store_any(rayId, true);
                active = false;
            } else if constexpr (ANY) {
                leaf = 0;
                if (ref < 0) { leaf = ref; ref = RT_NO_CHILD; }        // a second leaf was waiting in `ref`
                if (ref == RT_NO_CHILD) pop_or_finish();               // look for an inner node (retires the ray if nothing is left)
            } else pop_or_finish();
        }
        if (STATS && lane == 0) st_[9] += clock64() - tL_;
        if constexpr (TIMING) { tm_[4]++; tm_[5] += clock64() - tL_; }
    }
    if (STATS && lane == 0) st_[11] = clock64() - tStart_;
    if constexpr (TIMING) { tm_[8] = clock64() - tStart_; if (stats && lane == 0) for (int q = 0; q < 9; ++q) atomicAdd(&stats[q], tm_[q]); }
    if (STATS && stats) {
        for (int q = 0; q < 16; ++q) {
            unsigned long long v = st_[q];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0 && v) atomicAdd(&stats[q], v);
        }
    }
    if (tally) {
        unsigned long long s = traced;                     // 64-bit: a batch of 64-spp frames traces more than 2^32 rays per launch set
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0 && s) atomicAdd(tally, s);
    }
    if (gatherLoads) {
        unsigned long long g = gathers;
        for (int off = 32; off > 0; off >>= 1) g += __shfl_down(g, off, 64);
        if (lane == 0 && g) atomicAdd(gatherLoads, g);
    }
}

// ---- packet traversal (round 4) ----------------------------------------------------------------------
// The AO rays of one hit leave from ONE point (computeAO: org = hp + N * aoBias, rt_lighting.glsl:721-757) and are short (aoRadius 0.8): the
// four of them visit nearly the same part of the tree -- traced one by one they fetch 39.8 four-wide node records and 8.8 leaves per hit on the
// bench mesh, as a packet 14.0 and 3.7 (tools/r04_packet_proto.py).  They are 83 % of the any-hit rays of a frame, and the any-hit launch runs at
// the vector L1's access rate.  So one LANE walks the tree once for the up to four rays of a hit: every node record and every
// triangle record is fetched once and tested against the rays that entered its parent (a 4-bit mask travels with every stack entry), a ray leaves
// the packet when it is occluded.  Every (ray, box) and (ray, triangle) test is the arithmetic of the single-ray kernel on the same operands, and a
// ray's answer is the OR over the reference's leaves whose own box the ray passes ("any-hit rays walk 4-wide nodes") -- which is
// what this computes, in another order -- so the answers are the same bits.
struct PacketSrc {       // packet p -> hit j = p % nLive, ray group g = p / nLive: rays i = 4 g .. 4 g + 3 (< A) at [i * stride + j]
    const float4 *o, *d;     // org == null (rt_debug_trace kind 4): a packet leaves from the origin record of its first ray, o[.], tMax words in tm
    const float *tm;
    const float4 *org;       // the frames' dense AO slots: one origin per hit, org[j]; tMax is the .w of the direction record
    uint8_t *occ;
    const uint32_t *liveCount;
    uint32_t c0, cap, stride;
    int A;
    uint32_t nLive;
    RT_DEV void prepare() { uint32_t h = *liveCount; nLive = min(h, c0 + cap) - min(h, c0); }
    RT_DEV uint32_t size() const { return nLive * (uint32_t)((A + 3) / 4); }
};
// stack / register entry: [31:28] rays of the packet that passed the node's box, [27] leaf, [26:0] inner node index or leaf code (first << 3 | count - 1); 0 = none
RT_DEV uint32_t pk_entry(uint32_t mask, int ref) { return (mask << 28) | (ref < 0 ? (0x08000000u | (uint32_t)(-ref - 1)) : (uint32_t)ref); }
RT_DEV bool pk_is_leaf(uint32_t e) { return (e & 0x08000000u) != 0u; }

__global__ __launch_bounds__(256, 4) void k_trace_packets(const DevFrame *__restrict__ fr, const float4 *__restrict__ w4, const float4 *__restrict__ pairs, PacketSrc src,
                                                          uint32_t *head, unsigned long long *tally, unsigned long long *gatherLoads, TraceTune tune, int stackEntries) {
    uint32_t *stk = reinterpret_cast<uint32_t *>(rt_dyn_lds) + (threadIdx.x >> 6) * stackEntries * 64 + (threadIdx.x & 63);
    const DevScene sc = fr->sc;
    const float eps = fr->u.eps;
    src.prepare();
    const uint32_t n = src.size();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t runLen = tune.chunk > 0 ? (uint32_t)max(tune.chunk, 8) : min(256u, max(64u, ((n / (3u * 4u * gridDim.x) + 63u) / 64u) * 64u));
    // per-lane packet state
    V3 ro = mk3(0.0f), rd[4], rdInv[4];
    float tMax[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { rd[r] = mk3(0.0f); rdInv[r] = mk3(0.0f); tMax[r] = -1.0f; }
    uint32_t alive = 0;          // rays of the packet not decided yet
    uint32_t occl = 0;           // rays found occluded
    uint32_t cur = 0, leafE = 0; // node in hand / postponed leaf (entries, 0 = none)
    int sp = 0;
    uint32_t token = 0;          // address of the packet's first ray
    uint32_t nRays = 0;          // rays of the packet that exist (i < A)
    bool active = false;
    bool exhausted = (n == 0);
    uint32_t traced = 0, gathers = 0;
    uint32_t runNext = 0, runEnd = 0;
    const uint32_t shard = (blockIdx.x * 4u + (threadIdx.x >> 6)) % kShards;
    bool homeDry = false;
    const uint32_t nRuns = (n + runLen - 1u) / runLen;

    auto retire = [&]() {
#pragma unroll
        for (int r = 0; r < 4; ++r) if ((uint32_t)r < nRays && !(tMax[r] < 0.0f)) src.occ[token + (uint32_t)r * src.stride] = (occl >> r) & 1u;
        active = false;
    };
    auto pop_or_finish = [&]() {
        cur = 0;
        while (sp > 0) {
            sp--;
            uint32_t e = stk[sp * 64];
            const uint32_t m = (e >> 28) & alive;
            if (m == 0u) continue;                              // every ray that entered this subtree has been decided since
            e = (e & 0x0fffffffu) | (m << 28);
            if (pk_is_leaf(e) && leafE == 0u) { leafE = e; continue; }   // leaves wait; keep looking for an inner node
            cur = e;                                                      // an inner node, or a second leaf (the lane then waits)
            break;
        }
        if (cur == 0u && leafE == 0u) retire();
    };

    for (;;) {
        const unsigned long long idleMask = __ballot(!active);
        const int nIdle = __popcll(idleMask);
        if (!exhausted && nIdle >= tune.refillMin) {
            if (runNext >= runEnd) {
                auto runsOf = [&](uint32_t sh) { return sh < nRuns ? (nRuns - sh + kShards - 1u) / kShards : 0u; };
                uint32_t k = 0, from = shard;
                bool got = false;
                if (!homeDry) {
                    if (lane == 0) k = atomicAdd(&head[shard * kShardStride], 1u);
                    k = __shfl(k, 0, 64);
                    got = k < runsOf(shard);
                    homeDry = !got;
                }
                while (!got) {
                    const uint32_t c = __hip_atomic_load(&head[lane * kShardStride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    unsigned long long open = __ballot(c < runsOf(lane));
                    if (open == 0ull) break;
                    const unsigned long long rot = (open >> shard) | (shard ? (open << (64u - shard)) : 0ull);
                    from = (shard + (uint32_t)__ffsll((long long)rot) - 1u) % kShards;
                    if (lane == 0) k = atomicAdd(&head[from * kShardStride], 1u);
                    k = __shfl(k, 0, 64);
                    got = k < runsOf(from);
                }
                if (!got) { exhausted = true; continue; }
                const unsigned long long base = ((unsigned long long)k * kShards + from) * runLen;
                runNext = (uint32_t)base;
                runEnd = (uint32_t)min((unsigned long long)n, base + runLen);
            }
            // every packet of the run exists: the i-th idle lane takes the i-th packet left
            const uint32_t nTake = min((uint32_t)nIdle, runEnd - runNext);
            const uint32_t rank = (uint32_t)__popcll(idleMask & ((1ull << lane) - 1ull));
            if (!active && rank < nTake) {
                const uint32_t p = runNext + rank;
                const uint32_t g = p / src.nLive, j = p % src.nLive;
                token = (4u * g) * src.stride + j;
                nRays = min(4u, (uint32_t)src.A - 4u * g);
                ro = f4xyz(src.org ? src.org[j] : src.o[token]);        // one origin for the packet
                alive = 0; occl = 0; sp = 0; cur = 0; leafE = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    tMax[r] = -1.0f;
                    if ((uint32_t)r < nRays) {
                        const uint32_t a = token + (uint32_t)r * src.stride;
                        float4 dd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        if (src.org) { dd = src.d[a]; tMax[r] = dd.w; } else tMax[r] = src.tm[a];
                        if (!(tMax[r] < 0.0f)) {
                            rd[r] = f4xyz(src.org ? dd : src.d[a]);
                            rdInv[r] = mk3(1.0f / rd[r].x, 1.0f / rd[r].y, 1.0f / rd[r].z);
                            traced++;
                            float tmin;
                            if (sc.hasBVH && !tune.skipTraversal && slab(ro, rdInv[r], ld3(sc.rootMin), ld3(sc.rootMax), tmin) && !(tmin > tMax[r])) alive |= 1u << r;
                        }
                    }
                }
                active = true;
                if (alive == 0u) retire();
                else {
                    const uint32_t e = pk_entry(alive, sc.rootRef4);
                    if (pk_is_leaf(e)) leafE = e; else cur = e;   // (single-leaf tree)
                }
            }
            runNext += nTake;
            continue;
        }
        if (__ballot(active) == 0ull) {
            if (exhausted) break;
            continue;
        }
        // ---- inner nodes
        for (;;) {
            const bool searching = active && cur != 0u && !pk_is_leaf(cur);
            const unsigned long long sm = __ballot(searching);
            if (sm == 0ull) break;
            if (__popcll(sm) < tune.minSearch && __ballot(active && leafE != 0u) != 0ull) break;
            if (searching) {
                gathers += 7u;
                const uint32_t pm = cur >> 28;
                const v4f *ndv = reinterpret_cast<const v4f *>(w4 + (size_t)(cur & 0x07ffffffu) * 8);
                v4f q0 = ndv[0], q1 = ndv[1], q2 = ndv[2], q3 = ndv[3], q4 = ndv[4], q5 = ndv[5], q6 = ndv[6];
                pin(q0); pin(q1); pin(q2); pin(q3); pin(q4); pin(q5); pin(q6);
                uint32_t cm0 = 0, cm1 = 0, cm2 = 0, cm3 = 0;   // per child: the rays that pass its box
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float t0, t1, t2, t3;
                    const bool h0 = slab(ro, rdInv[r], mk3(q0.x, q1.x, q2.x), mk3(q3.x, q4.x, q5.x), t0) && t0 <= tMax[r];
                    const bool h1 = slab(ro, rdInv[r], mk3(q0.y, q1.y, q2.y), mk3(q3.y, q4.y, q5.y), t1) && t1 <= tMax[r];
                    const bool h2 = slab(ro, rdInv[r], mk3(q0.z, q1.z, q2.z), mk3(q3.z, q4.z, q5.z), t2) && t2 <= tMax[r];
                    const bool h3 = slab(ro, rdInv[r], mk3(q0.w, q1.w, q2.w), mk3(q3.w, q4.w, q5.w), t3) && t3 <= tMax[r];
                    cm0 |= (h0 ? 1u : 0u) << r; cm1 |= (h1 ? 1u : 0u) << r; cm2 |= (h2 ? 1u : 0u) << r; cm3 |= (h3 ? 1u : 0u) << r;
                }
                const uint32_t in = pm & alive;   // rays that entered this node and are still undecided
                uint32_t nxt = 0;
                auto take = [&](uint32_t cm, int ref) {
                    cm &= in;
                    if (cm == 0u) return;
                    uint32_t e = pk_entry(cm, ref);
                    if (pk_is_leaf(e) && leafE == 0u) { leafE = e; return; }
                    if (nxt == 0u) { nxt = e; return; }
                    if (!pk_is_leaf(e) && pk_is_leaf(nxt)) { const uint32_t t = nxt; nxt = e; e = t; }   // go on with the inner node, defer the leaf
                    stk[sp * 64] = e;
                    sp++;
                };
                take(cm0, (int)f2u(q6.x)); take(cm1, (int)f2u(q6.y)); take(cm2, (int)f2u(q6.z)); take(cm3, (int)f2u(q6.w));
                if (nxt == 0u) pop_or_finish();
                else cur = nxt;
            }
        }
        // ---- leaves
        if (active && leafE != 0u) {
            const uint32_t v = leafE & 0x07ffffffu;
            const int first = (int)(v >> 3), count = (int)(v & 7u) + 1;
            uint32_t m = (leafE >> 28) & alive;
            auto test_tri = [&](V3 v0, V3 e1, V3 e2) {
                // tri_hit (rt_bvh.glsl:154-170) for every ray of the leaf's mask; tvec, qvec and dot(e2, qvec) do not depend on the direction
                const V3 tvec = ro - v0;
                const V3 qvec = cross(tvec, e1);
                const float te = dot(e2, qvec);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const V3 pvec = cross(rd[r], e2);
                    const float det = dot(e1, pvec);
                    const float invDet = 1.0f / det;
                    const float u = dot(tvec, pvec) * invDet;
                    const float vv = dot(rd[r], qvec) * invDet;
                    const float tt = te * invDet;
                    const bool hit = !(__builtin_fabsf(det) < 1e-8f) && !(u < 0.0f || u > 1.0f) && !(vv < 0.0f || u + vv > 1.0f) && !(tt < eps || tt > tMax[r]);
                    if (hit && ((m >> r) & 1u)) { occl |= 1u << r; alive &= ~(1u << r); m &= ~(1u << r); }
                }
            };
            for (int i = 0; i + 2 <= count && m != 0u; i += 2) {
                const v4f *tv = reinterpret_cast<const v4f *>(pairs + (size_t)(first + (i >> 1)) * 5);
                gathers += 5u;
                v4f r0 = tv[0], r1 = tv[1], r2 = tv[2], r3 = tv[3], r4 = tv[4];
                pin(r0); pin(r1); pin(r2); pin(r3); pin(r4);
                test_tri(mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x));
                if (m != 0u) test_tri(mk3(r2.y, r2.z, r2.w), mk3(r3.x, r3.y, r3.z), mk3(r3.w, r4.x, r4.y));
            }
            if ((count & 1) && m != 0u) {
                const v4f *tv = reinterpret_cast<const v4f *>(pairs + (size_t)(first + (count >> 1)) * 5);
                gathers += 3u;
                v4f r0 = tv[0], r1 = tv[1], r2 = tv[2];
                pin(r0); pin(r1); pin(r2);
                test_tri(mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x));
            }
            leafE = 0;
            if (alive == 0u) retire();
            else {
                if (cur != 0u && pk_is_leaf(cur)) { leafE = cur; cur = 0; }   // a second leaf was waiting in `cur`
                if (cur == 0u) pop_or_finish();
            }
        }
    }
    if (tally) {
        unsigned long long t = traced;
        for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
        if (lane == 0 && t) atomicAdd(tally, t);
    }
    if (gatherLoads) {
        unsigned long long g = gathers;
        for (int off = 32; off > 0; off >>= 1) g += __shfl_down(g, off, 64);
        if (lane == 0 && g) atomicAdd(gatherLoads, g);
    }
}

// Workgroups of a persistent traversal grid: the resident 256-thread workgroups per CU (8 at most) times the CUs, gridPct per cent of that, 8 at least.
// The runtime's answer is kept per (device, kernel, LDS bytes): a process may hold contexts on devices of different shapes
template <class Kernel>
unsigned persistent_grid(Kernel kernel, size_t ldsBytes, int cus, int gridPct) {
    thread_local std::map<std::tuple<int, const void *, size_t>, int> occ;
    int dev = 0;
    (void)hipGetDevice(&dev);
    int &perCU = occ[std::make_tuple(dev, (const void *)kernel, ldsBytes)];
    if (perCU == 0) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, 256, ldsBytes) != hipSuccess || perCU < 1) perCU = 1;
        perCU = std::min(perCU, 8);
    }
    return (unsigned)std::max(8, cus * perCU * gridPct / 100);
}

// One trace launch, apart from its rays.  The fields a caller may leave out come last.
struct TraceLaunch {
    hipStream_t st; int cus, gridPct, depth;   // the device's CUs, the share of the resident grid to launch (per cent), the binary tree's depth (stack size)
    const DevFrame *fr;                    // the frame descriptor, on the device
    const DevScene &scene;                 // host copy of its scene: the node forms rt_upload_bvh built
    uint32_t *head;                        // the launch's cursors: kHeadWords words, zero
    TraceTune tune;
    unsigned long long *tally = nullptr, *gatherLoads = nullptr;   // the rays traced / the 16-byte gather loads issued are added here
    unsigned long long *stats = nullptr;   // RT_TRACE_STATS / RT_TRACE_TIMING sums: launches the diagnostic build
    unsigned maxBlocks = 0;                // ray queries: no more workgroups than the rays can occupy (0: whatever fits)
};

// What a scene offers a launch (rt_trace_build.hpp)
inline rtl::TraceForms trace_forms(const DevScene &sc) { return rtl::TraceForms{sc.q4 != nullptr, sc.wF != nullptr, sc.iN2 != nullptr, sc.iN4 != nullptr, sc.iQ4 != nullptr, sc.anyStack}; }
inline const float4 *trace_nodes(const DevScene &sc, rtl::TraceNodes which) {
    switch (which) {
        case rtl::TN_WF: return sc.wF;
        case rtl::TN_IN2: return sc.iN2;
        case rtl::TN_W4: return sc.w4;
        case rtl::TN_Q4: return sc.q4;
        case rtl::TN_IN4: return sc.iN4;
        case rtl::TN_IQ4: return sc.iQ4;
        default: return sc.wnodesW;
    }
}

// One trace launch: the build rtl::trace_build chooses (rt_trace_build.cpp: the rules, tested without a GPU), its arrays, and the kernel of that build out of the
// kept builds of this hit kind.  Returns the RT_BUILD_* bits of the build launched (rt_debug_builds); 0 -- nothing was launched -- for a build that is not kept,
// which trace_build never returns (tests/test_trace_build_host.py).
template <class Src, bool ANY, size_t... I>
uint32_t launch_trace_of(const TraceLaunch &t, const Src &src, const rtl::TraceBuild &b, std::index_sequence<I...>) {
    constexpr const uint32_t *kept = ANY ? rtl::kAnyBuilds : rtl::kClosestBuilds;
    const DevScene &hs = t.scene;
    const float4 *nodes = trace_nodes(hs, b.nodes), *pairRecords = b.implPairs ? hs.iPairs : hs.pairs, *leafBoxes = b.implLeafBoxes ? hs.iLeafBox : hs.leafBox;
    auto go = [&](auto kernel) {
        // Resident 256-thread workgroups per CU follow from the LDS footprint and the kernel's registers: the persistent grid is exactly what fits
        unsigned blocks = persistent_grid(kernel, b.ldsBytes, t.cus, t.gridPct);
        if (t.maxBlocks) blocks = std::min(blocks, t.maxBlocks);   // (ray queries: no more waves than the rays can occupy)
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), b.ldsBytes, t.st, t.fr, nodes, pairRecords, src, t.head, t.tally, t.gatherLoads, t.tune, b.stack, t.stats, leafBoxes);
        return true;
    };
    const bool launched = ((b.opt == kept[I] && go(&k_trace<Src, ANY, kept[I]>)) || ...);
    return launched ? (uint32_t)(RT_BUILD_LAUNCHED | b.opt) << (ANY ? RT_BUILD_ANY_SHIFT : 0) : 0u;
}
template <class Src, bool ANY>
uint32_t launch_trace(const TraceLaunch &t, const Src &src) {
    const rtl::TraceBuild b = rtl::trace_build(ANY, t.tune, trace_forms(t.scene), t.depth, t.stats != nullptr);
    return launch_trace_of<Src, ANY>(t, src, b, std::make_index_sequence<ANY ? rtl::kNAnyBuilds : rtl::kNClosestBuilds>{});
}
// ... closest- or any-hit by a run-time choice (the debug and query entries)
template <class Src> uint32_t launch_trace_kind(bool any, const TraceLaunch &t, const Src &src) { return any ? launch_trace<Src, true>(t, src) : launch_trace<Src, false>(t, src); }

// rt_trace_rays: the call's uEPS / uINF and the scene into the query's frame descriptor, the cursor words zeroed -- on the stream, so that a steady
// stream of queries needs no host copy and no synchronisation
__global__ __launch_bounds__(256) void k_query_prep(DevFrame *fr, DevScene sc, float eps, float inf, uint32_t *head) {
    for (uint32_t i = threadIdx.x; i < kHeadWords; i += blockDim.x) head[i] = 0u;
    if (threadIdx.x == 0) { fr->sc = sc; scene_take_root_box(fr->sc); fr->u.eps = eps; fr->u.inf = inf; }
}

uint32_t launch_packets(const TraceLaunch &t, PacketSrc src) {   // (stats and maxBlocks are not for packets)
    const DevScene &hs = t.scene;
    const rtl::TraceBuild b = rtl::trace_build(true, t.tune, trace_forms(hs), t.depth, false);   // the any-hit stack and its LDS bytes; the packets walk w4 whatever the build
    const unsigned blocks = persistent_grid(k_trace_packets, b.ldsBytes, t.cus, t.gridPct);
    hipLaunchKernelGGL(k_trace_packets, dim3(blocks), dim3(256), b.ldsBytes, t.st, t.fr, hs.w4, hs.pairs, src, t.head, t.tally, t.gatherLoads, t.tune, b.stack);
    return (uint32_t)RT_BUILD_PACKETS << RT_BUILD_ANY_SHIFT;
}
}  // namespace
