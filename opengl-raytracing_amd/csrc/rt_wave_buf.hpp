// rt_wave_buf.hpp -- the records every part of the wavefront pipeline shares: stage ids, the hit record, the frame's arrays (WaveBuf), the batched list append and
// the cursor constants of the trace launches.
// Part of the rt_wave.hip translation unit: included by it alone, behind its `#pragma clang fp contract(off)` and `using namespace rtd;`.
#pragma once
#include "rt_batch_order.hpp"
#include "rt_wave.hpp"

// stage ids (rt_stage_name in rt_api.hip)
enum { ST_PRIMARY = 1, ST_TRACE_PRIMARY, ST_POST_PRIMARY, ST_GEN_DIRECT, ST_TRACE_SHADOW, ST_TRACE_GI, ST_GEN_GI, ST_RESOLVE, ST_COMBINE, ST_TRACE_AO = 13 };

struct HitRec { uint32_t slot; float t; int tri; };

struct WaveBuf {
    // per frame
    uint32_t *cand;          // candidate pixel slots
    uint32_t *counts;        // [0] candidates, [1] hits, [2..] traced-ray tallies
    uint32_t *heads;         // ray cursors, one per trace launch
    float *primT;            // per candidate
    int *primTri;
    HitRec *hits;
    // per chunk of CH hits
    // Shadow queue 1: (A + 4*SPP + 2) slots x CH.  Every slot has a direction record in shD.  The A AO slots are DENSE slots: the record is {dir, limit} -- limit =
    // tMax, < 0 = no ray -- and the origin, one for all AO rays of the hit (computeAO_BVH), is aoOrg[j].  The light slots behind them keep an origin record and a
    // tMax / liveness word of their own (hp + L*e differs from ray to ray): shO / shT, indexed by the slot's address LESS the A * CH dense ones.
    float4 *shO, *shD;
    float *shT, *sh2T;       // per-slot tMax (any-hit); < 0 = no ray in this slot (4 B instead of a 32-B record)
    // Light-slot liveness masks: bit b of shLive = light-slot entry b of queue 1 (the index of shO / shT) holds a ray, bit a of sh2Live = entry a of
    // queue 2 does.  Cleared before the chunk's k_gen_direct, set by the generators (live_set); shT / sh2T of a dead slot are then not written at all.
    // Null (RT_LIGHT_MASKS=0): a dead slot is marked by shT / sh2T < 0, as before.  The lane's own memory, not the planned ray arena.
    unsigned long long *shLive, *sh2Live;
    float4 *aoOrg;           // per hit: hp + N * aoBias, written once (AO ray 0)
    uint8_t *occ1;
    // Bounce queue: SPP dense slots x CH, record {dir, 1.0 = a ray was cast | < 0 = none}; the origin hp + N * eps (bounce_origin) belongs to the hit: giOrg[j],
    // written once by sample 0 whether or not that sample casts.  (RT_BIN_GI permutes the records of a workgroup: there giOrg holds one origin per RECORD.)
    float4 *giD, *giOrg;
    float *giT;
    int *giTri;
    float4 *sh2O, *sh2D;     // shadow queue 2: 6 slots x q2Stride, entries compacted over the (hit, sample) pairs whose bounce hit
    uint32_t q2Stride;       // entries per slot of queue 2: CH * SPP (every bounce ray may hit) for small launch sets; for large ones (round 5) a capacity PREDICTED from the bounce
                             // hits of earlier batches -- a (hit, sample) pair whose entry lies beyond it is not queued: k_gen_gi_overflow traces its six rays in place
    uint8_t *occOvf;         // answers of those rays, [6][CH * SPP] (per lane, like occ2)
    uint8_t *occ2;
    int *giPos;              // per (sample, hit): entry in queue 2, -1 when the bounce ray missed or was not cast
    int *giPerm;             // RT_BIN_GI=1 (experiment, round 4): per (sample, hit) the bounce queue entry its ray was sorted to; null = entry (sample, hit) itself
    uint32_t *giHit;         // RT_BOUNCE_PROBE: bounce queue addresses whose any-hit probe found a triangle (dense, CH * SPP entries at most; per lane, like giT)
    // per frame, per pixel slot: everything the frame produced BEFORE the temporal resolve (the only history-dependent step)
    float4 *pendC;           // curr.rgb (frame average, fp32), motion.x
    float *pendMy;           // motion.y
    uint2 *pendPos, *pendNrm;
    uint32_t CH;             // chunk capacity (hits)
    int A;                   // AO rays per hit (0 when AO is off)
    int SPP;
    // slot of shadow queue 1 for ray k of sample s: A AO slots, then the four disk-light rays of every sample, then ONE sun and ONE point-light
    // slot per hit -- those two rays do not depend on the sample (rt_lighting.glsl:114-214), sample 0 traces them and the others reuse its answer,
    // so samples > 0 own no slot for them (round 4: 22 instead of 28 slots per hit at 4 spp)
    __device__ __forceinline__ uint32_t gi_entry(int s, uint32_t j) const { const uint32_t a = (uint32_t)s * CH + j; return giPerm ? (uint32_t)giPerm[a] : a; }
    __device__ __forceinline__ uint32_t sh1_light(uint32_t a) const { return a - (uint32_t)A * CH; }   // address of a light slot -> entry of shO / shT
    __device__ __forceinline__ uint32_t sh1_slot(int s, int k) const { return (uint32_t)(k < 4 ? A + s * 4 + k : A + 4 * SPP + (k - 4)); }
};

namespace {
// block_append (rt_wave_stages.hpp) for kAppendBatch sub-blocks of 256 items handled by one workgroup: still ONE atomic, for 2048 items.  (With one
// atomic per 256 items k_primary spent 0.10 ms of a 1080p frame queueing 8100 atomics on one word; now 0.025 ms.)
//   note(k, pred) for every sub-block k, commit(counter), then index(k) -> position of this thread's item of sub-block k.
// All 256 threads call every method, with the same k.
constexpr int kAppendBatch = 8;
struct BatchAppend {
    uint32_t bits = 0;
    uint32_t (*cnt)[4];
    uint32_t *base;
    RT_DEV void note(int k, bool pred) {
        unsigned long long m = __ballot(pred);
        if (pred) bits |= 1u << k;
        if ((threadIdx.x & 63) == 0) cnt[k][threadIdx.x >> 6] = (uint32_t)__popcll(m);
    }
    RT_DEV void commit(uint32_t *counter) {
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tot = 0;
            for (int k = 0; k < kAppendBatch; ++k) tot += cnt[k][0] + cnt[k][1] + cnt[k][2] + cnt[k][3];
            *base = tot ? atomicAdd(counter, tot) : 0u;
        }
        __syncthreads();
    }
    RT_DEV bool mine(int k) const { return (bits >> k) & 1u; }
    RT_DEV uint32_t index(int k) const {
        const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        uint32_t off = *base;
        for (int kk = 0; kk < k; ++kk) off += cnt[kk][0] + cnt[kk][1] + cnt[kk][2] + cnt[kk][3];
        for (uint32_t i = 0; i < wv; ++i) off += cnt[k][i];
        const unsigned long long m = __ballot(mine(k));
        return off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    }
};
#define RT_BATCH_APPEND(name) __shared__ uint32_t name##_cnt[kAppendBatch][4]; __shared__ uint32_t name##_base; BatchAppend name; name.cnt = name##_cnt; name.base = &name##_base

// The same append with a wave's items laid out lane by lane, and a lane's kAppendBatch items side by side (rt_batch_order.hpp): k_primary_interleaved's order for a batch
// of frames, whose iterations are the frames of one spatial tile.  Still ONE atomic per workgroup; the waves keep their ballots instead of their counts.
//   note(k, pred) for every sub-block k, commit(counter), then index(k) -> position of this thread's item of sub-block k.
struct InterleavedAppend {
    uint32_t bits = 0, first = 0;
    unsigned long long (*bal)[4];
    uint32_t *base;
    RT_DEV void note(int k, bool pred) {
        const unsigned long long m = __ballot(pred);
        if (pred) bits |= 1u << k;
        if ((threadIdx.x & 63) == 0) bal[k][threadIdx.x >> 6] = m;
    }
    RT_DEV void commit(uint32_t *counter) {
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tot = 0;
            for (int k = 0; k < kAppendBatch; ++k) for (int i = 0; i < 4; ++i) tot += (uint32_t)__popcll(bal[k][i]);
            *base = tot ? atomicAdd(counter, tot) : 0u;
        }
        __syncthreads();
        const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        first = *base;
        for (uint32_t i = 0; i < wv; ++i) for (int k = 0; k < kAppendBatch; ++k) first += (uint32_t)__popcll(bal[k][i]);
        first += interleaved_lane_start(&bal[0][wv], 4, kAppendBatch, lane);
    }
    RT_DEV bool mine(int k) const { return (bits >> k) & 1u; }
    RT_DEV uint32_t index(int k) const { return interleaved_index(first, bits, k); }
};
#define RT_INTERLEAVED_APPEND(name) __shared__ unsigned long long name##_bal[kAppendBatch][4]; __shared__ uint32_t name##_base; InterleavedAppend name; name.bal = name##_bal; name.base = &name##_base

// Light-slot liveness (WaveBuf::shLive / sh2Live): the lanes that call this together set bit `bit` of `live` where `on`.  A wave with no live lane issues no
// memory operation.  Where the live lanes stand on consecutive bits in lane order (k_gen_direct: one sample, consecutive hits) ONE lane ORs the wave's ballot,
// shifted, into the one or two words it straddles; where they stand in two neighbouring words otherwise (queue 2's compacted entries) one lane ORs the two
// words, put together in a scalar loop; else (a wave across a sample boundary) every live lane ORs its own bit.  The words are shared with neighbouring waves:
// atomics, whose value is not read (no return: they do not wait for memory).
RT_DEV void live_set(unsigned long long *live, uint32_t bit, bool on) {
    const unsigned long long m = __ballot(on);
    if (m == 0ull) return;
    const uint32_t lane = threadIdx.x & 63u;
    const int first = __ffsll((long long)m) - 1;
    const uint32_t b0 = (uint32_t)__shfl((int)bit, first, 64);                             // the first live lane's bit: the row starts there
    const bool row = __ballot(on && bit - b0 != lane - (uint32_t)first) == 0ull;
    if (row) {
        if ((int)lane == first) {
            const unsigned long long mm = m >> first;
            const uint32_t sh = b0 & 63u;
            (void)__hip_atomic_fetch_or(&live[b0 >> 6], mm << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (sh != 0u && (mm >> (64u - sh)) != 0ull) (void)__hip_atomic_fetch_or(&live[(b0 >> 6) + 1u], mm >> (64u - sh), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
    }
    // Not a row, but all in the first live lane's word or the next (queue 2: an entry is the pair's rank among the workgroup's bounce hits, so the bits are
    // consecutive over the CALLING lanes and skip the others): the two words are put together bit by bit from the live lanes' values -- a wave-uniform loop of
    // scalar instructions, at most 64 rounds -- and one lane ORs them in.  (One atomic per live lane made k_gen_gi 20 % longer on the 1 M-triangle scene, where
    // most bounce rays hit: profiles/r19_light_masks.txt 4.)
    const uint32_t w0 = b0 >> 6;
    if (__ballot(on && (bit >> 6) - w0 > 1u) == 0ull) {
        unsigned long long lo = 0ull, hi = 0ull;
        for (unsigned long long rem = m; rem != 0ull; rem &= rem - 1ull) {
            const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)bit, __ffsll((long long)rem) - 1);
            if ((b >> 6) == w0) lo |= 1ull << (b & 63u);
            else hi |= 1ull << (b & 63u);
        }
        if ((int)lane == first) {
            (void)__hip_atomic_fetch_or(&live[w0], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (hi != 0ull) (void)__hip_atomic_fetch_or(&live[w0 + 1u], hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else if (on) (void)__hip_atomic_fetch_or(&live[bit >> 6], 1ull << (bit & 63u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The ray cursors of one trace launch (WaveBuf::heads, k_trace's scheduler): sharded, each shard on a line of its own.
constexpr uint32_t kShards = 64, kShardStride = 32;   // cursor shards per trace launch, uint32 words between them (128 B)
constexpr uint32_t kHeadWords = kShards * kShardStride;

// live hits of the chunk starting at c0: |[c0, c0+CH) ∩ [0, hits)|, written without a wrapping subtraction (hipcc -O3 was
// seen to drop the `h > c0 ? ... : 0` guard of the obvious form, turning empty chunks into full ones)
RT_DEV uint32_t chunk_live(const WaveBuf &wb, uint32_t c0) { uint32_t h = wb.counts[1]; return min(h, c0 + wb.CH) - min(h, c0); }
}  // namespace
