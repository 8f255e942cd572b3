// rt_wave_plan.hpp -- what a launch set of the wavefront pipeline (rt_wave.hip) can know without a device: the options of the environment,
// the queue plan (slots per hit, chunk capacity, deferral, the capacity of shadow queue 2, the split of a hit count into chunks) and ONE description per
// arena, from which both its byte count and the pointers into it come.  No HIP, no context: rt_wave_render follows the plan, rt_hybrid.hip lays its arena out
// with the same cursor, and rt_debug_wave_plan hands the plan out without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/rt_mi355.h"

namespace rtl {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Every environment variable of frame rendering, read ONCE per lane, at rt_wave_create (RtWaveOptions, include/rt_mi355.h, is the same record handed to
// rt_debug_wave_plan).  wave_default_options carries the defaults and the measurements behind them.
using WaveOptions = RtWaveOptions;
WaveOptions wave_default_options();
// The one getenv reader of frame rendering in rt_wave.hip (the traversal builds' switches are tune_from_env's: a kernel argument, shared with the debug entries).
WaveOptions wave_options_from_env();
// RT_BATCH_INTERLEAVE (default 1): a batch's candidate list pixel-major, the frames of a pixel side by side (k_primary_interleaved, rt_batch_order.hpp); 0: frame-major, as the
// slots are.  Read beside wave_options_from_env, once per lane; an order of the lists, not a term of the plan.
int batch_interleave_from_env();
// RT_BEAM_CULL (DESIGN.md 4.2 "Beam cull"): finish the tiles whose every primary ray surely misses the mesh in front of the primary launch (k_beam_cull).
// -1 (default, "auto"): launch sets of two or more frames over a scene that fits L2; 1: every launch set, single frames as well; 0: never, the A/B switch.  Read beside batch_interleave_from_env, once per lane.
int beam_cull_from_env();

// RT_BOUNCE_PROBE (auto): the bounce rays are walked any-hit first while the share of them that hit, in earlier launch sets, is below kProbeShareMax.  The
// any-hit walk proves a miss at 0.72 of the closest-hit walk's cost on the bench view (profiles/r06_bounce_probe.txt); a hit pays both walks, so the probe
// pays while share < 1 - 0.72, less the second launch -- kProbeShareMax keeps a margin.  Nothing known (share 0): the closest-hit launch alone.  Both
// paths are exact, so a wrong guess costs time, never bits.
constexpr double kProbeShareMax = 0.15;
inline bool wave_probe_on(const WaveOptions &o, double share) { return o.probeMode == 1 || (o.probeMode < 0 && share > 0.0 && share < kProbeShareMax); }

// ---- one description per arena: a list of (array, element bytes, count) that a cursor walks, counting or handing out addresses

enum WaveArray {
    WA_CAND, WA_PRIMT, WA_PRIMTRI, WA_HITS, WA_PENDC, WA_PENDPOS, WA_PENDNRM, WA_PENDMY,      // frame arena (per pixel slot)
    WA_SHO, WA_SHD, WA_SHT, WA_AOORG, WA_GID, WA_GIORG, WA_SH2O, WA_SH2D, WA_SH2T,             // ray arena: queue 1, the bounce queue, queue 2
    WA_OCC1, WA_GIT, WA_GITRI, WA_OCC2, WA_OCCOVF, WA_GIPOS, WA_GIPERM, WA_GIHIT,               // result arena (what k_combine reads)
    WA_COUNT
};
const char *wave_array_name(int id);   // the WaveBuf member's name
constexpr size_t kHitRecBytes = 12;    // HitRec {slot, t, tri}

struct ArenaSpan { int id; size_t elemBytes, count; bool reservedOnly; };   // reservedOnly: the span is part of the total, the array is not handed out (null)
struct ArenaList {
    int n = 0;
    ArenaSpan a[9];
    size_t align = 256, slack = 0;   // every array starts at a multiple of `align`; `slack` bytes behind the last one
    void add(int id, size_t elemBytes, size_t count, bool reservedOnly = false) { a[n++] = ArenaSpan{id, elemBytes, count, reservedOnly}; }
};
// base == null: the cursor only counts
struct ArenaCursor {
    char *base = nullptr;
    size_t align = 256, off = 0;
    void *take(size_t bytes) { const size_t at = off; off += align_up(bytes, align); return base ? base + at : nullptr; }
    template <class T> T *take_n(size_t count) { return static_cast<T *>(take(count * sizeof(T))); }
};
size_t arena_bytes(const ArenaList &l);                            // the allocation: the walk's end + slack
// out[id] = address of every array of the list (null: reservedOnly); offsets[i], when given, = the offset of span i
void arena_carve(const ArenaList &l, void *base, void *out[WA_COUNT], size_t *offsets = nullptr);

// ---- the queue plan of a launch set

ArenaList frame_arena(size_t slots);   // the per-lane frame arrays of `slots` pixel slots (a multiple of 256)

struct ChunkSplit { int nChunks; size_t ch, room; };   // chunks that hold hits, hits per chunk (a multiple of 256), hits a growing arena is sized for

struct WavePlan {
    WaveOptions opt;
    size_t slots = 0;         // pixel slots of all frames of the batch
    int spp = 1, ao = 0;      // samples per pixel, AO rays per hit (0: AO off)
    int S1 = 0, S2 = 0, L1 = 0;   // slots per hit of shadow queue 1 (WaveBuf::sh1_slot), of shadow queue 2, light slots of queue 1
    size_t giOrgs = 1;        // bounce origins per hit (RT_BIN_GI: one per record)
    size_t perHit = 0;        // budget estimate of the queue bytes per hit (no 256-byte rounding)
    size_t chBudget = 0;      // chunk capacity the budget allows
    bool deferred = false;    // sized from the hit count, read back behind k_post_primary, instead of from the pixel slots
    bool tooLarge = false;    // chBudget * max(S1, S2) reaches 2^31 entries: refused (kTooLargeMessage)

    // entries per slot of shadow queue 2 for a chunk of `ch` hits: the worst case, or -- predict -- from the share of bounce hits seen so far
    size_t q2_entries(size_t ch, bool predict, double share) const;
    int chunks_upper_bound() const { return (int)((slots + chBudget - 1) / chBudget); }   // every pixel slot a hit
    ChunkSplit split(size_t hits) const;
    ArenaList ray_arena(size_t ch, size_t q2Entries) const;
    ArenaList result_arena(size_t ch) const;
    size_t ray_bytes(size_t ch, bool predict, double share) const { return arena_bytes(ray_arena(ch, q2_entries(ch, predict, share))); }
    size_t result_bytes(size_t ch) const { return arena_bytes(result_arena(ch)); }
};
extern const char *const kTooLargeMessage;
// aoRays: 0 when AO is off
WavePlan wave_plan(size_t slots, int spp, int aoRays, const WaveOptions &opt);
// the same for a pipeline that has no lane (rt_debug_wave_plan): RtWavePlan of include/rt_mi355.h.  hits < 0: before the hit count is known.
void wave_plan_describe(const WavePlan &p, long long hits, double share, RtWavePlan &out);

}  // namespace rtl
