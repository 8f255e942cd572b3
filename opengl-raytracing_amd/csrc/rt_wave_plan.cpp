// rt_wave_plan.cpp -- the ray-queue planner of the wavefront pipeline (rt_wave_plan.hpp).  Plain arithmetic: no HIP, no context.
#include "rt_wave_plan.hpp"

#include <cstdlib>
#include <cstring>
#include <string>

namespace rtl {

WaveOptions wave_default_options() {
    WaveOptions o;
    std::memset(&o, 0, sizeof o);
    // ray-queue budget per frame lane; 288 GB of HBM make this cheap.  16 GB hold the queues of a whole batch of eight 1080p / 4 spp frames (7.4 M hits x
    // 2.1 KB) in ONE chunk: no hit-count read-back, half the launches (1.76-1.80 -> 1.68-1.72 ms per frame against 8 GB; profiles/r03_experiments.txt)
    o.budgetBytes = (uint64_t)16 << 30;
    o.q2Predict = 1;    // RT_Q2_PREDICT=0: always the worst case, as in rounds 1-4 (A/B)
    o.probeMode = -1;   // RT_BOUNCE_PROBE: 0 never, 1 always, -1 (auto) while the bounce-hit share of earlier launch sets is below kProbeShareMax
    return o;
}

WaveOptions wave_options_from_env() {
    WaveOptions o = wave_default_options();
    auto num = [](const char *name, int32_t &set, int32_t &value) { if (const char *e = getenv(name)) { set = 1; value = atoi(e); } };
    int32_t set = 0, v = 0;
    if (const char *e = getenv("RT_QUEUE_BUDGET_MB")) o.budgetBytes = (uint64_t)((size_t)atoll(e) << 20);
    if (const char *e = getenv("RT_Q2_CAP")) { o.q2CapSet = 1; o.q2Cap = (uint64_t)(size_t)atoll(e); }   // tests: force the overflow path
    if (const char *e = getenv("RT_Q2_PREDICT")) o.q2Predict = atoi(e) != 0;
    if (const char *e = getenv("RT_BIN_GI")) o.binGi = atoi(e) != 0;   // (experiment) bounce rays sorted by direction inside each workgroup of k_gen_direct
    if (const char *e = getenv("RT_PACKET_AO")) o.packetAO = atoi(e) != 0;   // (measured option, round 4) the AO rays of a hit traced as one packet (k_trace_packets) instead of one by one in the any-hit launch
    if (const char *e = getenv("RT_CHUNKS_FROM_SLOTS")) o.chunksFromSlots = atoi(e) != 0;   // (tests) launch the chunk loop for every pixel slot, as rounds 1-2 did
    if (const char *e = getenv("RT_BOUNCE_PROBE")) o.probeMode = std::string(e) == "auto" ? -1 : (atoi(e) != 0 ? 1 : 0);
    if (const char *e = getenv("RT_CU_SPLIT")) o.cuSplit = std::max(1, std::min(7, atoi(e)));
    num("RT_SHADE_PRIORITY", o.shadePrioritySet, o.shadePriority);
    num("RT_DEBUG_SKIP_TRAVERSAL", o.skipTraversalSet, o.skipTraversal);
    set = 0; num("RT_GRID_PCT", set, v); if (set) o.gridPct = std::max(1, v);
    set = 0; num("RT_GRID_PCT_PRIMARY", set, v); if (set) o.gridPctPrimary = std::max(1, v);
    num("RT_CHUNK_PRIMARY", o.chunkPrimarySet, o.chunkPrimary);
    num("RT_TRACE_STATS", o.traceStatsSet, o.traceStats);
    num("RT_TRACE_TIMING", o.traceTimingSet, o.traceTiming);
    return o;
}

int batch_interleave_from_env() {
    const char *e = getenv("RT_BATCH_INTERLEAVE");
    return e ? (atoi(e) != 0 ? 1 : 0) : 1;
}

int beam_cull_from_env() {
    const char *e = getenv("RT_BEAM_CULL");
    if (!e || !*e || !strcmp(e, "auto")) return -1;
    return atoi(e) != 0 ? 1 : 0;
}

const char *wave_array_name(int id) {
    static const char *const names[WA_COUNT] = {"cand", "primT", "primTri", "hits", "pendC", "pendPos", "pendNrm", "pendMy", "shO", "shD", "shT", "aoOrg", "giD",
                                                "giOrg", "sh2O", "sh2D", "sh2T", "occ1", "giT", "giTri", "occ2", "occOvf", "giPos", "giPerm", "giHit"};
    return id >= 0 && id < WA_COUNT ? names[id] : "";
}

size_t arena_bytes(const ArenaList &l) {
    ArenaCursor c;
    c.align = l.align;
    for (int i = 0; i < l.n; ++i) (void)c.take(l.a[i].elemBytes * l.a[i].count);
    return c.off + l.slack;
}
void arena_carve(const ArenaList &l, void *base, void *out[WA_COUNT], size_t *offsets) {
    ArenaCursor c;
    c.base = static_cast<char *>(base);
    c.align = l.align;
    for (int i = 0; i < l.n; ++i) {
        if (offsets) offsets[i] = c.off;
        void *p = c.take(l.a[i].elemBytes * l.a[i].count);
        out[l.a[i].id] = l.a[i].reservedOnly ? nullptr : p;
    }
}

const char *const kTooLargeMessage = "ray queue chunk exceeds 2^31 entries; lower RT_QUEUE_BUDGET_MB";

// Round 4: a launch set whose queues would be large if every pixel slot were a hit (a batch of eight 1080p frames: 30 GB) is sized from its HIT count --
// read back once, behind k_post_primary, on this lane's stream only (the other lanes keep the GPU busy: 1.726 vs 1.719 ms per frame with and without
// that read-back, profiles/r04_experiments.txt) -- instead of from the budget.  Small launch sets (and RT_CHUNKS_FROM_SLOTS) are sized from their pixel
// slots as before and never wait for the host.
constexpr size_t kComfortBytes = (size_t)4 << 30;

WavePlan wave_plan(size_t slots, int spp, int aoRays, const WaveOptions &opt) {
    WavePlan p;
    p.opt = opt;
    p.slots = slots;
    const int SPP = p.spp = std::max(spp, 1);
    const int A = p.ao = std::max(aoRays, 0);
    p.S1 = A + 4 * SPP + 2; p.S2 = 6 * SPP;   // WaveBuf::sh1_slot
    // chunk capacity from the budget
    // bytes per hit: 36 per light ray (origin, direction, tMax word), 16 per dense ray (AO, bounce) + 16 per hit and dense group for its origin; results as before
    p.L1 = p.S1 - A;                                        // light slots of shadow queue 1
    p.giOrgs = opt.binGi ? (size_t)SPP : 1;                 // bounce origins per hit (RT_BIN_GI: one per record)
    p.perHit = (size_t)(p.L1 + p.S2) * 36 + (size_t)(A + SPP) * 16 + (size_t)((A > 0 ? 1 : 0) + p.giOrgs) * 16 + (size_t)p.S1 + (size_t)SPP * 12 + (size_t)p.S2;
    p.chBudget = align_up(std::min(slots, std::max<size_t>((size_t)opt.budgetBytes / p.perHit, 4096)), 256);
    p.deferred = !opt.chunksFromSlots && arena_bytes(p.ray_arena(p.chBudget, p.chBudget * (size_t)SPP)) > kComfortBytes;   // (every bounce ray a hit)
    p.tooLarge = p.chBudget * (size_t)std::max(p.S1, p.S2) >= ((size_t)1 << 31);
    return p;
}

// Shadow queue 2 (round 5): six ray records per bounce HIT, behind queue 1 in the same allocation.  Sized for the worst case -- every bounce ray
// hits -- it was 48 % of the ray arenas; on the bench view 1 % of that is used.  A LARGE launch set (sized from its hit count anyway) sizes it from what earlier
// launch sets needed: twice the largest share of (hit, sample) pairs that bounced so far + slack, the worst case while nothing is known; pairs beyond the capacity -- a
// view whose bounce hits more than doubled -- are traced in place by k_gen_gi_overflow instead of queued (an order of magnitude slower per ray: 1 M-triangle scene, 20 ms
// per frame with half the pairs overflowing -- hence never a guess below the worst case).  Small launch sets take the worst case, no question asked of the device.
size_t WavePlan::q2_entries(size_t ch, bool predict, double share) const {
    const size_t worst = ch * (size_t)spp;
    size_t n2 = (opt.q2Predict && predict && share > 0.0) ? std::max<size_t>((size_t)(2.0 * share * (double)worst) + 65536, worst / 32) : worst;
    if (opt.q2CapSet) n2 = std::max<size_t>((size_t)opt.q2Cap, 64);   // tests: force the overflow path
    return align_up(std::min(n2, worst), 64);
}

// More than one chunk: the hits are dealt over equal chunks.
ChunkSplit WavePlan::split(size_t hits) const {
    ChunkSplit s;
    s.nChunks = (int)((hits + chBudget - 1) / chBudget);
    s.ch = s.nChunks > 0 ? align_up((hits + (size_t)s.nChunks - 1) / (size_t)s.nChunks, 256) : chBudget;
    // the arenas hold this launch set's hits (+ 6 % when they have to grow); a set of several chunks gets the whole budget at once: its chunk size
    // changes with the number of frames in the batch (20 M hits = 3 x 6.7 M, 17 M = 2 x 8.6 M), and growing a 16 GB arena in the middle of a run
    // is a device-wide synchronisation plus a large allocation (the 1 M-triangle scene at --steps 20: 47.6 instead of 18.7 ms per frame)
    s.room = s.nChunks > 1 ? chBudget : std::min(chBudget, align_up(s.ch + s.ch / 16, 256));
    return s;
}

// per-frame arena: candidates, primary answers, hits, and everything the frame produced before the temporal resolve
ArenaList frame_arena(size_t slots) {
    ArenaList l;
    l.align = 16;      // slots is a multiple of 256: every sub-array stays 16-byte aligned with nothing between them
    l.add(WA_CAND, 4, slots); l.add(WA_PRIMT, 4, slots); l.add(WA_PRIMTRI, 4, slots); l.add(WA_HITS, kHitRecBytes, slots);
    l.add(WA_PENDC, 16, slots); l.add(WA_PENDPOS, 8, slots); l.add(WA_PENDNRM, 8, slots); l.add(WA_PENDMY, 4, slots);
    return l;
}
// ray records + liveness words (read by the traversal launches only: a SHARED arena can be handed on as soon as the last of them is done) ...
// (shadow queue 2 -- six slots per bounce HIT -- has a slack of its own since round 5)
ArenaList WavePlan::ray_arena(size_t ch, size_t n2) const {
    ArenaList l;
    l.slack = 2 * 4096;
    l.add(WA_SHO, 16, ch * (size_t)L1); l.add(WA_SHD, 16, ch * (size_t)S1); l.add(WA_SHT, 4, ch * (size_t)L1); l.add(WA_AOORG, 16, ch);
    l.add(WA_GID, 16, ch * (size_t)spp); l.add(WA_GIORG, 16, ch * giOrgs);
    l.add(WA_SH2O, 16, n2 * 6); l.add(WA_SH2D, 16, n2 * 6); l.add(WA_SH2T, 4, n2 * 6);
    return l;
}
// ... and the results k_combine reads (1 byte per any-hit ray, 4 + 4 per bounce ray, 4 per (hit, sample)) + the bounce probe's hit list (4 per bounce ray): the lane's own
ArenaList WavePlan::result_arena(size_t ch) const {
    ArenaList l;
    l.slack = 4096;
    const size_t pairs = ch * (size_t)spp;
    l.add(WA_OCC1, 1, ch * (size_t)S1); l.add(WA_GIT, 4, pairs); l.add(WA_GITRI, 4, pairs); l.add(WA_OCC2, 1, ch * (size_t)S2); l.add(WA_OCCOVF, 1, ch * (size_t)S2);
    l.add(WA_GIPOS, 4, pairs);
    if (opt.binGi) l.add(WA_GIPERM, 4, pairs);
    l.add(WA_GIHIT, 4, pairs);
    if (!opt.binGi) l.add(WA_GIPERM, 4, pairs, true);   // always reserved, so that the lane's arrays do not depend on the experiment
    return l;
}

static void describe_arena(const ArenaList &l, size_t allocBytes, RtWavePlanArena &out) {
    void *unused[WA_COUNT];
    size_t offsets[9];
    arena_carve(l, nullptr, unused, offsets);
    out.bytes = arena_bytes(l);
    out.allocBytes = allocBytes;
    out.nArrays = l.n;
    for (int i = 0; i < l.n; ++i) {
        std::strncpy(out.arrays[i].name, wave_array_name(l.a[i].id), sizeof out.arrays[i].name - 1);
        out.arrays[i].offset = l.a[i].reservedOnly ? ~(uint64_t)0 : offsets[i];
        out.arrays[i].bytes = l.a[i].elemBytes * l.a[i].count;
    }
}

void wave_plan_describe(const WavePlan &p, long long hits, double share, RtWavePlan &out) {
    std::memset(&out, 0, sizeof out);
    out.options = p.opt;
    out.slots = p.slots; out.perHit = p.perHit; out.chBudget = p.chBudget;
    out.spp = p.spp; out.ao = p.ao; out.S1 = p.S1; out.S2 = p.S2; out.L1 = p.L1; out.deferred = p.deferred ? 1 : 0;
    // as rt_wave_render goes: the hit count is read back for a deferred set and for one of several chunks, never under RT_CHUNKS_FROM_SLOTS
    ChunkSplit s{p.chunks_upper_bound(), p.chBudget, p.chBudget};
    const bool known = hits >= 0 && (p.deferred || s.nChunks > 1) && !p.opt.chunksFromSlots;
    if (known) { s = p.split((size_t)hits); if (!p.deferred) s.room = p.chBudget; }
    s.room = std::max(s.room, s.ch);
    const bool predict = known && p.deferred;
    out.nChunks = s.nChunks; out.ch = s.ch; out.room = s.room;
    out.q2Entries = p.q2_entries(s.ch, predict, share);
    describe_arena(frame_arena(p.slots), arena_bytes(frame_arena(p.slots)), out.frame);
    describe_arena(p.ray_arena(s.ch, out.q2Entries), p.ray_bytes(s.room, predict, share), out.rays);
    describe_arena(p.result_arena(s.ch), p.result_bytes(s.room), out.results);
}

}  // namespace rtl
