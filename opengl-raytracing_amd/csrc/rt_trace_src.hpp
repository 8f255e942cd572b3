// rt_trace_src.hpp -- the ray sources of the persistent traversal kernel (k_trace, rt_trace.hpp): where a launch's rays come from and where their answers go.
// Part of the rt_wave.hip translation unit: included by it alone, behind its `#pragma clang fp contract(off)` and `using namespace rtd;`.
#pragma once
#include "rt_wave_buf.hpp"

namespace {
// primary ray of pixel (px, py) in the batch's k-th frame: that frame's jitter (rt.frag:58-68)
RT_DEV V3 primaryDirK(const DevFrame *fr, int k, int px, int py) { return primaryDirJ(fr->u, (float)px + 0.5f, (float)py + 0.5f, fr->jitterK[k][0], fr->jitterK[k][1]); }

// The ray-source protocol: what k_trace (and nothing else) asks of the `Src` it is built for.  Ray r, r < size(), is a SLOT that may or may not hold a ray.
//   prepare()                          once per lane, first: cache what only the device knows (queue lengths); size(): the slots the scheduler cuts into runs
//   probe(r, payload)                  refill: window lane i probes slot r0 + i -- its tMax, < 0 = no ray -- and notes in `payload` what the taker needs
//   route(payload, e)                  window entry e's payload, moved across lanes to the idle lane that takes the entry
//   take(r, payload, ro, rd, token)    that lane reads its ray; `token` is what the store_* get back when the ray retires
//   store_closest(token, t, tri) / store_any(token, occluded)   the answer: from pop_or_finish, the leaf phase, or start_ray for a ray that misses the root box
//   dense(r0, r1)                      true: (nearly) every slot of the window [r0, r1) is a ray -- no probe, the i-th idle lane calls
//   probe_take(r0 + i, ro, rd, token)  tMax and record in one round trip (< 0 leaves the lane idle)
// AddrSrc: the parts most sources share -- the payload is one address, nothing to prepare, no any-hit answer, no dense slots.  A source derives from AddrSrc<itself>
// (an empty base of a type of its own, so that a source wrapped as another's first member keeps its offsets) and defines what differs.
template <class Self> struct AddrSrc {
    struct Payload { uint32_t a; };
    RT_DEV static Payload route(const Payload &p, int e) { Payload q; q.a = (uint32_t)__shfl((int)p.a, e, 64); return q; }
    RT_DEV void prepare() {}
    RT_DEV void store_any(uint32_t, bool) const {}
    RT_DEV bool dense(uint32_t, uint32_t) const { return false; }
    RT_DEV float probe_take(uint32_t, V3 &, V3 &, uint32_t &) const { return -1.0f; }
};

// Sparse answers (round 17): for the frame's own primary and any-hit sources -- PrimarySrc, QueueSrc::store_any, DualQueueSrc -- an answer array holds the MISS answer
// before the launch starts (primTri = -1, occ = 0: written coalesced by whoever writes the ray at the same index: k_primary, GenDirectTracer, GenGiTracer), and the launch
// overwrites it only for a hit or an occlusion: a retiring miss stores nothing.  Everything else stores every answer: the bounce queue's launches (BounceProbeSrc,
// QueueSrc::store_closest -- pre-filling giTri was measured and gained nothing) and the sources over the caller's memory or a dense list (IndexedSrc,
// IndexedDenseSrc, CompactSrc, QuerySrc, SceneSrc).
struct PrimarySrc : AddrSrc<PrimarySrc> {   // ray i = primary ray of candidate i
    const DevFrame *fr;
    const uint32_t *cand;
    const uint32_t *count;
    float *outT;
    int *outTri;
    RT_DEV uint32_t size() const { return *count; }
    // probe / take: see QueueSrc.  Every candidate is a ray; what the window read brings in is the candidate's pixel slot.
    struct Payload { uint32_t slot; };
    RT_DEV float probe(uint32_t i, Payload &p) const { p.slot = cand[i]; return fr->u.inf; }
    RT_DEV static Payload route(const Payload &p, int e) { Payload q; q.slot = (uint32_t)__shfl((int)p.slot, e, 64); return q; }
    RT_DEV void take(uint32_t i, const Payload &p, V3 &ro, V3 &rd, uint32_t &token) const {
        token = i;
        int px, py;
        pixel_of_slot_div(fr->g, (int)(p.slot >> 8), (int)(p.slot & 255u), px, py);   // (the traversal kernels keep the dividing form, rt_frame.hpp)
        ro = ld3(fr->u.camPos);
        rd = primaryDirK(fr, sub_frame_of_slot_div(fr->g, p.slot), px, py);
    }
    RT_DEV void store_closest(uint32_t i, float t, int tri) const { if (tri >= 0) { outT[i] = t; outTri[i] = tri; } }   // misses are pre-filled, see above
};
struct QueueSrc : AddrSrc<QueueSrc> {     // slot-major queue: ray r -> (slot = r / n, j = r % n) at [slot*stride + j], n = live entries
    const float4 *o, *d;         // d: every slot; o / tm: the slots behind the dense ones, entry [address - denseSlots * stride]
    const float *tm;             // per-slot tMax / liveness
    const uint32_t *liveCount;   // device counter the live entry count derives from
    uint32_t c0, cap, stride, slots;
    uint32_t denseSlots;         // the first `denseSlots` slots hold a ray for (nearly) every entry (AO slots, the bounce queue): see dense() below.  Their record is
                                 // ONE float4 {dir, tMax / liveness}; the origin belongs to the entry, not the slot: org[j] (orgStride = 0), or to the record: org[address]
    const float4 *org;
    uint32_t orgStride;          // 0, or `stride`
    RT_DEV uint32_t nDense() const { return denseSlots * stride; }
    float *outT;
    int *outTri;
    uint8_t *outOcc;
    uint32_t nLive;              // cached by prepare(): the count is final before this kernel starts
    RT_DEV void prepare() { uint32_t h = *liveCount; nLive = min(h, c0 + cap) - min(h, c0); }   // no wrapping subtraction, see chunk_live
    RT_DEV uint32_t size() const { return nLive * slots; }
    RT_DEV uint32_t addr(uint32_t r) const { return (r / nLive) * stride + (r % nLive); }
    // probe(r): window lane `lane` reads slot r's 4-byte liveness / tMax word (< 0 = no ray was cast into this slot); consecutive
    // r are consecutive words, so a 64-lane probe is one coalesced 256-byte read and dead slots (the disk-light samples of
    // surfaces facing away from the light, the sun / point rays of samples > 0) never touch their 32-byte records.  The scheduler
    // routes the queue address of each live slot to the lane that takes it (route: a cross-lane move); take: its record.
    // (Reading the records together with the liveness words -- one round trip per refill instead of two -- was measured slower for
    // the shadow queue, where 55 % of the slots are dead: 1.07 vs 1.01 ms.)
    RT_DEV float probe(uint32_t r, Payload &p) const { p.a = addr(r); return p.a < nDense() ? d[p.a].w : tm[p.a - nDense()]; }   // (dense slots here: RT_DENSE_TAKE=0, or a run across the last dense slot's end)
    RT_DEV void take(uint32_t, const Payload &p, V3 &ro, V3 &rd, uint32_t &token) const {
        token = p.a;                     // results go to the same queue address: no second div/mod at retirement
        const float4 oo = p.a < nDense() ? org[orgStride ? p.a : p.a % stride] : o[p.a - nDense()], dd = d[p.a];
        ro = f4xyz(oo); rd = f4xyz(dd);
    }
    RT_DEV void store_closest(uint32_t a, float t, int tri) const { outT[a] = t; outTri[a] = tri; }
    RT_DEV void store_any(uint32_t a, bool occ) const { if (occ) outOcc[a] = 1; }   // "not occluded" is pre-filled, see above
    // Dense slots (round 4): where (nearly) every entry is a ray the liveness probe is a wasted round trip -- the i-th idle lane takes the i-th entry
    // left and reads liveness word and record together; an entry that is dead after all (AO radius 0, GI switched off) just leaves its lane idle.
    RT_DEV bool dense(uint32_t r0, uint32_t r1) const { return r1 > r0 && (r1 - 1u) / nLive < denseSlots; }
    RT_DEV float probe_take(uint32_t r, V3 &ro, V3 &rd, uint32_t &token) const {
        const uint32_t sl = r / nLive, j = r % nLive, a = sl * stride + j;
        const float4 oo = org[sl * orgStride + j], dd = d[a];
        token = a;
        ro = f4xyz(oo); rd = f4xyz(dd);
        return dd.w;
    }
};

// Light-slot liveness masks: the frames' shadow queues.  Behind the dense slots, bit [address - denseSlots * stride] of `live` says whether
// the slot holds a ray -- the index of o / tm --, and tm of a dead slot is not written at all.  A source with the MaskedSrc trait adds to the protocol:
//   masked()                        the launch has masks; false (live == null, RT_LIGHT_MASKS=0): the source is the unmasked one, dead slots carry tm < 0
//   dense_end(), masked_end()       the slots r in between are the masked ones; those in front are dense slots, those behind an unmasked queue: probed and taken as ever
//   segment(r, rEnd)                the slots from r on that share a queue and a slot (consecutive addresses, consecutive bits), at most up to rEnd
//   take_live(a, ro, rd, token)     tMax and record of the live slot with payload address a, in ONE round trip
// QueueSrc itself stays as it is, for the bounce queue and the debug entries: a member more would move the kernel arguments of their builds.
struct MaskSeg { const unsigned long long *live; uint32_t bit, a, len; };   // the mask array, the bit and the payload address of slot r, slots in the segment
struct MaskedQueueSrc : QueueSrc {
    const unsigned long long *live;
    unsigned long long *maskStat;   // rt_debug_light_masks: [0] mask words scanned [1] masked refill passes; null until the entry was called
    RT_DEV bool masked() const { return live != nullptr; }
    RT_DEV unsigned long long *mask_stat() const { return maskStat; }
    RT_DEV uint32_t dense_end() const { return denseSlots * nLive; }
    RT_DEV uint32_t masked_end() const { return size(); }
    RT_DEV MaskSeg segment(uint32_t r, uint32_t rEnd) const {
        const uint32_t sl = r / nLive, j = r - sl * nLive;
        MaskSeg s;
        s.live = live; s.a = sl * stride + j; s.bit = s.a - nDense(); s.len = min(rEnd - r, nLive - j);
        return s;
    }
    RT_DEV float take_live(uint32_t a, V3 &ro, V3 &rd, uint32_t &token) const {
        token = a;
        const float t = tm[a - nDense()];
        const float4 oo = o[a - nDense()], dd = d[a];
        ro = f4xyz(oo); rd = f4xyz(dd);
        return t;
    }
};

// Two any-hit queues traced by ONE persistent launch (direct shadows + AO, then the shadows at the bounce hits): a second
// launch would pay the ~0.15 ms ramp-up / drain latency of a persistent grid again for a few thousand rays.
struct DualQueueSrc {
    MaskedQueueSrc a, b;
    uint32_t na;
    RT_DEV void prepare() { a.prepare(); b.prepare(); na = a.size(); }
    RT_DEV uint32_t size() const { return na + b.size(); }
    RT_DEV bool masked() const { return a.masked(); }                  // (queue 1, or both: RT_LIGHT_MASKS=2)
    RT_DEV uint32_t masked_end() const { return b.masked() ? size() : na; }
    RT_DEV unsigned long long *mask_stat() const { return a.maskStat; }
    RT_DEV uint32_t dense_end() const { return a.dense_end(); }       // (queue 2 has no dense slots)
    RT_DEV MaskSeg segment(uint32_t r, uint32_t rEnd) const {
        if (r < na) return a.segment(r, min(rEnd, na));
        MaskSeg s = b.segment(r - na, rEnd - na);
        s.a |= 0x80000000u;
        return s;
    }
    RT_DEV float take_live(uint32_t pa, V3 &ro, V3 &rd, uint32_t &token) const {
        const float t = (pa & 0x80000000u) ? b.take_live(pa & 0x7fffffffu, ro, rd, token) : a.take_live(pa, ro, rd, token);
        token = pa;
        return t;
    }
    typedef QueueSrc::Payload Payload;
    RT_DEV float probe(uint32_t r, Payload &p) const {
        if (r < na) return a.probe(r, p);
        const float t = b.probe(r - na, p);
        p.a |= 0x80000000u;               // results of the second queue (addresses stay below 2^31: checked on the host)
        return t;
    }
    RT_DEV static Payload route(const Payload &p, int e) { return QueueSrc::route(p, e); }
    RT_DEV void take(uint32_t r, const Payload &p, V3 &ro, V3 &rd, uint32_t &token) const {
        Payload q;
        q.a = p.a & 0x7fffffffu;
        if (p.a & 0x80000000u) b.take(r, q, ro, rd, token); else a.take(r, q, ro, rd, token);
        token = p.a;
    }
    RT_DEV void store_closest(uint32_t, float, int) const {}
    RT_DEV void store_any(uint32_t token, bool occ) const {
        if (!occ) return;
        if (token & 0x80000000u) b.outOcc[token & 0x7fffffffu] = 1;
        else a.outOcc[token] = 1;
    }
    RT_DEV bool dense(uint32_t r0, uint32_t r1) const { return r1 <= na && a.dense(r0, r1); }
    RT_DEV float probe_take(uint32_t r, V3 &ro, V3 &rd, uint32_t &token) const { return a.probe_take(r, ro, rd, token); }
};

// The bounce queue walked ANY-hit first (RT_BOUNCE_PROBE): almost every bounce ray misses, and a miss does not depend on the
// order the walk visits the leaves in.  A ray whose any-hit walk with tMax = uINF (the closest-hit launch's own start value) finds no triangle
// gets the closest-hit launch's miss answer here -- its triangle, -1; the distance uINF is not stored, nothing reads giT of a ray without a triangle --; the few that hit are listed in `hitters` and walked again by the closest-hit
// kernel (IndexedSrc), unchanged.  Bit-identical because both walks test the same leaves against the same exact boxes with the same tri_hit,
// whose acceptance is monotone in tBest -- true of the 4-wide tree rt_upload_bvh collapses from the binary one (exact or quantised nodes),
// not of RT_ANYHIT_TREE=sah, where the probe is never launched.
struct BounceProbeSrc {
    QueueSrc q;                  // the bounce queue: the .w of its records is a liveness value (1.0), NOT a distance
    uint32_t *hitters, *hitCount;
    float inf;                   // uINF of the frame (the host copy of its descriptor): the closest-hit walk's start value and its answer for a miss
    RT_DEV void prepare() { q.prepare(); }
    RT_DEV uint32_t size() const { return q.size(); }
    typedef QueueSrc::Payload Payload;
    RT_DEV float probe(uint32_t r, Payload &p) const { const float t = q.probe(r, p); return t < 0.0f ? t : inf; }
    RT_DEV static Payload route(const Payload &p, int e) { return QueueSrc::route(p, e); }
    RT_DEV void take(uint32_t r, const Payload &p, V3 &ro, V3 &rd, uint32_t &token) const { q.take(r, p, ro, rd, token); }
    RT_DEV void store_closest(uint32_t, float, int) const {}
    RT_DEV void store_any(uint32_t a, bool hit) const {
        const unsigned long long m = __ballot(hit);   // the lanes that retire a hit in this step append together: one atomic per wave
        if (!hit) { q.outTri[a] = -1; return; }   // (no t for a miss: every reader of giT looks at giTri first)
        const uint32_t lane = threadIdx.x & 63u;
        const int leader = __ffsll((long long)m) - 1;
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(hitCount, (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, leader, 64);
        hitters[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = a;
    }
    RT_DEV bool dense(uint32_t r0, uint32_t r1) const { return q.dense(r0, r1); }
    RT_DEV float probe_take(uint32_t r, V3 &ro, V3 &rd, uint32_t &token) const { const float t = q.probe_take(r, ro, rd, token); return t < 0.0f ? t : inf; }
};

// A dense list of queue addresses (rt_hybrid.hip): ray r is the record at idx[r]; every listed record is a ray.
struct IndexedSrc : AddrSrc<IndexedSrc> {
    const uint32_t *idx;
    const uint32_t *count;
    const float4 *o, *d;
    float *outT;
    int *outTri;
    uint32_t n;
    RT_DEV void prepare() { n = *count; }
    RT_DEV uint32_t size() const { return n; }
    RT_DEV float probe(uint32_t r, Payload &p) const { p.a = idx[r]; return 1.0f; }
    RT_DEV void take(uint32_t, const Payload &p, V3 &ro, V3 &rd, uint32_t &token) const {
        token = p.a;
        const float4 oo = o[p.a], dd = d[p.a];
        ro = f4xyz(oo); rd = f4xyz(dd);
    }
    RT_DEV void store_closest(uint32_t a, float t, int tri) const { outT[a] = t; outTri[a] = tri; }
};

// The same list over the DENSE slots of a queue (the re-trace of the bounce probe's hits): record d[a] = {dir, .}, origin org[a % stride] (orgStride = 0) or org[a].
struct IndexedDenseSrc : AddrSrc<IndexedDenseSrc> {
    const uint32_t *idx;
    const uint32_t *count;
    const float4 *org, *d;
    uint32_t stride, orgStride;
    float *outT;
    int *outTri;
    uint32_t n;
    RT_DEV void prepare() { n = *count; }
    RT_DEV uint32_t size() const { return n; }
    RT_DEV float probe(uint32_t r, Payload &p) const { p.a = idx[r]; return 1.0f; }
    RT_DEV void take(uint32_t, const Payload &p, V3 &ro, V3 &rd, uint32_t &token) const {
        token = p.a;
        const float4 oo = org[orgStride ? p.a : p.a % stride], dd = d[p.a];
        ro = f4xyz(oo); rd = f4xyz(dd);
    }
    RT_DEV void store_closest(uint32_t a, float t, int tri) const { outT[a] = t; outTri[a] = tri; }
};

// A dense array of ray records (rt_hybrid.hip, round 4): ray r is the record o[r] / d[r]; its answer goes to outT / outTri at dst[r] (the asking
// thread's log entry).  The list length is read on the device and clipped to the array's capacity (an overflowing pass is redone by the host).
struct CompactSrc : AddrSrc<CompactSrc> {
    const float4 *o, *d;
    const uint32_t *dst;
    const uint32_t *count;
    const uint32_t *flags;   // bits 2 | 4: a pass outgrew its arrays -- the queue is incomplete and must not be traced
    uint32_t cap;
    uint32_t capOut;         // RT_HYBRID_CHECK=1: entries of outT / outTri; an answer addressed beyond them raises bit 32 of *flags instead of being stored (0: unchecked)
    float *outT;
    int *outTri;
    uint32_t n;
    RT_DEV void prepare() { n = (*flags & 6u) ? 0u : min(*count, cap); }
    RT_DEV uint32_t size() const { return n; }
    RT_DEV float probe(uint32_t r, Payload &p) const { p.a = r; return 1.0f; }
    RT_DEV void take(uint32_t, const Payload &p, V3 &ro, V3 &rd, uint32_t &token) const {
        token = dst[p.a];
        const float4 oo = o[p.a], dd = d[p.a];
        ro = f4xyz(oo); rd = f4xyz(dd);
    }
    RT_DEV void store_closest(uint32_t a, float t, int tri) const {
        if (capOut && a >= capOut) { atomicOr(const_cast<uint32_t *>(flags), 32u); return; }
        outT[a] = t; outTri[a] = tri;
    }
};

// User rays of rt_trace_rays: ray i at o[i * os] / d[i * ds] (strides in floats, >= 3) in the caller's memory, an optional per-ray tMax
// (< 0: an empty slot, answered where the probe meets it: a miss, not occluded).  Without tMax every entry is a ray: the dense take, no liveness
// probe.  Closest-hit rays start with best = tMax (QueryTMax below).  A closest-hit answer is one 16-byte RtHit; its u, v are recomputed when the ray
// retires, from the ray re-read here and the winning triangle, with triHit's operations (rt_bvh.glsl:154-170) -- the walk itself carries nothing extra.
struct QuerySrc : AddrSrc<QuerySrc> {
    const float *o, *d;
    const float *tm;             // null: no tMax
    uint32_t os, ds, n;
    float inf;                   // uINF of the call: the tMax of a ray without one
    const float4 *tris;          // the uploaded tris12: [v0 -][e1 -][e2 -] per triangle
    float4 *hits;                // closest-hit: RtHit {t, prim, u, v} per ray (null for any-hit)
    float *normals;              // closest-hit, optional: 3 floats per ray
    uint8_t *occ;                // any-hit
    RT_DEV uint32_t size() const { return n; }
    RT_DEV V3 origin(uint32_t i) const { return ld3(o + (size_t)i * os); }
    RT_DEV V3 dir(uint32_t i) const { return ld3(d + (size_t)i * ds); }
    RT_DEV void store_empty(uint32_t i) const {
        if (hits) store_closest(i, inf, -1);
        else occ[i] = 0;
    }
    RT_DEV float probe(uint32_t i, Payload &p) const {
        p.a = i;
        if (!tm) return inf;
        const float t = tm[i];
        if (t < 0.0f) store_empty(i);   // (a slot left over in one window is probed again in the next: the same bytes again)
        return t;
    }
    RT_DEV void take(uint32_t, const Payload &p, V3 &ro, V3 &rd, uint32_t &token) const { token = p.a; ro = origin(p.a); rd = dir(p.a); }
    RT_DEV void store_closest(uint32_t i, float t, int tri) const {
        float u = 0.0f, v = 0.0f;
        V3 nrm = mk3(0.0f);
        if (tri >= 0) {
            const V3 ro = origin(i), rd = dir(i);
            const float4 *T = tris + (size_t)tri * 3;
            const V3 v0 = f4xyz(T[0]), e1 = f4xyz(T[1]), e2 = f4xyz(T[2]);
            const V3 pvec = cross(rd, e2);                 // tri_hit's operations, in its order
            const float invDet = 1.0f / dot(e1, pvec);
            const V3 tvec = ro - v0;
            u = dot(tvec, pvec) * invDet;
            v = dot(rd, cross(tvec, e1)) * invDet;
            if (normals) nrm = normalize(cross(e1, e2));   // hitOut.n of traceBVH
        }
        hits[i] = make_float4(t, __int_as_float(tri), u, v);
        if (normals) { normals[(size_t)i * 3] = nrm.x; normals[(size_t)i * 3 + 1] = nrm.y; normals[(size_t)i * 3 + 2] = nrm.z; }
    }
    RT_DEV void store_any(uint32_t i, bool hit) const { occ[i] = hit ? 1 : 0; }
    RT_DEV bool dense(uint32_t, uint32_t) const { return tm == nullptr; }
    RT_DEV float probe_take(uint32_t r, V3 &ro, V3 &rd, uint32_t &token) const { token = r; ro = origin(r); rd = dir(r); return inf; }
};
// The mesh leg of rt_trace_scene_rays / rt_pick_pixels.  The analytic leg (rt_scene_query.hip) has already written every ray's answer into
// the caller's outputs: the analytic scene's, bounded by tMax (hybrid mode), or a miss / "not occluded" (BVH mode), so this source never stores an empty
// slot.  Rays are the caller's strided arrays, or pixel rays built here from the uniform block of the query's frame descriptor (primaryDirJ, as the frame
// builds them) -- whenever a ray is taken and again when its answer is stored.
//   BVH mode: the probe returns tMax (uINF without), every walked ray stores its answer: the bytes of QuerySrc.
//   hybrid, closest: the walk is the frame's, unbounded (best = uINF, as traceScene's bvh_closest); the mesh answer t_m replaces the stored one only at
//   t_m < t_a -- traceScene's rule, the earlier object wins a tie -- and t_m <= tMax.  t_a is the t the analytic leg stored (uINF: none, or beyond tMax).
//   (Not a walk bounded by min(t_a, tMax): a triangle flush with a face of its box can lie a few ulps before that box's slab entry, so a bound
//   equal to its t culls it -- a mesh resting on the floor would then lose to the floor although the frame shows it)
//   hybrid, any: rays the analytic scene occludes are not walked (empty slots); the others take traceBVHShadow's answer.
struct SceneSrc : AddrSrc<SceneSrc> {
    const float *o, *d;
    const int32_t *xy;           // pixel rays (null: o / d)
    const RtUniforms *cam;       // pixel rays: the query's uniform block (in its frame descriptor)
    const float *tm;             // null: no tMax
    uint32_t os, ds, n;
    float inf;
    bool hybrid;
    const float4 *tris;
    float4 *hits;                // closest-hit (null for any-hit)
    int32_t *objects;
    float *normals, *points;
    uint8_t *occ;                // any-hit
    RT_DEV uint32_t size() const { return n; }
    RT_DEV V3 origin(uint32_t i) const { return xy ? ld3(cam->camPos) : ld3(o + (size_t)i * os); }
    RT_DEV V3 dir(uint32_t i) const {
        if (!xy) return ld3(d + (size_t)i * ds);
        return primaryDirJ(*cam, (float)xy[(size_t)i * 2] + 0.5f, (float)xy[(size_t)i * 2 + 1] + 0.5f, cam->jitter[0], cam->jitter[1]);
    }
    RT_DEV float probe(uint32_t i, Payload &p) const {
        p.a = i;
        if (!hits) {
            if (hybrid && occ[i]) return -1.0f;   // occluded by the analytic scene
            return tm[i];
        }
        const float b = tm ? tm[i] : inf;
        return (hybrid && !(b < 0.0f)) ? inf : b;
    }
    RT_DEV void take(uint32_t, const Payload &p, V3 &ro, V3 &rd, uint32_t &token) const { token = p.a; ro = origin(p.a); rd = dir(p.a); }
    RT_DEV void store_closest(uint32_t i, float t, int tri) const {
        if (hybrid && !(tri >= 0 && t < hits[i].x && (!tm || t <= tm[i]))) return;   // the analytic answer stands
        float u = 0.0f, v = 0.0f;
        V3 nrm = mk3(0.0f), pt = mk3(0.0f);
        if (tri >= 0) {
            const V3 ro = origin(i), rd = dir(i);
            const float4 *T = tris + (size_t)tri * 3;
            const V3 v0 = f4xyz(T[0]), e1 = f4xyz(T[1]), e2 = f4xyz(T[2]);
            const V3 pvec = cross(rd, e2);                 // tri_hit's operations, in its order (QuerySrc::store_closest)
            const float invDet = 1.0f / dot(e1, pvec);
            const V3 tvec = ro - v0;
            u = dot(tvec, pvec) * invDet;
            v = dot(rd, cross(tvec, e1)) * invDet;
            if (normals) nrm = normalize(cross(e1, e2));   // hit.n of traceScene / traceBVH
            pt = ro + rd * t;                              // hit.p
        }
        hits[i] = make_float4(t, __int_as_float(tri), u, v);
        if (objects) objects[i] = tri >= 0 ? RT_OBJECT_MESH : RT_OBJECT_NONE;
        if (normals) { normals[(size_t)i * 3] = nrm.x; normals[(size_t)i * 3 + 1] = nrm.y; normals[(size_t)i * 3 + 2] = nrm.z; }
        if (points) { points[(size_t)i * 3] = pt.x; points[(size_t)i * 3 + 1] = pt.y; points[(size_t)i * 3 + 2] = pt.z; }
    }
    RT_DEV void store_any(uint32_t i, bool hit) const { occ[i] = hit ? 1 : 0; }
    RT_DEV bool dense(uint32_t, uint32_t) const { return tm == nullptr; }
    RT_DEV float probe_take(uint32_t r, V3 &ro, V3 &rd, uint32_t &token) const { token = r; ro = origin(r); rd = dir(r); return inf; }
};

// Closest-hit rays of a source with this trait start their walk with best = the tMax the source hands out (QuerySrc) instead of uINF; the frame
// sources keep uINF (a compile-time choice: their kernels are the same instructions as without it).
template <class Src> struct QueryTMax { static constexpr bool value = false; };
template <> struct QueryTMax<QuerySrc> { static constexpr bool value = true; };
template <> struct QueryTMax<SceneSrc> { static constexpr bool value = true; };
// The sources with light-slot liveness masks (MaskedQueueSrc above): k_trace builds its masked refill for them alone, every other build keeps its instructions.
template <class Src> struct MaskedSrc { static constexpr bool value = false; };
template <> struct MaskedSrc<MaskedQueueSrc> { static constexpr bool value = true; };
template <> struct MaskedSrc<DualQueueSrc> { static constexpr bool value = true; };
}  // namespace
