// rt_wave_stages.hpp -- the shading stages of the wavefront pipeline (see rt_wave.hip): primary, post_primary, gen_direct, gen_gi, combine, resolve, and the tracer
// policies through which they run the reference's shading code.
// Part of the rt_wave.hip translation unit: included by it alone, behind its `#pragma clang fp contract(off)` and `using namespace rtd;`.
#pragma once
#include <type_traits>

#include "rt_beam.hpp"    // the beam cull's interval arithmetic (k_beam_cull)
#include "rt_trace.hpp"   // rt_dyn_lds (k_gen_gi_overflow's stacks)

namespace {
// ---- finishing a pixel.  rt.frag:184-196 = frame average -> TAA resolve against the history -> 4 target stores.  The history
// read is the ONLY dependency of a frame on its predecessor, so the stages stash the pre-resolve values and a final k_resolve
// does TAA + stores.  Frames f and f+1 run on two streams and overlap everywhere except resolve(f) -> resolve(f+1), which
// keeps the GPU busy when one frame's stages are latency-bound (tile-parallel ranks with 1/8 of the pixels, small frames).
RT_DEV void finish_pixel(const DevFrame *fr, const WaveBuf &wb, int slot, V3 frameSum, V2 motionOut, V4 gpos, V4 gnrm) {
    const int SPP = max(fr->u.spp, 1);
    V3 curr = frameSum / (float)SPP;
    wb.pendC[slot] = make_float4(curr.x, curr.y, curr.z, motionOut.x);
    wb.pendMy[slot] = motionOut.y;
    wb.pendPos[slot] = pack_half4(gpos);
    wb.pendNrm[slot] = pack_half4(gnrm);
}
// History of the still-camera resolve inside a batch: frame k > 0 reads what frame k-1 of the same batch just produced, rounded to
// fp16 as the RGBA16F target would hold it.
struct ChainedHistory {
    HistoryTex tex;
    bool chained;
    V4 value;
    RT_DEV V4 own() const { return chained ? value : tex.own(); }
    RT_DEV V4 at(float u, float v) const { return tex.at(u, v); }   // reprojection: never inside a batch (static camera only)
};
__global__ __launch_bounds__(256) void k_resolve(const DevFrame *__restrict__ fr, Targets tg, WaveBuf wb) {
    const RtUniforms &u = fr->u;
    int px, py;
    if (!pixel_of_slot(fr->g, blockIdx.x, threadIdx.x, px, py)) return;
    const int slot = blockIdx.x * 256 + threadIdx.x;
    float uvx = ((float)px + 0.5f) / (float)fr->g.W, uvy = ((float)py + 0.5f) / (float)fr->g.H;   // rt_fullscreen.vert:44
    ChainedHistory hist;
    hist.tex.prev = tg.prev; hist.tex.prevAll = tg.prevAll; hist.tex.blockSlots = tg.blockSlots; hist.tex.g = &fr->g; hist.tex.slot = slot;
    hist.chained = false;
    const int K = max(fr->g.batch, 1);
    const int perFrame = fr->g.nLocalTiles * 256;   // slots of one frame of the batch
    uint2 colorBits = make_uint2(0u, 0u);
    V2 motionOut = mk2(0.0f, 0.0f);
    int sk = slot;
    for (int k = 0; k < K; ++k, sk += perFrame) {
        float4 pc = wb.pendC[sk];
        V3 curr = mk3(pc.x, pc.y, pc.z);
        motionOut = mk2(pc.w, wb.pendMy[sk]);
        V2 taaMotion = (u.cameraMoved == 1) ? motionOut : mk2(0.0f, 0.0f);
        V4 taa = resolveTAA(u, curr, uvx, uvy, taaMotion, u.frameIndex + k, hist);
        colorBits = pack_half4(taa);
        hist.chained = true;
        hist.value = unpack_half4(colorBits);        // what the next frame's texture(uPrevAccum, uv) returns: the fp16 target
    }
    sk -= perFrame;                                  // the targets hold the batch's last frame
    tg.color[slot] = colorBits;
    tg.motion[slot] = pack_half2(motionOut);
    tg.gpos[slot] = wb.pendPos[sk];
    tg.gnrm[slot] = wb.pendNrm[sk];
}
RT_DEV void finish_miss(const DevFrame *fr, const WaveBuf &wb, int slot, int px, int py, V3 dir) {
    const RtUniforms &u = fr->u;
    Frag F;
    F.u = &u; F.sc = &fr->sc; F.fcx = (float)px + 0.5f; F.fcy = (float)py + 0.5f;
    F.frameIndex = u.frameIndex + sub_frame_of_slot(fr->g, (uint32_t)slot);
    Work w;
    V3 r = sky<false>(F, dir, w);
    V3 frameSum = mk3(0.0f);
    const int SPP = max(u.spp, 1);
    for (int s = 0; s < SPP; ++s) frameSum = frameSum + r;   // the reference adds the same radiance SPP times
    V2 motionOut = (u.cameraMoved == 1) ? mk2(4.0f, 4.0f) : mk2(0.0f, 0.0f);
    finish_pixel(fr, wb, slot, frameSum, motionOut, mk4(0, 0, 0, 0), mk4(0, 0, 0, 0));
}
RT_DEV void slot_to_pixel(const FrameGeom &g, uint32_t slot, int &px, int &py) { pixel_of_slot(g, (int)(slot >> 8), (int)(slot & 255u), px, py); }

// block-level append (all 256 threads must call): ONE atomic per workgroup on the list counter -- a single
// counter word sustains only ~88 M atomics/s, which per-wave appends of a 1080p frame would saturate.
RT_DEV uint32_t block_append(bool pred, uint32_t *counter) {
    __shared__ uint32_t s_cnt[4];
    __shared__ uint32_t s_base;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long m = __ballot(pred);
    if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        s_base = tot ? atomicAdd(counter, tot) : 0u;
    }
    __syncthreads();
    uint32_t off = s_base;
    for (uint32_t i = 0; i < wv; ++i) off += s_cnt[i];
    uint32_t r = off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();   // s_cnt / s_base may be reused by a second append in the same kernel
    return r;
}

// ---- stage: beam cull (RT_BEAM_CULL) -------------------------------------------------
// One wave per local spatial tile, in front of the primary stage: tileDead[lt] = 1 when every primary ray of the tile, in every frame of the launch set, surely
// misses the mesh (rt_beam.hpp has the argument; rt_debug_beam_cull is the same verdict on the host).  The lanes share the tile's 256 x batch rays and reduce their
// rdInv components to [L, H] per axis; then lane i stands on frontier node i of the interval walk: a level is one record load per lane, two ballots and a
// compaction by rank (the order of a level's nodes does not matter to the verdict).  stat (rt_debug_beam_cull_stats, null until the entry was called): tiles, dead
// tiles, tiles kept because a level overflowed, levels walked.
RT_DEV int nth_set_bit(unsigned long long m, int j) {   // position of the j-th set bit of m, j < popcount(m)
    int pos = 0;
    for (int w = 32; w >= 1; w >>= 1) {
        const int c = __popcll((m >> pos) & ((1ull << w) - 1ull));
        if (j >= c) { j -= c; pos += w; }
    }
    return pos;
}
__global__ __launch_bounds__(256) void k_beam_cull(const DevFrame *__restrict__ fr, uint8_t *__restrict__ tileDead, unsigned long long *__restrict__ stat) {
    const int lane = (int)(threadIdx.x & 63u), lt = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
    const int nl = fr->g.nLocalTiles, batch = max(fr->g.batch, 1);
    if (lt >= nl) return;   // (whole waves)
    rtbeam::Interval I;
    rtbeam::interval_clear(I);
    bool bad = false;
    for (int k = 0; k < batch; ++k)
        for (int q = 0; q < 4; ++q) {
            int px, py;
            if (!pixel_of_slot(fr->g, k * nl + lt, q * 64 + lane, px, py)) continue;
            const V3 dir = primaryDirK(fr, k, px, py);
            const V3 rdInv = mk3(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);   // primary_pixel's three divisions
            const float r[3] = {rdInv.x, rdInv.y, rdInv.z};
            for (int a = 0; a < 3; ++a) {
                if (!rtbeam::usable(r[a])) bad = true;
                else { I.L[a] = fminr(I.L[a], r[a]); I.H[a] = fmaxr(I.H[a], r[a]); }
            }
        }
    for (int off = 32; off > 0; off >>= 1)
        for (int a = 0; a < 3; ++a) { I.L[a] = fminr(I.L[a], __shfl_xor(I.L[a], off, 64)); I.H[a] = fmaxr(I.H[a], __shfl_xor(I.H[a], off, 64)); }
    const float ro[3] = {fr->u.camPos[0], fr->u.camPos[1], fr->u.camPos[2]};
    int verdict = rtbeam::kAlive, levels = 0;
    if (fr->sc.hasBVH && __ballot(bad) == 0ull && rtbeam::interval_ok(I.L, I.H)) {
        if (rtbeam::slab_fails_ok(ro, fr->sc.rootMin, fr->sc.rootMax, I.L, I.H)) verdict = rtbeam::kDead;
        else if (fr->sc.rootRefW >= 0) {
            const float4 *nodes = fr->sc.wnodesW;
            int node = fr->sc.rootRefW, n = 1;   // lane i < n stands on frontier node `node`
            verdict = rtbeam::kDead;
            while (n > 0) {
                ++levels;
                bool in0 = false, in1 = false, leaf = false;
                int r0 = 0, r1 = 0;
                if (lane < n) {
                    const float4 *rec = nodes + (size_t)node * 4;
                    const float4 a = rec[0], b = rec[1], c = rec[2], d = rec[3];
                    const float lo0[3] = {a.x, a.y, a.z}, hi0[3] = {b.x, b.y, b.z}, lo1[3] = {c.x, c.y, c.z}, hi1[3] = {d.x, d.y, d.z};
                    r0 = (int)f2u(a.w); r1 = (int)f2u(b.w);
                    const bool s0 = !rtbeam::slab_fails_ok(ro, lo0, hi0, I.L, I.H), s1 = !rtbeam::slab_fails_ok(ro, lo1, hi1, I.L, I.H);
                    leaf = (s0 && r0 < 0) || (s1 && r1 < 0);
                    in0 = s0 && r0 >= 0; in1 = s1 && r1 >= 0;
                }
                if (__ballot(leaf) != 0ull) { verdict = rtbeam::kAlive; break; }
                const unsigned long long m0 = __ballot(in0), m1 = __ballot(in1);
                const int p0 = __popcll(m0), total = p0 + __popcll(m1);
                if (total > rtbeam::kFrontier) { verdict = rtbeam::kOverflow; break; }
                // the next frontier: the surviving left children in lane order, then the right ones
                const bool fromLeft = lane < p0;
                const int src = lane < total ? nth_set_bit(fromLeft ? m0 : m1, fromLeft ? lane : lane - p0) : 0;
                const int fromL = __shfl(r0, src, 64), fromR = __shfl(r1, src, 64);
                node = fromLeft ? fromL : fromR;
                n = total;
            }
        }
    }
    if (lane == 0) {
        tileDead[lt] = verdict == rtbeam::kDead ? 1 : 0;
        if (stat) {
            atomicAdd(&stat[0], 1ull);
            if (verdict == rtbeam::kDead) atomicAdd(&stat[1], 1ull);
            if (verdict == rtbeam::kOverflow) atomicAdd(&stat[2], 1ull);
            if (levels) atomicAdd(&stat[3], (unsigned long long)levels);
        }
    }
}
// the primary stage's reading of those flags: local tile `tile` of the batch (< nLocalTiles * batch) lies in a dead spatial tile
RT_DEV bool tile_is_dead(const DevFrame *__restrict__ fr, int tile) {
    const uint8_t *dead = fr->tileDead;
    return dead && dead[tile - sub_frame_of_tile(fr->g, tile) * max(fr->g.nLocalTiles, 1)] != 0;
}

// ---- stage: primary ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_primary(const DevFrame *__restrict__ fr, Targets tg, WaveBuf wb) {   // workgroup = kAppendBatch tiles
    const RtUniforms &u = fr->u;
    RT_BATCH_APPEND(ap);
    for (int k = 0; k < kAppendBatch; ++k) {
        const int tile = blockIdx.x * kAppendBatch + k;
        int px, py;
        const bool live = tile < fr->g.nLocalTiles * max(fr->g.batch, 1) && pixel_of_slot(fr->g, tile, threadIdx.x, px, py);
        const int slot = tile * 256 + threadIdx.x;
        bool cand = false;
        if (live) {
            V3 dir = primaryDirK(fr, sub_frame_of_tile(fr->g, tile), px, py);
            if (tile_is_dead(fr, tile)) finish_miss(fr, wb, slot, px, py, dir);   // the beam cull: what k_post_primary would have called, with the same arguments
            else {
                V3 rdInv = mk3(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
                float tmin;
                cand = fr->sc.hasBVH && slab(ld3(u.camPos), rdInv, ld3(fr->sc.rootMin), ld3(fr->sc.rootMax), tmin) && !(tmin > u.inf);
                if (!cand) finish_miss(fr, wb, slot, px, py, dir);
            }
        }
        ap.note(k, cand);
    }
    ap.commit(&wb.counts[0]);
    for (int k = 0; k < kAppendBatch; ++k) {
        const uint32_t idx = ap.index(k);
        if (ap.mine(k)) { wb.cand[idx] = (uint32_t)((blockIdx.x * kAppendBatch + k) * 256 + threadIdx.x); wb.primTri[idx] = -1; }   // the miss answer: PrimarySrc stores hits only
    }
}
// k_primary's pixel body for local tile `tile`: the primary ray against the root box.  A pixel that misses it is finished here; the others are candidates.
// (k_primary keeps its own copy, so that a single frame runs the code it always ran.)
RT_DEV bool primary_pixel(const DevFrame *__restrict__ fr, const WaveBuf &wb, int tile) {
    const RtUniforms &u = fr->u;
    int px, py;
    const bool live = tile < fr->g.nLocalTiles * max(fr->g.batch, 1) && pixel_of_slot(fr->g, tile, threadIdx.x, px, py);
    const int slot = tile * 256 + threadIdx.x;
    bool cand = false;
    if (live) {
        V3 dir = primaryDirK(fr, sub_frame_of_tile(fr->g, tile), px, py);
        if (tile_is_dead(fr, tile)) { finish_miss(fr, wb, slot, px, py, dir); return false; }   // the beam cull, as in k_primary
        V3 rdInv = mk3(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
        float tmin;
        cand = fr->sc.hasBVH && slab(ld3(u.camPos), rdInv, ld3(fr->sc.rootMin), ld3(fr->sc.rootMax), tmin) && !(tmin > u.inf);
        if (!cand) finish_miss(fr, wb, slot, px, py, dir);
    }
    return cand;
}
// The same stage for a batch of frames (RT_BATCH_INTERLEAVE; a kernel of its own, so that k_primary keeps its code): the workgroup's kAppendBatch iterations walk
// the frames of a spatial tile before the next tile (batch_tile_of_virtual) and a wave appends pixel by pixel, each pixel's frames side by side
// (InterleavedAppend) -- the same candidates in the same slots, in another order of the list, and with it of every later list and queue: the frames of a pixel,
// nearly the same rays, share a wave.
__global__ __launch_bounds__(256) void k_primary_interleaved(const DevFrame *__restrict__ fr, Targets tg, WaveBuf wb) {
    const int batch = max(fr->g.batch, 1), nl = fr->g.nLocalTiles, total = nl * batch;
    RT_INTERLEAVED_APPEND(ap);
    for (int k = 0; k < kAppendBatch; ++k) {
        const int v = blockIdx.x * kAppendBatch + k;
        ap.note(k, primary_pixel(fr, wb, v < total ? batch_tile_of_virtual(v, batch, nl) : total));   // (total: no tile, nothing live)
    }
    ap.commit(&wb.counts[0]);
    for (int k = 0; k < kAppendBatch; ++k) {
        if (!ap.mine(k)) continue;
        const uint32_t idx = ap.index(k);
        wb.cand[idx] = (uint32_t)(batch_tile_of_virtual(blockIdx.x * kAppendBatch + k, batch, nl) * 256 + threadIdx.x);
        wb.primTri[idx] = -1;
    }
}

// ---- stage: post_primary -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_post_primary(const DevFrame *__restrict__ fr, Targets tg, WaveBuf wb) {   // workgroup = kAppendBatch x 256 candidates
    const uint32_t n = wb.counts[0];
    RT_BATCH_APPEND(ap);
    for (int k = 0; k < kAppendBatch; ++k) {
        const uint32_t i = (blockIdx.x * kAppendBatch + k) * 256 + threadIdx.x;
        bool hit = false;
        if (i < n) {
            hit = wb.primTri[i] >= 0;
            if (!hit) {
                const uint32_t slot = wb.cand[i];
                int px, py;
                slot_to_pixel(fr->g, slot, px, py);
                finish_miss(fr, wb, (int)slot, px, py, primaryDirK(fr, sub_frame_of_slot(fr->g, slot), px, py));
            }
        }
        ap.note(k, hit);
    }
    ap.commit(&wb.counts[1]);
    for (int k = 0; k < kAppendBatch; ++k) {
        const uint32_t idx = ap.index(k);
        if (ap.mine(k)) {
            const uint32_t i = (blockIdx.x * kAppendBatch + k) * 256 + threadIdx.x;
            HitRec h;
            h.slot = wb.cand[i]; h.t = wb.primT[i]; h.tri = wb.primTri[i];
            wb.hits[idx] = h;
        }
    }
}

// ---- tracer policies ---------------------------------------------------------------------------
RT_DEV float4 mkf4(V3 v, float w) { return make_float4(v.x, v.y, v.z, w); }
RT_DEV float below(float r) { return (r > 0.0f) ? u2f(f2u(r) - 1u) : -1.0f; }   // largest float < r (r > 0), else "no ray"

// rt_debug_disk_skip: five sums per generator kernel -- (hit, sample) pairs through directLightBVH, pairs with diskUnlit, pairs whose wave skipped the disk
// loop, waves, waves that skipped it.  One lane per wave adds; only when the entry has switched counting on (stat != null).
RT_DEV void disk_stat_add(unsigned long long *stat, bool unlit, bool skipped) {
    const unsigned long long act = __ballot(1), un = __ballot(unlit);
    if ((int)(threadIdx.x & 63) != __ffsll((long long)act) - 1) return;
    atomicAdd(&stat[0], (unsigned long long)__popcll(act));
    atomicAdd(&stat[1], (unsigned long long)__popcll(un));
    atomicAdd(&stat[3], 1ull);
    if (skipped) { atomicAdd(&stat[2], (unsigned long long)__popcll(act)); atomicAdd(&stat[4], 1ull); }
}

struct GenDirectTracer {   // records first-generation rays of (hit j, sample s)
    static constexpr bool kSkipUnlitDisk = true;
    static constexpr bool kFrameLd2 = true;   // load_hit fills Frag::ld2x / ld2y
    unsigned long long *stat;
    RT_DEV void disk_stat(int, bool unlit, bool skipped) { if (stat) disk_stat_add(stat, unlit, skipped); }
    WaveBuf wb;
    uint32_t j;
    int s;
    uint32_t shadowMask;
    bool giCast;
    RT_DEV bool shadow(int, int k, V3 ro, V3 rd, float tMax, bool matters) {
        shadowMask |= 1u << k;
        // sun (k = 4) and point-light (k = 5) rays start at hp + N*e / hp + L*e towards a fixed light: the same ray for every
        // sample of the pixel (rt_lighting.glsl:114-214 never look at the seed) -- sample 0 traces it, the others reuse its answer
        if (k >= 4 && s > 0) return false;
        uint32_t a = wb.sh1_slot(s, k) * wb.CH + j;
        const uint32_t al = wb.sh1_light(a);
        // dead ray (its answer is multiplied by zero): its liveness bit stays clear and nothing is stored; without masks its tMax word says so
        if (wb.shLive) live_set(wb.shLive, al, matters);
        else if (!matters) wb.shT[al] = -1.0f;
        if (!matters) return false;
        wb.shT[al] = fmaxr(tMax, 0.0f);
        wb.shO[al] = mkf4(ro, 0.0f);
        wb.shD[a] = mkf4(rd, 0.0f);
        wb.occ1[a] = 0;                  // "not occluded": the any-hit launch stores occlusions only
        return false;
    }
    V3 giRo, giRd;   // RT_BIN_GI: the bounce ray is kept here and written by the workgroup's sort (k_gen_direct)
    RT_DEV int gi(V3 ro, V3 rd, V3 &, V3 &) {
        giCast = true;
        if (wb.giPerm) { giRo = ro; giRd = rd; return -1; }
        uint32_t a = (uint32_t)s * wb.CH + j;
        wb.giD[a] = mkf4(rd, 1.0f);      // the origin is the hit's: giOrg[j], written by sample 0 (k_gen_direct)
        return -1;
    }
    RT_DEV bool ao(int i, V3 org, V3 dir, float radius) {
        uint32_t a = (uint32_t)i * wb.CH + j;
        if (i == 0) wb.aoOrg[j] = mkf4(org, 0.0f);   // one origin for the hit's AO rays (only sample 0's thread gets here)
        wb.shD[a] = mkf4(dir, below(radius));         // closest t < radius  <=>  any hit with t <= pred(radius)
        wb.occ1[a] = 0;
        return false;
    }
};
// gi() of the tracers behind the bounce launch: the recorded answer of the bounce ray of (hit j, sample s) -- 1, its hit point and normal -- or 0 for a miss
template <bool SMOOTH> RT_DEV int bounce_hit(const WaveBuf &wb, const DevScene *sc, const float4 *nrm, int s, uint32_t j, V3 ro, V3 rd, V3 &hp, V3 &hn) {
    uint32_t a = wb.gi_entry(s, j);
    int tri = wb.giTri[a];
    if (tri < 0) return 0;
    hp = ro + rd * wb.giT[a];
    hn = SMOOTH ? hitNormal(sc->tris, nrm, tri, ro, rd) : tri_normal(*sc, tri);
    return 1;
}
template <bool SMOOTH> struct GenGiTracer {       // reads the bounce result, records the shadow rays at the bounce hit
    static constexpr bool kSkipUnlitDisk = true;
    static constexpr bool kFrameLd2 = true;   // load_hit fills Frag::ld2x / ld2y
    unsigned long long *stat;
    RT_DEV void disk_stat(int, bool unlit, bool skipped) { if (stat) disk_stat_add(stat + 5, unlit, skipped); }
    WaveBuf wb;
    const DevScene *sc;
    const float4 *nrm;   // SMOOTH: DevFrame::nrmRows, the bounce hit's corner normals
    float inf;
    uint32_t j;
    int s;
    uint32_t pos;
    uint32_t shadowMask;
    RT_DEV bool shadow(int seg, int k, V3 ro, V3 rd, float tMax, bool matters) {
        if (seg != SEG_GI_DIRECT) return false;
        if (pos >= wb.q2Stride) return false;          // beyond the queue's capacity: k_gen_gi_overflow traces this pair's rays itself
        uint32_t a = (uint32_t)k * wb.q2Stride + pos;
        shadowMask |= 1u << k;
        if (wb.sh2Live) live_set(wb.sh2Live, a, matters);
        else if (!matters) wb.sh2T[a] = -1.0f;
        if (!matters) return false;
        wb.sh2T[a] = fmaxr(tMax, 0.0f);
        wb.sh2O[a] = mkf4(ro, 0.0f);
        wb.sh2D[a] = mkf4(rd, 0.0f);
        wb.occ2[a] = 0;
        return false;
    }
    RT_DEV int gi(V3 ro, V3 rd, V3 &hp, V3 &hn) { return bounce_hit<SMOOTH>(wb, sc, nrm, s, j, ro, rd, hp, hn); }
    RT_DEV bool ao(int, V3, V3, float) { return false; }
};
template <bool SMOOTH, bool COLOR> struct CombineTracer {     // reads everything
    static constexpr bool kSkipUnlitDisk = true;
    static constexpr bool kFrameLd2 = true;   // load_hit fills Frag::ld2x / ld2y
    RT_DEV void disk_stat(int, bool, bool) {}
    WaveBuf wb;
    const DevScene *sc;
    const float4 *nrm;   // SMOOTH: DevFrame::nrmRows, the bounce hit's corner normals
    const float4 *col;   // COLOR: DevFrame::colRows, the bounce hit's corner colours
    uint32_t j;
    int s;
    RT_DEV bool shadow(int seg, int k, V3, V3, float, bool matters) {
        if (!matters) return false;
        if (seg == SEG_DIRECT) return wb.occ1[wb.sh1_slot(k >= 4 ? 0 : s, k) * wb.CH + j] != 0;   // sun / point: sample 0's ray
        const uint32_t gp = (uint32_t)wb.giPos[(uint32_t)s * wb.CH + j];
        return (gp < wb.q2Stride ? wb.occ2[(uint32_t)k * wb.q2Stride + gp] : wb.occOvf[(uint32_t)k * (wb.CH * (uint32_t)wb.SPP) + gp]) != 0;
    }
    RT_DEV int gi(V3 ro, V3 rd, V3 &hp, V3 &hn) { return bounce_hit<SMOOTH>(wb, sc, nrm, s, j, ro, rd, hp, hn); }
    using BounceAlbedo = HeldAlbedo;
    RT_DEV int gi(V3 ro, V3 rd, V3 &hp, V3 &hn, const HeldAlbedo &, HeldAlbedo &albedo) {   // COLOR builds: the normal first, then the colour, one row at a time
        if (gi(ro, rd, hp, hn) == 0) return 0;
        albedo.c = hitColor(sc->tris, col, wb.giTri[wb.gi_entry(s, j)], ro, rd);
        return 1;
    }
    RT_DEV bool ao(int i, V3, V3, float radius) { return radius > 0.0f && wb.occ1[(uint32_t)i * wb.CH + j] != 0; }
};

// ... and with the albedo texture of DESIGN.md 14.15 (DevFrame::uvRows != null): the bounce hit's albedo is its colour times its texel; col may be null
template <bool SMOOTH> struct CombineTexTracer : CombineTracer<SMOOTH, true> {
    using Base = CombineTracer<SMOOTH, true>;
    using Base::gi;
    const float4 *uv;            // DevFrame::uvRows, the bounce hit's corner UVs
    const rtuv::Texture *tex;    // DevFrame::tex
    RT_DEV int gi(V3 ro, V3 rd, V3 &hp, V3 &hn, const HeldAlbedo &, HeldAlbedo &albedo) {   // the normal first, then the albedo, one row at a time
        if (Base::gi(ro, rd, hp, hn) == 0) return 0;
        albedo.c = hitAlbedoTex(this->sc->tris, this->col, uv, *tex, this->wb.giTri[this->wb.gi_entry(this->s, this->j)], ro, rd);
        return 1;
    }
};

struct HitCtx { Frag F; V3 dir, hp, hn; int px, py; uint32_t slot; };
template <bool SMOOTH> RT_DEV HitCtx load_hit(const DevFrame *fr, const HitRec &h) {
    HitCtx c;
    c.slot = h.slot;
    slot_to_pixel(fr->g, h.slot, c.px, c.py);
    c.F.u = &fr->u; c.F.sc = &fr->sc; c.F.fcx = (float)c.px + 0.5f; c.F.fcy = (float)c.py + 0.5f;
    const int k = sub_frame_of_slot(fr->g, h.slot);
    c.F.frameIndex = fr->u.frameIndex + k;
    c.F.ld2x = fr->ld2K[k][0]; c.F.ld2y = fr->ld2K[k][1];   // cpOffset's halton pair, once per sub-frame on the host
    c.dir = primaryDirK(fr, k, c.px, c.py);
    c.hp = ld3(fr->u.camPos) + c.dir * h.t;
    c.hn = SMOOTH ? hitNormal(fr->sc.tris, fr->nrmRows, h.tri, ld3(fr->u.camPos), c.dir) : tri_normal(fr->sc, h.tri);
    return c;
}

// ---- stage: gen_direct  (thread = (hit j, sample s), s-major so a wave shares s) -----------------
template <bool SMOOTH> RT_DEV void gen_direct_body(const DevFrame *__restrict__ fr, WaveBuf wb, uint32_t c0, unsigned long long *diskStat) {
    const RtUniforms &u = fr->u;
    const uint32_t live = chunk_live(wb, c0);
    const uint32_t tid = blockIdx.x * 256 + threadIdx.x;
    const bool mine = live != 0 && tid < live * (uint32_t)wb.SPP;
    if (!mine && (!wb.giPerm || live == 0 || blockIdx.x * 256u >= live * (uint32_t)wb.SPP)) return;   // (the sort below needs whole workgroups)
    int s = 0;
    uint32_t j = 0;
    if (mine) sample_and_hit(tid, live, wb.SPP, s, j);
    GenDirectTracer tr;
    tr.wb = wb; tr.j = j; tr.s = s; tr.shadowMask = 0; tr.giCast = false; tr.stat = diskStat;
    tr.giRo = mk3(0.0f); tr.giRd = mk3(0.0f);
    if (mine) {
        HitCtx c = load_hit<SMOOTH>(fr, wb.hits[c0 + j]);
        const int SPP = max(u.spp, 1);
        const int seed = (int)((uint32_t)c.F.frameIndex * (uint32_t)SPP + (uint32_t)s);
        (void)directLightBVH(tr, c.F, SEG_DIRECT, c.hp, c.hn, seed, -c.dir);
        if (s == 0 && !wb.shLive)         // (with liveness masks the bit of a slot that was not set is clear already)
            for (int k = 4; k < 6; ++k)   // sun / point rays are conditional (rt_lighting.glsl:123,194)
                if (!(tr.shadowMask & (1u << k))) wb.shT[wb.sh1_light(wb.sh1_slot(0, k) * wb.CH + j)] = -1.0f;
        Work w;
        if (u.enableGI == 1) (void)oneBounceGIBVH<GenDirectTracer, false>(tr, c.F, c.hp, c.hn, c.F.frameIndex, seed, w);
        if (u.enableGI == 1 && !wb.giPerm) {
            if (!tr.giCast) wb.giD[(uint32_t)s * wb.CH + j].w = -1.0f;
            // the bounce origin of the hit's samples, once: from sample 0 even when its own direction declines (cosTheta), another sample's may not
            if (s == 0) wb.giOrg[j] = mkf4(bounce_origin(c.hp, normalize(c.hn), u.eps), 0.0f);
        }
        if (s == 0 && wb.A > 0) (void)computeAO_BVH(tr, c.F, c.hp, c.hn, c.F.frameIndex);
    }
    if (wb.giPerm) {
        // EXPERIMENT (RT_BIN_GI=1): the workgroup's 256 bounce rays -- 256 consecutive hits of one sample, i.e. neighbouring
        // pixels -- are written sorted by direction (octant, then two bits of each |component|), so that quad-mates of the bounce launch start out
        // with like rays.  Results stay addressable through giPerm; nothing else changes, frames are bit-identical.
        __shared__ uint32_t sKey[256], sAddr[256];
        uint32_t key = 0xffffffffu;
        if (mine && tr.giCast) {
            const V3 d = tr.giRd;
            const uint32_t oct = (d.x < 0.0f ? 1u : 0u) | (d.y < 0.0f ? 2u : 0u) | (d.z < 0.0f ? 4u : 0u);
            auto q2 = [](float v) { return (uint32_t)min(3, (int)(__builtin_fabsf(v) * 4.0f)); };
            key = (oct << 6) | (q2(d.x) << 4) | (q2(d.y) << 2) | q2(d.z);
        }
        sKey[threadIdx.x] = key;
        sAddr[threadIdx.x] = mine ? (uint32_t)s * wb.CH + j : 0xffffffffu;
        __syncthreads();
        uint32_t rank = 0;
        for (uint32_t i = 0; i < 256u; ++i) { const uint32_t ki = sKey[i]; rank += (ki < key || (ki == key && i < threadIdx.x)) ? 1u : 0u; }
        // thread t's record goes to the address of the rank-th thread; threads outside the list (not mine) have the largest keys AND the largest
        // thread indices, so the first `mine` ranks map onto the `mine` addresses
        const uint32_t target = sAddr[rank];
        if (mine) {
            wb.giPerm[(uint32_t)s * wb.CH + j] = (int)target;
            if (tr.giCast) { wb.giOrg[target] = mkf4(tr.giRo, 0.0f); wb.giD[target] = mkf4(tr.giRd, 1.0f); }   // (one origin per record here: the sort moves records between hits)
            else wb.giD[target].w = -1.0f;
        }
    }
}
// the stage as it always was, and with the smooth normals of DESIGN.md 14.13 (DevFrame::nrmRows != null): a build of its own, so that the first keeps its code
__global__ __launch_bounds__(256) void k_gen_direct(const DevFrame *__restrict__ fr, WaveBuf wb, uint32_t c0, unsigned long long *diskStat) { gen_direct_body<false>(fr, wb, c0, diskStat); }
__global__ __launch_bounds__(256) void k_gen_direct_smooth(const DevFrame *__restrict__ fr, WaveBuf wb, uint32_t c0, unsigned long long *diskStat) { gen_direct_body<true>(fr, wb, c0, diskStat); }

// ---- stage: gen_gi -------------------------------------------------------------------------------
// rt_debug_gi_list: two sums over the bounce-hit generators -- (hit, sample) pairs visited, pairs shaded.  One lane per wave adds, once the entry switched counting on.
RT_DEV void gi_list_stat_add(unsigned long long *stat, bool visited, bool shaded) {
    const unsigned long long act = __ballot(1), vi = __ballot(visited), sh = __ballot(shaded);
    if ((int)(threadIdx.x & 63) != __ffsll((long long)act) - 1) return;
    if (vi) atomicAdd(&stat[0], (unsigned long long)__popcll(vi));
    if (sh) atomicAdd(&stat[1], (unsigned long long)__popcll(sh));
}
template <bool SMOOTH> RT_DEV void gen_gi_body(const DevFrame *__restrict__ fr, WaveBuf wb, uint32_t c0, uint32_t *giCount, unsigned long long *diskStat, unsigned long long *listStat) {
    const RtUniforms &u = fr->u;
    const uint32_t live = chunk_live(wb, c0);
    const uint32_t tid = blockIdx.x * 256 + threadIdx.x;
    const bool mine = live != 0 && tid < live * (uint32_t)wb.SPP;
    int s = 0;
    uint32_t j = 0;
    if (mine) sample_and_hit(tid, live, wb.SPP, s, j);
    const uint32_t a = (uint32_t)s * wb.CH + j;
    const uint32_t ae = mine ? wb.gi_entry(s, j) : 0u;   // where this (hit, sample)'s bounce ray and its answer are
    const bool bounced = mine && wb.giD[ae].w >= 0.0f && wb.giTri[ae] >= 0;
    const uint32_t pos = block_append(bounced, giCount);   // compact the (hit, sample) pairs that need second-generation rays
    if (listStat) gi_list_stat_add(listStat, mine, bounced);
    if (!mine) return;
    wb.giPos[a] = bounced ? (int)pos : -1;
    if (!bounced) return;
    GenGiTracer<SMOOTH> tr;
    tr.wb = wb; tr.sc = &fr->sc; tr.nrm = SMOOTH ? fr->nrmRows : nullptr; tr.inf = u.inf; tr.j = j; tr.s = s; tr.pos = pos; tr.shadowMask = 0; tr.stat = diskStat;
    HitCtx c = load_hit<SMOOTH>(fr, wb.hits[c0 + j]);
    const int SPP = max(u.spp, 1);
    const int seed = (int)((uint32_t)c.F.frameIndex * (uint32_t)SPP + (uint32_t)s);
    Work w;
    (void)oneBounceGIBVH<GenGiTracer<SMOOTH>, false>(tr, c.F, c.hp, c.hn, c.F.frameIndex, seed, w);
    if (pos < wb.q2Stride && !wb.sh2Live)   // (with liveness masks the bit of a slot that was not set is clear already)
        for (int k = 0; k < 6; ++k)
            if (!(tr.shadowMask & (1u << k))) wb.sh2T[(uint32_t)k * wb.q2Stride + pos] = -1.0f;
}
// the stage as it always was, and with the smooth normals of DESIGN.md 14.13 (DevFrame::nrmRows != null): a build of its own, so that the first keeps its code
__global__ __launch_bounds__(256) void k_gen_gi(const DevFrame *__restrict__ fr, WaveBuf wb, uint32_t c0, uint32_t *giCount, unsigned long long *diskStat, unsigned long long *listStat) { gen_gi_body<false>(fr, wb, c0, giCount, diskStat, listStat); }
__global__ __launch_bounds__(256) void k_gen_gi_smooth(const DevFrame *__restrict__ fr, WaveBuf wb, uint32_t c0, uint32_t *giCount, unsigned long long *diskStat, unsigned long long *listStat) { gen_gi_body<true>(fr, wb, c0, giCount, diskStat, listStat); }

// The same stage behind a bounce probe (RT_BOUNCE_PROBE, giPerm == null): the probe left the queue addresses of the bounce rays that hit in a dense list
// (BounceProbeSrc::hitters, re-traced closest-hit since), so only those are visited -- on the bench view 54 419 of 29.6 M (hit, sample) pairs per launch set --
// instead of every pair.  A fixed grid strides over the list, whose length only the device knows.  giPos is written for the pairs that bounced and for no other:
// CombineTracer reads it behind gi() == 1 alone, k_gen_gi_overflow walks the same list.  Queue 2 positions are dealt in list order instead of pair order; an
// entry's position is only ever reached through giPos, so frames do not change.
template <bool SMOOTH> RT_DEV void gen_gi_listed_body(const DevFrame *__restrict__ fr, WaveBuf wb, uint32_t c0, const uint32_t *hitList, const uint32_t *hitCount, uint32_t *giCount, unsigned long long *diskStat, unsigned long long *listStat) {
    const RtUniforms &u = fr->u;
    const uint32_t n = min(*hitCount, wb.CH * (uint32_t)wb.SPP);
    for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {   // whole workgroups: block_append
        const uint32_t i = base + threadIdx.x;
        const bool mine = i < n;
        const uint32_t a = mine ? hitList[i] : 0u;
        const bool bounced = mine && wb.giTri[a] >= 0;
        const uint32_t pos = block_append(bounced, giCount);
        if (listStat) gi_list_stat_add(listStat, mine, bounced);
        if (!bounced) continue;
        const int s = (int)(a / wb.CH);
        const uint32_t j = a % wb.CH;
        wb.giPos[a] = (int)pos;
        GenGiTracer<SMOOTH> tr;
        tr.wb = wb; tr.sc = &fr->sc; tr.nrm = SMOOTH ? fr->nrmRows : nullptr; tr.inf = u.inf; tr.j = j; tr.s = s; tr.pos = pos; tr.shadowMask = 0; tr.stat = diskStat;
        HitCtx c = load_hit<SMOOTH>(fr, wb.hits[c0 + j]);
        const int SPP = max(u.spp, 1);
        const int seed = (int)((uint32_t)c.F.frameIndex * (uint32_t)SPP + (uint32_t)s);
        Work w;
        (void)oneBounceGIBVH<GenGiTracer<SMOOTH>, false>(tr, c.F, c.hp, c.hn, c.F.frameIndex, seed, w);
        if (pos < wb.q2Stride && !wb.sh2Live)
            for (int k = 0; k < 6; ++k)
                if (!(tr.shadowMask & (1u << k))) wb.sh2T[(uint32_t)k * wb.q2Stride + pos] = -1.0f;
    }
}
// the stage as it always was, and with the smooth normals of DESIGN.md 14.13 (DevFrame::nrmRows != null): a build of its own, so that the first keeps its code
__global__ __launch_bounds__(256) void k_gen_gi_listed(const DevFrame *__restrict__ fr, WaveBuf wb, uint32_t c0, const uint32_t *hitList, const uint32_t *hitCount, uint32_t *giCount, unsigned long long *diskStat, unsigned long long *listStat) { gen_gi_listed_body<false>(fr, wb, c0, hitList, hitCount, giCount, diskStat, listStat); }
__global__ __launch_bounds__(256) void k_gen_gi_listed_smooth(const DevFrame *__restrict__ fr, WaveBuf wb, uint32_t c0, const uint32_t *hitList, const uint32_t *hitCount, uint32_t *giCount, unsigned long long *diskStat, unsigned long long *listStat) { gen_gi_listed_body<true>(fr, wb, c0, hitList, hitCount, giCount, diskStat, listStat); }

// Shadow queue 2 of a large launch set holds a PREDICTED number of bounce hits (rt_wave_render).  The (hit, sample) pairs beyond it -- none, unless the view changed so
// that more than twice as many bounce rays hit as in any batch before -- get their six shadow rays traced right here, one thread per pair, with the megakernel's any-hit
// walk (bvh_anyhit: the same answers as the any-hit launch, tests/test_gpu_parity.py), into occOvf.  Launched behind every k_gen_gi of such a set; returns at once when
// nothing overflowed.  Behind k_gen_gi_listed it walks the probe's hit list (hitList != null) as that kernel did: giPos of a pair outside the list is not written
// there and may hold an earlier launch set's value.
template <bool SMOOTH> struct GenGiOverflowTracer {
    static constexpr bool kSkipUnlitDisk = true;
    static constexpr bool kFrameLd2 = true;   // load_hit fills Frag::ld2x / ld2y
    RT_DEV void disk_stat(int, bool, bool) {}
    WaveBuf wb;
    const DevScene *sc;
    const float4 *nrm;   // SMOOTH: DevFrame::nrmRows, the bounce hit's corner normals
    float eps;
    StackEntry *stk;
    uint32_t j;
    int s;
    uint32_t pos;
    RT_DEV bool shadow(int seg, int k, V3 ro, V3 rd, float tMax, bool matters) {
        if (seg != SEG_GI_DIRECT) return false;
        bool occ = false;
        if (matters) { Work w; occ = bvh_anyhit<false>(*sc, ro, rd, eps, fmaxr(tMax, 0.0f), stk, w); }
        wb.occOvf[(uint32_t)k * (wb.CH * (uint32_t)wb.SPP) + pos] = occ ? 1 : 0;
        return false;
    }
    RT_DEV int gi(V3 ro, V3 rd, V3 &hp, V3 &hn) { return bounce_hit<SMOOTH>(wb, sc, nrm, s, j, ro, rd, hp, hn); }
    RT_DEV bool ao(int, V3, V3, float) { return false; }
};
template <bool SMOOTH> RT_DEV void gen_gi_overflow_body(const DevFrame *__restrict__ fr, WaveBuf wb, uint32_t c0, const uint32_t *giCount, int stackEntries, const uint32_t *hitList, const uint32_t *hitCount) {
    if (*giCount <= wb.q2Stride) return;      // the normal case: a small fixed grid that leaves at once (a grid of one thread per pair -- 29 000 workgroups for a batch of eight
                                              // 1080p frames -- cost 2 % of a frame just to be dispatched and return)
    const uint32_t live = chunk_live(wb, c0);
    if (live == 0) return;
    const uint32_t n = hitList ? min(*hitCount, wb.CH * (uint32_t)wb.SPP) : live * (uint32_t)wb.SPP;
    for (uint32_t tid = blockIdx.x * 256 + threadIdx.x; tid < n; tid += gridDim.x * 256) {
        int s = (int)(tid / live);
        uint32_t j = tid % live;
        if (hitList) {
            const uint32_t a = hitList[tid];
            if (wb.giTri[a] < 0) continue;    // listed, but k_gen_gi_listed did not shade it: no giPos
            s = (int)(a / wb.CH); j = a % wb.CH;
        }
        const int gp = wb.giPos[(uint32_t)s * wb.CH + j];
        if (gp < 0 || (uint32_t)gp < wb.q2Stride) continue;
        GenGiOverflowTracer<SMOOTH> tr;
        tr.wb = wb; tr.sc = &fr->sc; tr.nrm = SMOOTH ? fr->nrmRows : nullptr; tr.eps = fr->u.eps; tr.j = j; tr.s = s; tr.pos = (uint32_t)gp;
        tr.stk = reinterpret_cast<StackEntry *>(rt_dyn_lds) + (threadIdx.x >> 6) * stackEntries * 64 + (threadIdx.x & 63);
        HitCtx c = load_hit<SMOOTH>(fr, wb.hits[c0 + j]);
        const int SPP = max(fr->u.spp, 1);
        const int seed = (int)((uint32_t)c.F.frameIndex * (uint32_t)SPP + (uint32_t)s);
        Work w;
        (void)oneBounceGIBVH<GenGiOverflowTracer<SMOOTH>, false>(tr, c.F, c.hp, c.hn, c.F.frameIndex, seed, w);
    }
}
// the stage as it always was, and with the smooth normals of DESIGN.md 14.13 (DevFrame::nrmRows != null): a build of its own, so that the first keeps its code
__global__ __launch_bounds__(256) void k_gen_gi_overflow(const DevFrame *__restrict__ fr, WaveBuf wb, uint32_t c0, const uint32_t *giCount, int stackEntries, const uint32_t *hitList, const uint32_t *hitCount) { gen_gi_overflow_body<false>(fr, wb, c0, giCount, stackEntries, hitList, hitCount); }
__global__ __launch_bounds__(256) void k_gen_gi_overflow_smooth(const DevFrame *__restrict__ fr, WaveBuf wb, uint32_t c0, const uint32_t *giCount, int stackEntries, const uint32_t *hitList, const uint32_t *hitCount) { gen_gi_overflow_body<true>(fr, wb, c0, giCount, stackEntries, hitList, hitCount); }

// ---- stage: combine (thread = hit) ---------------------------------------------------------------
template <bool SMOOTH, bool COLOR, bool TEX = false> RT_DEV void combine_body(const DevFrame *__restrict__ fr, Targets tg, WaveBuf wb, uint32_t c0) {
    const RtUniforms &u = fr->u;
    const uint32_t live = chunk_live(wb, c0);
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= live) return;
    HitCtx c = load_hit<SMOOTH>(fr, wb.hits[c0 + j]);
    const int SPP = max(u.spp, 1);
    using Tracer = typename std::conditional<TEX, CombineTexTracer<SMOOTH>, CombineTracer<SMOOTH, COLOR>>::type;
    Tracer tr;
    tr.wb = wb; tr.sc = &fr->sc; tr.nrm = SMOOTH ? fr->nrmRows : nullptr; tr.col = COLOR ? fr->colRows : nullptr; tr.j = j; tr.s = 0;
    if constexpr (TEX) { tr.uv = fr->uvRows; tr.tex = &fr->tex; }
    Work w;
    V2 prevNDC = ndcFromWorld(prevHitPoint(fr->sc.tris, fr->prevTris, wb.hits[c0 + j].tri, ld3(u.camPos), c.dir, c.hp), u.prevViewProj), currNDC = ndcFromWorld(c.hp, u.currViewProj);
    V2 motionOut = mk2(currNDC.x - prevNDC.x, currNDC.y - prevNDC.y);
    V3 nn = SMOOTH ? c.hn : normalize(c.hn);   // the smooth normal is rt_hit_normals' to the bit: GNRM is f16 of it, not of a second normalisation
    float ao = 1.0f;
    if (u.enableAO == 1) ao = computeAO_BVH(tr, c.F, c.hp, c.hn, c.F.frameIndex);
    V3 frameSum = mk3(0.0f);
    if constexpr (COLOR) {   // per-vertex colours: the primary hit's colour once per hit, in front of the sample loop
        HeldAlbedo albedo;
        if constexpr (TEX) albedo.c = hitAlbedoTex(fr->sc.tris, fr->colRows, fr->uvRows, fr->tex, wb.hits[c0 + j].tri, ld3(u.camPos), c.dir);
        else albedo.c = hitColor(fr->sc.tris, fr->colRows, wb.hits[c0 + j].tri, ld3(u.camPos), c.dir);
        for (int s = 0; s < SPP; ++s) {
            tr.s = s;
            int seed = (int)((uint32_t)c.F.frameIndex * (uint32_t)SPP + (uint32_t)s);
            frameSum = frameSum + shadeSampleBVH<Tracer, false, true>(tr, c.F, c.hp, c.hn, -c.dir, seed, ao, w, &albedo);
        }
    } else {
        for (int s = 0; s < SPP; ++s) {
            tr.s = s;
            int seed = (int)((uint32_t)c.F.frameIndex * (uint32_t)SPP + (uint32_t)s);
            frameSum = frameSum + shadeSampleBVH<Tracer, false>(tr, c.F, c.hp, c.hn, -c.dir, seed, ao, w);
        }
    }
    finish_pixel(fr, wb, (int)c.slot, frameSum, motionOut, mk4(c.hp.x, c.hp.y, c.hp.z, 1.0f), mk4(nn.x, nn.y, nn.z, 0.0f));
}
// the stage as it always was, and with the smooth normals of DESIGN.md 14.13 (DevFrame::nrmRows != null): a build of its own, so that the first keeps its code
__global__ __launch_bounds__(256) void k_combine(const DevFrame *__restrict__ fr, Targets tg, WaveBuf wb, uint32_t c0) { combine_body<false, false>(fr, tg, wb, c0); }
__global__ __launch_bounds__(256) void k_combine_smooth(const DevFrame *__restrict__ fr, Targets tg, WaveBuf wb, uint32_t c0) { combine_body<true, false>(fr, tg, wb, c0); }
// ... and with the per-vertex colours of DESIGN.md 14.14 (DevFrame::colRows != null): the only stage that evaluates the shading, so the only one built again
__global__ __launch_bounds__(256) void k_combine_color(const DevFrame *__restrict__ fr, Targets tg, WaveBuf wb, uint32_t c0) { combine_body<false, true>(fr, tg, wb, c0); }
__global__ __launch_bounds__(256) void k_combine_smooth_color(const DevFrame *__restrict__ fr, Targets tg, WaveBuf wb, uint32_t c0) { combine_body<true, true>(fr, tg, wb, c0); }
// ... and with the albedo texture of DESIGN.md 14.15 (DevFrame::uvRows != null): two builds, the colours behind a run-time test of DevFrame::colRows
__global__ __launch_bounds__(256) void k_combine_tex(const DevFrame *__restrict__ fr, Targets tg, WaveBuf wb, uint32_t c0) { combine_body<false, true, true>(fr, tg, wb, c0); }
__global__ __launch_bounds__(256) void k_combine_smooth_tex(const DevFrame *__restrict__ fr, Targets tg, WaveBuf wb, uint32_t c0) { combine_body<true, true, true>(fr, tg, wb, c0); }

__global__ void k_accum_tally(const uint32_t *counts, unsigned long long *acc, int frames) {
    // acc: [0] candidates [1] hits [2] primary rays traced [3] shadow [4] bounce [5] bounce-shadow (the traversal kernels add to
    // [2..5] themselves) [6] frames
    int i = threadIdx.x;
    if (i < 2) acc[i] += counts[i];
    if (i == 6) acc[6] += (unsigned long long)frames;
}
}  // namespace
