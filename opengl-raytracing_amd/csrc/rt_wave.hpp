// rt_wave.hpp -- interface between rt_api.hip and the wavefront pipeline (rt_wave.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "rt_frame.hpp"

struct RtContext;
struct RtWave;
struct RtHybrid;

// Ray-queue arenas of a context, shared by its frame lanes (round 4): lane l uses arena l % n and waits for the arena's previous user (another
// lane's batch, from its first shading launch to its last) through an event.  n == number of lanes: every lane its own arena, as in rounds 1-3.
struct RtArenaPool;
RtArenaPool *rt_arena_pool_create(int arenas);
void rt_arena_pool_destroy(RtArenaPool *p);
size_t rt_arena_pool_bytes(const RtArenaPool *p);
int rt_arena_pool_count(const RtArenaPool *p);
size_t rt_wave_frame_bytes(const RtWave *w);   // per-lane frame arrays (candidates, hits, pre-resolve stash)
size_t rt_hybrid_arena_bytes(const RtHybrid *h);

RtWave *rt_wave_create(int computeUnits, RtArenaPool *pool, int lane);   // pool: the context's ray arenas; the lane reads its options (rtl::wave_options_from_env) here, once
void rt_wave_destroy(RtWave *w);
const char *rt_wave_error(const RtWave *w);
// Renders one frame of a BVH scene into `tg` on `stream`.  `host` is the host copy of *dFrame.  Only the final temporal
// resolve waits for `evPrevDone` (the previous frame's completion event, may be null).  cacheResident: the BVH arrays fit the 32 MB of L2
// (sizes the persistent grids, see rt_wave_render).
int rt_wave_render(RtWave *w, RtContext *ctx, hipStream_t stream, const rtd::DevFrame *dFrame, const rtd::DevFrame &host,
                   rtd::Targets tg, unsigned long long *counters, bool count, int treeDepth, hipEvent_t evPrevDone, bool cacheResident);

// tallies accumulated since the last reset, 16 words: [0] candidate pixels [1] hit pixels [2] primary [3] shadow+AO
// [4] bounce [5] bounce-shadow rays actually traversed, [6] frames, [8..10] 16-byte gather loads issued by the primary /
// any-hit / bounce traversal launches, [11..13] the same after merging the lanes of a wave that read the same record (only
// counted by the diagnostic kernels, RT_TRACE_STATS=1; 0 otherwise)
int rt_wave_traced(RtWave *w, hipStream_t stream, unsigned long long *out16, bool reset);
// RT_BOUNCE_PROBE since the last reset, 4 words: [0] bounce rays walked any-hit first [1] of them re-traced closest-hit (the probe found a triangle)
// [2] bounce launches (chunks) with the probe [3] without it
int rt_wave_bounce_probe(RtWave *w, hipStream_t stream, unsigned long long *out4, bool reset);
// The disk-light skip of the shading stages since the last reset, 10 words: for k_gen_direct [0] (hit, sample) pairs shaded [1] pairs with diskUnlit
// [2] pairs whose wave skipped the disk loop [3] waves [4] waves that skipped; [5..9] the same for k_gen_gi.  The generators count from the first call on.
int rt_wave_disk_skip(RtWave *w, hipStream_t stream, unsigned long long *out10, bool reset);
// The bounce-hit generator (k_gen_gi / k_gen_gi_listed) since the last reset, 4 words: [0] (hit, sample) pairs it visited [1] pairs it shaded (their bounce ray hit)
// [2] launches over the bounce probe's hit list [3] launches over every pair.  [0] and [1] count from the first call on.
int rt_wave_gi_list(RtWave *w, hipStream_t stream, unsigned long long *out4, bool reset);
// The light-slot liveness masks since the last reset, 6 words: [0] bits the generators set for shadow queue 1 [1] for queue 2 [2] mask words the
// any-hit launches scanned [3] their masked refill passes [4] [5] mask words of the lane's last chunk, queue 1 / queue 2 (0: RT_LIGHT_MASKS=0).  [0] - [3] count
// from the first call on.
int rt_wave_light_masks(RtWave *w, hipStream_t stream, unsigned long long *out6, bool reset);
// The beam cull (RT_BEAM_CULL).  rt_wave_beam_flags: called by rt_render_frame(s) BEFORE the frame descriptor `host` goes to the device -- the
// lane's flags for this launch set (DevFrame::tileDead; k_beam_cull fills them in front of the primary stage), or null when the set is not culled.
// rt_wave_beam_cull: since the last reset, 4 words: [0] tiles walked [1] dead tiles [2] tiles kept because a level of the walk overflowed [3] levels walked;
// counted from the first call on.  rt_wave_beam_read: the n flags of the lane's last culled launch set (RT_ERR_STATE: none, or not n tiles).
const uint8_t *rt_wave_beam_flags(RtWave *w, hipStream_t stream, const rtd::DevFrame &host, int treeDepth, bool cacheResident);
int rt_wave_beam_cull(RtWave *w, hipStream_t stream, unsigned long long *out4, bool reset);
int rt_wave_beam_read(RtWave *w, hipStream_t stream, uint8_t *out, size_t n);
// The share of bounce hits of earlier launch sets (what shadow queue 2 is sized from and the bounce probe is chosen by) belongs to a scene and a frame size:
// rt_upload_bvh and rt_resize forget it (an spp change does so in rt_wave_render)
void rt_wave_forget_share(RtWave *w);
// rt_upload_bvh: whether the any-hit tree is the collapse of the binary tree -- the bounce probe's exactness needs it (false: RT_ANYHIT_TREE=sah)
void rt_wave_set_probe_tree(RtWave *w, bool collapsed);

// Closest-hit traversal of the rays listed in idx[0 .. *count) (queue addresses into o / d) with the persistent kernel of the wavefront
// pipeline; results to outT / outTri at the same address.  heads: rt_wave_head_words() zeroed uint32 cursor words.
// -> the RT_BUILD_* bits of the build launched, as every trace entry below; 0: the library holds no kernel for the chosen build and nothing was launched.
uint32_t rt_wave_trace_closest_indexed(hipStream_t st, int cus, int treeDepth, const rtd::DevFrame *dFrame, const rtd::DevScene &hostScene, const uint32_t *idx,
                                       const uint32_t *count, const float4 *o, const float4 *d, float *outT, int *outTri, uint32_t *heads);
// The same over a dense array of records o[r] / d[r], r < min(*count, cap); the answer of record r goes to outT / outTri at dst[r].
// Nothing is traced when *flags has bit 2 or 4 set (rt_hybrid.hip: a pass that outgrew its arrays left the queue incomplete).
uint32_t rt_wave_trace_closest_compact(hipStream_t st, int cus, int treeDepth, const rtd::DevFrame *dFrame, const rtd::DevScene &hostScene, const float4 *o, const float4 *d,
                                   const uint32_t *dst, const uint32_t *count, const uint32_t *flags, uint32_t cap, float *outT, int *outTri, uint32_t *heads,
                                   uint32_t capOut = 0);   // capOut != 0 (RT_HYBRID_CHECK): entries of outT / outTri, checked before every store
// rt_debug_trace kinds 2 - 4 (diagnostics): rays through the production traversal kernels with the build the environment selects; the RT_BUILD_* bits of
// the build launched are returned.
uint32_t rt_wave_debug_trace(hipStream_t st, int cus, int treeDepth, const rtd::DevFrame *dFrame, const rtd::DevScene &hostScene, bool any, const float4 *o, const float4 *d,
                             const float *tm, const uint32_t *liveCount, uint32_t n, float *outT, int *outTri, uint8_t *outOcc, uint32_t *heads);
uint32_t rt_wave_debug_packets(hipStream_t st, int cus, int treeDepth, const rtd::DevFrame *dFrame, const rtd::DevScene &hostScene, const float4 *o, const float4 *d,
                               const float *tm, const uint32_t *liveCount, uint32_t nPackets, uint8_t *outOcc, uint32_t *heads);
// rt_trace_rays: n user rays (strides in floats) through the production traversal launch; dFrame / heads are the context's query scratch, written on
// `st` first.  Closest-hit answers to hits (RtHit) and normals (may be null), any-hit answers to occ.  Returns the RT_BUILD_* bits of the build.
uint32_t rt_wave_trace_query(hipStream_t st, int cus, int treeDepth, rtd::DevFrame *dFrame, const rtd::DevScene &hostScene, bool any, const float *o, int os,
                             const float *d, int ds, const float *tm, float eps, float inf, uint32_t n, void *hits, float *normals, uint8_t *occ, uint32_t *heads);
// rt_trace_scene_rays / rt_pick_pixels: the rays and outputs of one scene query.  Ray i is o[i * os] / d[i * ds] (strides in floats), or --
// when xy is set -- the primary ray of pixel (xy[2i], xy[2i + 1]) of the uniform block in the query's frame descriptor.  Outputs other than hits / occ
// may be null.  hits: one RtHit (float4) per ray for closest hit, null for any hit.
struct SceneRays {
    const float *o, *d;
    int os, ds;
    const int32_t *xy;
    const float *tm;
    uint32_t n;
    float4 *hits;
    int32_t *objects;
    float *normals, *points;
    uint8_t *occ;
};
// rt_scene_query.hip: the analytic leg, one lane per ray -- traceAnalyticCore (analytic and hybrid modes; BVH mode: every answer a miss), bounded by tm, into
// the caller's outputs -- and the query scratch (dFrame = u and the scene, heads zeroed) for the mesh leg that follows on `st`.  flags: RT_QUERY_SKIP_*.
void rt_scene_query_analytic(hipStream_t st, const RtUniforms &u, const rtd::DevScene &sc, int flags, const SceneRays &r, rtd::DevFrame *dFrame, uint32_t *heads);
// rt_wave.hip: the mesh leg through the production traversal launch (SceneSrc).  hybrid: merged into the analytic answers the outputs hold (mesh wins at a
// strictly smaller t; any hit: rays already occluded are not walked); else BVH mode, the bytes of rt_wave_trace_query plus objects / points.  dFrame and heads
// were written by rt_scene_query_analytic.  Returns the RT_BUILD_* bits of the build.
uint32_t rt_wave_trace_scene(hipStream_t st, int cus, int treeDepth, const rtd::DevFrame *dFrame, const rtd::DevScene &hostScene, bool hybrid, const SceneRays &r,
                             float inf, uint32_t *heads);
// RT_BUILD_* bits (include/rt_mi355.h) of the traversal builds this lane's frames launched since the last reset
uint32_t rt_wave_builds(RtWave *w, bool reset);
size_t rt_wave_head_words();

// rt_hybrid.hip -- EXTENSION: the hybrid scene (analytic objects + mesh, N diffuse bounces) in stages: shading passes that replay answered mesh
// queries and queue the open ones, persistent traversal launches in between.  Bit-identical to the megakernel's hybrid frames.
struct RtHybrid;
RtHybrid *rt_hybrid_create(int computeUnits);
void rt_hybrid_destroy(RtHybrid *h);
const char *rt_hybrid_error(const RtHybrid *h);
int rt_hybrid_render(RtHybrid *h, RtContext *ctx, hipStream_t stream, const rtd::DevFrame *dFrame, const rtd::DevFrame &host, rtd::Targets tg, int treeDepth,
                     hipEvent_t evPrevDone);

// stage timing hooks (rt_api.hip); stage ids index rt_stage_name()
void rt_stage_begin(RtContext *c, int stage, hipStream_t on = nullptr);   // on == nullptr: the context's stream
void rt_stage_end(RtContext *c, int stage, int launches, hipStream_t on = nullptr);

// rt_raster.hip -- the raster preview (renderRaster): mesh slots, the binned rasteriser, its outputs and tallies.  Errors: rt_raster_error.
struct RtRaster;
RtRaster *rt_raster_create();
void rt_raster_destroy(RtRaster *r);
const char *rt_raster_error(const RtRaster *r);
void rt_raster_force_bin_capacity(RtRaster *r, size_t pairs);   // 0: automatic
int rt_raster_set_mesh(RtRaster *r, int slot, const float *positions, int nVerts, const uint32_t *indices, int nIdx);
// Slots bound to the context's dynamic mesh.  What a raster call needs of the mesh, resolved by rt_api.hip at every call: the device
// arrays where they lie and, for the first half of the event scheme of DESIGN.md 14.4, the context's other lanes with one event each: the call
// records it on the lane and waits for it before its setup launches.  Used only by a call that names a bound slot.  The second half is
// rt_raster_order_after: a stream that is about to carry writes to the mesh waits for the event behind a raster call that read it on another stream.
struct RtRasterDynamic {
    const float *pos; const uint32_t *idx; const uint16_t *partOf; const float *partM;   // positions, index triples, [triangle] -> part, [part] -> 16 floats
    int nTris, nParts;
    int nOthers; hipStream_t others[8]; hipEvent_t evOther[8];
};
int rt_raster_bind_dynamic(RtRaster *r, int slot, int mode);
int rt_raster_order_after(RtRaster *r, hipStream_t s);
int rt_raster_set_part_colors(RtRaster *r, int slot, const float *rgb, int nParts);
// dyn: null when the context has no dynamic mesh (a draw naming a bound slot is then RT_ERR_STATE)
int rt_raster_render(RtRaster *r, hipStream_t stream, int W, int H, const RtRasterDraw *draws, int nDraws, const float *view16, const float *proj16,
                     const RtRasterDynamic *dyn);
// the device buffers of the last raster frame; RT_ERR_STATE as rt_raster_read
int rt_raster_buffers(RtRaster *r, int W, int H, void **rgba8, void **primId, void **depth24, size_t *bytesEach);
// W x H: the context's framebuffer; RT_ERR_STATE when the last raster frame has another size
int rt_raster_read(RtRaster *r, int W, int H, uint8_t *rgba8, uint32_t *primId, uint32_t *depth24);
int rt_raster_stats(RtRaster *r, RtRasterStats *out);
