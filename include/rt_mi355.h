/* include/rt_mi355.h -- C ABI of librt_mi355.so, the MI355X (gfx950) drop-in for the reference's
 * ray-trace pass.
 *
 * The reference (Darky-The-Dragon/OpenGL-RayTracing) has no plugin/FFI seam; the narrowest one is
 *     void renderRay(AppState&, int fbw, int fbh, bool cameraMoved,
 *                    const glm::mat4& currView, const glm::mat4& currProj);     include/render/render.h:19
 * whose real contract is "set ~75 uniforms, bind 4 resources, draw one full-screen triangle"
 * (src/render/render.cpp:55-194).  Each entry point below names the reference interface it replaces.
 * INTEGRATION.md shows the call-site a maintainer would change.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function returns RT_OK (0) or a
 * negative RtStatus and never throws; the caller owns all host pointers and the library copies
 * during the call; one context is driven from one thread at a time; the library owns device
 * memory and its HIP stream.  Matrices are column-major float[16] (glm / glUniformMatrix4fv with
 * transpose = GL_FALSE, src/render/Shader.cpp:190-192).  Images are row-major with ROW 0 = BOTTOM
 * row (GL window origin, what glReadPixels returns).
 */
#ifndef RT_MI355_H
#define RT_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum RtStatus {
    RT_OK = 0,
    RT_ERR_INVALID = -1,      /* bad argument */
    RT_ERR_NO_DEVICE = -2,    /* no HIP device / HIP runtime unusable: the product path never falls back to a CPU */
    RT_ERR_HIP = -3,          /* a HIP call failed; rt_last_error() has the text */
    RT_ERR_STATE = -4,        /* call order (e.g. render before resize) */
    RT_ERR_UNSUPPORTED = -5,  /* valid request this build cannot serve (stated in the message) */
    RT_ERR_IO = -6            /* file could not be read / parsed */
} RtStatus;

/* The uniform block of the ray-trace program: shaders/rt/rt_uniforms.glsl:25-177, same order.
 * All members are 4 bytes wide, so the struct has no padding. */
typedef struct RtUniforms {
    float eps, pi, inf;                                   /* uEPS uPI uINF  (RenderParams.h:229-231) */
    float camPos[3], camRight[3], camUp[3], camFwd[3];
    float tanHalfFov, aspect;
    int32_t frameIndex;                                   /* set by the library from its accumulation state */
    int32_t spp;
    float resolution[2];
    float jitter[2];
    int32_t enableJitter;
    int32_t useBVH, nodeCount, triCount;
    int32_t showMotion;
    float prevViewProj[16], currViewProj[16];
    int32_t cameraMoved;
    float taaStillThresh, taaHardMovingThresh;
    float taaHistoryMinWeight, taaHistoryAvgWeight, taaHistoryMaxWeight, taaHistoryBoxSize;
    int32_t enableTAA;
    float giScaleAnalytic, giScaleBVH;
    int32_t enableGI, enableAO, aoSamples;
    float aoRadius, aoBias, aoMin;
    int32_t useEnvMap;
    float envIntensity;
    int32_t sunEnabled;
    float sunColor[3], sunIntensity, sunDir[3];
    int32_t skyEnabled;
    float skyColor[3], skyIntensity, skyUpDir[3];
    int32_t pointLightEnabled;
    float pointLightPos[3], pointLightColor[3], pointLightIntensity;
    float matAlbedoColor[3], matAlbedoSpecStrength, matAlbedoGloss;
    float matGlassAlbedo[3], matGlassIOR, matGlassDistortion;
    int32_t matGlassEnabled;
    float matMirrorAlbedo[3], matMirrorGloss;
    int32_t matMirrorEnabled;
} RtUniforms;

/* include/render/RenderParams.h:14-239, same order and defaults (rt_default_render_params). */
typedef struct RtRenderParams {
    int32_t sppPerFrame; float exposure;
    float matAlbedoColor[3], matAlbedoSpecStrength, matAlbedoGloss;
    int32_t matGlassEnabled; float matGlassColor[3], matGlassIOR, matGlassDistortion;
    int32_t matMirrorEnabled; float matMirrorColor[3], matMirrorGloss;
    int32_t enableJitter; float jitterStillScale, jitterMovingScale;
    int32_t enableGI; float giScaleAnalytic, giScaleBVH;
    int32_t enableEnvMap; float envMapIntensity;
    int32_t sunEnabled; float sunColor[3], sunIntensity, sunYaw, sunPitch;
    int32_t skyEnabled; float skyColor[3], skyIntensity, skyYaw, skyPitch;
    int32_t pointLightEnabled; float pointLightColor[3], pointLightIntensity, pointLightPos[3];
    int32_t pointLightOrbitEnabled; float pointLightOrbitRadius, pointLightOrbitSpeed, pointLightYaw, pointLightPitch;
    int32_t enableAO, aoSamples; float aoRadius, aoBias, aoMin;
    int32_t enableTAA; float taaStillThresh, taaHardMovingThresh, taaHistoryMinWeight, taaHistoryAvgWeight,
        taaHistoryMaxWeight, taaHistoryBoxSize;
    int32_t enableSVGF; float svgfVarMax, svgfKVar, svgfKColor, svgfKVarMotion, svgfKColorMotion, svgfStrength;
    float motionScale;
} RtRenderParams;

/* Camera state, include/io/Camera.h:21-109 (degrees). */
typedef struct RtCamera { float pos[3], yaw, pitch, fov, aspect; } RtCamera;

/* Work counters in the reference's units: a "ray" is one call of traceBVH /
 * traceBVHShadow / traceAnalyticCore; node/tri fetches are nodeFetch()/triFetch() calls of
 * shaders/rt/rt_bvh.glsl (48 B each in the reference layout). */
typedef struct RtCounters {
    uint64_t raysClosest, raysShadow, raysAnalytic, nodeFetch, triFetch, envLookup, hitPixels;
    /* nodeFetch + triFetch split by the kind of ray: primary rays (rt.frag:86), traceBVHShadow rays, computeAO's rays
     * (rt_lighting.glsl:721-757); what is left belongs to the bounce's closest-hit rays. */
    uint64_t fetchPrimary, fetchShadow, fetchAO;
} RtCounters;

typedef enum RtPipeline {
    RT_PIPELINE_AUTO = 0,       /* wavefront pipeline for BVH scenes, megakernel for the analytic scene, staged replay for the hybrid extension */
    RT_PIPELINE_MEGAKERNEL = 1, /* one thread per pixel, the whole fragment program in one kernel */
    RT_PIPELINE_WAVEFRONT = 2   /* staged: primary -> ray generation -> persistent traversal -> combine */
} RtPipeline;

typedef struct RtDeviceConfig {
    int32_t device;        /* HIP device ordinal */
    int32_t rank;          /* tile-parallel rank of this context, 0 <= rank < worldSize */
    int32_t worldSize;     /* number of GPUs sharing one frame (1 = whole frame here) */
    int32_t pipeline;      /* RtPipeline */
    int32_t countWork;     /* non-zero: kernels maintain RtCounters (slower) */
    int32_t reserved[3];
} RtDeviceConfig;

typedef struct RtContext RtContext;

enum { RT_TARGET_COLOR = 0, RT_TARGET_MOTION = 1, RT_TARGET_GPOS = 2, RT_TARGET_GNRM = 3 };  /* rt.frag:29-38 */
enum { RT_FORMAT_F16 = 0, RT_FORMAT_F32 = 1 };

#define RT_TILE_DIM 16               /* framebuffer tiles are RT_TILE_DIM x RT_TILE_DIM pixels */
#define RT_TILE_PIXELS 256

/* ---------------------------------------------------------------- device side */

/* Replaces: GL context + FBO/texture creation (Application::initGLResources, application.cpp:195-205). */
int rt_create(const RtDeviceConfig *cfg, RtContext **out);
void rt_destroy(RtContext *ctx);
const char *rt_last_error(const RtContext *ctx);   /* ctx may be NULL: error of the last failed rt_create */

/* Replaces upload_bvh_tbo (include/scene/bvh.h:121, src/scene/bvh.cpp:141-221): takes the reference's
 * two RGBA32F texture-buffer payloads (12 floats per node, 12 per triangle) and repacks them into
 * the device layout.  nNodes == 0 / nTris == 0 clears the scene. */
int rt_upload_bvh(RtContext *ctx, const float *nodes12, int nNodes, const float *tris12, int nTris);

/* Replaces the glTexImage2D face uploads of loadCubeMapFromCross / createDummyCubeMap
 * (src/render/cubemap.cpp:7-31, 67-91): 6 faces in GL order +X -X +Y -Y +Z -Z, faceSize^2 texels of
 * `channels` (3 or 4) bytes, rows in upload order.  faces == NULL installs the 1x1 dummy
 * (128,128,255) of cubemap.cpp:13. */
/* The same builder as rt_build_bvh (below), run on the context's GPU: identical node numbering, ranges and boxes and the same
 * set of triangles in every leaf whenever no two triangles tie at a median.  Unlike rt_build_bvh, whose std::nth_element leaves
 * tied ranges and the order inside a leaf to the library, this builder is fully specified ("the tie rule"): level
 * by level, from input order, every inner range is sorted STABLY by the sortable key of the centroid along its axis, so triangles
 * with bit-equal keys keep the order they had and the order of the rows inside every leaf is defined; boxes are reduced in the
 * keys' order, in which -0 lies below +0.  tests/bvh_build_ref.py restates it in numpy and the device is compared with it bit
 * for bit.  rt_build_bvh remains the path that is bit-equal to the reference's own build; this is the fast one.
 * Returns the number of nodes (or a negative RtStatus); nodes12 needs room for 2*nTris nodes. */
int rt_build_bvh_gpu(RtContext *ctx, const float *tris9, int nTris, float *nodes12, float *tris12);

int rt_upload_env(RtContext *ctx, const uint8_t *faces, int faceSize, int channels);

/* Replaces Accum::recreate + GBuffer::recreate (src/render/accum.cpp:106-, gbuffer.cpp:12-53):
 * allocates COLOR0 ping-pong (RGBA16F), motion (RG16F), world pos / normal (RGBA16F); clears
 * history; frameIndex = 0. */
int rt_resize(RtContext *ctx, int width, int height);

/* Replaces Accum::reset (src/render/accum.cpp:98-102). */
int rt_reset_accum(RtContext *ctx);

/* accum.frameIndex (include/render/accum.h:125-128): the value the next frame will see as uFrameIndex. */
int rt_frame_index(const RtContext *ctx);

/* Replaces the ray pass of renderRay (src/render/render.cpp:58-194 + swapAfterFrame :242; the present
 * pass :199-239 is not part of this path).  `u` is the uniform block; u->frameIndex is ignored and
 * replaced by rt_frame_index().  Asynchronous on the context's stream. */
int rt_render_frame(RtContext *ctx, const RtUniforms *u);

/* `count` consecutive frames (us[i] = the uniform block of frame rt_frame_index() + i) with as few launches as possible: runs of
 * frames that differ only in uJitter / uFrameIndex and have uCameraMoved == 0 -- an accumulating static camera, every BASELINE
 * configuration -- are rendered up to 16 at a time by one set of kernel launches (BVH scenes, wavefront pipeline); anything else
 * falls back to one rt_render_frame per frame.  In the reference this is `count` turns of Application::mainLoop with a standing camera
 * (src/app/application.cpp:381-459: beginFrame, cameraMoved == false, the jitter of :398-405, renderRay, endFrame).
 * Bit-identical to `count` calls of rt_render_frame; afterwards the four targets hold
 * the last frame.  This is what keeps a tile-parallel rank busy: with 1/8 of the pixels a single frame is too little work per launch. */
int rt_render_frames(RtContext *ctx, const RtUniforms *us, int count);

/* The reference call-site in one call: mainLoop steps application.cpp:381-405 + renderRay + endFrame
 * (:459).  Keeps FrameState (prev/curr view-projection) inside the context.  currView/currProj may
 * be NULL: they are then derived from `cam` (Camera.cpp:66-73). */
int rt_render_ray(RtContext *ctx, const RtRenderParams *params, const RtCamera *cam, int useBVH, int showMotion,
                  const float *currView, const float *currProj);

/* ---- EXTENSION, not in the reference (BASELINE configs[2-3] "bunny + glass + mirror ..., 4 bounces": the reference's
 * BVH mode has neither analytic objects nor materials, rt.frag:84-106).  RtUniforms.useBVH == RT_SCENE_HYBRID renders the ANALYTIC
 * branch of rt.frag (:108-163) with the uploaded BVH mesh added to the analytic scene as one more object (material id 5: the default
 * branch of getMaterial, rt_materials.glsl:123-124), so the glass sphere refracts it, the mirror reflects it, it casts and receives
 * shadows, AO and GI.  giBounces > 1 lengthens the analytic GI path (oneBounceGIAnalytic) to that many diffuse bounces.  With an empty
 * BVH and giBounces == 1 this is the reference's analytic mode bit for bit.  Parity: this repository's own oracle only.
 * Pipelines: staged (RT_PIPELINE_AUTO / _WAVEFRONT: shading passes that replay answered mesh queries and queue the open ones, persistent
 * closest-hit traversal launches in between; csrc/rt_hybrid.hip) or the megakernel (RT_PIPELINE_MEGAKERNEL); same frames bit for bit. */
#define RT_SCENE_HYBRID 2
/* envFilter: model of texture(uEnvMap, dir)'s LINEAR filter (src/render/cubemap.cpp:56-58 GL_RGB8, :95-102 LINEAR / CLAMP_TO_EDGE).
 *   0 (default): bilinear weights from the fractional texel coordinates in exact fp32.
 *   1: the texel coordinates u = s*N - 0.5, v = t*N - 0.5 are first rounded to nearest on a grid of 1/256 texel (8 fractional bits of
 *      sub-texel precision, as GPU samplers filter RGB8), the weights (1-a)(1-b) ... then follow exactly; kept so that a capture from
 *      a real GL driver can be compared under either model.  Same texels, same face selection, same clamping. */
typedef struct RtExtension { int32_t giBounces; int32_t envFilter; int32_t reserved[2]; } RtExtension;
int rt_set_extension(RtContext *ctx, const RtExtension *ext);   /* applies to the frames rendered after the call */

/* `count` rt_render_ray calls with an unchanged camera and unchanged parameters, rendered through rt_render_frames (batched). */
int rt_render_ray_frames(RtContext *ctx, const RtRenderParams *params, const RtCamera *cam, int useBVH, int showMotion, int count);

int rt_synchronize(RtContext *ctx);

/* Read one render target of the last frame into host memory: full width x height image, row 0 =
 * bottom, channels 4/2/4/4, as half bit patterns (RT_FORMAT_F16) or floats (RT_FORMAT_F32, exact
 * widening).  With worldSize > 1 only this rank's tiles are filled, the rest is zero. */
int rt_read_target(RtContext *ctx, int which, void *dst, int dstFormat);

/* Inverse of rt_read_target for RT_FORMAT_F16: overwrite one render target "of the last frame" from a full
 * width x height host image (row 0 = bottom); a rank takes its own tiles.  Writing RT_TARGET_COLOR replaces the
 * accumulation history the next frame reads (uPrevAccum) -- what glTexSubImage2D on Accum::readTex() would do in
 * the reference (src/render/accum.cpp:8-20) -- so an accumulation can be restored from a saved frame or a test can
 * hand the renderer a known history.  The frame index is not touched (see rt_render_frame: it comes from RtUniforms). */
int rt_write_target(RtContext *ctx, int which, const void *src, int srcFormat);

/* Present pass of renderRay (src/render/render.cpp:199-239 = shaders/rt/rt_present.frag): SVGF-lite 7x7 filter,
 * ACES, gamma 1/2.2 (or the motion visualisation) over the four targets of the last frame -> RGBA8, width*height*4
 * bytes, row 0 = bottom.  RtPresentParams = the uniforms of rt_present.frag:38-50; rt_make_present_params fills
 * them from RenderParams as render.cpp:209-235 does.  Single-rank contexts only (the 7x7 taps cross tile borders). */
typedef struct RtPresentParams {
    float exposure; int32_t showMotion; float motionScale; float resolution[2];
    float varMax, kVar, kColor, kVarMotion, kColorMotion, svgfStrength; int32_t enableSVGF;
} RtPresentParams;
void rt_make_present_params(const RtRenderParams *p, int showMotion, int fbw, int fbh, RtPresentParams *out);
int rt_present(RtContext *ctx, const RtPresentParams *p, uint8_t *dstRGBA8);

/* Tile-parallel plumbing for a host that runs the exchange itself (e.g. through torch.distributed on these device pointers;
 * the library's own RCCL path is rt_comm_init / rt_gather_frame / rt_exchange_history below).
 * Local layout: [localTile][RT_TILE_PIXELS][channels] halfs, localTile = globalTile / worldSize for
 * globalTile % worldSize == rank, globalTile = tileY * tilesX + (tileX + rowShift) % tilesX, rowShift = 0 for worldSize 1 and
 * (11 * tileY) % tilesX otherwise: a rank's tiles are scattered over the frame, not fixed columns (csrc/rt_frame.hpp, tiles.py). */
int rt_local_target(RtContext *ctx, int which, void **devPtr, size_t *bytes);
/* bytes every rank must contribute so that all ranks send equally sized blocks (padded local size) */
int rt_gather_block_bytes(const RtContext *ctx, int which, size_t *bytes);
/* On the gathering rank: gatheredDev holds worldSize blocks of rt_gather_block_bytes() in rank order;
 * writes the row-major full frame (halfs) to dstDev (device memory, width*height*channels*2 bytes). */
int rt_assemble_gathered(RtContext *ctx, int which, const void *gatheredDev, void *dstDev);
/* the context's HIP stream (hipStream_t) so a caller can order its own work after the frame */
int rt_stream(RtContext *ctx, void **hipStream);

/* Tile-parallel frame with a MOVING camera.  Reprojection (rt_taa.glsl:116-179) reads the previous frame at arbitrary
 * pixels, i.e. in other ranks' tiles, so every rank needs the whole previous COLOR0.  After rt_render_frame(f) the host
 * all-gathers the ranks' COLOR0 blocks (rt_local_target / rt_gather_block_bytes) into the buffer returned by
 * rt_history_exchange_buffer -- worldSize blocks, rank-major, on rt_stream() -- and then calls rt_history_exchanged();
 * frame f+1 may then be rendered with cameraMoved = 1 (without the exchange: RT_ERR_STATE).  Static-camera frames need
 * no exchange: a pixel only reads its own history.  Both calls refer to the frame rendered last. */
int rt_history_exchange_buffer(RtContext *ctx, void **devPtr, size_t *bytes);
int rt_history_exchanged(RtContext *ctx);

/* Present pass over a tile-parallel frame on the gathering rank: the four arguments are device arrays of worldSize gathered
 * blocks each (as filled by the gather of COLOR / MOTION / GPOS / GNRM, rank-major, rt_gather_block_bytes per block). */
int rt_present_gathered(RtContext *ctx, const RtPresentParams *p, const void *gatheredColor, const void *gatheredMotion,
                        const void *gatheredGPos, const void *gatheredGNrm, uint8_t *dstRGBA8);

/* ---- the exchange itself, owned by the library ("the library owns device memory, streams and the RCCL
 * communicator"; 8e: gather for a static camera, all-gather of the history for a moving one).  One process per GPU; every call
 * below is collective over the ranks of the frame (RtDeviceConfig.rank / worldSize) and asynchronous on the stream of the frame
 * rendered last.  A C++ host needs nothing else to render tile-parallel: csrc/rt_cli.cpp --ranks N.
 *   rank 0:  rt_comm_unique_id(id)  -> hand the 128 bytes to the other ranks by any means (file, pipe, MPI, torch store)
 *   all:     rt_comm_init(ctx, id)  -> ncclCommInitRank
 *   per gathered frame:  rt_render_frame / rt_render_ray; rt_gather_frame(ctx, RT_TARGET_COLOR)   [+ rt_exchange_history]
 *   rank 0:  rt_read_gathered(ctx, RT_TARGET_COLOR, halfs)   or rt_gathered_frame() for the device pointer
 * Static camera: a pixel only reads its own history (rt_taa.glsl:86-105), which stays rank-local, so intermediate frames need
 * not be gathered at all -- call rt_gather_frame every k-th frame (BASELINE configs[4]: once per 32 accumulated frames). */
#define RT_COMM_ID_BYTES 128
int rt_comm_unique_id(void *id, size_t bytes);                         /* any process; needs librccl */
int rt_comm_init(RtContext *ctx, const void *id, size_t bytes);
int rt_comm_destroy(RtContext *ctx);                                   /* also done by rt_destroy */
int rt_gather_frame(RtContext *ctx, int which);                        /* worldSize == 1: a device copy + un-tiling, no RCCL */
int rt_gathered_frame(RtContext *ctx, int which, void **devPtr, size_t *bytes);   /* rank 0: row-major width x height halfs, row 0 = bottom */
int rt_read_gathered(RtContext *ctx, int which, void *dstHalfs);       /* rank 0: synchronises, copies that frame to the host */
int rt_present_last_gathered(RtContext *ctx, const RtPresentParams *p, uint8_t *dstRGBA8);   /* rank 0, after rt_gather_frame of all 4 targets */
int rt_exchange_history(RtContext *ctx);                               /* all-gather of COLOR0 + rt_history_exchanged() */
/* What the communicator itself reports (ncclCommCount / ncclCommUserRank; -1 = no communicator) and what the gathers of this
 * context moved: a tile-parallel run's line can then say which exchange really ran (bench.py's config.gather).  Device time of
 * the gathers: stage "gather" of rt_get_stage_times.  bytesIn: bytes received by the gathering rank (others: bytes sent). */
typedef struct RtCommInfo { int32_t commWorld, commRank, rank, worldSize; uint64_t gathers, gatherBytes, historyExchanges; } RtCommInfo;
int rt_comm_info(RtContext *ctx, RtCommInfo *out);

int rt_get_counters(RtContext *ctx, RtCounters *out);   /* needs countWork; totals since rt_reset_counters */
int rt_reset_counters(RtContext *ctx);

/* What rt_upload_bvh made of the scene: the device arrays of DESIGN.md 3 (64-byte two-child records for closest-hit rays, 128-byte
 * four-child records for any-hit rays, 80-byte triangle-pair records, the reference's 48-byte triangles for normals) and their
 * sizes -- the bytes a traversal launch has to bring in at most once (bench.py's HBM roofline).  When the any-hit tree is larger than
 * 4 MB the any-hit launches walk its quantised form instead: bytesNodes4 is then 64 bytes per four-child record + 32
 * bytes of exact box per leaf. */
#define RT_SCENE_QNODES_REJECTED 1   /* quantised any-hit nodes were asked for (tree size or RT_QNODES) but could not be built: the exact nodes are walked */
#define RT_SCENE_IMPLICIT 4          /* RT_IMPLICIT=1 and every leaf sits at one depth: closest-hit rays walk 48-byte records without child references */
#define RT_SCENE_NOT_FUSED 2         /* RT_FUSED=1 but some inner box is not the union of its children's: closest-hit rays walk the 64-byte records, not the fused ones */
typedef struct RtSceneInfo {
    int32_t nNodes, nTris, nInner, treeDepth, nWide4, nPairs;
    uint64_t bytesNodes2, bytesNodes4, bytesPairs, bytesTris;
    int32_t nFused;   /* fused closest-hit records (128 B per even-level inner node; 0: not built), DESIGN.md 4.2 */
    int32_t flags;    /* RT_SCENE_* */
    int32_t implicitDepth;   /* depth every leaf sits at when RT_SCENE_IMPLICIT is set */
    int32_t reserved;
} RtSceneInfo;
int rt_get_scene_info(const RtContext *ctx, RtSceneInfo *out);

/* Device memory behind the context: the ray-queue arenas of the wavefront pipeline (RtArenaPool: shared by the frame lanes), the
 * per-lane frame arrays (candidate / hit lists, pre-resolve stash), the hybrid extension's arena, and the device's free / total bytes
 * (hipMemGetInfo) -- bench.py reports them, so that the footprint of the timed mode is part of its line. */
typedef struct RtMemoryInfo { uint64_t queueArenaBytes, frameArrayBytes, hybridArenaBytes, deviceFreeBytes, deviceTotalBytes; int32_t queueArenas, lanes; } RtMemoryInfo;
int rt_get_memory_info(RtContext *ctx, RtMemoryInfo *out);

/* Rays the wavefront pipeline actually traversed since the last reset (identical rays of the reference -- the SPP
 * copies of a primary ray, the per-sample copies of the AO rays -- are traced once; disk-light shadow rays whose
 * weight is exactly zero are not traced at all).  RtCounters keeps counting in the reference's units.
 * gatherLoads*: 16-byte per-lane gather loads (BVH node and triangle records) the three traversal launches issued -- the unit of
 * the L1 gather roofline they run against (one divergent 16-byte lane-load per clock and CU, tools/gather.hip).
 * mergedLoads*: the same loads after merging the lanes of a wave that stand on the same record (they read the same 16-byte pieces,
 * which the vector L1 serves as ONE cache access): what the one-access-per-clock ceiling applies to.  Counted only by the
 * diagnostic traversal kernels (environment RT_TRACE_STATS=1 when the context renders); 0 otherwise. */
typedef struct RtTracedRays {
    uint64_t candidatePixels, hitPixels, primary, shadow, bounce, bounceShadow, frames;
    uint64_t gatherLoadsPrimary, gatherLoadsShadow, gatherLoadsBounce;
    uint64_t mergedLoadsPrimary, mergedLoadsShadow, mergedLoadsBounce;
    uint64_t ao, gatherLoadsAO;   /* AO rays traced as packets (one walk of the tree for the rays of a hit, round 4; not contained in `shadow`) and
                                   * the gather loads of that launch */
} RtTracedRays;
int rt_get_traced_rays(RtContext *ctx, RtTracedRays *out, int reset);

/* Device timing of the dominant kernel(s): HIP events recorded on the context's stream around each
 * stage of every frame since the last reset.  stage names: rt_stage_name(i). */
#define RT_MAX_STAGES 14
typedef struct RtStageTimes { int32_t nStages; int32_t frames; double ms[RT_MAX_STAGES]; uint64_t launches[RT_MAX_STAGES]; } RtStageTimes;
int rt_enable_stage_timing(RtContext *ctx, int enable);
int rt_get_stage_times(RtContext *ctx, RtStageTimes *out);   /* synchronises */
const char *rt_stage_name(int stage);

/* Diagnostics used by the parity tests: evaluate one device function of the float model on arrays
 * (op: 0 sin, 1 cos, 2 exp2, 3 log2, 4 pow(a,b), 5 f32->f16 bits, 6 rand(a,b,frame=c) bits,
 * 7 a/b, 8 sqrt(a), 9 1/sqrt(a), 10 the cube-map texel decode of code a (0..255), 11 halton(a, b) of rt_common.glsl:106-116,
 * 12 / 13 the sample / the hit a generator thread works on: a, b, c carry uint32 bit patterns -- thread index, live hits of the chunk, spp).  Arrays are host memory of n floats (out: n uint32 bit patterns). */
int rt_debug_eval(RtContext *ctx, int op, const float *a, const float *b, const float *c, uint32_t *out, int n);
/* Trace n rays against the uploaded BVH with the device traversal: kind 0 = closest hit (out: t, then
 * hit point xyz, then normal xyz; t = inf on miss), kind 1 = any hit within tMax (out[0] = 1/0).
 * kinds 2 / 3: the same two questions put to the wavefront pipeline's own traversal kernels (persistent launch, refill scheduler, the
 * any-hit node form rt_upload_bvh chose, the kernel build the environment selects for frames) -- kind 2: out[0] = t (inf on miss), out[1] = index of the
 * triangle hit, -1 on a miss; kind 3: out[0] = 1/0, a ray with tMax < 0 is an empty slot (out[0] = 0).
 * kind 4: any-hit rays through the packet kernel of RT_PACKET_AO (k_trace_packets), out[0] = 1/0 as kind 3.  n must be a multiple of four: rays 4 p .. 4 p + 3
 * form packet p, which leaves from the origin of its first ray (the caller guarantees that all four share it, as the AO rays of one hit do); a ray with
 * tMax < 0 is an empty slot (out[0] = 0), so packets of one to three live rays can be expressed. */
int rt_debug_trace(RtContext *ctx, int kind, const float *origins, const float *dirs, const float *tMax, float eps,
                   float inf, float *out7, int n);
/* Which traversal kernel builds ran: the RT_BUILD_* bits of every k_trace / k_trace_packets launch of this context's wavefront frames and of
 * rt_debug_trace kinds 2 - 4 since the last reset, ORed -- bits [0, 16) for the closest-hit launches, the same bits << RT_BUILD_ANY_SHIFT for the
 * any-hit launches.  Host-side bookkeeping at launch time: no synchronisation, no device work. */
#define RT_BUILD_LAUNCHED 0x001   /* a k_trace build ran */
#define RT_BUILD_LEAFB4   0x002   /* four-triangle leaf groups (RT_LEAFB / RT_LEAFB_CLOSEST = 4) */
#define RT_BUILD_STATS    0x004   /* counting build (RT_TRACE_STATS) */
#define RT_BUILD_COOP     0x008   /* quad-cooperative node fetch (RT_COOP) */
#define RT_BUILD_NEAR     0x010   /* near-first any-hit walk (RT_NEAR_FIRST) */
#define RT_BUILD_QN1      0x020   /* quantised any-hit nodes, seven-wave build (RT_QNODES=1) */
#define RT_BUILD_QN2      0x040   /* quantised any-hit nodes (RT_QNODES=2, or chosen by rt_upload_bvh) */
#define RT_BUILD_FUSE     0x080   /* fused closest-hit records (RT_FUSED) */
#define RT_BUILD_IMPL     0x100   /* implicit records (RT_IMPLICIT) */
#define RT_BUILD_TIMING   0x200   /* time-stamped production build (RT_TRACE_TIMING) */
#define RT_BUILD_PACKETS  0x400   /* (any-hit half) the packet kernel k_trace_packets ran (RT_PACKET_AO, rt_debug_trace kind 4) */
#define RT_BUILD_BOUNCE_PROBE 0x800   /* (any-hit half) bounce rays were walked any-hit first, the hits re-traced closest-hit (RT_BOUNCE_PROBE) */
#define RT_BUILD_ANY_SHIFT 16
int rt_debug_builds(RtContext *ctx, uint32_t *out, int reset);
/* The bounce probe of the wavefront frames.  Environment RT_BOUNCE_PROBE=0|1|auto (default auto): 0 traces the bounce rays with the
 * closest-hit launch alone; 1 walks them any-hit first with tMax = uINF -- a ray that misses is answered there, the few that hit are traced again by the
 * closest-hit launch -- in every launch set; auto does so while the share of bounce rays that hit, measured on earlier launch sets of the scene, is small.
 * Never under RT_ANYHIT_TREE=sah.  Frames are bit-identical either way.  Counts since the last reset, summed over the frame lanes (synchronises):
 * probed = bounce rays walked any-hit first, retraced = those of them traced again (the probe found a triangle), probeLaunches / closestLaunches = bounce
 * launches (one per chunk of a launch set) with / without the probe.  rt_get_traced_rays counts every bounce ray once either way. */
typedef struct RtBounceProbe { uint64_t probed, retraced, probeLaunches, closestLaunches; } RtBounceProbe;
int rt_debug_bounce_probe(RtContext *ctx, RtBounceProbe *out, int reset);
/* The disk-light skip of the wavefront frames' shading stages: a wave whose hits all face away from the whole disk light does not evaluate
 * the four disk samples, which add exactly zero there.  Counts since the last reset, summed over the frame lanes (synchronises), for the two ray generators:
 * pairs = (hit, sample) pairs shaded, unlit = pairs the per-hit test proved unlit, skipped = pairs whose wave skipped the loop, waves / wavesSkipped = the
 * waves they ran in.  The kernels count only from the first call of this entry on (a kernel argument that is null before): call it once, with reset, first. */
typedef struct RtDiskSkip { uint64_t directPairs, directUnlit, directSkipped, directWaves, directWavesSkipped, giPairs, giUnlit, giSkipped, giWaves, giWavesSkipped; } RtDiskSkip;
int rt_debug_disk_skip(RtContext *ctx, RtDiskSkip *out, int reset);
/* The bounce-hit generator of the wavefront frames, the stage that records the shadow rays at the bounce hits.  Behind a bounce probe it walks
 * the probe's list of hits (k_gen_gi_listed); otherwise -- no probe, RT_BIN_GI=1 -- it visits every (hit, sample) pair (k_gen_gi).  Counts since the last reset,
 * summed over the frame lanes (synchronises): visited = pairs the generator looked at, shaded = pairs whose bounce ray hit, listedLaunches / pairLaunches =
 * launches (one per chunk of a launch set) over the list / over every pair.  visited and shaded count only from the first call of this entry on (a kernel
 * argument that is null before): call it once, with reset, first. */
typedef struct RtGiList { uint64_t visited, shaded, listedLaunches, pairLaunches; } RtGiList;
int rt_debug_gi_list(RtContext *ctx, RtGiList *out, int reset);
/* The light-slot liveness masks of the wavefront frames: the ray generators mark the light slots of the two shadow queues that hold a ray in
 * bit masks beside the queues, and the any-hit launch deals its refills from those bits.  Environment RT_LIGHT_MASKS=1 (default): shadow queue 1; 2: queue 2
 * as well (measured option); 0: neither (a dead slot is then a tMax word < 0, as before); frames are bit-identical in all three.  Counts since the last reset, summed over the frame lanes (synchronises): bits1 / bits2 = bits
 * set for shadow queue 1 / 2 (= the light rays cast), wordsScanned = 64-bit mask words the any-hit launches read, refillPasses = their masked refill passes,
 * maskWords1 / maskWords2 = mask words of each lane's last chunk (0 with RT_LIGHT_MASKS=0).  The first four count only from the first call of this entry on:
 * call it once, with reset, first. */
typedef struct RtLightMasks { uint64_t bits1, bits2, wordsScanned, refillPasses, maskWords1, maskWords2; } RtLightMasks;
int rt_debug_light_masks(RtContext *ctx, RtLightMasks *out, int reset);
/* Diagnostics: the per-hit test beside the code it stands for.  For n pairs (hp, normal; 3 floats each) flags[i] bit 0 = the test holds, bit 1 = one of the
 * four disk samples of `seeds` (pixel, frame) seeds had geom != 0; maxDot[i] = the largest dot(N, L) those samples computed.  u supplies uPI. */
int rt_debug_disk_unlit(RtContext *ctx, const RtUniforms *u, const float *hp, const float *normals, int n, int seeds, uint8_t *flags, float *maxDot);

/* ---- raster preview: renderRaster (src/render/render.cpp:244-295, shaders/basic.vert / basic.frag), the reference's other frame
 * mode.  Flat-coloured meshes, MVP transform, GL_LESS depth test on a D24 buffer, no MSAA, no culling; the rules a GL 4.1 driver
 * follows in that state are restated bit for bit in DESIGN.md 11 (tests/raster_ref.py mirrors them).  Single-rank contexts only. */
#define RT_MAX_RASTER_MESHES 8
/* Mesh::setupMesh (include/scene/mesh.h:170-214): positions (3 floats per vertex) + triangle index list, checked once on the host
 * (nIdx % 3 == 0, every index < nVerts).  nVerts == 0 frees the slot. */
int rt_raster_mesh(RtContext *ctx, int slot, const float *positions, int nVerts, const uint32_t *indices, int nIdx);
/* one glDrawElements of renderRaster: mesh slot, model matrix (column-major), uColor */
typedef struct RtRasterDraw { int32_t mesh; float model[16]; float color[3]; } RtRasterDraw;
/* The draw list of renderRaster (ground, bunny, sphere, point-light marker when params->pointLightEnabled): returns the number of
 * draws written to out[4] (0..4).  A negative slot skips its draw (a model the reference did not load draws nothing). */
int rt_raster_scene_draws(const RtRenderParams *params, int groundSlot, int bunnySlot, int sphereSlot, RtRasterDraw out[4]);
/* Clear + the draws into the context's raster buffers (RGBA8, primitive id, depth; allocated on the first call, sized by
 * rt_resize).  Enqueued on rt_stream()'s stream; it does not wait for the device, except that growing a buffer (first call, a new
 * framebuffer size, more triangles, more bin pairs than before) frees and allocates device memory, which synchronises.  view16 /
 * proj16: currView / currProj (column-major).  Touches no ray target, no accumulation history and no frame index. */
int rt_render_raster(RtContext *ctx, const RtRasterDraw *draws, int nDraws, const float *view16, const float *proj16);
/* Synchronises; copies width x height pixels (row 0 = bottom) of the last rt_render_raster.  Any pointer may be NULL.  RT_ERR_STATE
 * when rt_resize changed the framebuffer size since that call (the buffers are sized by the framebuffer: render again first).  primId: the
 * global primitive index (draw's offset in the draw list + triangle's position in its index buffer), 0xFFFFFFFF on the background;
 * depth24: the D24 value (0xFFFFFF on the background). */
int rt_read_raster(RtContext *ctx, uint8_t *rgba8, uint32_t *primId, uint32_t *depth24);
/* What the last rt_render_raster did (synchronises).  trianglesIn = trianglesSetUp + trianglesDropped (dropped: non-finite, clipped
 * away or of zero area); trianglesClipped: went through the clipper; binEntries: (tile, triangle) pairs; binCapacity: pairs the bin
 * arrays held (entries beyond it were rasterised from the triangle list instead); deviceMs: HIP events around the call's launches. */
typedef struct RtRasterStats {
    uint64_t trianglesIn, trianglesDropped, trianglesClipped, trianglesSetUp, binEntries, binCapacity, rasterBytes;
    double deviceMs;
} RtRasterStats;
int rt_get_raster_stats(RtContext *ctx, RtRasterStats *out);
/* Diagnostics used by the tests: the bin arrays of the following rt_render_raster calls hold exactly `pairs` (tile, triangle) pairs,
 * so that the path past the capacity runs; 0 returns to automatic sizing. */
int rt_debug_raster_bin_capacity(RtContext *ctx, uint64_t pairs);
/* ---- raster draws of the dynamic mesh.  Bind a raster mesh slot to the context's dynamic mesh (rt_mesh_upload /
 * rt_mesh_upload_parts): draws naming the slot read the mesh's device positions and indices where they lie -- no copy, no index validation
 * (the upload did it), no allocation, no host wait.  A bound draw d is, by definition, the run of draws, one per non-empty part p in part
 * order, that rt_render_raster would execute from static slots holding the mesh's device positions as they stand when the call's setup work
 * runs on the stream, the index triples [partFirst[p], partFirst[p+1]), model = rt_mat4_mul(d.model, table[p]) with the table
 * (rt_mesh_part_matrices) as it stands at that moment, and the part's colour if a colour table is set, else d.color: every buffer and every
 * RtRasterStats count equal that list's bit for bit.  Input triangle t of the draw is global primitive base + t (base: the triangles of the
 * draws before d), so primId - base indexes the caller's index buffer and its part is rt_mesh_hit_parts' (the part whose range holds it).
 *   The binding is to "the context's dynamic mesh", resolved at each rt_render_raster: it follows a later rt_mesh_upload / rt_mesh_upload_parts
 * without rebinding, and a draw naming a bound slot while there is no mesh (never uploaded, released, or released by rt_upload_bvh) is
 * RT_ERR_STATE with nothing enqueued, as for an empty slot.  No tree is needed: positions, indices, the part lookup and the matrix table are
 * read, never the BVH, so a bound draw works before the first rt_mesh_rebuild.  rt_raster_mesh on a bound slot replaces the binding (nVerts == 0
 * unbinds); binding a slot that holds an uploaded mesh frees that mesh (after the wait rt_raster_mesh makes).  Several slots may be bound, in
 * either mode; RT_RASTER_BIND_PARTS on a mesh from plain rt_mesh_upload is its one part; a bound slot may be passed to rt_raster_scene_draws.
 *   Ordering: a raster call that names a bound slot sees every rt_mesh_set_positions / rt_mesh_set_part_matrices and every write of the caller
 * ordered on rt_stream()'s stream -- as it was when they were enqueued -- before the call, and is finished with positions and matrices before
 * any such write or mesh update enqueued after it; both by events, with no host wait.  Calls that name no bound slot gain no wait.
 *   RT_ERR_INVALID: a slot outside 0..RT_MAX_RASTER_MESHES-1, a mode other than the two. */
#define RT_RASTER_BIND_SINGLE 0   /* the draw's model matrix for every triangle, as rt_mesh_rebuild(ctx, M) gathers; the matrix table is not touched */
#define RT_RASTER_BIND_PARTS  1   /* per part p: model_p = rt_mat4_mul(draw.model, table[p]), table = rt_mesh_part_matrices() */
int rt_raster_mesh_dynamic(RtContext *ctx, int slot, int mode);
/* Optional flat colour per part for a slot bound with RT_RASTER_BIND_PARTS: nParts x 3 floats (host), packed as the draw colour is (unorm8 of
 * clamp) and kept on the device; rgb == NULL or nParts == 0 returns to the draw's own colour.  May wait for a raster call in flight and
 * allocate.  RT_ERR_INVALID: a slot not bound in parts mode, a negative count.  A table whose count differs from the mesh's part count when a
 * draw uses it makes that rt_render_raster RT_ERR_STATE (nothing enqueued; the previous raster frame stays readable). */
int rt_raster_part_colors(RtContext *ctx, int slot, const float *rgb, int nParts);
/* Device pointers of the last raster frame (RGBA8, primitive id, depth24; width x height uint32 each, row 0 = bottom), valid until the next
 * rt_render_raster that grows them or rt_resize; reads must be ordered on rt_stream()'s stream.  Any pointer may be NULL.  RT_ERR_STATE as
 * rt_read_raster.  No host wait. */
int rt_raster_targets(RtContext *ctx, void **rgba8, void **primId, void **depth24, size_t *bytesEach);

/* ---------------------------------------------------------------- ray queries against the uploaded BVH
 * "Here are N rays; what does each one hit?" through the persistent traversal kernels the frames use (same node form and build).
 * kind RT_QUERY_CLOSEST: traceBVH (shaders/rt/rt_bvh.glsl:186-243) with uEPS = eps and uINF = inf -- one RtHit per ray: t and prim (row of
 *   the uploaded tris12) of the reference's answer, u, v the barycentrics of triHit (:154-170) on that triangle; a miss is {inf, -1, 0, 0}.
 *   With tMax, ray i starts with best = tMax[i]: a hit exactly when the reference's t <= tMax[i] (then the same t and prim).  normals (may be
 *   NULL): 3 floats per ray, normalize(cross(e1, e2)) of the hit as traceBVH stores it in hitOut.n, zeros on a miss.
 * kind RT_QUERY_ANY: traceBVHShadow (:260-304) -- occluded[i] = 1 when a triangle is hit within [eps, tMax[i]], else 0.  tMax is required.
 * origins / dirs: float32, ray i at [i * stride .. i * stride + 2], stride >= 3 floats ([N,3], [N,4], or one interleaved [N,6] / [N,8]
 * array passed as two pointers).  tMax (optional for closest-hit): tMax[i] < 0 marks an empty slot, answered as a miss / not occluded.
 * n == 0 is a no-op.  RT_ERR_STATE when no BVH is uploaded.  A query reads the BVH only: no target, history, frame index, counter or
 * traced-ray tally changes.  rt_upload_bvh, rt_resize and rt_destroy wait for queries in flight. */
#define RT_QUERY_CLOSEST 0
#define RT_QUERY_ANY 1
typedef struct RtHit { float t; int32_t prim; float u, v; } RtHit;   /* 16 bytes, written as one store */
/* Device pointers; enqueued on rt_stream()'s stream; no host synchronisation and, after the first call, no allocation. */
int rt_trace_rays(RtContext *ctx, int kind, const float *origins, int originStride, const float *dirs, int dirStride,
                  const float *tMax, float eps, float inf, int n, RtHit *hits, float *normals, uint8_t *occluded);
/* The same with host pointers: stages through the context's buffer and synchronises (C hosts, numpy). */
int rt_trace_rays_host(RtContext *ctx, int kind, const float *origins, int originStride, const float *dirs, int dirStride,
                       const float *tMax, float eps, float inf, int n, RtHit *hits, float *normals, uint8_t *occluded);

/* ---------------------------------------------------------------- scene queries and pixel picking
 * The scene a frame rendered with *u shows, in every mode of u->useBVH: 0 the analytic scene (traceAnalyticCore, rt_scene_analytic.glsl:132-167),
 * 1 the uploaded BVH (traceBVH: the bytes of rt_trace_rays), RT_SCENE_HYBRID the analytic scene plus the mesh as one more object.  u->eps / u->inf are
 * uEPS / uINF, u->pointLightEnabled / u->pointLightPos place the marker sphere.  u->nodeCount / u->triCount are checked as rt_render_frame checks them
 * (RT_ERR_STATE when they name more than was uploaded); either 0: the scene has no mesh.  Analytic-mode queries need no BVH.
 * kind RT_QUERY_CLOSEST: one RtHit per ray.  A mesh hit: prim and u, v as rt_trace_rays.  An analytic hit: prim -1, u = v = 0.  A miss: {inf, -1, 0, 0}.
 *   Objects are tested in list order (floor, albedo, glass, mirror sphere, marker, mesh); a later object wins only at a strictly smaller t.
 *   objects (may be NULL): RT_OBJECT_* per ray.  normals (may be NULL): 3 floats, the hit's normal as the scene query stores it (plane normal,
 *   normalize(p - c) on a sphere, normalize(cross(e1, e2)) on the mesh).  points (may be NULL): 3 floats, ro + rd * t.  Both zero on a miss.
 *   tMax (optional): ray i is a hit exactly when the unbounded answer has t <= tMax[i], and then it is that answer (BVH mode: the bytes of
 *   rt_trace_rays with the same tMax); tMax[i] < 0 marks an empty slot.
 * kind RT_QUERY_ANY: occluded[i] = 1 when the analytic scene's closest t <= tMax[i], or (BVH / hybrid) traceBVHShadow finds a triangle within
 *   [eps, tMax[i]] -- the closest answer's t <= tMax[i], except for a triangle flush with a face of its BVH box at a tMax within rounding of its t
 *   (DESIGN.md 13.2).  tMax is required.
 *   occludedToward (rt_lighting.glsl:49-60) tests h.t < maxT - eps: pass tMax = nextafterf(maxT - eps, 0) for that test.
 * flags: RT_QUERY_SKIP_GLASS / RT_QUERY_SKIP_MARKER leave the glass sphere / the marker out (traceAnalyticIgnoreGlass / traceAnalyticIgnorePointLight,
 *   rt_scene_analytic.glsl:175-196); analytic objects only.
 * Rays, strides and alignment as rt_trace_rays; n == 0 is a no-op.  Device pointers; enqueued on rt_stream()'s stream; no host synchronisation and,
 * after the first call, no allocation.  No target, history, frame index, counter, traced-ray tally or rt_debug_builds bit changes. */
#define RT_QUERY_SKIP_GLASS 1
#define RT_QUERY_SKIP_MARKER 2
#define RT_OBJECT_NONE (-1)
#define RT_OBJECT_FLOOR 0
#define RT_OBJECT_ALBEDO_SPHERE 1
#define RT_OBJECT_GLASS_SPHERE 2
#define RT_OBJECT_MIRROR_SPHERE 3
#define RT_OBJECT_POINT_LIGHT 4
#define RT_OBJECT_MESH 5
int rt_trace_scene_rays(RtContext *ctx, const RtUniforms *u, int kind, int flags, const float *origins, int originStride,
                        const float *dirs, int dirStride, const float *tMax, int n,
                        RtHit *hits, int32_t *objects, float *normals, float *points, uint8_t *occluded);
/* Pixel (xy[2i], xy[2i + 1]) (row 0 = bottom, as rt_read_target) along the frame's primary ray: origin u->camPos, direction
 * primaryDirJ(u, x + 0.5, y + 0.5, u->jitter) (rt.frag:58-68, honouring enableJitter), answered as RT_QUERY_CLOSEST.  Any integer pair is a ray.
 * For every pixel of a frame rendered with *u: RT_TARGET_GPOS == (f16(points), 1) on a hit, zero on a miss, RT_TARGET_GNRM == (f16(normalize(normals)), 0). */
int rt_pick_pixels(RtContext *ctx, const RtUniforms *u, const int32_t *xy, int n,
                   RtHit *hits, int32_t *objects, float *normals, float *points);
/* The same with host pointers: staged through the context's buffer, synchronises. */
int rt_trace_scene_rays_host(RtContext *ctx, const RtUniforms *u, int kind, int flags, const float *origins, int originStride,
                             const float *dirs, int dirStride, const float *tMax, int n,
                             RtHit *hits, int32_t *objects, float *normals, float *points, uint8_t *occluded);
int rt_pick_pixels_host(RtContext *ctx, const RtUniforms *u, const int32_t *xy, int n,
                        RtHit *hits, int32_t *objects, float *normals, float *points);

/* ---------------------------------------------------------------- multi-hit queries: the K nearest hits and the hit count per ray
 * What lies behind the first surface: the layers under a cursor, every part a probe passes through, entry / exit pairs, the crossing count.
 *   For ray i with the limit T = tMax ? tMax[i] : inf, S is the set of triangles traceBVHShadow's loop (shaders/rt/rt_bvh.glsl:260-304) would accept
 * at the limit T with its `return true` removed: the root and every node on the way to the triangle's leaf pass aabbHit(...) && tmin <= T, and the
 * triangle passes triHit(ro, rd, T_i, T) with uEPS = eps.  The order of the visit is no part of it.  Nothing is culled against a hit already found
 * (DESIGN.md 20.2): the walk visits every box along the ray up to T, so bound the work with tMax.
 *   counts[i] = |S|.  hits[i * maxHits + j], j < min(maxHits, |S|), are the maxHits smallest elements of S under (key(t), prim) ascending: prim is the row
 * of tris12 as in rt_trace_rays, key(t) = bits(t) ^ (bits(t) >> 31 ? 0xFFFFFFFF : 0x80000000) -- the numeric order for every ordinary t, and an order
 * for the NaN t a degenerate ray gets through triHit's comparisons (positive NaNs last).  A record is {t, prim, u, v} with u, v as rt_trace_rays
 * computes them; slots j >= |S| hold the miss record {inf, -1, 0, 0}.  tMax[i] < 0 marks an empty slot: count 0, every slot a miss.  maxHits == 0 asks
 * for the counts alone.  The records are RtHit's: the flattened array is an input of rt_mesh_hit_parts, _normals, _colors, _uvs, _texels and
 * _prev_points as it stands (a miss answers zeros or -1 there).
 *   counts[i] > 0 exactly when rt_trace_rays' RT_QUERY_ANY says occluded at the same tMax, and without tMax exactly when RT_QUERY_CLOSEST hits; the
 * closest answer is an element of S, so key(hits[i * maxHits].t) <= key(closest t).
 *   rt_multi_hits is the definition: host arrays, no context, no GPU; nodes12 / tris12 as rt_build_bvh returns them (a single leaf is a tree).  It
 * returns RT_ERR_INVALID for the refusals below that apply to it, and for nodes that are no tree over the rows.
 *   rt_trace_rays_multi: device pointers; enqueued on rt_stream()'s stream; no host synchronisation and, after the context's first query, no allocation.
 * Rays and strides as rt_trace_rays.  hits: n * maxHits records, 16-byte aligned, required unless maxHits == 0; counts may be NULL unless maxHits == 0.
 * RT_ERR_INVALID: maxHits outside 0 .. RT_MULTI_HIT_MAX, n < 0, strides below 3, null or misaligned arrays, n * maxHits beyond INT32_MAX, ray arrays
 * beyond 2^32 floats.  RT_ERR_STATE: no BVH uploaded.  A refused call writes nothing; n == 0 is a no-op.  Frame state stays untouched as with rt_trace_rays.
 *   rt_pick_pixels_multi: pixel (xy[2i], xy[2i + 1]) along the frame's own primary ray, built on the device exactly as rt_pick_pixels builds it (jitter
 * included), with eps = u->eps and the limit u->inf.  The BVH scene only: u->useBVH != 1 is RT_ERR_INVALID; u->nodeCount / u->triCount are checked as
 * rt_pick_pixels checks them (either 0: no mesh, every count 0).
 *   The _host twins take host pointers, stage through the context's buffer and synchronise. */
#define RT_MULTI_HIT_MAX 32
int rt_multi_hits(const float *nodes12, int nNodes, const float *tris12, int nTris, const float *origins, int originStride,
                  const float *dirs, int dirStride, const float *tMax, float eps, float inf, int n, int maxHits, RtHit *hits, int32_t *counts);
int rt_trace_rays_multi(RtContext *ctx, const float *origins, int originStride, const float *dirs, int dirStride,
                        const float *tMax /* may be NULL */, float eps, float inf, int n, int maxHits, RtHit *hits, int32_t *counts);
int rt_trace_rays_multi_host(RtContext *ctx, const float *origins, int originStride, const float *dirs, int dirStride,
                             const float *tMax, float eps, float inf, int n, int maxHits, RtHit *hits, int32_t *counts);
int rt_pick_pixels_multi(RtContext *ctx, const RtUniforms *u, const int32_t *xy, int n, int maxHits, RtHit *hits, int32_t *counts);
int rt_pick_pixels_multi_host(RtContext *ctx, const RtUniforms *u, const int32_t *xy, int n, int maxHits, RtHit *hits, int32_t *counts);

/* ---------------------------------------------------------------- nearest-point queries: the closest surface point of the mesh per point
 * How far a point is from the surface and where the nearest surface point lies: proximity and contact tests, snapping, projecting points onto the
 * mesh, taking colour, UV or normal from the nearest surface point.
 *   Point i is points[i * stride .. i * stride + 2] (stride >= 3 floats).  Its limit is L = +inf without maxDist, else maxDist[i] * maxDist[i] rounded
 * once in float32; maxDist[i] < 0 or a non-finite coordinate marks an empty slot.  With lb(box, p) the squared distance from p to a box and d2(t) the
 * squared distance from p to row t by Ericson's closest-point walk over the row as stored (DESIGN.md 21.1 has every operation),
 *     e(t) = max(d2(t), lb(box(n), p) for every node n from the root to t's leaf)          (a NaN d2 stays NaN)
 * and the answer is the triangle least under (e(t), prim) ascending among those with e(t) <= L: prim is the row of tris12 as in rt_trace_rays.  The
 * order of the visit is no part of it.  e(t) differs from d2(t) only where rounding made a triangle look nearer than a box around it.
 *   hits[i] = {t = e, prim, u, v}: t is the squared distance, the nearest point is v0 + u e1 + v e2 of the row; closest (3 floats per point, may be
 * NULL) receives it.  No triangle within L, an empty slot or no scene: {+inf, -1, 0, 0} and a zero point (the float +inf: there is no uINF here).  The
 * records are RtHit's: an input of rt_mesh_hit_parts, _normals, _colors, _uvs and _texels as it stands -- the part, smooth normal, colour, UV or texel
 * of the nearest surface point.
 *   rt_nearest_points is the definition: host arrays, no context, no GPU; nodes12 / tris12 as rt_build_bvh returns them (a single leaf is a tree).  It
 * returns RT_ERR_INVALID for the refusals below that apply to it, and for nodes that are no tree over the rows.
 *   rt_query_nearest: device pointers; enqueued on rt_stream()'s stream; no host synchronisation and, after the context's first query, no allocation.
 * It walks the two-child records and triangle rows every scene form has, culling against its best: an unbounded query of a point far from the mesh
 * costs more than one near it, so give maxDist where a bound is known.  visits (may be NULL): visits[i] = the number of boxes whose lb the walk
 * evaluated for point i, 0 for an empty slot -- a diagnostic that depends on the visit order and is no part of the definition.  hits: n records,
 * 16-byte aligned.  RT_ERR_INVALID: n < 0, a stride below 3, null or misaligned arrays, a point array beyond 2^32 floats.  RT_ERR_STATE: no BVH
 * uploaded.  A refused call writes nothing; n == 0 is a no-op.  Frame state stays untouched as with rt_trace_rays.
 *   The _host twin takes host pointers, stages through the context's buffer and synchronises. */
int rt_nearest_points(const float *nodes12, int nNodes, const float *tris12, int nTris, const float *points, int stride,
                      const float *maxDist /* may be NULL */, int n, RtHit *hits, float *closest /* may be NULL */);
int rt_query_nearest(RtContext *ctx, const float *points, int stride, const float *maxDist, int n, RtHit *hits, float *closest, int32_t *visits);
int rt_query_nearest_host(RtContext *ctx, const float *points, int stride, const float *maxDist, int n, RtHit *hits, float *closest, int32_t *visits);

/* ---------------------------------------------------------------- proximity queries: the K nearest triangles and the count within a radius
 * Which triangles lie within r of a probe, how many, and the K nearest features where one nearest point is ambiguous: a contact manifold instead of
 * one contact, a brush or selection sphere, a trigger volume against a skinned or refitted mesh, density.
 *   Points, stride, maxDist, the limit L, empty slots and e(t) exactly as for the nearest-point queries above.  For point i, S is the set of rows t of
 * tris12 with e(t) <= L true (a NaN e or a NaN L accepts nothing).  The order of the visit is no part of it.
 *   counts[i] = |S| (counts may be NULL unless maxHits == 0).  hits[i * maxHits + j], j < min(maxHits, |S|), are the maxHits least elements of S under
 * (e(t), prim) ascending, each {t = e, prim, u, v} with u, v as rt_nearest_points computes them; slots j >= |S| hold the miss record {+inf, -1, 0, 0}.
 * closest (3 floats per record, n * maxHits * 3 in all, may be NULL) receives the point v0 + u e1 + v e2 of each record, zeros for a miss slot.
 * maxHits == 0 asks for the counts alone.  The records are RtHit's: the flattened array is an input of rt_mesh_hit_parts, _normals, _colors, _uvs and
 * _texels as it stands.
 *   With maxHits == 1, hits and closest equal rt_nearest_points' / rt_query_nearest's on the same arguments bit for bit; counts[i] > 0 exactly when
 * the nearest-point query answers point i at the same maxDist.
 *   rt_nearest_points_multi is the definition: host arrays, no context, no GPU; nodes12 / tris12 as rt_build_bvh returns them (a single leaf is a tree).
 * It returns RT_ERR_INVALID for the refusals below that apply to it, and for nodes that are no tree over the rows.
 *   rt_query_nearest_multi: device pointers; enqueued on rt_stream()'s stream; no host synchronisation and, after the context's first query, no allocation.
 * Without counts the walk culls against its maxHits-th best; with counts (or maxHits == 0) every row within L matters and it culls against L alone:
 * an unbounded count visits the whole tree, so give maxDist with counts.  visits (may be NULL) as rt_query_nearest's: a diagnostic.  hits: n * maxHits
 * records, 16-byte aligned, required unless maxHits == 0.  RT_ERR_INVALID: maxHits outside 0 .. RT_NEAREST_MULTI_MAX, maxHits == 0 without counts,
 * n * maxHits beyond INT32_MAX, n < 0, a stride below 3, null or misaligned arrays, a point array beyond 2^32 floats.  RT_ERR_STATE: no BVH uploaded.
 * A refused call writes nothing; n == 0 is a no-op.  Frame state stays untouched as with rt_trace_rays.
 *   The _host twin takes host pointers, stages through the context's buffer and synchronises. */
#define RT_NEAREST_MULTI_MAX 32
int rt_nearest_points_multi(const float *nodes12, int nNodes, const float *tris12, int nTris, const float *points, int stride,
                            const float *maxDist /* may be NULL */, int n, int maxHits, RtHit *hits, int32_t *counts /* may be NULL */,
                            float *closest /* may be NULL */);
int rt_query_nearest_multi(RtContext *ctx, const float *points, int stride, const float *maxDist, int n, int maxHits, RtHit *hits, int32_t *counts,
                           float *closest, int32_t *visits);
int rt_query_nearest_multi_host(RtContext *ctx, const float *points, int stride, const float *maxDist, int n, int maxHits, RtHit *hits, int32_t *counts,
                                float *closest, int32_t *visits);
/* (tests) The launch of rt_query_nearest_multi for a stack of stackEntries (1 .. 64) per lane and maxHits records: threads per block and its LDS bytes. */
int rt_debug_nearest_multi_block(int stackEntries, int maxHits, int *threads, int64_t *ldsBytes);

/* ---------------------------------------------------------------- box queries: the triangles overlapping an axis-aligned box, per box
 * Which triangles touch a volume: trigger volumes, brush and marquee selection through hidden layers, broad-phase pairs for a narrow phase of the
 * caller's own, conservative voxelisation -- against the uploaded BVH or the dynamic mesh after any rebuild, refit or update.
 *   Box i is boxes[i * stride .. i * stride + 5] = lo.xyz, hi.xyz (stride >= 6 floats), the closed box Q = [lo, hi]: touching counts.  A NaN component
 * or lo > hi on any axis marks an empty slot (count 0, nothing listed); +-inf components are legal, a box that spans everything lists everything.  A
 * box [bmin, bmax] overlaps Q when on all three axes !(bmax < lo) && !(hi < bmin): comparisons only.
 *   Row t of tris12 is accepted when (a) the box of every node from the root to t's leaf overlaps Q and (b) the 13-axis separating-axis test finds no
 * separating axis between Q and the triangle a = v0, b = fl(v0 + e1), c = fl(v0 + e2) -- the three points rt_build_bvh and the refit take the boxes
 * from.  The test forms no centre and no half-extent: the box axes by the overlap test above on the componentwise min / max of a, b, c; the normal
 * cross(e1, e2), on which the triangle projects to dot(n, a); the nine axes cross(unit_k, f), f = e1, fl(e2 - e1), e2, on which it projects to the min
 * and max of its vertices' projections.  On these ten the box projects to [sum_k min(n_k lo_k, n_k hi_k), sum_k max(n_k lo_k, n_k hi_k)], and an axis
 * separates only when tmax < bmin || bmax < tmin is true: a NaN (0 * inf, inf - inf, an overflowed product) never separates, so infinite and huge
 * boxes err towards overlap.  DESIGN.md 23.1 has every operation.  For trees whose node boxes are the float min / max of a, b, c of their rows --
 * every tree this library builds -- (b) implies (a).
 *   The list of box i is its accepted rows in the order of a depth-first walk that takes the RIGHT child before the left and the rows of a leaf
 * ascending: a function of the tree and the box alone.  For the trees rt_build_bvh and the device builders make, that walk meets the rows in
 * ascending order, so the list is ascending in prim; for other trees it is the walk order.
 *   counts[i] = the number of accepted rows (counts may be NULL when prims is given).  prims (may be NULL: the counts alone): slot i starts at
 * offsets[i] and holds offsets[i + 1] - offsets[i] entries (none if that is negative, or the start is) -- offsets has n + 1 entries -- or, with offsets
 * NULL, starts at i * cap and holds cap entries.  The first min(capacity, counts[i]) rows of the list are written there; entries past them are NOT
 * written.  Two patterns follow: count, exclusive scan, list -- the exact list in two calls; or one call with a fixed cap, where counts[i] > cap
 * says that slot i overflowed.  {0, prim, 1/3, 1/3} is an RtHit for the rt_mesh_hit_* queries (the part, colour or normal of a listed triangle).
 *   rt_box_overlaps is the definition: host arrays, no context, no GPU; nodes12 / tris12 as rt_build_bvh returns them (a single leaf is a tree).  It
 * returns RT_ERR_INVALID for the refusals below that apply to it, and for nodes that are no tree over the rows.
 *   rt_query_boxes: device pointers (offsets included: it is not inspected on the host); enqueued on rt_stream()'s stream; no host synchronisation
 * and, after the context's first query, no allocation.  One lane walks one box: a single box that lists tens of thousands of rows is serial in its
 * lane.  visits (may be NULL): visits[i] = the number of boxes tested for box i -- 1 + twice the inner nodes entered, 0 for an empty slot -- which
 * here is a function of the tree and the box.  RT_ERR_INVALID: n < 0, a stride below 6, null boxes, prims and counts both NULL, prims without offsets
 * and cap < 0 or n * cap beyond INT32_MAX, misaligned arrays, a box array beyond 2^32 floats.  RT_ERR_STATE: no BVH uploaded.  A refused call writes
 * nothing; n == 0 is a no-op.  Frame state stays untouched as with rt_trace_rays.
 *   The _host twin takes host pointers, stages through the context's buffer and synchronises; its prims array holds offsets[n] entries (offsets must
 * then be ascending from 0), or n * cap. */
int rt_box_overlaps(const float *nodes12, int nNodes, const float *tris12, int nTris, const float *boxes, int stride /* >= 6: lo.xyz, hi.xyz */, int n,
                    const int32_t *offsets /* n + 1 entries, or NULL */, int cap, int32_t *prims /* may be NULL */, int32_t *counts /* may be NULL, not both */);
int rt_query_boxes(RtContext *ctx, const float *boxes, int stride, int n, const int32_t *offsets, int cap, int32_t *prims, int32_t *counts, int32_t *visits);
int rt_query_boxes_host(RtContext *ctx, const float *boxes, int stride, int n, const int32_t *offsets, int cap, int32_t *prims, int32_t *counts,
                        int32_t *visits);

/* ---------------------------------------------------------------- triangle queries: the mesh triangles a query triangle intersects
 * The narrow phase after the box query's broad phase: a tool, a collider, a cutting plane, cloth or another pose of the same model tested against the
 * uploaded BVH or the dynamic mesh after any rebuild, refit or update.
 *   Query i is qtris[i * stride .. i * stride + 8] = p0.xyz, p1.xyz, p2.xyz (stride >= 9 floats).  A NaN in any of the nine components marks an empty
 * slot (count 0, nothing listed, visits 0); +-inf and huge coordinates are legal and err towards overlap.  [qlo, qhi] is the componentwise fmin / fmax
 * of the three points.
 *   Row t of tris12 is accepted when (a) the box of every node from the root to t's leaf overlaps [qlo, qhi] -- rt_box_overlaps' comparisons, so the
 * walk, its order and visits are those of the box query for that box -- and (b) none of 20 axes separates the query from the triangle a = v0,
 * b = fl(v0 + e1), c = fl(v0 + e2): the three box axes by comparisons of [min3, max3](a, b, c) with [qlo, qhi]; then, with f = e1, fl(e2 - e1), e2
 * and g = fl(p1 - p0), fl(p2 - p1), fl(p2 - p0), the normals n = cross(e1, e2) and m = cross(g1, g3), the nine cross(f_i, g_j), the three cross(n, f_i)
 * and the three cross(m, g_j).  On such an axis both triangles project to the min / max of dot(axis, point) over their three points (a NaN operand
 * ignored), and the axis separates only when Tmax < Qmin || Qmax < Tmin is true: a NaN never separates.  The six in-plane axes decide coplanar pairs.
 * Degenerate triangles (a segment, a point, a zero-area row) lose axes and err towards overlap.  A pair that shares a point in all three floats is
 * accepted; a query made of a row's own a, b, c lists that row.  DESIGN.md 24.1 has every operation.  For the trees this library builds (b) implies
 * (a).
 *   List order, counts, prims, offsets and cap: word for word as rt_box_overlaps above -- right child first, the rows of a leaf ascending (ascending
 * in prim for the library's trees); the first min(capacity, counts[i]) rows are written, entries past them are NOT written.
 *   rt_tri_overlaps is the definition: host arrays, no context, no GPU.  rt_query_tris: device pointers, enqueued on rt_stream()'s stream, no host
 * synchronisation and, after the context's first query, no allocation; one lane walks one query.  visits (may be NULL): 1 + twice the inner nodes
 * entered, 0 for an empty slot.  RT_ERR_INVALID: n < 0, a stride below 9, null qtris, prims and counts both NULL, prims without offsets and cap < 0 or
 * n * cap beyond INT32_MAX, misaligned arrays, a triangle array beyond 2^32 floats.  RT_ERR_STATE: no BVH uploaded.  A refused call writes nothing;
 * n == 0 is a no-op.  Frame state stays untouched.  The _host twin takes host pointers, stages through the context's buffer and synchronises; its
 * prims array holds offsets[n] entries (offsets must then be ascending from 0), or n * cap. */
int rt_tri_overlaps(const float *nodes12, int nNodes, const float *tris12, int nTris, const float *qtris, int stride /* >= 9: p0.xyz, p1.xyz, p2.xyz */, int n,
                    const int32_t *offsets /* n + 1 entries, or NULL */, int cap, int32_t *prims /* may be NULL */, int32_t *counts /* may be NULL, not both */);
int rt_query_tris(RtContext *ctx, const float *qtris, int stride, int n, const int32_t *offsets, int cap, int32_t *prims, int32_t *counts, int32_t *visits);
int rt_query_tris_host(RtContext *ctx, const float *qtris, int stride, int n, const int32_t *offsets, int cap, int32_t *prims, int32_t *counts,
                       int32_t *visits);

/* ---------------------------------------------------------------- hull queries: the triangles in a frustum or an oriented box; marquee picking
 * The volumes an axis-aligned box does not fit: the frustum behind a rectangle of a perspective view (marquee selection through hidden layers), a
 * trigger volume that moves with a part (a box under the part's model matrix), a sheared box.  All are one shape, a convex hexahedron given by its
 * eight corners -- the image of a box under an affine or projective map.
 *   Query i is hulls[i * stride .. i * stride + 23] = c0.xyz .. c7.xyz (stride >= 24 floats).  Corner k has bit 0 for the low or high end along the
 * shape's first parameter, bit 1 along the second, bit 2 along the third (for a frustum: x, y and depth).  A NaN in any of the 24 floats marks an empty
 * slot (count 0, nothing listed, visits 0); +-inf and huge coordinates are legal and err towards overlap.  The solid is the convex hull of the eight
 * points.  The caller supplies planar, convex faces; where they are not planar the test still never misses a real overlap -- every axis it tries
 * projects all eight points -- and errs towards overlap.  [lo, hi] is the componentwise fmin / fmax of the corners.
 *   Formed once per query: the six face normals -- for the faces {0,2,4,6}, {1,3,5,7}, {0,1,4,5}, {2,3,6,7}, {0,1,2,3}, {4,5,6,7}, written (a, b, c, d),
 * cross(fl(c_d - c_a), fl(c_c - c_b)), the cross product of the face's diagonals, so that a face collapsed to a point (the apex of a pyramid) leaves its
 * neighbours' normals intact and has the zero normal itself, which never separates -- and the hull's interval on each, the min / max of dot(normal, c_k)
 * over the eight corners, a NaN operand ignored.
 *   Row t of tris12 is accepted when (a) every node from the root to t's leaf passes the node test -- its box overlaps [lo, hi] by rt_box_overlaps'
 * comparisons, and none of the six face normals parts the box from the hull: the box projects to its corners through dot's own three steps, the least
 * and the greatest kept at each, and a normal separates only when bmax < hmin || hmax < bmin is true -- and (b) none of 46 axes separates the hull from
 * the triangle a = v0, b = fl(v0 + e1), c = fl(v0 + e2), tried in this order: the three box axes by comparisons of [min3, max3](a, b, c) with [lo, hi];
 * the six face normals against the kept intervals; n = cross(e1, e2); the 36 axes cross(f_i, d_e) with f = e1, fl(e2 - e1), e2 and d_e = fl(c_j - c_i)
 * for the edges (0,1), (2,3), (4,5), (6,7), (0,2), (1,3), (4,6), (5,7), (0,4), (1,5), (2,6), (3,7), the edge loop outside.  On a projected axis the hull is
 * the min / max of dot(axis, c_k) and the triangle that of dot(axis, point); the axis separates only when Tmax < Hmin || Hmax < Tmin is true: a NaN
 * never separates.  On the 43 projected axes, and in the node test, only finite projections separate: a hull some 1e19 across that is not
 * axis-aligned has normals and edge products that overflow, dot then gives inf for some points and NaN for others, and an interval of the points that
 * happened to stay finite would be no interval of the hull.  So each side's interval counts only when the float sum of its projections (the eight
 * corners' ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), the row's (ta + tb) + tc) is finite -- an inf or a NaN among them stays in the sum --,
 * and a node's box only when it and its interval on the normal lie within +-1e38 (comparisons, which a NaN fails).  That is how infinite and huge hulls err towards overlap.  Degenerate hulls (a point, a segment, a quad) and rows lose axes and err towards overlap; a pair that shares a point in all three
 * floats is accepted.  DESIGN.md 26.1 has every operation.  For the trees this library builds, node boxes are the float min / max of a, b, c of their
 * rows and the box's interval on a normal contains the dot of every point inside the box, so (b) implies (a): the list is the set of rows the row test
 * accepts, whatever the walk.
 *   List order, counts, prims, offsets and cap: word for word as rt_box_overlaps above -- right child first, the rows of a leaf ascending; the first
 * min(capacity, counts[i]) rows are written, entries past them are NOT written.
 *   rt_hull_overlaps is the definition: host arrays, no context, no GPU.  rt_query_hulls: device pointers, enqueued on rt_stream()'s stream, no host
 * synchronisation and, after the context's first query, no allocation; one lane walks one query.  visits (may be NULL): the node boxes tested, 1 + twice
 * the inner nodes entered, 0 for an empty slot -- never more than rt_query_boxes' on [lo, hi].  RT_ERR_INVALID: n < 0, a stride below 24, null hulls,
 * prims and counts both NULL, prims without offsets and cap < 0 or n * cap beyond INT32_MAX, misaligned arrays, a hull array beyond 2^32 floats.
 * RT_ERR_STATE: no BVH uploaded.  A refused call writes nothing; n == 0 is a no-op.  Frame state stays untouched.  The _host twin takes host pointers,
 * stages through the context's buffer and synchronises; its prims array holds offsets[n] entries (offsets must then be ascending from 0), or n * cap.
 *
 *   The corner makers, host only, no context, no GPU.  rt_box_corners: corner k of box i (boxes[i * stride ..] = lo.xyz, hi.xyz, stride >= 6) is
 * M * (k&1 ? hi.x : lo.x, k&2 ? hi.y : lo.y, k&4 ? hi.z : lo.z, 1) in rt_gather_triangles' expression, into corners24[i * 24 ..].  M16s NULL is the
 * identity, which copies; else matrix i is M16s[i * matStride ..], matStride 0 (one matrix for all boxes) or 16 (one per box, as the part matrices
 * lie in rt_mesh_part_matrices' table).  A NaN component or lo > hi writes 24 NaNs, an empty slot.  RT_ERR_INVALID: n < 0, a stride below 6, another
 * matStride, null arrays with n > 0.
 *   rt_rect_frusta: rect i is rects[i * stride ..] = (x0, y0, x1, y1) (stride >= 4) in pixel-corner coordinates of the frame u describes, row 0 at the
 * bottom as rt_pick_pixels counts rows: pixel (x, y) covers [x, x + 1] x [y, y + 1].  Any floats are legal, outside the frame too; a NaN, x1 < x0 or
 * y1 < y0 writes 24 NaNs.  The direction through the frame point (fx, fy) is primaryDirJ's before its normalize, jitter honoured as there:
 * D(fx, fy)[a] = (camFwd[a] + (nx * camRight[a]) * sx) + (ny * camUp[a]) * sy with nx = ((fx + jx) / resolution[0]) * 2 - 1, ny likewise, sx = tanHalfFov *
 * aspect, sy = tanHalfFov.  Its depth along camFwd is 1, so the near and far faces are planes of constant depth, and corner k is
 * fma(D(k&1 ? x1 : x0, k&2 ? y1 : y0)[a], k&4 ? far : tNear, camPos[a]).  tNear >= 0; 0 gives the pyramid from the eye.  far = max(tFar, tNear) when
 * tFar >= 0; tFar < 0 is "to the far side of the scene": with s the greatest dot(camFwd, fl(rootCorner_k - camPos)) over the eight corners of
 * [rootMin, rootMax], far = fmax(fma(|s|, 2^-10, s), tNear) -- widened so that rounding cannot cut off the farthest vertex.  Only the camera fields of u
 * are read: camPos, camRight, camUp, camFwd, tanHalfFov, aspect, resolution, jitter, enableJitter.  RT_ERR_INVALID: null u, rootMin or rootMax, a
 * resolution <= 0, a negative or NaN tNear, a NaN tFar, a stride below 4, n < 0, null arrays with n > 0.
 *   rt_pick_rects: marquee picking.  A kernel writes rt_rect_frusta's 24 floats per rect into corners -- a required device array of n * 24 floats, an
 * output the caller can draw -- with the root box of the uploaded BVH or the dynamic mesh as it stands on the device; then the hull query runs on
 * corners, on the same stream and with no host wait.  Everything else -- offsets, cap, prims, counts, visits, the refusals, "a refused call writes
 * nothing" and "no allocation after the context's first query" -- as rt_query_hulls, plus rt_rect_frusta's refusals.  The _host twin as above; its
 * corners array is host memory. */
int rt_hull_overlaps(const float *nodes12, int nNodes, const float *tris12, int nTris, const float *hulls, int stride /* >= 24: c0.xyz .. c7.xyz */, int n,
                     const int32_t *offsets /* n + 1 entries, or NULL */, int cap, int32_t *prims /* may be NULL */, int32_t *counts /* may be NULL, not both */);
int rt_query_hulls(RtContext *ctx, const float *hulls, int stride, int n, const int32_t *offsets, int cap, int32_t *prims, int32_t *counts, int32_t *visits);
int rt_query_hulls_host(RtContext *ctx, const float *hulls, int stride, int n, const int32_t *offsets, int cap, int32_t *prims, int32_t *counts,
                        int32_t *visits);
int rt_box_corners(const float *boxes, int stride /* >= 6 */, int n, const float *M16s /* NULL: the identity */, int matStride /* 0 or 16 */,
                   float *corners24);
int rt_rect_frusta(const RtUniforms *u, const float *rootMin, const float *rootMax, const float *rects, int stride /* >= 4: x0, y0, x1, y1 */, int n,
                   float tNear, float tFar /* < 0: to the far side of the scene */, float *corners24);
int rt_pick_rects(RtContext *ctx, const RtUniforms *u, const float *rects, int stride, int n, float tNear, float tFar, float *corners /* n * 24 floats */,
                  const int32_t *offsets, int cap, int32_t *prims, int32_t *counts, int32_t *visits);
int rt_pick_rects_host(RtContext *ctx, const RtUniforms *u, const float *rects, int stride, int n, float tNear, float tFar, float *corners,
                       const int32_t *offsets, int cap, int32_t *prims, int32_t *counts, int32_t *visits);

/* ---------------------------------------------------------------- dynamic mesh: the BVH scene rebuilt on the device
 * Replaces rebuild_bvh_from_model_path / a change of AppState::bvhTransform (gather_model_triangles + build_bvh + upload_bvh_tbo on every change of
 * the model or its transform).  Contract: after rt_mesh_rebuild(ctx, M) the context's scene is, byte for byte in every device array, what
 * rt_gather_triangles_checked(positions, indices, M) -> rt_build_bvh_gpu -> rt_upload_bvh would have installed -- reached without copying geometry or
 * records to or from the host, without allocating and without blocking the host.  Frames, the hybrid extension, ray / scene queries and picking work
 * unchanged on it.
 *  - rt_upload_bvh after rt_mesh_upload installs its scene as always and releases the dynamic mesh; a later rt_mesh_rebuild is RT_ERR_INVALID.
 *    rt_mesh_rebuild before rt_mesh_upload: RT_ERR_INVALID as well.
 *  - rt_mesh_upload removes whatever scene the context had (as rt_upload_bvh does) and installs none: the context has no BVH until the first rebuild.
 *  - A rebuild does not reset the accumulation (neither does rt_upload_bvh): call rt_reset_accum or render with cameraMoved, as the application does.
 *  - The quantised any-hit form is built under rt_upload_bvh's rule (tree size, RT_QNODES).  Whether it could be built is known on the device only and the
 *    host chooses the kernel, so when -- and only when -- that form is in use, rt_mesh_rebuild reads one status word back and waits for the rebuild: the
 *    one host wait of the path (RtMeshInfo.hostSyncs).  On failure the scene carries RT_SCENE_QNODES_REJECTED and the exact nodes are walked.
 *  - RT_FUSED, RT_IMPLICIT and RT_ANYHIT_TREE=sah (measured and rejected record forms) are not rebuilt on the device: rt_mesh_upload returns
 *    RT_ERR_UNSUPPORTED under any of them and says which.
 *  - The bounce-share prediction of the wavefront frames survives the rebuilds of one mesh (same topology; frames do not depend on it);
 *    rt_mesh_upload forgets it, as rt_upload_bvh does.
 *  - Tile-parallel ranks each rebuild their own copy; nothing is exchanged. */
/* What the triangle count alone determines: the builder splits every range at its middle and stops at <= 8 triangles, so numbering, links, leaf ranges,
 * record counts, stack need and array sizes of every device record form follow from nTris.  quantised / bytesNodes4: under rt_upload_bvh's rule for the
 * quantised any-hit form (RT_QNODES in this process's environment), assuming it can be built.  Host only.  nTris <= 0: RT_ERR_INVALID; nTris >= 2^28 or a
 * depth beyond 32: RT_ERR_UNSUPPORTED, as rt_upload_bvh refuses them. */
typedef struct RtBvhLayout {
    int32_t nTris, nNodes, nInner, treeDepth, nWide4, nPairs, anyStack, quantised;
    uint64_t bytesNodes2, bytesNodes4, bytesPairs, bytesTris;   /* as RtSceneInfo reports them */
} RtBvhLayout;
int rt_bvh_layout(int nTris, RtBvhLayout *out);
/* Mesh::setupMesh's arrays (3 floats per vertex, index triples), checked as rt_gather_triangles_checked checks them (every index < nVerts) and
 * nIdx % 3 == 0.  Keeps both on the device, lays the topology out on the host, uploads the index tables and allocates, once, every scene array and all
 * build scratch.  May synchronise and allocate; the only call of the group that may.  nIdx == 0 releases the mesh (and the scene it installed). */
int rt_mesh_upload(RtContext *ctx, const float *positions, int nVerts, const uint32_t *indices, int nIdx);
/* The device array of object-space positions (nVerts x 3 floats) for a caller that deforms the mesh on the device; writes must be ordered on
 * rt_stream()'s stream, as the rays of rt_trace_rays.  Refused (no mesh), it leaves *devPtr NULL and *bytes 0, as every accessor of this group does.
 * rt_mesh_set_positions: the same from host memory (nVerts x 3 floats), copied on that stream. */
int rt_mesh_positions(RtContext *ctx, void **devPtr, size_t *bytes);
int rt_mesh_set_positions(RtContext *ctx, const float *positions);
/* Gather with the model matrix M16 (column-major; NULL: identity), build, emit every record form, install.  Enqueued on rt_stream()'s stream, ordered
 * after the frames and queries already enqueued on every frame lane and before whatever is enqueued next, by events.  No allocation; no host wait
 * except the one named above. */
int rt_mesh_rebuild(RtContext *ctx, const float *M16);
/* Refit: the second build mode.  Keeps the tree of the most recent rt_mesh_rebuild -- node numbering, links, leaf ranges and which input triangle sits
 * in which row of the triangle array -- and recomputes, on the device, everything that depends on coordinates from the current device positions and M16
 * (NULL: identity): the triangles, every node's box bottom-up, the root box and every record form a rebuild emits.  No sort, so a fraction of a rebuild's
 * cost.  Contract: afterwards the scene is, byte for byte in every device array and in RtSceneInfo, what rt_upload_bvh installs from
 * rt_refit_bvh(rt_gather_triangles_checked(positions, indices, M16), order, nodes12, tris12) with route A's arrays of the last rebuild and rt_mesh_order's
 * order.  Enqueued, ordered and installed exactly as rt_mesh_rebuild: no allocation, no host wait but the one status-word read of the quantised form
 * (RtMeshInfo.hostSyncs counts it; on failure RT_SCENE_QNODES_REJECTED), accumulation and bounce-share prediction kept.  RT_ERR_INVALID without a mesh
 * and before the first rt_mesh_rebuild of the current mesh; rt_mesh_upload / rt_upload_bvh forget the tree as they forget the mesh.
 * A refitted tree is exact for any deformation, but the further triangles move apart from where the last rebuild found them, the more its boxes overlap
 * and the slower it is to walk.  rt_mesh_measure / rt_mesh_quality measure that on the device and rt_mesh_update refits or rebuilds by it (below). */
int rt_mesh_refit(RtContext *ctx, const float *M16);
/* Refits since rt_mesh_upload and since the last rt_mesh_rebuild (either pointer may be NULL, not both).  RtMeshInfo.rebuilds counts rebuilds only. */
int rt_mesh_refit_count(RtContext *ctx, uint64_t *total, uint64_t *sinceRebuild);
/* order[i] = the input triangle (index triple i of rt_mesh_upload's indices) that is row i of the device triangle array since the last rebuild --
 * rt_build_bvh_order's meaning, so order[prim] ties a query's or a pick's answer to the caller's index buffer.  A refit does not change it.
 * rt_mesh_order copies nTris entries out and synchronises; rt_mesh_order_device hands out a device array (nTris x int32) that is valid until the next
 * rt_mesh_rebuild and is written, at the first call after a rebuild, on rt_stream()'s stream: order reads of it there.  RT_ERR_INVALID before the first
 * rebuild. */
int rt_mesh_order(RtContext *ctx, int32_t *order);
int rt_mesh_order_device(RtContext *ctx, void **devPtr, size_t *bytes);
/* ---- parts: a mesh is a list of parts, each with its own model matrix on the device; a hit maps back to (part, triangle of the part).
 * A part is a contiguous run of index triples: partFirst has nParts + 1 entries in triangle units, partFirst[0] == 0, partFirst[nParts] == nIdx / 3,
 * non-decreasing.  Empty parts are legal anywhere and their matrices are ignored.  Parts share the one position pool: a vertex used by several parts is
 * transformed once per use, under each part's matrix.  1 <= nParts <= RT_MAX_MESH_PARTS.  rt_mesh_upload makes a mesh of one part, and
 * rt_mesh_rebuild(ctx, M) / rt_mesh_refit(ctx, M) keep their meaning -- one M for every triangle -- on any mesh; they neither read nor write the table. */
#define RT_MAX_MESH_PARTS 65535
/* rt_mesh_upload with a part table: RT_ERR_INVALID, with a message, for a broken partFirst, a part count out of range or a null table, besides
 * rt_mesh_upload's own causes (and its RT_ERR_UNSUPPORTED ones).  Allocates, besides what rt_mesh_upload allocates, the parts table, the per-triangle
 * part lookup and the matrix table (RtMeshInfo.allocations counts them), and sets every matrix to the identity.  nIdx == 0 releases the mesh. */
int rt_mesh_upload_parts(RtContext *ctx, const float *positions, int nVerts, const uint32_t *indices, int nIdx,
                         const int32_t *partFirst, int nParts);
/* *nParts = the part count of the current mesh; the nParts + 1 boundaries are copied when partFirst != NULL and capacity >= nParts + 1 (partFirst ==
 * NULL asks for the count only; a smaller capacity: RT_ERR_INVALID).  RT_ERR_INVALID without a mesh. */
int rt_mesh_parts(RtContext *ctx, int32_t *partFirst, int capacity, int *nParts);
/* The matrix table: nParts x 16 float32 on the device, column-major, for a caller that writes matrices on the device; writes must be ordered on
 * rt_stream()'s stream, exactly as for rt_mesh_positions.  rt_mesh_set_part_matrices: `count` matrices from host memory into entries first .., copied on
 * that stream as rt_mesh_set_positions copies positions; a range outside the table: RT_ERR_INVALID. */
int rt_mesh_part_matrices(RtContext *ctx, void **devPtr, size_t *bytes);
int rt_mesh_set_part_matrices(RtContext *ctx, int first, int count, const float *M16s);
/* rt_mesh_rebuild / rt_mesh_refit with the gather of rt_gather_triangles_parts under the matrices that are in the table when the call's work runs on
 * the stream.  Contracts: after the rebuild the scene is, byte for byte in every device array and in RtSceneInfo, what rt_gather_triangles_parts ->
 * rt_build_bvh_gpu -> rt_upload_bvh installs in a fresh context; after the refit, what rt_upload_bvh installs from
 * rt_refit_bvh(rt_gather_triangles_parts(...), order, nodes12, tris12) with route A's arrays of the last rebuild and rt_mesh_order's order.  Everything
 * else is the single-matrix calls': the same ordering by events, no allocation, no host wait but the status-word read of the quantised form
 * (RtMeshInfo.hostSyncs), accumulation and bounce-share prediction kept, RtMeshInfo.rebuilds and rt_mesh_refit_count count them, the same RT_ERR_INVALID
 * cases.  The four update calls may be mixed freely; a refit keeps the tree of the most recent rebuild of either kind. */
int rt_mesh_rebuild_parts(RtContext *ctx);
int rt_mesh_refit_parts(RtContext *ctx);
/* Hit -> part, on the device: for hit i of n RtHit records (rt_trace_rays, rt_trace_scene_rays, rt_pick_pixels), parts[i] = the part whose range holds
 * t = order[prim] (rt_mesh_order's order) and tris[i] = t - partFirst[parts[i]]; a prim outside [0, nTris) -- a miss, an analytic hit, a stale value --
 * gives parts[i] = tris[i] = -1 and reads nothing out of bounds.  Device pointers; either output may be NULL, not both.  Enqueued on rt_stream()'s
 * stream: no host wait, no allocation; the order array is derived on first use after a rebuild, as by rt_mesh_order_device.  RT_ERR_INVALID before the
 * first rebuild.  _host: the same with host pointers, staged through the context's buffer; synchronises. */
int rt_mesh_hit_parts(RtContext *ctx, const RtHit *hits, int n, int32_t *parts, int32_t *tris);
int rt_mesh_hit_parts_host(RtContext *ctx, const RtHit *hits, int n, int32_t *parts, int32_t *tris);
/* ---- tree quality: what refitting has cost the tree, measured on the device, and the refit-or-rebuild policy on top of it.
 * The metric is rt_bvh_cost's (host side, below): the surface-area heuristic with both unit costs 1, in units of the root's area, summed as integers so
 * that the device reproduces the host's bits.  It is a measurement: what ratio is worth a rebuild depends on the scene, and is the caller's argument. */
typedef struct RtBvhCost {
    uint64_t innerQ, leafQ;        /* sum of q over inner nodes / of q * count over leaves; q = floor(half-area * 2^(32 - rootExp)) */
    double rootArea;               /* node 0's half-area dx*dy + dy*dz + dz*dx, in double */
    double inner, leaf, cost;      /* innerQ, leafQ back in units of rootArea; cost = inner + leaf */
    int32_t rootExp;               /* frexp's exponent of rootArea */
    int32_t degenerate;            /* rootArea == 0: every sum is zero and means nothing */
    int32_t nInner, nLeaves;
} RtBvhCost;
typedef struct RtMeshQuality {
    RtBvhCost cost;
    uint64_t update;               /* serial of the update that was measured: rebuilds + refits of the current mesh up to and including it */
    int32_t refitsSinceRebuild;    /* of that update: 0 = the tree as its rebuild left it */
    int32_t skipped;               /* rt_mesh_measure calls of the current mesh that found every result slot in flight */
} RtMeshQuality;
/* Enqueues the measurement of the current tree on rt_stream()'s stream: behind the update that wrote the boxes, before the next update (which waits for
 * every lane).  No host wait (RtMeshInfo.hostSyncs does not move), no allocation: accumulators, a ring of RT_MESH_QUALITY_SLOTS pinned result slots and
 * their events belong to the upload (RtMeshInfo.allocations).  When every slot is still in flight the call measures nothing, counts that
 * (RtMeshQuality.skipped) and returns RT_OK.  RT_ERR_INVALID without a mesh (rt_upload_bvh releases it) or before the mesh's first rebuild. */
#define RT_MESH_QUALITY_SLOTS 8
int rt_mesh_measure(RtContext *ctx);
/* which = RT_MESH_QUALITY_LATEST: the newest result that has arrived; RT_MESH_QUALITY_BASELINE: the result for the current tree as its last rebuild left
 * it (refitsSinceRebuild == 0).  wait == 0 never blocks (it polls events) and returns RT_ERR_STATE when no such result has arrived; wait != 0 first
 * waits for the newest enqueued measurement.  The doubles are computed on the host from the device's integer sums with rt_bvh_cost's expressions, so
 * the record equals rt_bvh_cost of the host route's nodes12 bit for bit. */
enum { RT_MESH_QUALITY_LATEST = 0, RT_MESH_QUALITY_BASELINE = 1 };
int rt_mesh_quality(RtContext *ctx, int which, int wait, RtMeshQuality *out);
/* One animation step: refit or rebuild, decided on the host from results that have already arrived, then a measurement of the new tree enqueued.
 * mode = RT_MESH_UPDATE_SINGLE: gather under M16 (NULL: identity), as rt_mesh_rebuild / rt_mesh_refit; RT_MESH_UPDATE_PARTS: under the matrix table,
 * as rt_mesh_rebuild_parts / rt_mesh_refit_parts (M16 must be NULL).  The update itself is the one of those four calls: ordering, install, counters and
 * the quantised form's status read are theirs.  rebuildAbove has no default: NaN or a value below 1 is RT_ERR_INVALID.  The rule:
 *   1. no tree: rebuild;
 *   2. no arrived baseline for the current tree and none in flight: rebuild (so a tree built by the plain calls and never measured is replaced once);
 *   3. the baseline in flight, or the baseline or the latest record degenerate: refit;
 *   4. otherwise rebuild exactly when latest.cost > (double)rebuildAbove * baseline.cost, latest = the newest arrived result of the current tree.
 * The call never waits, so the decision at step k rests on the tree of step k - 1 at the latest, and on an older one when the device lags; a caller who
 * synchronises between steps gets a deterministic sequence.  *action (may be NULL) receives RT_MESH_DID_REFIT or RT_MESH_DID_REBUILD.
 * The four plain update calls neither measure nor decide. */
enum { RT_MESH_UPDATE_SINGLE = 0, RT_MESH_UPDATE_PARTS = 1 };
enum { RT_MESH_DID_REFIT = 0, RT_MESH_DID_REBUILD = 1 };
int rt_mesh_update(RtContext *ctx, int mode, const float *M16, float rebuildAbove, int *action);
/* ---- skinning: the positions of the dynamic mesh rewritten on the device from rest positions and a table of bone matrices, so that
 * a host that links only this library animates an articulated model without a kernel of its own and without a host round trip per step.
 * Linear-blend skinning with RT_SKIN_INFLUENCES influences per vertex: boneIdx4 / weights4 hold nVerts x 4 bone indices / weights, and
 *   position[v] = sum over k of weights4[4v+k] * (table[boneIdx4[4v+k]] * rest[v]),
 * evaluated exactly as rt_skin_positions (host side, below) defines it, bit for bit.  Weights need not sum to one and may be negative; an influence of
 * weight +-0 is skipped, and a vertex all of whose influences are skipped keeps its rest position.  1 <= nBones <= RT_MAX_MESH_BONES.
 * Skinning writes rt_mesh_positions() and nothing else: follow it with rt_mesh_refit / rt_mesh_rebuild / rt_mesh_update (or their _parts forms, which
 * apply the part matrices on top), and bound raster draws read the skinned positions where they lie.  Normals are derived from the geometry, as
 * everywhere in the library. */
#define RT_SKIN_INFLUENCES 4
#define RT_MAX_MESH_BONES 65536
/* The skin of the current mesh: rest positions (nVerts x 3 floats; NULL: a device-to-device snapshot of rt_mesh_positions() as it stands on
 * rt_stream()'s stream), bone indices and weights (nVerts x 4 each, nVerts of the current mesh), validated as rt_skin_positions validates them: an
 * index >= nBones (whatever its weight), a non-finite weight, a null table or nBones outside 1 .. RT_MAX_MESH_BONES is RT_ERR_INVALID, with a message.
 * Allocates the rest array, the two tables and the bone table (nBones x 16 floats, 64-byte aligned entries, every matrix the identity) and uploads
 * them; RtMeshInfo.allocations counts them.  May synchronise and allocate; the only call of this group that may.  nBones == 0 releases the skin (the
 * arrays may then be NULL).  A second upload replaces the first.  RT_ERR_INVALID without a mesh; rt_mesh_upload, rt_mesh_upload_parts and
 * rt_upload_bvh release the skin with the mesh.  No tree is needed: skinning before the first rebuild is legal. */
int rt_mesh_skin_upload(RtContext *ctx, const float *rest, const uint16_t *boneIdx4, const float *weights4, int nBones);
/* The bone table: nBones x 16 float32 on the device, column-major, for a caller that writes matrices on the device; writes must be ordered on
 * rt_stream()'s stream, exactly as for rt_mesh_part_matrices.  rt_mesh_set_bones: `count` matrices from host memory into entries first .., copied on
 * that stream, ordered after the work already enqueued on every frame lane and before whatever a lane is given next; a range outside the table:
 * RT_ERR_INVALID.  Bone matrices are not inspected, as the part matrices are not.  RT_ERR_INVALID without a skin. */
int rt_mesh_bones(RtContext *ctx, void **devPtr, size_t *bytes);
int rt_mesh_set_bones(RtContext *ctx, int first, int count, const float *M16s);
/* The device array of rest positions (nVerts x 3 floats) the skin reads.  rt_mesh_morph(ctx, RT_MORPH_TO_REST) blends morph targets into it (below);
 * a caller with a deformer of its own writes it, ordered on rt_stream()'s stream, before a skin.  RT_ERR_INVALID without a skin. */
int rt_mesh_rest_positions(RtContext *ctx, void **devPtr, size_t *bytes);
/* Enqueues positions := skin(rest, tables, bone table) on rt_stream()'s stream, reading the bone table as it stands when the kernel runs.  Ordered as
 * the update calls are: after the frames, queries and bound raster draws already enqueued on any lane, before whatever is enqueued next, by events --
 * so rt_mesh_set_bones, rt_mesh_skin, the update calls, frames and queries take effect in call order wherever frames have moved rt_stream().  No
 * allocation, no host wait (RtMeshInfo.hostSyncs does not move).  RT_ERR_INVALID without a mesh or without a skin. */
int rt_mesh_skin(RtContext *ctx);
/* ---- morph targets: sparse per-vertex deltas blended on the device under a table of weights, the first stage of
 * weights -> morph -> bones -> skin -> rt_mesh_update -> frame, raster preview, picking; a face rig or a corrective-shape rig needs no kernel of the
 * host's own and no host round trip per step.
 * Targets are given the way parts are: targetFirst holds nTargets + 1 non-decreasing entry numbers from 0 to nEntries; entry e of target t
 * (targetFirst[t] <= e < targetFirst[t+1]) moves vertex vertIdx[e] by deltas[3e .. 3e+2].  Empty targets are legal, and a target may name a vertex more
 * than once.  The result is
 *   dst[v] = base[v] + the terms weight[t] * delta of the entries that name v, added one by one in input order,
 * evaluated exactly as rt_morph_positions (host side, below) defines it, bit for bit; an entry whose weight is +-0 is skipped, and a vertex without
 * any other keeps its base position.  1 <= nTargets <= RT_MAX_MORPH_TARGETS.  The device reads the entries in a packed form, slices of 64 vertices
 * padded to their longest entry list (rt_debug_morph_pack, below); RtMorphInfo says what it costs. */
#define RT_MAX_MORPH_TARGETS 65536
/* nSlices: slices of 64 vertices; maxPerVertex: the longest entry list of a vertex; entries: as given; paddedEntries: 16-byte records on the device;
 * bytes: device bytes of the morph's four arrays (records, slice table, base, weight table). */
typedef struct RtMorphInfo { int32_t nVerts, nTargets, nSlices, maxPerVertex; uint64_t entries, paddedEntries, bytes; } RtMorphInfo;
/* The morph targets of the current mesh: base positions (nVerts x 3 floats of the current mesh; NULL: a device-to-device snapshot, as it stands after
 * everything enqueued, of the rest array when the mesh has a skin, else of rt_mesh_positions()) and the targets, validated as rt_morph_positions
 * validates them: a null array, nTargets outside 1 .. RT_MAX_MORPH_TARGETS, a broken targetFirst, a vertIdx >= nVerts or a non-finite delta is
 * RT_ERR_INVALID, with a message; RT_ERR_UNSUPPORTED when the packed form would reach 2^31 records.  Waits for every lane, packs on the host,
 * allocates the base array, the slice table, the records and the weight table (nTargets floats, all zero) and uploads them; RtMeshInfo.allocations and
 * scratchBytes count them.  May synchronise and allocate; the only call of this group that may.  nTargets == 0 releases the morph (the arrays may
 * then be NULL).  A second upload replaces the first.  RT_ERR_INVALID without a mesh; rt_mesh_upload, rt_mesh_upload_parts and rt_upload_bvh
 * release the morph with the mesh; uploading or releasing a skin does not touch it.  No tree is needed. */
int rt_mesh_morph_upload(RtContext *ctx, const float *base, const int32_t *targetFirst, const uint32_t *vertIdx, const float *deltas, int nTargets);
/* The base array (nVerts x 3 floats) and the weight table (nTargets floats, zero after the upload) on the device, for a caller that writes them
 * there; writes must be ordered on rt_stream()'s stream, exactly as for rt_mesh_bones.  rt_mesh_set_morph_weights: `count` weights from host memory
 * into entries first .., copied on that stream, ordered after the work already enqueued on every frame lane and before whatever a lane is given
 * next; a range outside the table: RT_ERR_INVALID.  Weights are not inspected, as bone matrices are not.  RT_ERR_INVALID without a morph. */
int rt_mesh_morph_base(RtContext *ctx, void **devPtr, size_t *bytes);
int rt_mesh_morph_weights(RtContext *ctx, void **devPtr, size_t *bytes);
int rt_mesh_set_morph_weights(RtContext *ctx, int first, int count, const float *weights);
/* Enqueues dst := morph(base, targets, weight table) on rt_stream()'s stream, reading the weight table as it stands when the kernel runs.  Ordered as
 * rt_mesh_skin is, by events, so rt_mesh_set_morph_weights, rt_mesh_morph, rt_mesh_set_bones, rt_mesh_skin, the update calls, frames and queries
 * take effect in call order wherever frames have moved rt_stream(); a morph to the positions also waits for the bound raster draws already
 * enqueued.  No allocation, no host wait (RtMeshInfo.hostSyncs does not move).  RT_ERR_INVALID without a mesh, without a morph, for an unknown dst or
 * for RT_MORPH_TO_REST without a skin. */
#define RT_MORPH_TO_POSITIONS 0   /* writes rt_mesh_positions() */
#define RT_MORPH_TO_REST      1   /* writes rt_mesh_rest_positions(): follow with rt_mesh_skin; RT_ERR_INVALID without a skin */
int rt_mesh_morph(RtContext *ctx, int dst);
/* What the current morph holds.  RT_ERR_INVALID without a morph. */
int rt_mesh_morph_info(RtContext *ctx, RtMorphInfo *out);
/* ---- previous pose and object motion: EXTENSION, not in the reference, whose motion target and reprojection offset are
 * ndcFromWorld(hp, currViewProj) - ndcFromWorld(hp, prevViewProj) with one world point hp (rt.frag, rt_taa.glsl:175-179) -- exact while nothing but the
 * camera moves, and wrong at every pixel a skinned, morphed or re-placed mesh covers.  With motion enabled the mesh keeps its previous pose as rows:
 * prevTris, nTris rows of 48 bytes in the tris12 layout [v0 -][e1 -][e2 -], row i belonging to the same input triangle (rt_mesh_order's order[i]) as row
 * i of the device triangle array and holding, byte for byte, the row that input triangle had in the triangle array before the most recent update.  Rows
 * are copied and permuted, never recomputed, so the previous pose is right however the positions were produced: one matrix, part matrices, skin, morph,
 * or the caller's own kernel.  Off until asked for; while it is off every kernel's output is what it was.
 *   Every update -- rt_mesh_rebuild, rt_mesh_refit, their _parts forms, rt_mesh_update in both modes -- moves the previous pose while motion is enabled:
 * the rows it is about to replace become the previous pose, row i afterwards the old row of input triangle order_new[i] (a refit keeps the order; a
 * rebuild carries the old rows across its reordering).  The mesh's first rebuild has no old rows: the previous pose is then the new rows, zero motion.
 * All of it is part of the update's own ordered work on rt_stream()'s stream: no allocation, no host wait (RtMeshInfo.hostSyncs moves only by the
 * quantised form's status read, as before); frames and queries already enqueued keep the pose they were enqueued with.  rt_mesh_set_positions,
 * rt_mesh_skin and rt_mesh_morph touch neither the triangle array nor the previous pose.
 *   Frames: while the installed scene is the dynamic mesh's, motion is enabled and u->useBVH == 1, a primary hit on row tri with barycentrics (a, b) --
 * the u, v rt_pick_pixels returns for that pixel -- takes prevNDC = ndcFromWorld(prevHp, prevViewProj) with prevHp as rt_hit_motion (below) defines it,
 * on both pipelines; hp, RT_TARGET_GPOS, RT_TARGET_GNRM, the miss rule ((4, 4) under cameraMoved), resolveTAA, the batching rule of rt_render_frames
 * and the tile-parallel exchange are unchanged, and a frame changes no mesh state.  The hybrid scene (RT_SCENE_HYBRID) keeps the reference's motion.
 * rt_render_frame(s) take cameraMoved from the caller and never latch: render the frame after an update with cameraMoved = 1, so that the resolve
 * reprojects, and call rt_mesh_motion_latch when the mesh comes to rest.  rt_render_ray / rt_render_ray_frames keep their FrameState inside the
 * context and do it themselves: the context remembers "an update since the last latch"; a frame rendered in that state gets cameraMoved = 1 (and with
 * it the moving jitter scale) even under an unchanged camera, and behind that frame the call latches; rt_render_ray_frames renders its first frame
 * that way and batches the rest.  With motion disabled none of these entry points changes. */
/* on != 0: allocates prevTris and the scratch a rebuild carries old rows across in (nTris rows each; RtMeshInfo.allocations and scratchBytes count
 * them) and, if the mesh has a tree, latches.  on == 0 releases both.  May synchronise and allocate; the only call of this group that may.  No tree is
 * needed to enable.  RT_ERR_INVALID without a mesh; rt_mesh_upload, rt_mesh_upload_parts and rt_upload_bvh release it with the mesh. */
int rt_mesh_motion_enable(RtContext *ctx, int on);
/* previous pose := current pose.  Enqueued on rt_stream()'s stream and ordered exactly as the update calls are: after the frames and queries already
 * enqueued on every lane, before whatever is enqueued next, by events.  No allocation, no host wait.  RT_ERR_INVALID without a mesh, without motion
 * enabled, or before the mesh's first rebuild. */
int rt_mesh_motion_latch(RtContext *ctx);
/* Where each hit point was in the previous pose: for the RtHit and points outputs of rt_trace_rays (points = origin + dir * t), rt_trace_scene_rays or
 * rt_pick_pixels, prevPoints (3 floats per hit) equals rt_hit_motion's prevPoints bit for bit under the device's two triangle arrays as they stand when
 * the kernel runs; zeros for a prim outside [0, nTris) -- a miss, an analytic hit, a stale value -- with nothing read out of bounds.  Device pointers,
 * hits 16-byte aligned; enqueued on rt_stream()'s stream like rt_mesh_hit_parts: no allocation, no host wait.  RT_ERR_INVALID without a mesh, without
 * motion enabled, or before the first rebuild.  _host: the same with host pointers, staged through the context's buffer; synchronises. */
int rt_mesh_hit_prev_points(RtContext *ctx, const RtHit *hits, const float *points, int n, float *prevPoints);
int rt_mesh_hit_prev_points_host(RtContext *ctx, const RtHit *hits, const float *points, int n, float *prevPoints);
/* ---- smooth vertex normals: EXTENSION, not in the reference, which shades every mesh hit with the triangle's own normal
 * normalize(cross(e1, e2)) (triHit, rt_bvh.glsl:168) -- right for a static scan, faceted on an articulated model, with facets that crawl as it deforms.
 * With normals enabled the mesh keeps, on the device, one area-weighted normal per vertex and the three corner normals of every row of the triangle
 * array (nrmRows: nTris rows of 48 bytes, three float4 (nx, ny, nz, 0), row i beside row i of the triangle array, its corners those of input triangle
 * rt_mesh_order's order[i]), both exactly as rt_vertex_normals (below) defines them, bit for bit.  They are computed from the rows, so they are
 * world-space normals and right however the positions were produced: one matrix, part matrices, skin, morph, or the caller's own kernel.  Off until
 * asked for; while it is off every kernel's output is what it was.  Hard edges are the caller's to make, by duplicating vertices.
 *   Every update -- rt_mesh_rebuild, rt_mesh_refit, their _parts forms, rt_mesh_update in both modes -- recomputes them behind its new rows while normals
 * are enabled, as part of its own ordered work on rt_stream()'s stream (a rebuild derives the order array for itself first): no allocation, no host
 * wait (RtMeshInfo.hostSyncs moves only by the quantised form's status read, as before); frames and queries already enqueued keep the normals they were
 * enqueued with.  rt_mesh_set_positions, rt_mesh_skin, rt_mesh_morph and rt_mesh_motion_latch do not touch them.
 *   Frames: while the installed scene is the dynamic mesh's, normals are enabled and u->useBVH == 1, the normal of a mesh hit -- the primary hit and the
 * bounce hit, on both pipelines -- is the smooth one: with (a, b) the hit's barycentrics on its row, computed with the operations of rt_pick_pixels' u, v
 * in their order, it is what rt_hit_normals (below) defines from the row's three corner normals.  So RT_TARGET_GNRM, direct light, AO, the bounce and
 * its direct light use it wherever the reference uses h.n, and rt_mesh_hit_normals on a pixel's pick is that pixel's GNRM: the target holds the
 * halves of exactly those floats (the reference's second normalize(h.n) in front of the store is not applied to a normal that is already the definition's).  A flat region -- three bit-equal corner normals -- shades with exactly the reference's bits.  Traversal, hp, RT_TARGET_GPOS, RT_TARGET_MOTION,
 * resolveTAA and the miss rule are unchanged.  The face normal stays in: rt_trace_rays' and rt_pick_pixels' optional normal outputs, the hybrid scene
 * (RT_SCENE_HYBRID) and the analytic scene, and the raster preview.  Known, not solved: ray origins are offset along the smooth normal, as the
 * reference offsets along h.n; at a grazing silhouette that can start a ray under a neighbouring facet. */
/* incidences: index-buffer entries (3 nTris); paddedEntries: 4-byte entries of the packed adjacency on the device; bytes: device bytes of the five arrays
 * (adjacency, its slice table, face vectors, vertex normals, nrmRows). */
typedef struct RtNormalInfo { int32_t nVerts, nTris, nSlices, maxPerVertex; uint64_t incidences, paddedEntries, bytes; } RtNormalInfo;
/* on != 0: waits for every lane, reads the mesh's index buffer back, packs the vertex -> triangle adjacency on the host (rt_debug_normal_pack, below),
 * allocates it, the face vectors, the vertex normals and nrmRows (RtMeshInfo.allocations and scratchBytes count them) and, if the mesh has a tree,
 * computes the normals at once.  on == 0 releases everything.  May synchronise and allocate; the only call of this group that may.  No tree is needed
 * to enable.  RT_ERR_INVALID without a mesh; RT_ERR_UNSUPPORTED when the packed adjacency would reach 2^31 entries; rt_mesh_upload,
 * rt_mesh_upload_parts and rt_upload_bvh release it with the mesh. */
int rt_mesh_normals_enable(RtContext *ctx, int on);
/* The device array of vertex normals: nVerts x 4 floats (nx, ny, nz, 0), written on rt_stream()'s stream by the update calls: order reads of it there.
 * RT_ERR_INVALID without a mesh or without normals enabled. */
int rt_mesh_vertex_normals(RtContext *ctx, void **devPtr, size_t *bytes);
/* The shading normal of each hit: for the RtHit outputs of rt_trace_rays, rt_trace_scene_rays or rt_pick_pixels, normals (3 floats per hit) equals
 * rt_hit_normals' out3 bit for bit under the device's triangle array and normals as they stand when the kernel runs; zeros for a prim outside
 * [0, nTris) -- a miss, an analytic hit, a stale value -- with nothing read out of bounds.  Device pointers, hits 16-byte aligned; enqueued on
 * rt_stream()'s stream like rt_mesh_hit_prev_points: no allocation, no host wait.  RT_ERR_INVALID without a mesh, without normals enabled, or before
 * the first rebuild.  _host: the same with host pointers, staged through the context's buffer; synchronises. */
int rt_mesh_hit_normals(RtContext *ctx, const RtHit *hits, int n, float *normals);
int rt_mesh_hit_normals_host(RtContext *ctx, const RtHit *hits, int n, float *normals);
/* ---- per-vertex colours: EXTENSION, not in the reference, which shades every mesh hit with the constant albedo 0.85 (directLightBVH,
 * rt_lighting.glsl) -- right for its one grey model, wrong for several parts in one scene.  With colours enabled the mesh keeps, on the device, one colour
 * per vertex (nVerts float4 (r, g, b, 0): linear RGB albedo, initialised to 0.85) and the three corner colours of every row of the triangle array
 * (colRows: nTris rows of 48 bytes, three float4 (r, g, b, 0), row i beside row i of the triangle array, its corners those of input triangle
 * rt_mesh_order's order[i]), exactly as rt_color_rows (below) defines them.  Off until asked for; while it is off every kernel's output is what it was.
 *   Every update -- rt_mesh_rebuild, rt_mesh_refit, their _parts forms, rt_mesh_update in both modes -- gathers the rows again behind its new rows while
 * colours are enabled, as part of its own ordered work on rt_stream()'s stream (a rebuild derives the order array for itself first): no allocation, no
 * host wait; frames and queries already enqueued keep the colours they were enqueued with.  Writing colours does not touch the rows: an update or
 * rt_mesh_colors_refresh does.
 *   Frames: while the installed scene is the dynamic mesh's, colours are enabled and u->useBVH == 1, the albedo of a mesh hit is what rt_hit_colors
 * (below) defines at the hit's barycentrics (those of rt_pick_pixels' u, v): the primary hit's colour is the albedo of its direct light (diffuse term and
 * sky term) and the factor of its bounce; the bounce hit's colour is the albedo of the bounce hit's direct light -- a red wall tints the floor beside it.
 * specStrength 0.25 and gloss 32 stay constants.  No ray, no geometry, no normal, RT_TARGET_GPOS / GNRM / MOTION, resolveTAA and the miss rule change.
 * A mesh whose colours are all 0.85 renders bit for bit as with colours disabled.  Out of scope: per-vertex specular and gloss (textures and UVs: below),
 * colours in the hybrid scene (RT_SCENE_HYBRID), the analytic scene and the raster preview (which keeps its draw and part colours), colours read from
 * .obj files. */
/* on != 0: waits for every lane, allocates the vertex colours (every vertex (0.85, 0.85, 0.85, 0)) and colRows (RtMeshInfo.allocations and scratchBytes
 * count both) and, if the mesh has a tree, fills the rows at once.  on == 0 releases both.  May synchronise and allocate; the only call of this group
 * that may.  No tree is needed to enable.  on != 0 while colours are enabled changes nothing: the colours and the rows stay, nothing is allocated (disable
 * first to start again from 0.85).  RT_ERR_INVALID without a mesh; rt_mesh_upload, rt_mesh_upload_parts and rt_upload_bvh release them with the
 * mesh. */
int rt_mesh_colors_enable(RtContext *ctx, int on);
/* The device array of vertex colours: nVerts x 4 floats (r, g, b, 0).  The caller may write it on rt_stream()'s stream; device-written colours are taken
 * as they are.  RT_ERR_INVALID without a mesh or without colours enabled. */
int rt_mesh_colors(RtContext *ctx, void **devPtr, size_t *bytes);
/* Colours first .. first + count - 1 from rgb3 (3 floats per vertex, host memory, copied before the call returns), written and ordered like
 * rt_mesh_set_bones: behind everything enqueued on any lane, before whatever a lane is given next; as there, the copy leaves pageable memory, so the
 * host may spend the copy's time in the call.  RT_ERR_INVALID without a mesh or colours, for a
 * range outside [0, nVerts], a null rgb3 with count > 0, or a component that is non-finite or negative.  Does not touch the rows. */
int rt_mesh_set_colors(RtContext *ctx, const float *rgb3, int first, int count);
/* The row gather alone (k_corner_rows<ColorAttr>), for a caller who changed colours and not positions; enqueued and ordered exactly as rt_mesh_motion_latch is: no
 * allocation, no host wait.  RT_ERR_INVALID without a mesh, without colours enabled, or before the first rebuild. */
int rt_mesh_colors_refresh(RtContext *ctx);
/* The colour of each hit: for the RtHit outputs of rt_trace_rays, rt_trace_scene_rays or rt_pick_pixels, colors (3 floats per hit) equals rt_hit_colors'
 * out3 bit for bit under the device's colRows as they stand when the kernel runs; zeros for a prim outside [0, nTris) -- a miss, an analytic hit, a stale
 * value -- with nothing read out of bounds.  Device pointers, hits 16-byte aligned; enqueued on rt_stream()'s stream like rt_mesh_hit_normals: no
 * allocation, no host wait.  RT_ERR_INVALID without a mesh, without colours enabled, or before the first rebuild.  _host: the same with host pointers,
 * staged through the context's buffer; synchronises. */
int rt_mesh_hit_colors(RtContext *ctx, const RtHit *hits, int n, float *colors);
int rt_mesh_hit_colors_host(RtContext *ctx, const RtHit *hits, int n, float *colors);
/* ---- UVs and an albedo texture: EXTENSION, not in the reference.  With UVs enabled the mesh keeps, on the device, one UV per vertex
 * (nVerts float2, zeros at first) and the three corner UVs of every row of the triangle array (uvRows: nTris rows of 32 bytes, (u0, v0, u1, v1),
 * (u2, v2, 0, 0), row i beside row i of the triangle array, its corners those of input triangle rt_mesh_order's order[i]), exactly as rt_uv_rows (below)
 * defines them.  A texture is W x H RGBA8 texels (1 <= W, H <= 16384), row 0 at v = 0 (GL upload order), alpha stored and ignored, decoded through a
 * 256-entry table and sampled as rt_sample_texture (below) defines.  Off until asked for; while it is off every kernel's output is what it was.
 *   Every update -- rt_mesh_rebuild, rt_mesh_refit, their _parts forms, rt_mesh_update in both modes -- gathers the UV rows again behind the colours'
 * gather while UVs are enabled, inside its own ordered work on rt_stream()'s stream: no allocation, no host wait.  Writing UVs does not touch the rows:
 * an update or rt_mesh_uvs_refresh does.
 *   Frames: while the installed scene is the dynamic mesh's, UVs are enabled, a texture is present and u->useBVH == 1, the albedo of a mesh hit is
 * base * texel per channel, one rounded product: base is what the hit's albedo was (rt_hit_colors' blend, or 0.85 with colours off), texel is
 * rt_sample_texture at rt_hit_uvs' UV, both at the hit's barycentrics (those of rt_pick_pixels' u, v).  It applies where the colours apply: the primary
 * hit's albedo and bounce factor, and the bounce hit's albedo.  A caller who wants the texture alone enables colours and sets them to 1.  specStrength
 * and gloss stay constants; no ray, normal, RT_TARGET_GPOS / GNRM / MOTION or resolveTAA changes.  An all-255 texture renders bit for bit as no texture.
 * Out of scope: mipmaps and ray differentials, more than one texture (parts share an atlas), alpha and cut-outs, normal / specular / gloss maps,
 * textures in the hybrid scene, the analytic scene and the raster preview. */
enum { RT_TEX_LINEAR = 0, RT_TEX_NEAREST = 1, RT_TEX_REPEAT = 0, RT_TEX_CLAMP = 2, RT_TEX_UNORM = 0, RT_TEX_SRGB = 4 };
#define RT_TEX_MAX_SIZE 16384
/* on != 0: waits for every lane, allocates the vertex UVs (zeros) and uvRows (RtMeshInfo.allocations and scratchBytes count both) and, if the mesh has
 * a tree, fills the rows at once.  on == 0 releases both.  May synchronise and allocate; the only call of the UV group that may.  on != 0 while UVs are
 * enabled changes nothing.  RT_ERR_INVALID without a mesh; rt_mesh_upload, rt_mesh_upload_parts and rt_upload_bvh release them with the mesh. */
int rt_mesh_uvs_enable(RtContext *ctx, int on);
/* The device array of vertex UVs: nVerts x 2 floats.  The caller may write it on rt_stream()'s stream.  RT_ERR_INVALID (outputs cleared) without a
 * mesh or without UVs enabled. */
int rt_mesh_uvs(RtContext *ctx, void **devPtr, size_t *bytes);
/* UVs first .. first + count - 1 from uv2 (2 floats per vertex, host memory, copied before the call returns), ordered like rt_mesh_set_colors.
 * RT_ERR_INVALID without a mesh or UVs, for a range outside [0, nVerts], a null uv2 with count > 0, or a non-finite component (negative values are
 * fine).  Does not touch the rows. */
int rt_mesh_set_uvs(RtContext *ctx, const float *uv2, int first, int count);
/* The row gather alone (k_corner_rows<UvAttr>), ordered exactly as rt_mesh_colors_refresh: no allocation, no host wait.  RT_ERR_INVALID without a mesh, without
 * UVs enabled, or before the first rebuild. */
int rt_mesh_uvs_refresh(RtContext *ctx);
/* The mesh's texture: rgba8 holds W x H texels of 4 bytes, row 0 at v = 0; flags: RT_TEX_* or'ed.  An attachment of its own (the texels and the 1 KB
 * decode table; RtMeshInfo counts them): waits for every lane, may allocate; a second upload of the same size reuses the block.  rgba8 == NULL with
 * W == H == 0 releases it.  RT_ERR_INVALID without a mesh, for a size outside 1 .. RT_TEX_MAX_SIZE, unknown flag bits or a null rgba8 with a size.
 * Released with the mesh. */
int rt_mesh_texture_upload(RtContext *ctx, const uint8_t *rgba8, int W, int H, int flags);
/* The device texels (W * H * 4 bytes), so that a caller can write them on rt_stream()'s stream (video textures): frames and queries read the texels as
 * they stand in stream order, no refresh call is needed.  RT_ERR_INVALID (outputs cleared) without a mesh or a texture. */
int rt_mesh_texture(RtContext *ctx, void **devPtr, size_t *bytes, int *W, int *H);
/* The UV of each hit (uvs: 2 floats per hit, rt_hit_uvs' out2 bit for bit under the device's uvRows) and the texture sample there (texels: 3 floats
 * per hit, rt_sample_texture at that UV, not multiplied by the colour); zeros for a prim outside [0, nTris), nothing read out of bounds.  Pointers,
 * alignment and ordering as rt_mesh_hit_colors.  RT_ERR_INVALID without a mesh, without UVs enabled, before the first rebuild, and for
 * rt_mesh_hit_texels without a texture.  _host: host pointers, staged; synchronises. */
int rt_mesh_hit_uvs(RtContext *ctx, const RtHit *hits, int n, float *uvs);
int rt_mesh_hit_uvs_host(RtContext *ctx, const RtHit *hits, int n, float *uvs);
int rt_mesh_hit_texels(RtContext *ctx, const RtHit *hits, int n, float *texels);
int rt_mesh_hit_texels_host(RtContext *ctx, const RtHit *hits, int n, float *texels);
/* allocations: device / pinned allocations made by the mesh path so far (all of them in rt_mesh_upload, rt_mesh_skin_upload, rt_mesh_morph_upload, rt_mesh_motion_enable, rt_mesh_normals_enable, rt_mesh_colors_enable, rt_mesh_uvs_enable and rt_mesh_texture_upload); hostSyncs: host waits made by rt_mesh_rebuild and rt_mesh_refit. */
typedef struct RtMeshInfo { int32_t nVerts, nTris; uint64_t rebuilds, allocations, hostSyncs, scratchBytes, sceneBytes; } RtMeshInfo;
int rt_get_mesh_info(RtContext *ctx, RtMeshInfo *out);
/* Diagnostics: one device scene array, padding included, copied to the host (synchronises) -- for scenes installed by rt_upload_bvh or rt_mesh_rebuild
 * alike; it is what makes the contract above checkable.  *bytes = size of the array (0: absent); dst == NULL only asks for the size; a capacity below
 * it: RT_ERR_INVALID. */
enum { RT_SCENE_ARRAY_TRIS = 0, RT_SCENE_ARRAY_PAIRS = 1, RT_SCENE_ARRAY_NODES2 = 2, RT_SCENE_ARRAY_NODES2W = 3, RT_SCENE_ARRAY_NODES4 = 4,
       RT_SCENE_ARRAY_QNODES4 = 5, RT_SCENE_ARRAY_LEAFBOX = 6,
       /* the optional record forms of rt_upload_bvh (RT_FUSED, RT_IMPLICIT): fused hubs; implicit two-child records, pair records, four-wide records,
        * quantised four-wide records and leaf boxes */
       RT_SCENE_ARRAY_FUSED = 7, RT_SCENE_ARRAY_IMPL_NODES2 = 8, RT_SCENE_ARRAY_IMPL_PAIRS = 9, RT_SCENE_ARRAY_IMPL_NODES4 = 10,
       RT_SCENE_ARRAY_IMPL_QNODES4 = 11, RT_SCENE_ARRAY_IMPL_LEAFBOX = 12,
       /* the dynamic mesh's previous pose (rt_mesh_motion_enable): nTris rows of 48 bytes, no padding; size 0 while motion is not enabled */
       RT_SCENE_ARRAY_PREV_TRIS = 13,
       /* the dynamic mesh's corner normals (rt_mesh_normals_enable): nTris rows of 48 bytes, no padding; size 0 while normals are not enabled */
       RT_SCENE_ARRAY_NORMAL_ROWS = 14,
       /* the dynamic mesh's corner colours (rt_mesh_colors_enable): nTris rows of 48 bytes, no padding; size 0 while colours are not enabled */
       RT_SCENE_ARRAY_COLOR_ROWS = 15,
       /* the dynamic mesh's corner UVs (rt_mesh_uvs_enable): nTris rows of 32 bytes, no padding; size 0 while UVs are not enabled */
       RT_SCENE_ARRAY_UV_ROWS = 16 };
int rt_debug_read_scene(RtContext *ctx, int which, void *dst, size_t capacity, size_t *bytes);
/* Diagnostics, host side (no GPU needed, no context): what rt_upload_bvh would put on the device for these arrays -- the packers of
 * csrc/rt_scene_pack.cpp run and one array handed out, with rt_debug_read_scene's `which` values and size-query convention.
 * which = RT_SCENE_ARRAY_PACK_INFO: an RtPackInfo, the scalars the context takes from the packers.  opt == NULL: the options from the environment
 * (RT_QNODES, RT_FUSED, RT_IMPLICIT, RT_ANYHIT_TREE, RT_QNODES_SPARSE_BOXES), as an upload reads them.  Returns rt_upload_bvh's codes for a tree it
 * would refuse (message: rt_last_error(NULL)); RT_ERR_INVALID for null arrays or counts <= 0. */
typedef struct RtPackOptions {
    int32_t qnodes;            /* quantised any-hit nodes: -1 by the size of the tree, 0 never, > 0 always */
    int32_t fused, implicit, anyhitSah, sparseLeafBoxes;   /* booleans */
    int32_t reserved[3];
} RtPackOptions;
typedef struct RtPackInfo {
    int32_t nNodes, nTris, nInner, treeDepth, nWide4, nPairs, nFused, flags;   /* as RtSceneInfo */
    int32_t implicitDepth, implicitRecords;                                     /* implicit records: depth of the leaves, pair records per leaf slot */
    int32_t rootRef, rootRefW, rootRef4, anyStack;
    uint32_t leafBoxMagic;
    int32_t nLeafBoxes;
    int32_t collapsed4;        /* the four-wide tree is the binary tree collapsed (0: the RT_ANYHIT_TREE=sah tree) */
    float rootMin[3], rootMax[3];
    int32_t reserved;
} RtPackInfo;
enum { RT_SCENE_ARRAY_PACK_INFO = 100 };
int rt_debug_pack_scene(const float *nodes12, int nNodes, const float *tris12, int nTris, const RtPackOptions *opt, int which, void *dst, size_t capacity,
                        size_t *bytes);
/* Diagnostics, host side (no GPU needed, no context): what rt_mesh_morph_upload would put on the device for these targets -- the packer of
 * csrc/rt_morph_pack.cpp run and one array handed out, with rt_debug_pack_scene's size-query convention.  Slice s holds vertices
 * 64s .. 64s+63 and as many rows as the longest entry list among them; RT_MORPH_ARRAY_SLICE_FIRST: nSlices + 1 uint32 prefix sums of the rows;
 * RT_MORPH_ARRAY_ENTRIES: sliceFirst[nSlices] * 64 records of 16 bytes {dx, dy, dz (float bits), target (uint32)}, record (sliceFirst[s] + k) * 64 + l
 * the k-th entry of vertex 64s + l in input order, or the pad record {+0, +0, +0, 0xFFFFFFFF} where that vertex has no k-th entry or does not exist;
 * RT_MORPH_ARRAY_INFO: an RtMorphInfo.  Returns rt_mesh_morph_upload's codes for targets it would refuse. */
enum { RT_MORPH_ARRAY_SLICE_FIRST = 0, RT_MORPH_ARRAY_ENTRIES = 1, RT_MORPH_ARRAY_INFO = 100 };
int rt_debug_morph_pack(int nVerts, const int32_t *targetFirst, const uint32_t *vertIdx, const float *deltas, int nTargets, int which, void *dst, size_t capacity,
                        size_t *bytes);
/* Diagnostics, host side (no GPU needed, no context): what rt_mesh_normals_enable would put on the device for this index buffer -- the packer of
 * csrc/rt_normal_pack.cpp run and one array handed out, with rt_debug_pack_scene's size-query convention.  An incidence of vertex v is
 * a pair (k, c) with indices[3k + c] == v, ordered by k, then c.  Slice s holds vertices 64s .. 64s+63 and is as wide as the longest incidence list
 * among them; RT_NORMAL_ARRAY_SLICE_FIRST: nSlices + 1 uint32 prefix sums of width * 64, in entries; RT_NORMAL_ARRAY_ENTRIES: sliceFirst[nSlices] int32,
 * entry sliceFirst[s] + j * 64 + l the input triangle of the j-th incidence of vertex 64s + l, or -1 where that vertex has no j-th incidence or does
 * not exist; RT_NORMAL_ARRAY_INFO: an RtNormalInfo.  RT_ERR_INVALID: null indices, nIdx <= 0 or no multiple of 3, nVerts <= 0, an index >= nVerts, an
 * unknown array; RT_ERR_UNSUPPORTED when the padded entries would reach 2^31. */
enum { RT_NORMAL_ARRAY_SLICE_FIRST = 0, RT_NORMAL_ARRAY_ENTRIES = 1, RT_NORMAL_ARRAY_INFO = 100 };
int rt_debug_normal_pack(const uint32_t *indices, int nIdx, int nVerts, int which, void *dst, size_t capacity, size_t *bytes);
/* Diagnostics, host side (no GPU needed, no context): the ray-queue plan of one launch set of the wavefront pipeline (csrc/rt_wave_plan.cpp,
 * DESIGN.md 16) -- the arithmetic rt_render_frame(s) follows, for checks.  RtWaveOptions: every environment variable of frame rendering as a lane reads it
 * when the context is created; a "...Set" field says whether the variable was set at all where unset has a meaning of its own. */
typedef struct RtWaveOptions {
    uint64_t budgetBytes;      /* RT_QUEUE_BUDGET_MB << 20 */
    uint64_t q2Cap;            /* RT_Q2_CAP (tests: force the overflow path), used when q2CapSet */
    int32_t q2CapSet;
    int32_t q2Predict;         /* RT_Q2_PREDICT: 0 = shadow queue 2 always sized for the worst case */
    int32_t binGi, packetAO, chunksFromSlots;   /* RT_BIN_GI, RT_PACKET_AO, RT_CHUNKS_FROM_SLOTS: booleans */
    int32_t probeMode;         /* RT_BOUNCE_PROBE: 0 never, 1 always, -1 auto */
    int32_t cuSplit;           /* RT_CU_SPLIT: eighths of the CUs for the shading stream, 1..7; 0 = unset */
    int32_t shadePrioritySet, shadePriority;    /* RT_SHADE_PRIORITY */
    int32_t skipTraversalSet, skipTraversal;    /* RT_DEBUG_SKIP_TRAVERSAL */
    int32_t gridPct, gridPctPrimary;            /* RT_GRID_PCT, RT_GRID_PCT_PRIMARY: >= 1; 0 = unset (by the scene and the rank count) */
    int32_t chunkPrimarySet, chunkPrimary;      /* RT_CHUNK_PRIMARY */
    int32_t traceStatsSet, traceStats;          /* RT_TRACE_STATS */
    int32_t traceTimingSet, traceTiming;        /* RT_TRACE_TIMING */
    int32_t reserved;
} RtWaveOptions;
typedef struct RtWavePlanArray { char name[16]; uint64_t offset, bytes; } RtWavePlanArray;   /* name: the WaveBuf member; offset 2^64-1: reserved, not handed out */
typedef struct RtWavePlanArena { uint64_t bytes, allocBytes; int32_t nArrays, reserved; RtWavePlanArray arrays[9]; } RtWavePlanArena;
typedef struct RtWavePlan {
    RtWaveOptions options;     /* as used */
    uint64_t slots, perHit, chBudget;
    uint64_t ch, room;         /* hits per chunk, hits a growing arena is sized for (hits < 0: both chBudget) */
    uint64_t q2Entries;        /* entries per slot of shadow queue 2 at `ch` */
    int32_t spp, ao, S1, S2, L1, deferred;
    int32_t nChunks;           /* hits < 0: the upper bound, every pixel slot a hit */
    int32_t reserved;
    /* frame: per pixel slot.  rays / results: laid out for `ch` hits (bytes), allocated for `room` hits when they grow (allocBytes). */
    RtWavePlanArena frame, rays, results;
} RtWavePlan;
/* slots: pixel slots of the launch set, a multiple of 256.  aoRays: 0 = AO off.  opt == NULL: the options of the environment.  hits < 0: the plan before
 * the hit count is known; else the plan behind its read-back (ignored under RT_CHUNKS_FROM_SLOTS).  share: the share of (hit, sample) pairs whose bounce
 * ray hit in earlier launch sets, 0 = nothing known.  RT_ERR_UNSUPPORTED (message: rt_last_error(NULL)) for a chunk of 2^31 queue entries or more. */
int rt_debug_wave_plan(uint64_t slots, int spp, int aoRays, const RtWaveOptions *opt, int64_t hits, double share, RtWavePlan *out);
/* Diagnostics, host side (no GPU needed, no context): the k_trace build a traversal launch chooses (csrc/rt_trace_build.cpp) -- the other
 * half of what a frame decides before it launches, for checks.  RtTraceOptions: the switches of the environment that choose a build, as tune_from_env reads
 * them (RT_TRACE_TIMING, RT_COOP, RT_NEAR_FIRST, RT_QNODES, RT_FUSED, RT_IMPLICIT, RT_LEAFB, RT_LEAFB_CLOSEST). */
typedef struct RtTraceOptions { int32_t timing, coop, nearFirst, qnodes, fused, impl, leafb, leafbClosest; } RtTraceOptions;
typedef struct RtTraceCase {
    RtTraceOptions opt;
    int32_t any;                          /* any-hit launch (else closest-hit) */
    int32_t stats;                        /* the launch was given sums to add to: a frame's launch under RT_TRACE_STATS / RT_TRACE_TIMING */
    int32_t depth;                        /* of the binary tree (RtSceneInfo.treeDepth) */
    int32_t anyStack;                     /* RtPackInfo.anyStack; 0: not known */
    int32_t q4, wF, iN2, iN4, iQ4;        /* the scene has the record form (RT_SCENE_ARRAY_QNODES4, _FUSED, _IMPL_NODES2, _IMPL_NODES4, _IMPL_QNODES4 are not empty) */
    int32_t reserved;
} RtTraceCase;
enum { RT_TRACE_NODES_WNODESW = 0, RT_TRACE_NODES_WF = 1, RT_TRACE_NODES_IN2 = 2, RT_TRACE_NODES_W4 = 3, RT_TRACE_NODES_Q4 = 4, RT_TRACE_NODES_IN4 = 5,
       RT_TRACE_NODES_IQ4 = 6 };
typedef struct RtTraceBuild {
    uint32_t opt;                         /* RT_BUILD_LEAFB4 .. RT_BUILD_TIMING, unshifted, without RT_BUILD_LAUNCHED */
    int32_t nodes;                        /* RT_TRACE_NODES_*: the node array walked */
    int32_t implPairs, implLeafBoxes;     /* the implicit pair records / leaf boxes are read */
    int32_t stack;                        /* stack entries per lane */
    int32_t reserved;
    uint64_t ldsBytes;                    /* dynamic LDS per workgroup */
} RtTraceBuild;
/* rt_debug_trace_options: the switches of the environment.  rt_debug_trace_build: out[i] = the choice for cases[i], i < n.  rt_debug_trace_builds: the k_trace
 * builds the library holds for a hit kind (their `opt`), at most `capacity` of them into out (NULL: none); returns their number. */
int rt_debug_trace_options(RtTraceOptions *out);
int rt_debug_trace_build(const RtTraceCase *cases, int64_t n, RtTraceBuild *out);
int rt_debug_trace_builds(int any, uint32_t *out, int capacity);
/* Diagnostics, host side (no GPU needed, no context): the arithmetic the shading stages do without a division, as the host compiles it.
 * rt_debug_eval ops 10 (texel decode of code a) and 11 (halton(a, b)) evaluate the same functions on the device.
 *   rt_debug_texel_unorm8: out256[c] = the value the cube-map lookup gives texel code c (c / 255.0f, computed without the division).
 *   rt_debug_halton_pairs: out[2 i], out[2 i + 1] = (halton(f + 1, 2), halton(f + 1, 3)) for f = frame0 + i: what rt_render_frame(s) writes into the frame
 *     descriptor for uFrameIndex = f, and cpOffset (rt_lighting.glsl:280-289) otherwise evaluates per fragment.
 *   rt_debug_div_reciprocal: the word the host stores for divisor d when the largest dividend is nMax: floor(2^32 / d) + 1 when d >= 2 and nMax * d < 2^32,
 *     else 0 = "divide".  rt_debug_div_by: q[i] = n[i] / d and r[i] = n[i] % d as the kernels compute them from (d, rcp).
 *   rt_debug_frame_geom: the tile geometry of a w x h frame on `rank` of `world` for batches of `batch` frames with its three reciprocals (useReciprocals == 0:
 *     all zero, the dividing form); xy != NULL: for every pixel slot of the batch (nLocalTiles * batch * 256) the pixel and sub-frame (x, y, k) that slot maps
 *     to, or (-1, -1, -1) for padding. */
typedef struct RtFrameGeomInfo { int32_t tilesX, tilesY, nTiles, nLocalTiles; uint32_t rcpLocalTiles, rcpTilesX, rcpWorld; } RtFrameGeomInfo;
int rt_debug_texel_unorm8(float *out256);
int rt_debug_halton_pairs(int frame0, int count, float *out);
uint32_t rt_debug_div_reciprocal(uint32_t d, uint64_t nMax);
int rt_debug_div_by(uint32_t d, uint32_t rcp, const uint32_t *n, size_t count, uint32_t *q, uint32_t *r);
int rt_debug_frame_geom(int w, int h, int rank, int world, int batch, int useReciprocals, RtFrameGeomInfo *out, int32_t *xy);
/* Diagnostics, host side (no GPU needed, no context): the candidate order of a batch of frames (csrc/rt_batch_order.hpp, DESIGN.md 4.2 "Frame batching"), as
 * the host compiles the arithmetic of k_primary_interleaved.
 *   rt_debug_batch_tiles: out[v] = the local tile index lt' = k * nLocalTiles + lt that iteration v of that kernel's grid handles, v < batch * nLocalTiles:
 *     the frames k of spatial tile lt follow each other (v = lt * batch + k).
 *   rt_debug_batch_order: a workgroup of `waves` waves noted ballots[k * waves + w] in iteration k < n (bit l: lane l has a candidate).  out[(k * waves + w) *
 *     64 + l] = the position of that candidate relative to the workgroup's first, 0xffffffff where there is none: wave by wave, inside a wave lane by lane,
 *     and a lane's candidates by iteration. */
int rt_debug_batch_tiles(int batch, int nLocalTiles, int32_t *out);
int rt_debug_batch_order(const uint64_t *ballots, int n, int waves, uint32_t *out);
/* Diagnostics, host side (no GPU needed, no context): the beam cull of a batch's primary stage (csrc/rt_beam.hpp, csrc/rt_beam.cpp, DESIGN.md 4.2 "Beam cull"),
 * the functions k_beam_cull runs as the host compiles them.
 *   rt_debug_beam_cull: dead[lt] = 1 where every primary ray of local tile lt, in every one of the `batch` frames (jitters: batch pairs; NULL with batch 1 =
 *     u->jitter), surely misses the tree `records` (nInner two-child records of 16 floats, RT_SCENE_ARRAY_NODES2W; rootRef, rootMin, rootMax from RtPackInfo) --
 *     0 wherever the argument does not apply.  nLocalTiles must be the frame's (rt_debug_frame_geom).  stats, rdInvOut may be NULL; rdInvOut[((k H + y) W + x) 3 ..]
 *     = the reciprocal direction of pixel (x, y) in frame k, the floats the cull and the traversal see.
 *   rt_debug_beam_slab: n boxes (lo, hi) seen from n origins against n intervals [L, H] of reciprocal directions, three floats each: fails[i] = 1 when the slab
 *     test fails for every ray of the interval; bounds[4 i ..] = {tminLo, tminHi, tmaxLo, tmaxHi}, or four NaN where the argument does not apply.
 *   rt_debug_beam_cull_stats: the same four sums over the launch sets the context has culled on the device since the call before (reset != 0 clears them). */
typedef struct RtBeamCullStats { uint64_t tiles, deadTiles, overflowTiles, levels; } RtBeamCullStats;
int rt_debug_beam_cull(const RtUniforms *u, const float *jitters, int batch, int rank, int world, const float *records, int nInner, int rootRef,
                       const float *rootMin, const float *rootMax, uint8_t *dead, int nLocalTiles, RtBeamCullStats *stats, float *rdInvOut);
int rt_debug_beam_slab(int n, const float *ro, const float *lo, const float *hi, const float *L, const float *H, uint8_t *fails, float *bounds);
/*   rt_debug_beam_walk: n beams from the one origin ro against the tree: verdict[i] of the interval (L + 3 i, H + 3 i) = 0 dead, 1 alive, 2 kept because a level
 *     of the walk held more than 64 inner nodes; levels[i] (may be NULL) the levels walked. */
int rt_debug_beam_walk(int n, const float *ro, const float *L, const float *H, const float *records, int nInner, int rootRef, const float *rootMin,
                       const float *rootMax, uint8_t *verdict, int32_t *levels);
int rt_debug_beam_cull_stats(RtContext *ctx, RtBeamCullStats *out, int reset);
/* The dead flags of the launch set the context rendered last, copied to the host: out[nLocalTiles] (synchronises); RT_ERR_STATE when that set was not culled. */
int rt_debug_beam_cull_flags(RtContext *ctx, uint8_t *out, int nLocalTiles);

/* ---------------------------------------------------------------- host side (no GPU needed) */

void rt_default_render_params(RtRenderParams *p);      /* include/render/RenderParams.h:20-238 */
void rt_default_camera(RtCamera *c);                   /* include/app/state.h:129-131 */
void rt_default_bvh_transform(float *M16);             /* include/app/state.h:26-31 */
void rt_camera_view(const RtCamera *c, float *V16);    /* Camera::GetViewMatrix, src/io/Camera.cpp:66-68 */
void rt_camera_proj(const RtCamera *c, float *P16);    /* Camera::GetProjectionMatrix, :71-73 */
void rt_mat4_mul(const float *A16, const float *B16, float *out16);   /* FrameState::beginFrame P*V, frame_state.h:71 */
void rt_generate_jitter(int frameIndex, float *out2);  /* generateJitter2D, src/app/application.cpp:42-47 */
int rt_camera_moved(const float *currVP16, const float *prevVP16);    /* application.cpp:387-395 */

/* The glUniform* block of renderRay, src/render/render.cpp:67-167, with the jitter policy of
 * application.cpp:398-405.  envLoaded = (app.envMapTex != 0). */
void rt_make_uniforms(const RtRenderParams *p, const RtCamera *cam, const float *currView, const float *currViewProj,
                      const float *prevViewProj, int fbw, int fbh, int frameIndex, int cameraMoved, int useBVH,
                      int showMotion, int nodeCount, int triCount, int envLoaded, RtUniforms *out);

/* gather_model_triangles (include/scene/bvh.h:135, src/scene/bvh.cpp:225-246): 9 floats (v0,e1,e2) per
 * index triple after the model matrix.  Returns the triangle count. */
int rt_gather_triangles(const float *positions, const uint32_t *indices, int nIdx, const float *M16, float *outTris9);
/* the same with the vertex count: RT_ERR_INVALID if any index is out of range (use this one for data read from files) */
int rt_gather_triangles_checked(const float *positions, int nVerts, const uint32_t *indices, int nIdx, const float *M16, float *outTris9);

/* The gather of a mesh of parts (see rt_mesh_upload_parts for partFirst), and the definition rt_mesh_rebuild_parts / rt_mesh_refit_parts are tested
 * against: triangle i of part p is what rt_gather_triangles_checked computes under M16s + 16 * p, so the output is the concatenation of per-part
 * rt_gather_triangles_checked calls, bit for bit.  M16s == NULL: the identity for every part.  RT_ERR_INVALID for rt_gather_triangles_checked's
 * causes, nIdx % 3 != 0, a null or broken partFirst or nParts outside 1 .. RT_MAX_MESH_PARTS.  Returns the triangle count. */
int rt_gather_triangles_parts(const float *positions, int nVerts, const uint32_t *indices, int nIdx, const int32_t *partFirst, int nParts, const float *M16s,
                              float *outTris9);

/* Linear-blend skinning on host arrays, and the definition rt_mesh_skin is tested against (see rt_mesh_skin_upload for the arrays; bones16 holds
 * nBones column-major matrices).  For vertex v with rest position p = (x, y, z) the influences k = 0 .. 3 are visited in order: one whose weight is
 * +0 or -0 is skipped; otherwise q = B * p with B = bones16 + 16 * boneIdx4[4v+k] in rt_gather_triangles' expression, per component c
 * (B[c]*x + B[4+c]*y) + (B[8+c]*z + B[12+c]*1), and term = w * q; the first term initialises the sum, later ones are added in order.  A vertex with no
 * unskipped influence keeps its rest position bit for bit.  fp32 throughout, nothing fused: one influence of weight 1 is exactly the gather's
 * transform of the point.  out (nVerts x 3 floats) may be rest.  RT_ERR_INVALID: a null array, nVerts <= 0, nBones outside 1 .. RT_MAX_MESH_BONES, any
 * of the four indices of a vertex >= nBones whatever its weight, a non-finite weight.  Bone matrices are not inspected. */
int rt_skin_positions(const float *rest, int nVerts, const uint16_t *boneIdx4, const float *weights4, const float *bones16, int nBones, float *out);

/* Object motion of hits on the dynamic mesh on host arrays, and the definition rt_mesh_hit_prev_points and the frames' motion target are tested
 * against (see rt_mesh_motion_enable for prevTris12; tris12: the current rows, nTris of 12 floats each; points: 3 floats per hit).  For hit i with
 * p = hits[i].prim in [0, nTris), T = tris12 + 12 p, P = prevTris12 + 12 p, (a, b) = (hits[i].u, hits[i].v) and x = points + 3 i: if the nine geometry
 * floats of P (words 0-2, 4-6, 8-10) are bit-equal to those of T, prev = x bit for bit; otherwise per component c
 *   d = ((P.v0[c] - T.v0[c]) + (P.e1[c] - T.e1[c]) * a) + (P.e2[c] - T.e2[c]) * b,   prev = x + d,
 * fp32 with rounded products and sums, nothing fused.  motion = ndcFromWorld(x, u->currViewProj) - ndcFromWorld(prev, u->prevViewProj) with ndcFromWorld
 * as the frames evaluate it (rt_taa.glsl:175-179): per clip component fma(VP[8+k], z, fma(VP[4+k], y, VP[k] * x)) + VP[12+k], w = max(cw, 1e-6), two
 * divisions.  So a pose that did not change yields exactly the reference's motion, and the delta form keeps precision where the displacement is small
 * against the coordinates.  A prim outside [0, nTris) gives zeros in both outputs and reads nothing.  prevPoints (3 floats per hit) and motion2 (2 per
 * hit): either may be NULL, not both; u may be NULL when motion2 is.  RT_ERR_INVALID: a null required array, nTris <= 0, n < 0.  Needs no GPU. */
int rt_hit_motion(const RtUniforms *u, const float *tris12, const float *prevTris12, int nTris, const RtHit *hits, const float *points, int n, float *prevPoints,
                  float *motion2);

/* Smooth vertex normals on host arrays, and the definitions the device's normals, rt_mesh_hit_normals and the frames' normals are tested against
 * (tris12: the rows of the triangle array, nTris of 12 floats [v0 -][e1 -][e2 -]; order: row -> input triangle, rt_mesh_order's array; indices: the
 * 3 nTris indices of the input triangles).  fp32 in the device's float model: rounded products and sums, fused only where cross and dot write an fmaf.
 *   rt_vertex_normals: the face vector of input triangle k is cross(e1, e2) of the row r with order[r] == k, per component fmaf(a.y, b.z, -(a.z * b.y)),
 * not normalised, so the weighting is by area.  S[v] is the sum of the face vectors of every incidence (k, c) with indices[3k + c] == v, taken with k
 * ascending, then c; the first term initialises the sum; a triangle that names v twice contributes twice.  n[v] = S * (1 / sqrt(dot(S, S))) with
 * dot = fmaf(z, z, fmaf(y, y, x * x)) when dot(S, S) > 0 and finite, else three +0 (an isolated vertex, a zero or non-finite sum).  normals3: 3 floats
 * per vertex.  RT_ERR_INVALID: a null array, nTris <= 0, nVerts <= 0, an index >= nVerts, an order entry outside [0, nTris).
 *   rt_hit_normals: for hit i on row p = hits[i].prim in [0, nTris) with (a, b) = (hits[i].u, hits[i].v), the corner normals n0, n1, n2 are those of
 * vertices indices[3 order[p] + c].  If their nine floats are bit-equal corner to corner the answer is n0 bit for bit, unless n0 is all zero.  Otherwise
 * m = (n0 * ((1 - a) - b) + n1 * a) + n2 * b per component, and the answer is m * (1 / sqrt(dot(m, m))) when dot(m, m) > 0 and finite.  In every
 * remaining case (a zero n0 among bit-equal corners, a zero or non-finite m, NaN barycentrics) it is the row's face normal normalize(cross(e1, e2)),
 * the reference's.  A prim outside [0, nTris) gives zeros and reads nothing.  out3: 3 floats per hit.  RT_ERR_INVALID: a null array, nTris <= 0,
 * nVerts <= 0, n < 0, or a hit row whose order entry or indices are out of range.  Neither needs a GPU. */
int rt_vertex_normals(const float *tris12, const int32_t *order, int nTris, const uint32_t *indices, int nVerts, float *normals3);
int rt_hit_normals(const float *tris12, const int32_t *order, int nTris, const uint32_t *indices, const float *normals3, int nVerts, const RtHit *hits, int n,
                   float *out3);

/* Per-vertex colours on host arrays, and the definitions the device's colRows, rt_mesh_hit_colors and the frames' albedo are tested against (order:
 * row -> input triangle, rt_mesh_order's array; indices: the 3 nTris indices of the input triangles; colors: 3 floats per vertex).  fp32 in the device's
 * float model: every product and sum rounded on its own, no fmaf.
 *   rt_hit_colors: for hit i on row p = hits[i].prim in [0, nTris) with (a, b) = (hits[i].u, hits[i].v), the corner colours c0, c1, c2 are those of
 * vertices indices[3 order[p] + c].  If a or b is not finite the answer is c0 bit for bit.  Otherwise, per channel: c0's value bit for bit where the
 * three corner values of the channel are bit-equal -- so nine floats that are bit-equal corner to corner give c0 bit for bit, and a channel that is
 * constant over the mesh is not disturbed by the others -- and (c0 * ((1 - a) - b) + c1 * a) + c2 * b elsewhere.  Not clamped, not validated: the barycentrics of a real hit give a convex
 * combination up to rounding.  A prim outside [0, nTris) gives zeros and reads nothing.  tris12 (the rows of the triangle array) is not read -- the
 * barycentrics come with the hit -- and may be null.  out3: 3 floats per hit.  RT_ERR_INVALID: a null array, nTris <= 0, nVerts <= 0, n < 0, or a hit
 * row whose order entry or indices are out of range.
 *   rt_color_rows: rows12 gets nTris rows of 12 floats, three (r, g, b, 0); row i holds the corner colours of input triangle order[i].
 * RT_ERR_INVALID: a null array, nTris <= 0, nVerts <= 0, an order entry outside [0, nTris), an index >= nVerts.  Neither needs a GPU. */
int rt_hit_colors(const float *tris12, int nTris, const int32_t *order, const uint32_t *indices, const float *colors, int nVerts, const RtHit *hits, int n,
                  float *out3);
int rt_color_rows(const int32_t *order, const uint32_t *indices, const float *colors, int nTris, int nVerts, float *rows12);

/* UVs and textures on host arrays, and the definitions the device's uvRows, rt_mesh_hit_uvs, rt_mesh_hit_texels and the frames' texel are tested
 * against (order, indices as for rt_hit_colors; uvs: 2 floats per vertex).  fp32 in the device's float model: every product and sum rounded on its own.
 *   rt_uv_rows: out gets nTris rows of 8 floats, (u0, v0, u1, v1), (u2, v2, 0, 0); row i holds the corner UVs of input triangle order[i].
 *   rt_hit_uvs: per component rt_hit_colors' rule on the corner UVs: the first corner when a or b is not finite, the corner value bit for bit where the
 * three are bit-equal, (c0 * ((1 - a) - b) + c1 * a) + c2 * b elsewhere.  A prim outside [0, nTris) gives zeros and reads nothing.  out2: 2 floats per hit.
 *   rt_srgb_table: out[c] for texel code c, with x = c / 255.0: x <= 0.04045 ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4), in double, rounded to float;
 * out[0] == 0 and out[255] == 1 exactly.
 *   rt_sample_texture: out3[i] = the decoded RGB of the texture at uv2[i].  The decode table is texel code c -> c / 255 (RT_TEX_UNORM) or rt_srgb_table's
 * (RT_TEX_SRGB).  Per axis (u and W shown): a non-finite coordinate counts as 0; s = u - floorf(u) (REPEAT) or min(max(u, 0), 1) (CLAMP); LINEAR:
 * x = s * W - 0.5f, fl = floorf(x), f = x - fl, i0 = (int)fl, i1 = i0 + 1; NEAREST: i = (int)floorf(s * W); indices wrapped ((i % W) + W) % W under
 * REPEAT, clamped to [0, W - 1] under CLAMP.  NEAREST answers that texel; LINEAR per channel the decoded value bit for bit where the four decoded values
 * are bit-equal, ((t00 * w00 + t10 * w10) + t01 * w01) + t11 * w11 elsewhere, w00 = (1 - a)(1 - b), w10 = a (1 - b), w01 = (1 - a) b, w11 = a b with
 * (a, b) the two f.  Row 0 of the texels is v = 0.
 * RT_ERR_INVALID: a null array, a negative count, nTris <= 0, nVerts <= 0, an order entry or index out of range, W or H outside 1 .. RT_TEX_MAX_SIZE,
 * unknown flag bits.  None needs a GPU. */
int rt_uv_rows(const int32_t *order, const uint32_t *indices, const float *uvs, int nTris, int nVerts, float *out);
int rt_hit_uvs(const RtHit *hits, int n, const int32_t *order, const uint32_t *indices, const float *uvs, int nTris, int nVerts, float *out2);
int rt_srgb_table(float *out256);
int rt_sample_texture(const uint8_t *texels, int W, int H, int flags, const float *uv2, int n, float *out3);

/* Morph-target blending on host arrays, and the definition rt_mesh_morph is tested against (see rt_mesh_morph_upload for the arrays; weights holds
 * nTargets floats).  For vertex v, acc = base[v]; the entries that name v are visited in input order (ascending target, then position within the
 * target); with w = weights[t], an entry whose w is +0 or -0 is skipped, otherwise per component acc = acc + w * d: fp32, a rounded product and a
 * rounded sum, nothing fused.  A vertex with no unskipped entry keeps its base bits (-0 stays -0).  out (nVerts x 3 floats) may be base.
 * RT_ERR_INVALID: a null array, nVerts <= 0, nTargets outside 1 .. RT_MAX_MORPH_TARGETS, a targetFirst that does not start at 0 or decreases, a
 * vertIdx >= nVerts, a non-finite delta.  base and weights are not inspected. */
int rt_morph_positions(const float *base, int nVerts, const int32_t *targetFirst, const uint32_t *vertIdx, const float *deltas, int nTargets, const float *weights,
                       float *out);

/* build_bvh (include/scene/bvh.h:102, src/scene/bvh.cpp:94-137) + the packing half of upload_bvh_tbo
 * (:147-204).  nodes12 needs room for 2*nTris*12 floats, tris12 for nTris*12.  Returns the node count. */
int rt_build_bvh(const float *tris9, int nTris, float *nodes12, float *tris12);
/* rt_build_bvh (bit for bit the same nodes12 / tris12) plus order[i] = the input triangle that became row i of tris12: maps a query's
 * prim back to the mesh.  order needs room for nTris entries. */
int rt_build_bvh_order(const float *tris9, int nTris, float *nodes12, float *tris12, int32_t *order);
/* Refit on host arrays, and the definition rt_mesh_refit is tested against.  nodes12 (nNodes rows) / tris12 / order as rt_build_bvh_order produced them
 * (or rt_build_bvh_gpu plus rt_mesh_order); tris9 the new triangles in input order.  Rewrites row i of tris12 from triangle order[i] and the six bounds
 * floats of every node: min / max over the triangles of its range of the corners v0, v0 + e1, v0 + e2.  Links, first and count stay untouched.
 * The reduction orders floats as the device builder's sortable keys do: -0 lies below +0 (std::min / std::max would keep whichever came first).
 * Coordinates are finite and below 1e30 in magnitude, as for the builders.  RT_ERR_INVALID: a null array, counts <= 0, order not a permutation of
 * 0 .. nTris-1, or nodes that are not a tree in pre-order whose leaf ranges cover every row once.  With rt_upload_bvh it is a refit for hosts that
 * build on the CPU.  Returns RT_OK. */
int rt_refit_bvh(const float *tris9, int nTris, const int32_t *order, float *nodes12, int nNodes, float *tris12);
/* The quality metric of a tree, and the definition rt_mesh_quality is tested against.  nodes12 as rt_build_bvh, rt_build_bvh_gpu and rt_refit_bvh produce
 * them: min in floats 0-2, max in floats 4-6, count in float 9 (> 0: a leaf).  Per node d = max - min in fp32, widened to double, half-area
 * a = (dx*dy + dy*dz) + dz*dx (exact products; fp32 would overflow).  With A = node 0's half-area = m * 2^e (frexp), q = (uint64) floor(ldexp(a, 32 - e))
 * <= 2^32; innerQ = sum of q over inner nodes, leafQ = sum of q * count over leaves, inner = ldexp((double)innerQ, e - 32) / A, leaf likewise,
 * cost = inner + leaf.  Only integers are summed over nodes, so the result depends on the set of nodes, not on their order.  Below 2^28 triangles in
 * leaves of at most 8 neither sum can reach 2^64.  A == 0: degenerate = 1, every sum zero.  RT_ERR_INVALID: a null pointer,
 * nNodes <= 0, a negative count, a non-finite bound, a max below its min.  Needs no GPU.  Returns RT_OK. */
int rt_bvh_cost(const float *nodes12, int nNodes, RtBvhCost *out);

/* Stand-in for Model/Mesh + Assimp (include/scene/model.h:105-228) for plain .obj files: v / f records,
 * fan triangulation, negative indices.  Buffers are malloc'ed; release with rt_free. */
int rt_load_obj(const char *path, float **positions, int *nVerts, uint32_t **indices, int *nIdx);
/* rt_load_obj with texture coordinates: v, vt and f v/vt[/vn] records, the same fan triangulation and negative indices.  Vertex k is the k-th distinct
 * (v, vt) pair in order of first use by the faces; a corner without vt gets (0, 0) and pairs as vt = none.  positions: 3 floats per vertex, uvs: 2. */
int rt_load_obj_uv(const char *path, float **positions, float **uvs, int *nVerts, uint32_t **indices, int *nIdx);
/* PNG decode (8-bit RGB / RGBA / grey, non-interlaced; zlib) standing in for stbi_load at cubemap.cpp:40 */
int rt_load_png(const char *path, uint8_t **pixels, int *width, int *height, int *channels);
/* 8-bit PNG writer (zlib), rows top-to-bottom as stored; flipY != 0 writes the last row first, i.e. turns a
 * bottom-up GL image the right way round */
int rt_save_png(const char *path, const uint8_t *pixels, int width, int height, int channels, int flipY);
void rt_free(void *p);

/* The 4x3 cross slicing of loadCubeMapFromCross (src/render/cubemap.cpp:47-91).  faces needs
 * 6*(height/3)^2*channels bytes.  Returns faceSize, 0 if the image is not a valid cross. */
int rt_cubemap_from_cross(const uint8_t *img, int width, int height, int channels, uint8_t *faces);

int rt_sizeof_uniforms(void);
int rt_sizeof_render_params(void);
const char *rt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_MI355_H */
