"""Python host mirror of librt_mi355.so (ctypes over the C ABI of include/rt_mi355.h).

The product is the shared library (HIP kernels + C++17 host code).  This module is plumbing for
tests and bench.py: struct mirrors, thin call wrappers, and a `Renderer` that walks the same steps
as the reference's `Application::mainLoop` -> `renderRay` (src/app/application.cpp:381-459,
src/render/render.cpp:55-243).  It never renders on the CPU: every frame goes through
`rt_render_frame` on a gfx950 device, and loading fails loudly when the library is not built.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os
import types
from pathlib import Path

import numpy as np

from . import meshgen  # noqa: F401  (procedural scene inputs)

_PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = _PKG_DIR / "librt_mi355.so"

RT_OK = 0
RT_ERR_INVALID, RT_ERR_NO_DEVICE, RT_ERR_HIP, RT_ERR_STATE, RT_ERR_UNSUPPORTED, RT_ERR_IO = -1, -2, -3, -4, -5, -6
RT_TARGET_COLOR, RT_TARGET_MOTION, RT_TARGET_GPOS, RT_TARGET_GNRM = 0, 1, 2, 3
RT_FORMAT_F16, RT_FORMAT_F32 = 0, 1
RT_PIPELINE_AUTO, RT_PIPELINE_MEGAKERNEL, RT_PIPELINE_WAVEFRONT = 0, 1, 2
TARGET_CHANNELS = {0: 4, 1: 2, 2: 4, 3: 4}
RT_MAX_STAGES = 14
RT_COMM_ID_BYTES = 128

f32, i32 = C.c_float, C.c_int32


def _fields(spec):
    out = []
    for name, kind in spec:
        if isinstance(kind, tuple):
            out.append((name, kind[0] * kind[1]))
        else:
            out.append((name, kind))
    return out


class _Struct(C.Structure):
    def to_dict(self):
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = list(v) if hasattr(v, "__len__") else v
        return d

    def copy(self):
        other = type(self)()
        C.memmove(C.byref(other), C.byref(self), C.sizeof(self))
        return other


class RtUniforms(_Struct):  # include/rt_mi355.h RtUniforms == shaders/rt/rt_uniforms.glsl:25-177
    _fields_ = _fields([
        ("eps", f32), ("pi", f32), ("inf", f32),
        ("camPos", (f32, 3)), ("camRight", (f32, 3)), ("camUp", (f32, 3)), ("camFwd", (f32, 3)),
        ("tanHalfFov", f32), ("aspect", f32),
        ("frameIndex", i32), ("spp", i32),
        ("resolution", (f32, 2)), ("jitter", (f32, 2)), ("enableJitter", i32),
        ("useBVH", i32), ("nodeCount", i32), ("triCount", i32), ("showMotion", i32),
        ("prevViewProj", (f32, 16)), ("currViewProj", (f32, 16)), ("cameraMoved", i32),
        ("taaStillThresh", f32), ("taaHardMovingThresh", f32),
        ("taaHistoryMinWeight", f32), ("taaHistoryAvgWeight", f32), ("taaHistoryMaxWeight", f32), ("taaHistoryBoxSize", f32),
        ("enableTAA", i32),
        ("giScaleAnalytic", f32), ("giScaleBVH", f32), ("enableGI", i32), ("enableAO", i32), ("aoSamples", i32),
        ("aoRadius", f32), ("aoBias", f32), ("aoMin", f32),
        ("useEnvMap", i32), ("envIntensity", f32),
        ("sunEnabled", i32), ("sunColor", (f32, 3)), ("sunIntensity", f32), ("sunDir", (f32, 3)),
        ("skyEnabled", i32), ("skyColor", (f32, 3)), ("skyIntensity", f32), ("skyUpDir", (f32, 3)),
        ("pointLightEnabled", i32), ("pointLightPos", (f32, 3)), ("pointLightColor", (f32, 3)), ("pointLightIntensity", f32),
        ("matAlbedoColor", (f32, 3)), ("matAlbedoSpecStrength", f32), ("matAlbedoGloss", f32),
        ("matGlassAlbedo", (f32, 3)), ("matGlassIOR", f32), ("matGlassDistortion", f32), ("matGlassEnabled", i32),
        ("matMirrorAlbedo", (f32, 3)), ("matMirrorGloss", f32), ("matMirrorEnabled", i32),
    ])


class RtRenderParams(_Struct):  # include/render/RenderParams.h:14-239
    _fields_ = _fields([
        ("sppPerFrame", i32), ("exposure", f32),
        ("matAlbedoColor", (f32, 3)), ("matAlbedoSpecStrength", f32), ("matAlbedoGloss", f32),
        ("matGlassEnabled", i32), ("matGlassColor", (f32, 3)), ("matGlassIOR", f32), ("matGlassDistortion", f32),
        ("matMirrorEnabled", i32), ("matMirrorColor", (f32, 3)), ("matMirrorGloss", f32),
        ("enableJitter", i32), ("jitterStillScale", f32), ("jitterMovingScale", f32),
        ("enableGI", i32), ("giScaleAnalytic", f32), ("giScaleBVH", f32),
        ("enableEnvMap", i32), ("envMapIntensity", f32),
        ("sunEnabled", i32), ("sunColor", (f32, 3)), ("sunIntensity", f32), ("sunYaw", f32), ("sunPitch", f32),
        ("skyEnabled", i32), ("skyColor", (f32, 3)), ("skyIntensity", f32), ("skyYaw", f32), ("skyPitch", f32),
        ("pointLightEnabled", i32), ("pointLightColor", (f32, 3)), ("pointLightIntensity", f32), ("pointLightPos", (f32, 3)),
        ("pointLightOrbitEnabled", i32), ("pointLightOrbitRadius", f32), ("pointLightOrbitSpeed", f32),
        ("pointLightYaw", f32), ("pointLightPitch", f32),
        ("enableAO", i32), ("aoSamples", i32), ("aoRadius", f32), ("aoBias", f32), ("aoMin", f32),
        ("enableTAA", i32), ("taaStillThresh", f32), ("taaHardMovingThresh", f32), ("taaHistoryMinWeight", f32),
        ("taaHistoryAvgWeight", f32), ("taaHistoryMaxWeight", f32), ("taaHistoryBoxSize", f32),
        ("enableSVGF", i32), ("svgfVarMax", f32), ("svgfKVar", f32), ("svgfKColor", f32), ("svgfKVarMotion", f32),
        ("svgfKColorMotion", f32), ("svgfStrength", f32),
        ("motionScale", f32),
    ])


class RtCamera(_Struct):
    _fields_ = _fields([("pos", (f32, 3)), ("yaw", f32), ("pitch", f32), ("fov", f32), ("aspect", f32)])


class RtCounters(_Struct):
    _fields_ = [(n, C.c_uint64) for n in ("raysClosest", "raysShadow", "raysAnalytic", "nodeFetch", "triFetch", "envLookup", "hitPixels",
                                             "fetchPrimary", "fetchShadow", "fetchAO")]

    @property
    def rays(self):
        return self.raysClosest + self.raysShadow + self.raysAnalytic


class RtDeviceConfig(_Struct):
    _fields_ = _fields([("device", i32), ("rank", i32), ("worldSize", i32), ("pipeline", i32), ("countWork", i32), ("reserved", (i32, 3))])


class RtStageTimes(_Struct):
    _fields_ = [("nStages", i32), ("frames", i32), ("ms", C.c_double * RT_MAX_STAGES), ("launches", C.c_uint64 * RT_MAX_STAGES)]


class RtCommInfo(_Struct):
    _fields_ = [(n, i32) for n in ("commWorld", "commRank", "rank", "worldSize")] + [(n, C.c_uint64) for n in ("gathers", "gatherBytes", "historyExchanges")]


class RtTracedRays(_Struct):
    _fields_ = [(n, C.c_uint64) for n in ("candidatePixels", "hitPixels", "primary", "shadow", "bounce", "bounceShadow", "frames",
                                             "gatherLoadsPrimary", "gatherLoadsShadow", "gatherLoadsBounce",
                                             "mergedLoadsPrimary", "mergedLoadsShadow", "mergedLoadsBounce", "ao", "gatherLoadsAO")]

    @property
    def rays(self):
        return self.primary + self.shadow + self.bounce + self.bounceShadow + self.ao


class RtBounceProbe(_Struct):   # rt_debug_bounce_probe: the bounce probe's counts (RT_BOUNCE_PROBE)
    _fields_ = [(n, C.c_uint64) for n in ("probed", "retraced", "probeLaunches", "closestLaunches")]


class RtDiskSkip(_Struct):   # rt_debug_disk_skip: the disk-light skip of the shading stages
    _fields_ = [(n, C.c_uint64) for n in ("directPairs", "directUnlit", "directSkipped", "directWaves", "directWavesSkipped",
                                             "giPairs", "giUnlit", "giSkipped", "giWaves", "giWavesSkipped")]


class RtGiList(_Struct):   # rt_debug_gi_list: what the bounce-hit generator visited and shaded, and which kernel ran
    _fields_ = [(n, C.c_uint64) for n in ("visited", "shaded", "listedLaunches", "pairLaunches")]


class RtLightMasks(_Struct):   # rt_debug_light_masks: the light-slot liveness masks of the shadow queues (RT_LIGHT_MASKS)
    _fields_ = [(n, C.c_uint64) for n in ("bits1", "bits2", "wordsScanned", "refillPasses", "maskWords1", "maskWords2")]


class RtSceneInfo(_Struct):
    _fields_ = [(n, i32) for n in ("nNodes", "nTris", "nInner", "treeDepth", "nWide4", "nPairs")] + \
               [(n, C.c_uint64) for n in ("bytesNodes2", "bytesNodes4", "bytesPairs", "bytesTris")] + \
               [("nFused", i32), ("flags", i32), ("implicitDepth", i32), ("reserved", i32)]


class RtBvhLayout(_Struct):   # rt_bvh_layout: what the triangle count alone determines
    _fields_ = [(n, i32) for n in ("nTris", "nNodes", "nInner", "treeDepth", "nWide4", "nPairs", "anyStack", "quantised")] + \
               [(n, C.c_uint64) for n in ("bytesNodes2", "bytesNodes4", "bytesPairs", "bytesTris")]


class RtMeshInfo(_Struct):   # rt_get_mesh_info: the dynamic mesh and what its rebuilds cost the host
    _fields_ = [("nVerts", i32), ("nTris", i32)] + [(n, C.c_uint64) for n in ("rebuilds", "allocations", "hostSyncs", "scratchBytes", "sceneBytes")]


class RtMorphInfo(_Struct):   # rt_mesh_morph_info / rt_debug_morph_pack: the morph targets in their packed form
    _fields_ = [(n, i32) for n in ("nVerts", "nTargets", "nSlices", "maxPerVertex")] + [(n, C.c_uint64) for n in ("entries", "paddedEntries", "bytes")]


class RtNormalInfo(_Struct):   # rt_debug_normal_pack: the vertex -> triangle adjacency in its packed form
    _fields_ = [(n, i32) for n in ("nVerts", "nTris", "nSlices", "maxPerVertex")] + [(n, C.c_uint64) for n in ("incidences", "paddedEntries", "bytes")]


class RtBvhCost(_Struct):   # rt_bvh_cost: the quality metric of a tree
    _fields_ = [("innerQ", C.c_uint64), ("leafQ", C.c_uint64)] + [(n, C.c_double) for n in ("rootArea", "inner", "leaf", "cost")] + \
               [(n, i32) for n in ("rootExp", "degenerate", "nInner", "nLeaves")]


class RtMeshQuality(_Struct):   # rt_mesh_quality: one device measurement and the update it measured
    _fields_ = [("cost", RtBvhCost), ("update", C.c_uint64), ("refitsSinceRebuild", i32), ("skipped", i32)]


RT_MESH_QUALITY_SLOTS = 8
RT_MESH_QUALITY_LATEST, RT_MESH_QUALITY_BASELINE = 0, 1
RT_MESH_UPDATE_SINGLE, RT_MESH_UPDATE_PARTS = 0, 1
RT_MESH_DID_REFIT, RT_MESH_DID_REBUILD = 0, 1


# rt_debug_read_scene: the device scene arrays
RT_SCENE_ARRAY_TRIS, RT_SCENE_ARRAY_PAIRS, RT_SCENE_ARRAY_NODES2, RT_SCENE_ARRAY_NODES2W, RT_SCENE_ARRAY_NODES4, RT_SCENE_ARRAY_QNODES4, RT_SCENE_ARRAY_LEAFBOX = range(7)
SCENE_ARRAYS = {"tris": 0, "pairs": 1, "nodes2": 2, "nodes2w": 3, "nodes4": 4, "qnodes4": 5, "leafbox": 6}
# ... and the optional record forms (RT_FUSED, RT_IMPLICIT), which rt_debug_read_scene and rt_debug_pack_scene know as well
SCENE_ARRAYS_OPTIONAL = {"fused": 7, "impl_nodes2": 8, "impl_pairs": 9, "impl_nodes4": 10, "impl_qnodes4": 11, "impl_leafbox": 12}
# ... and the dynamic mesh's previous pose (rt_mesh_motion_enable): nTris rows of 48 bytes, empty while motion is not enabled
RT_SCENE_ARRAY_PREV_TRIS = 13
# ... and its corner normals (rt_mesh_normals_enable): nTris rows of 48 bytes, empty while normals are not enabled
RT_SCENE_ARRAY_NORMAL_ROWS = 14
# ... and its corner colours (rt_mesh_colors_enable): nTris rows of 48 bytes, empty while colours are not enabled
RT_SCENE_ARRAY_COLOR_ROWS = 15
# ... and its corner UVs (rt_mesh_uvs_enable): nTris rows of 32 bytes, empty while UVs are not enabled
RT_SCENE_ARRAY_UV_ROWS = 16
# texture flags (rt_mesh_texture_upload, rt_sample_texture): filter | wrap | encoding
TEX_LINEAR, TEX_NEAREST = 0, 1
TEX_REPEAT, TEX_CLAMP = 0, 2
TEX_UNORM, TEX_SRGB = 0, 4
TEX_MAX_SIZE = 16384
SCENE_ARRAYS_MESH = {"prev tris": 13, "normal rows": 14, "color rows": 15, "uv rows": 16}
MESH_GREY = 0.85   # the albedo of a mesh hit without colours, and of every vertex when colours are enabled
RT_SCENE_ARRAY_PACK_INFO = 100



class RtMemoryInfo(_Struct):
    _fields_ = [(n, C.c_uint64) for n in ("queueArenaBytes", "frameArrayBytes", "hybridArenaBytes", "deviceFreeBytes", "deviceTotalBytes")] + \
               [(n, i32) for n in ("queueArenas", "lanes")]


class RtExtension(_Struct):
    _fields_ = _fields([("giBounces", i32), ("envFilter", i32), ("reserved", (i32, 2))])


RT_SCENE_HYBRID = 2   # RtUniforms.useBVH: the analytic scene + the BVH mesh (extension, not in the reference)
RT_SCENE_QNODES_REJECTED, RT_SCENE_NOT_FUSED, RT_SCENE_IMPLICIT = 1, 2, 4   # RtSceneInfo.flags
# rt_debug_builds: RT_BUILD_* bits of the traversal kernel builds launched (closest-hit half; the any-hit half << RT_BUILD_ANY_SHIFT)
RT_BUILD_BITS = {"k_trace": 0x001, "LEAFB4": 0x002, "STATS": 0x004, "COOP": 0x008, "NEAR": 0x010, "QN1": 0x020, "QN2": 0x040, "FUSE": 0x080,
                 "IMPL": 0x100, "TIMING": 0x200, "PACKETS": 0x400}
RT_BUILD_BOUNCE_PROBE = 0x800   # (any-hit half) not a k_trace build but a path of the frame: the bounce rays were walked any-hit first (Renderer.bounce_probe)
RT_BUILD_ANY_SHIFT = 16


class RtPresentParams(_Struct):  # uniforms of shaders/rt/rt_present.frag:38-50
    _fields_ = _fields([("exposure", f32), ("showMotion", i32), ("motionScale", f32), ("resolution", (f32, 2)), ("varMax", f32), ("kVar", f32),
                        ("kColor", f32), ("kVarMotion", f32), ("kColorMotion", f32), ("svgfStrength", f32), ("enableSVGF", i32)])


RT_MAX_RASTER_MESHES = 8
RT_MAX_MESH_PARTS = 65535   # rt_mesh_upload_parts
RT_SKIN_INFLUENCES, RT_MAX_MESH_BONES = 4, 65536   # rt_mesh_skin_upload
RT_MAX_MORPH_TARGETS = 65536   # rt_mesh_morph_upload
RT_MORPH_TO_POSITIONS, RT_MORPH_TO_REST = 0, 1   # rt_mesh_morph
RT_MORPH_ARRAY_SLICE_FIRST, RT_MORPH_ARRAY_ENTRIES, RT_MORPH_ARRAY_INFO = 0, 1, 100   # rt_debug_morph_pack
RT_NORMAL_ARRAY_SLICE_FIRST, RT_NORMAL_ARRAY_ENTRIES, RT_NORMAL_ARRAY_INFO = 0, 1, 100   # rt_debug_normal_pack
NORMAL_PAD_ENTRY = -1   # an entry of the packed adjacency that stands for no incidence
MORPH_PAD_TARGET = 0xFFFFFFFF   # target of a pad record of the packed entries
RASTER_BACKGROUND = 0xFFFFFFFF   # rt_read_raster primId of a pixel no triangle covers (depth24 0xFFFFFF)
RT_RASTER_BIND_SINGLE, RT_RASTER_BIND_PARTS = 0, 1   # rt_raster_mesh_dynamic


class RtRasterDraw(_Struct):   # one glDrawElements of renderRaster (src/render/render.cpp:244-295)
    _fields_ = _fields([("mesh", i32), ("model", (f32, 16)), ("color", (f32, 3))])


class RtRasterStats(_Struct):
    _fields_ = [(n, C.c_uint64) for n in ("trianglesIn", "trianglesDropped", "trianglesClipped", "trianglesSetUp", "binEntries", "binCapacity",
                                           "rasterBytes")] + [("deviceMs", C.c_double)]


RT_QUERY_CLOSEST, RT_QUERY_ANY = 0, 1   # rt_trace_rays kinds
RT_MULTI_HIT_MAX = 32                    # most records per ray of the multi-hit queries
RT_NEAREST_MULTI_MAX = 32                # most records per point of the proximity queries
RT_QUERY_SKIP_GLASS, RT_QUERY_SKIP_MARKER = 1, 2   # rt_trace_scene_rays flags
# rt_trace_scene_rays / rt_pick_pixels objects: the device's material ids
RT_OBJECT_NONE, RT_OBJECT_FLOOR, RT_OBJECT_ALBEDO_SPHERE, RT_OBJECT_GLASS_SPHERE, RT_OBJECT_MIRROR_SPHERE, RT_OBJECT_POINT_LIGHT, RT_OBJECT_MESH = -1, 0, 1, 2, 3, 4, 5


class RtHit(_Struct):   # one closest-hit answer of rt_trace_rays: t, prim (row of tris12, -1 on a miss), barycentrics u, v
    _fields_ = [("t", C.c_float), ("prim", C.c_int32), ("u", C.c_float), ("v", C.c_float)]


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rt_mi355 error {code}: {msg}")
        self.code = code


_lib = None
_FP = C.POINTER(C.c_float)
_U8P = C.POINTER(C.c_uint8)
_U32P = C.POINTER(C.c_uint32)

# name -> (restype, argtypes); this is also the list of symbols include/rt_mi355.h declares.
SIGNATURES = {
    "rt_create": (C.c_int, [C.POINTER(RtDeviceConfig), C.POINTER(C.c_void_p)]),
    "rt_destroy": (None, [C.c_void_p]),
    "rt_last_error": (C.c_char_p, [C.c_void_p]),
    "rt_upload_bvh": (C.c_int, [C.c_void_p, _FP, C.c_int, _FP, C.c_int]),
    "rt_build_bvh_gpu": (C.c_int, [C.c_void_p, _FP, C.c_int, _FP, _FP]),
    "rt_upload_env": (C.c_int, [C.c_void_p, _U8P, C.c_int, C.c_int]),
    "rt_resize": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "rt_reset_accum": (C.c_int, [C.c_void_p]),
    "rt_frame_index": (C.c_int, [C.c_void_p]),
    "rt_render_frame": (C.c_int, [C.c_void_p, C.POINTER(RtUniforms)]),
    "rt_render_frames": (C.c_int, [C.c_void_p, C.POINTER(RtUniforms), C.c_int]),
    "rt_render_ray": (C.c_int, [C.c_void_p, C.POINTER(RtRenderParams), C.POINTER(RtCamera), C.c_int, C.c_int, _FP, _FP]),
    "rt_set_extension": (C.c_int, [C.c_void_p, C.POINTER(RtExtension)]),
    "rt_render_ray_frames": (C.c_int, [C.c_void_p, C.POINTER(RtRenderParams), C.POINTER(RtCamera), C.c_int, C.c_int, C.c_int]),
    "rt_synchronize": (C.c_int, [C.c_void_p]),
    "rt_read_target": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "rt_write_target": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "rt_make_present_params": (None, [C.POINTER(RtRenderParams), C.c_int, C.c_int, C.c_int, C.POINTER(RtPresentParams)]),
    "rt_present": (C.c_int, [C.c_void_p, C.POINTER(RtPresentParams), _U8P]),
    "rt_history_exchange_buffer": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_history_exchanged": (C.c_int, [C.c_void_p]),
    "rt_present_gathered": (C.c_int, [C.c_void_p, C.POINTER(RtPresentParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _U8P]),
    "rt_local_target": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_gather_block_bytes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]),
    "rt_assemble_gathered": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "rt_raster_mesh": (C.c_int, [C.c_void_p, C.c_int, _FP, C.c_int, _U32P, C.c_int]),
    "rt_raster_scene_draws": (C.c_int, [C.POINTER(RtRenderParams), C.c_int, C.c_int, C.c_int, C.POINTER(RtRasterDraw)]),
    "rt_render_raster": (C.c_int, [C.c_void_p, C.POINTER(RtRasterDraw), C.c_int, _FP, _FP]),
    "rt_read_raster": (C.c_int, [C.c_void_p, _U8P, _U32P, _U32P]),
    "rt_get_raster_stats": (C.c_int, [C.c_void_p, C.POINTER(RtRasterStats)]),
    "rt_debug_raster_bin_capacity": (C.c_int, [C.c_void_p, C.c_uint64]),
    "rt_raster_mesh_dynamic": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "rt_raster_part_colors": (C.c_int, [C.c_void_p, C.c_int, _FP, C.c_int]),
    "rt_raster_targets": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_comm_unique_id": (C.c_int, [C.c_void_p, C.c_size_t]),
    "rt_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rt_comm_destroy": (C.c_int, [C.c_void_p]),
    "rt_gather_frame": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_gathered_frame": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_read_gathered": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "rt_present_last_gathered": (C.c_int, [C.c_void_p, C.POINTER(RtPresentParams), _U8P]),
    "rt_exchange_history": (C.c_int, [C.c_void_p]),
    "rt_comm_info": (C.c_int, [C.c_void_p, C.POINTER(RtCommInfo)]),
    "rt_get_counters": (C.c_int, [C.c_void_p, C.POINTER(RtCounters)]),
    "rt_reset_counters": (C.c_int, [C.c_void_p]),
    "rt_get_scene_info": (C.c_int, [C.c_void_p, C.POINTER(RtSceneInfo)]),
    "rt_get_memory_info": (C.c_int, [C.c_void_p, C.POINTER(RtMemoryInfo)]),
    "rt_get_traced_rays": (C.c_int, [C.c_void_p, C.POINTER(RtTracedRays), C.c_int]),
    "rt_enable_stage_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_get_stage_times": (C.c_int, [C.c_void_p, C.POINTER(RtStageTimes)]),
    "rt_stage_name": (C.c_char_p, [C.c_int]),
    "rt_debug_eval": (C.c_int, [C.c_void_p, C.c_int, _FP, _FP, _FP, _U32P, C.c_int]),
    "rt_debug_trace": (C.c_int, [C.c_void_p, C.c_int, _FP, _FP, _FP, C.c_float, C.c_float, _FP, C.c_int]),
    "rt_debug_builds": (C.c_int, [C.c_void_p, _U32P, C.c_int]),
    "rt_debug_bounce_probe": (C.c_int, [C.c_void_p, C.POINTER(RtBounceProbe), C.c_int]),
    "rt_debug_disk_skip": (C.c_int, [C.c_void_p, C.POINTER(RtDiskSkip), C.c_int]),
    "rt_debug_gi_list": (C.c_int, [C.c_void_p, C.POINTER(RtGiList), C.c_int]),
    "rt_debug_light_masks": (C.c_int, [C.c_void_p, C.POINTER(RtLightMasks), C.c_int]),
    "rt_debug_disk_unlit": (C.c_int, [C.c_void_p, C.POINTER(RtUniforms), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int,
                                      C.POINTER(C.c_uint8), C.POINTER(C.c_float)]),
    "rt_trace_rays": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p,
                                C.c_void_p, C.c_void_p]),
    "rt_trace_rays_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_trace_scene_rays": (C.c_int, [C.c_void_p, C.POINTER(RtUniforms), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_trace_scene_rays_host": (C.c_int, [C.c_void_p, C.POINTER(RtUniforms), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_pick_pixels": (C.c_int, [C.c_void_p, C.POINTER(RtUniforms), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_pick_pixels_host": (C.c_int, [C.c_void_p, C.POINTER(RtUniforms), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_multi_hits": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int,
                                C.c_int, C.c_void_p, C.c_void_p]),
    "rt_trace_rays_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p]),
    "rt_trace_rays_multi_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p]),
    "rt_pick_pixels_multi": (C.c_int, [C.c_void_p, C.POINTER(RtUniforms), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_pick_pixels_multi_host": (C.c_int, [C.c_void_p, C.POINTER(RtUniforms), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_nearest_points": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_query_nearest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_query_nearest_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_nearest_points_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "rt_query_nearest_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_query_nearest_multi_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_debug_nearest_multi_block": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "rt_box_overlaps": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_query_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_query_boxes_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_tri_overlaps": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_query_tris": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_query_tris_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_hull_overlaps": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_query_hulls": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_query_hulls_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_box_corners": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "rt_rect_frusta": (C.c_int, [C.POINTER(RtUniforms), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "rt_pick_rects": (C.c_int, [C.c_void_p, C.POINTER(RtUniforms), C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                C.c_void_p, C.c_void_p]),
    "rt_pick_rects_host": (C.c_int, [C.c_void_p, C.POINTER(RtUniforms), C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "rt_bvh_layout": (C.c_int, [C.c_int, C.POINTER(RtBvhLayout)]),
    "rt_mesh_upload": (C.c_int, [C.c_void_p, _FP, C.c_int, _U32P, C.c_int]),
    "rt_mesh_positions": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_mesh_set_positions": (C.c_int, [C.c_void_p, _FP]),
    "rt_mesh_rebuild": (C.c_int, [C.c_void_p, _FP]),
    "rt_mesh_refit": (C.c_int, [C.c_void_p, _FP]),
    "rt_mesh_refit_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rt_mesh_order": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "rt_mesh_order_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_mesh_upload_parts": (C.c_int, [C.c_void_p, _FP, C.c_int, _U32P, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "rt_mesh_parts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]),
    "rt_mesh_part_matrices": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_mesh_set_part_matrices": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _FP]),
    "rt_mesh_rebuild_parts": (C.c_int, [C.c_void_p]),
    "rt_mesh_refit_parts": (C.c_int, [C.c_void_p]),
    "rt_mesh_hit_parts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_mesh_hit_parts_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "rt_mesh_measure": (C.c_int, [C.c_void_p]),
    "rt_mesh_quality": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(RtMeshQuality)]),
    "rt_mesh_update": (C.c_int, [C.c_void_p, C.c_int, _FP, C.c_float, C.POINTER(C.c_int)]),
    "rt_mesh_skin_upload": (C.c_int, [C.c_void_p, _FP, C.POINTER(C.c_uint16), _FP, C.c_int]),
    "rt_mesh_bones": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_mesh_set_bones": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _FP]),
    "rt_mesh_rest_positions": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_mesh_skin": (C.c_int, [C.c_void_p]),
    "rt_mesh_motion_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_mesh_motion_latch": (C.c_int, [C.c_void_p]),
    "rt_mesh_hit_prev_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rt_mesh_hit_prev_points_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rt_mesh_normals_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_mesh_vertex_normals": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_mesh_hit_normals": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rt_mesh_hit_normals_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rt_vertex_normals": (C.c_int, [_FP, C.POINTER(C.c_int32), C.c_int, _U32P, C.c_int, _FP]),
    "rt_hit_normals": (C.c_int, [_FP, C.POINTER(C.c_int32), C.c_int, _U32P, _FP, C.c_int, C.c_void_p, C.c_int, _FP]),
    "rt_debug_normal_pack": (C.c_int, [_U32P, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rt_mesh_colors_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_mesh_colors": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_mesh_set_colors": (C.c_int, [C.c_void_p, _FP, C.c_int, C.c_int]),
    "rt_mesh_colors_refresh": (C.c_int, [C.c_void_p]),
    "rt_mesh_hit_colors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rt_mesh_hit_colors_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rt_mesh_uvs_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_mesh_uvs": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_mesh_set_uvs": (C.c_int, [C.c_void_p, _FP, C.c_int, C.c_int]),
    "rt_mesh_uvs_refresh": (C.c_int, [C.c_void_p]),
    "rt_mesh_texture_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "rt_mesh_texture": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rt_mesh_hit_uvs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rt_mesh_hit_uvs_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rt_mesh_hit_texels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rt_mesh_hit_texels_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rt_uv_rows": (C.c_int, [C.POINTER(C.c_int32), _U32P, _FP, C.c_int, C.c_int, _FP]),
    "rt_hit_uvs": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), _U32P, _FP, C.c_int, C.c_int, _FP]),
    "rt_srgb_table": (C.c_int, [_FP]),
    "rt_sample_texture": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _FP, C.c_int, _FP]),
    "rt_load_obj_uv": (C.c_int, [C.c_char_p, C.POINTER(_FP), C.POINTER(_FP), C.POINTER(C.c_int), C.POINTER(_U32P), C.POINTER(C.c_int)]),
    "rt_hit_colors": (C.c_int, [_FP, C.c_int, C.POINTER(C.c_int32), _U32P, _FP, C.c_int, C.c_void_p, C.c_int, _FP]),
    "rt_color_rows": (C.c_int, [C.POINTER(C.c_int32), _U32P, _FP, C.c_int, C.c_int, _FP]),
    "rt_hit_motion": (C.c_int, [C.c_void_p, _FP, _FP, C.c_int, C.c_void_p, _FP, C.c_int, _FP, _FP]),
    "rt_mesh_morph_upload": (C.c_int, [C.c_void_p, _FP, C.POINTER(C.c_int32), _U32P, _FP, C.c_int]),
    "rt_mesh_morph_base": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_mesh_morph_weights": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "rt_mesh_set_morph_weights": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _FP]),
    "rt_mesh_morph": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_mesh_morph_info": (C.c_int, [C.c_void_p, C.POINTER(RtMorphInfo)]),
    "rt_get_mesh_info": (C.c_int, [C.c_void_p, C.POINTER(RtMeshInfo)]),
    "rt_debug_read_scene": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rt_default_render_params": (None, [C.POINTER(RtRenderParams)]),
    "rt_default_camera": (None, [C.POINTER(RtCamera)]),
    "rt_default_bvh_transform": (None, [_FP]),
    "rt_camera_view": (None, [C.POINTER(RtCamera), _FP]),
    "rt_camera_proj": (None, [C.POINTER(RtCamera), _FP]),
    "rt_mat4_mul": (None, [_FP, _FP, _FP]),
    "rt_generate_jitter": (None, [C.c_int, _FP]),
    "rt_camera_moved": (C.c_int, [_FP, _FP]),
    "rt_make_uniforms": (None, [C.POINTER(RtRenderParams), C.POINTER(RtCamera), _FP, _FP, _FP] + [C.c_int] * 9 + [C.POINTER(RtUniforms)]),
    "rt_gather_triangles": (C.c_int, [_FP, _U32P, C.c_int, _FP, _FP]),
    "rt_gather_triangles_checked": (C.c_int, [_FP, C.c_int, _U32P, C.c_int, _FP, _FP]),
    "rt_gather_triangles_parts": (C.c_int, [_FP, C.c_int, _U32P, C.c_int, C.POINTER(C.c_int32), C.c_int, _FP, _FP]),
    "rt_skin_positions": (C.c_int, [_FP, C.c_int, C.POINTER(C.c_uint16), _FP, _FP, C.c_int, _FP]),
    "rt_morph_positions": (C.c_int, [_FP, C.c_int, C.POINTER(C.c_int32), _U32P, _FP, C.c_int, _FP, _FP]),
    "rt_build_bvh": (C.c_int, [_FP, C.c_int, _FP, _FP]),
    "rt_build_bvh_order": (C.c_int, [_FP, C.c_int, _FP, _FP, C.POINTER(C.c_int32)]),
    "rt_refit_bvh": (C.c_int, [_FP, C.c_int, C.POINTER(C.c_int32), _FP, C.c_int, _FP]),
    "rt_bvh_cost": (C.c_int, [_FP, C.c_int, C.POINTER(RtBvhCost)]),
    "rt_debug_wave_plan": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_double, C.c_void_p]),   # RtWaveOptions, RtWavePlan: _wave_plan_types
    "rt_debug_trace_options": (C.c_int, [C.c_void_p]),                          # RtTraceOptions, RtTraceCase, RtTraceBuild: _trace_build_types
    "rt_debug_trace_build": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "rt_debug_trace_builds": (C.c_int, [C.c_int, _U32P, C.c_int]),
    "rt_debug_pack_scene": (C.c_int, [_FP, C.c_int, _FP, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rt_debug_morph_pack": (C.c_int, [C.c_int, C.POINTER(C.c_int32), _U32P, _FP, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rt_debug_texel_unorm8": (C.c_int, [_FP]),
    "rt_debug_halton_pairs": (C.c_int, [C.c_int, C.c_int, _FP]),
    "rt_debug_div_reciprocal": (C.c_uint32, [C.c_uint32, C.c_uint64]),
    "rt_debug_div_by": (C.c_int, [C.c_uint32, C.c_uint32, _U32P, C.c_size_t, _U32P, _U32P]),
    "rt_debug_frame_geom": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32)]),   # RtFrameGeomInfo
    "rt_debug_batch_tiles": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "rt_debug_batch_order": (C.c_int, [C.POINTER(C.c_uint64), C.c_int, C.c_int, _U32P]),
    "rt_debug_beam_cull": (C.c_int, [C.POINTER(RtUniforms), _FP, C.c_int, C.c_int, C.c_int, _FP, C.c_int, C.c_int, _FP, _FP, _U8P, C.c_int, C.c_void_p, _FP]),   # RtBeamCullStats
    "rt_debug_beam_slab": (C.c_int, [C.c_int, _FP, _FP, _FP, _FP, _FP, _U8P, _FP]),
    "rt_debug_beam_walk": (C.c_int, [C.c_int, _FP, _FP, _FP, _FP, C.c_int, C.c_int, _FP, _FP, _U8P, C.POINTER(C.c_int32)]),
    "rt_debug_beam_cull_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "rt_debug_beam_cull_flags": (C.c_int, [C.c_void_p, _U8P, C.c_int]),
    "rt_load_obj": (C.c_int, [C.c_char_p, C.POINTER(_FP), C.POINTER(C.c_int), C.POINTER(_U32P), C.POINTER(C.c_int)]),
    "rt_load_png": (C.c_int, [C.c_char_p, C.POINTER(_U8P), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rt_save_png": (C.c_int, [C.c_char_p, _U8P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rt_free": (None, [C.c_void_p]),
    "rt_cubemap_from_cross": (C.c_int, [_U8P, C.c_int, C.c_int, C.c_int, _U8P]),
    "rt_sizeof_uniforms": (C.c_int, []),
    "rt_sizeof_render_params": (C.c_int, []),
    "rt_version": (C.c_char_p, []),
}


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so / libhsa-runtime64.so (same
    SONAMEs as /opt/rocm's, found through libtorch's RPATH under a different file name).  If librt_mi355.so pulled in
    /opt/rocm's copy first, a later `import torch` (FrameGatherer, a user's own code) would load the bundled copy as a
    second runtime and fail with "No HIP GPUs are available".  When a torch wheel with bundled libraries is installed,
    load those first (no `import torch`); librt_mi355.so's NEEDED entries then bind to them by SONAME."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    d = Path(list(spec.submodule_search_locations)[0]) / "lib"
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        f = d / name
        if f.exists():
            try:
                C.CDLL(str(f), mode=C.RTLD_GLOBAL)
            except OSError:
                return


def lib():
    """Load librt_mi355.so (built by `make -C opengl-raytracing_amd` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RtError(RT_ERR_NO_DEVICE, f"{LIB_PATH} is not built; run __graft_entry__.build() (hipcc --offload-arch=gfx950). "
                                        "There is no CPU fallback.")
    _share_torch_hip_runtime()
    L = C.CDLL(str(LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    assert L.rt_sizeof_uniforms() == C.sizeof(RtUniforms), "RtUniforms layout drifted from include/rt_mi355.h"
    assert L.rt_sizeof_render_params() == C.sizeof(RtRenderParams), "RtRenderParams layout drifted"
    _lib = L
    return L


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the library: 128 bytes for rank 0 to hand to every rank's Renderer.comm_init."""
    buf = C.create_string_buffer(RT_COMM_ID_BYTES)
    rc = lib().rt_comm_unique_id(buf, RT_COMM_ID_BYTES)
    if rc != RT_OK:
        raise RtError(rc, (lib().rt_last_error(None) or b"").decode())
    return buf.raw


def _fp(a):
    return a.ctypes.data_as(_FP)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------------ host side
def default_render_params() -> RtRenderParams:
    p = RtRenderParams()
    lib().rt_default_render_params(C.byref(p))
    return p


def default_camera() -> RtCamera:
    c = RtCamera()
    lib().rt_default_camera(C.byref(c))
    return c


def closeup_camera() -> RtCamera:
    """Second camera of SURVEY.md 8d config 2: the mesh fills ~45 % of a 16:9 frame."""
    c = default_camera()
    c.pos[0], c.pos[1], c.pos[2] = -2.0, 1.5, 1.0
    c.yaw, c.pitch = -90.0, 0.0
    return c


def default_bvh_transform() -> np.ndarray:
    m = np.zeros(16, np.float32)
    lib().rt_default_bvh_transform(_fp(m))
    return m


def camera_view(cam) -> np.ndarray:
    m = np.zeros(16, np.float32)
    lib().rt_camera_view(C.byref(cam), _fp(m))
    return m


def camera_proj(cam) -> np.ndarray:
    m = np.zeros(16, np.float32)
    lib().rt_camera_proj(C.byref(cam), _fp(m))
    return m


def mat4_mul(a, b) -> np.ndarray:
    a, b = _f32(a), _f32(b)
    m = np.zeros(16, np.float32)
    lib().rt_mat4_mul(_fp(a), _fp(b), _fp(m))
    return m


def raster_scene_draws(params, ground=0, bunny=1, sphere=2) -> list:
    """renderRaster's draw list (ground, bunny, sphere, point-light marker) for the given mesh slots; a negative slot skips its draw."""
    out = (RtRasterDraw * 4)()
    n = lib().rt_raster_scene_draws(C.byref(params), ground, bunny, sphere, out)
    if n < 0:
        raise RtError(n, "rt_raster_scene_draws: bad arguments")
    return [out[i].copy() for i in range(n)]


def raster_draw(mesh, model=None, color=(1.0, 1.0, 1.0)) -> RtRasterDraw:
    d = RtRasterDraw(mesh=mesh)
    m = np.eye(4, dtype=np.float32).reshape(-1) if model is None else _f32(model).reshape(-1)
    for i in range(16):
        d.model[i] = float(m[i])
    for i in range(3):
        d.color[i] = float(color[i])
    return d


def raster_prim_parts(prim_id, base, part_first):
    """Primitive ids of a raster frame -> (part, tri), int32 arrays of prim_id's shape, for a draw of a slot bound to the dynamic mesh
    (Renderer.raster_mesh_dynamic): base is the number of triangles of the draws before it, part_first the mesh's boundaries (mesh_parts()).  The
    draw's input triangle is prim_id - base; part is the part whose range holds it and tri its index within that part, mesh_hit_parts' meaning
    (part_first[part] + tri indexes the caller's index buffer).  (-1, -1) outside the draw's range and on the background.  Pure numpy."""
    pf = np.asarray(part_first, np.int64).reshape(-1)
    prim = np.asarray(prim_id)
    t = prim.astype(np.int64) - int(base)
    ok = (prim != RASTER_BACKGROUND) & (t >= 0) & (t < pf[-1])
    part = np.searchsorted(pf, np.where(ok, t, 0), "right") - 1
    return np.where(ok, part, -1).astype(np.int32), np.where(ok, t - pf[part], -1).astype(np.int32)


def generate_jitter(frame_index: int) -> np.ndarray:
    j = np.zeros(2, np.float32)
    lib().rt_generate_jitter(frame_index, _fp(j))
    return j


def camera_moved(curr_vp, prev_vp) -> bool:
    a, b = _f32(curr_vp), _f32(prev_vp)
    return bool(lib().rt_camera_moved(_fp(a), _fp(b)))


def make_uniforms(params, cam, view, curr_vp, prev_vp, w, h, frame_index=0, camera_moved=False, use_bvh=False,
                  show_motion=False, node_count=0, tri_count=0, env_loaded=True) -> RtUniforms:
    u = RtUniforms()
    v, c, p = _f32(view), _f32(curr_vp), _f32(prev_vp)
    lib().rt_make_uniforms(C.byref(params), C.byref(cam), _fp(v), _fp(c), _fp(p), int(w), int(h), int(frame_index),
                           int(camera_moved), int(use_bvh), int(show_motion), int(node_count), int(tri_count), int(env_loaded),
                           C.byref(u))
    return u


def make_present_params(params, show_motion, w, h) -> RtPresentParams:
    pp = RtPresentParams()
    lib().rt_make_present_params(C.byref(params), int(show_motion), int(w), int(h), C.byref(pp))
    return pp


def gather_triangles(positions, indices, model=None) -> np.ndarray:
    pos = _f32(positions).reshape(-1)
    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    m = default_bvh_transform() if model is None else _f32(model)
    out = np.zeros((idx.size // 3, 9), np.float32)
    n = lib().rt_gather_triangles_checked(_fp(pos), pos.size // 3, idx.ctypes.data_as(_U32P), idx.size, _fp(m), _fp(out))
    if n < 0:
        raise RtError(n, "rt_gather_triangles: index out of range" if n == RT_ERR_INVALID else "rt_gather_triangles")
    return out[:n]


def gather_triangles_parts(positions, indices, part_first, models=None) -> np.ndarray:
    """The gather of a mesh of parts (rt_gather_triangles_parts): triangle i of part p under models[p] ([nParts,16] column-major; None: the identity
    for every part) -> [nTris,9].  The host definition mesh_rebuild_parts / mesh_refit_parts are tested against."""
    pos = _f32(positions).reshape(-1)
    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    pf = np.ascontiguousarray(part_first, dtype=np.int32).reshape(-1)
    m = None if models is None else _f32(models).reshape(-1)
    if m is not None and m.size != 16 * (pf.size - 1):
        raise RtError(RT_ERR_INVALID, f"gather_triangles_parts: {m.size} floats for {pf.size - 1} matrices")
    out = np.zeros((max(idx.size // 3, 1), 9), np.float32)
    n = lib().rt_gather_triangles_parts(_fp(pos), pos.size // 3, idx.ctypes.data_as(_U32P), idx.size, pf.ctypes.data_as(C.POINTER(C.c_int32)), pf.size - 1,
                                        None if m is None else _fp(m), _fp(out))
    if n < 0:
        raise RtError(n, "rt_gather_triangles_parts: an index out of range, indices that are no triangle list or a broken part table")
    return out[:n]


def _skin_tables(who, n_verts, bone_idx, weights):
    """bone_idx / weights as contiguous uint16 / float32 [n_verts,4]; an index that does not fit 16 bits is refused here, before the cast hides it."""
    bi = np.asarray(bone_idx)
    if bi.size != 4 * n_verts or np.asarray(weights).size != 4 * n_verts:
        raise RtError(RT_ERR_INVALID, f"{who}: {n_verts} vertices need {4 * n_verts} bone indices and weights, got {bi.size} and {np.asarray(weights).size}")
    if bi.size and (bi.min() < 0 or bi.max() > 65535):
        raise RtError(RT_ERR_INVALID, f"{who}: bone indices must lie in 0 .. 65535")
    return np.ascontiguousarray(bi, dtype=np.uint16).reshape(-1, 4), _f32(weights).reshape(-1, 4)


def skin_positions(rest, bone_idx, weights, bones) -> np.ndarray:
    """Linear-blend skinning on the host (rt_skin_positions), the definition Renderer.mesh_skin is tested against: rest [V,3], bone_idx / weights [V,4],
    bones [nBones,16] column-major (or [nBones,4,4] as default_bvh_transform lays one out) -> positions [V,3] float32.  An influence of weight +-0 is
    skipped; a vertex without any other keeps its rest position."""
    p = _f32(rest).reshape(-1, 3)
    b = _f32(bones)
    if b.size % 16:
        raise RtError(RT_ERR_INVALID, "skin_positions: bones must hold 16 floats per matrix")
    b = b.reshape(-1, 16)
    bi, w = _skin_tables("skin_positions", p.shape[0], bone_idx, weights)
    out = np.zeros_like(p)
    rc = lib().rt_skin_positions(_fp(p), p.shape[0], bi.ctypes.data_as(C.POINTER(C.c_uint16)), _fp(w), _fp(b), b.shape[0], _fp(out))
    if rc != RT_OK:
        raise RtError(rc, "rt_skin_positions: no vertices, a bone count outside 1 .. 65536, a bone index out of range or a weight that is not finite")
    return out


def hit_motion(u, tris12, prev_tris12, hits, points, want=("prev", "motion")):
    """Object motion of hits on the dynamic mesh on the host (rt_hit_motion), the definition Renderer.mesh_hit_prev_points and the frames' MOTION
    target are tested against: tris12 / prev_tris12 [T,12] the current and the previous rows, hits a RayHits / SceneHits or its [N,4] float32 record
    array, points [N,3] -> (prev_points [N,3], motion [N,2]) float32.  want names the outputs to compute; the other is None.  u (RtUniforms) may be
    None when motion is not wanted."""
    rec = np.ascontiguousarray(hits.record if isinstance(hits, RayHits) else hits)
    if rec.dtype != np.float32 or rec.ndim != 2 or rec.shape[1] != 4:
        raise RtError(RT_ERR_INVALID, f"hit_motion: records must be float32 [N,4], got {rec.dtype} {rec.shape}")
    t, p = _f32(tris12).reshape(-1, 12), _f32(prev_tris12).reshape(-1, 12)
    x = _f32(points).reshape(-1, 3)
    n = rec.shape[0]
    if p.shape != t.shape or x.shape[0] != n:
        raise RtError(RT_ERR_INVALID, f"hit_motion: {t.shape[0]} current and {p.shape[0]} previous rows, {n} hits and {x.shape[0]} points")
    prev = np.zeros((n, 3), np.float32) if "prev" in want else None
    mo = np.zeros((n, 2), np.float32) if "motion" in want else None
    rc = lib().rt_hit_motion(None if u is None else C.addressof(u), _fp(t), _fp(p), t.shape[0], C.c_void_p(rec.ctypes.data), _fp(x), n,
                             None if prev is None else _fp(prev), None if mo is None else _fp(mo))
    if rc != RT_OK:
        raise RtError(rc, "rt_hit_motion: a null array, no triangles, no output asked for, or motion without uniforms")
    return prev, mo


def _morph_targets(who, target_first, vert_idx, deltas):
    """target_first / vert_idx / deltas as contiguous int32 [T+1] / uint32 [E] / float32 [E,3]; what a cast would hide is refused here, and so is a
    table whose last entry is not the number of entries given, which the library could only take on trust."""
    tf, vi = np.asarray(target_first), np.asarray(vert_idx)
    if tf.ndim != 1 or tf.size < 1 or tf.size - 1 > RT_MAX_MORPH_TARGETS:
        raise RtError(RT_ERR_INVALID, f"{who}: target_first must hold 1 .. {RT_MAX_MORPH_TARGETS} targets' boundaries and the end")
    if tf.min() < 0 or tf.max() >= 2 ** 31 or (vi.size and (vi.min() < 0 or vi.max() >= 2 ** 32)):
        raise RtError(RT_ERR_INVALID, f"{who}: target_first must fit int32 and vert_idx uint32")
    d = _f32(deltas).reshape(-1, 3)
    if int(tf[-1]) != vi.size or d.shape[0] != vi.size:
        raise RtError(RT_ERR_INVALID, f"{who}: target_first ends at {int(tf[-1])}, with {vi.size} vertex indices and {d.shape[0]} deltas")
    return np.ascontiguousarray(tf, dtype=np.int32), np.ascontiguousarray(vi, dtype=np.uint32).reshape(-1), d


_I32P = C.POINTER(C.c_int32)


def morph_positions(base, target_first, vert_idx, deltas, weights) -> np.ndarray:
    """Morph-target blending on the host (rt_morph_positions), the definition Renderer.mesh_morph is tested against: base [V,3]; target t owns entries
    target_first[t] .. target_first[t+1], entry e moves vertex vert_idx[e] by weights[t] * deltas[e]; the terms are added to the base one by one in
    input order -> positions [V,3] float32.  An entry of weight +-0 is skipped; a vertex without any other keeps its base position."""
    p = _f32(base).reshape(-1, 3)
    tf, vi, d = _morph_targets("morph_positions", target_first, vert_idx, deltas)
    w = _f32(weights).reshape(-1)
    if w.size != tf.size - 1:
        raise RtError(RT_ERR_INVALID, f"morph_positions: {tf.size - 1} targets, {w.size} weights")
    out = np.zeros_like(p)
    rc = lib().rt_morph_positions(_fp(p), p.shape[0], tf.ctypes.data_as(_I32P), vi.ctypes.data_as(_U32P), _fp(d), tf.size - 1, _fp(w), _fp(out))
    if rc != RT_OK:
        raise RtError(rc, "rt_morph_positions: no vertices, no targets, a broken target_first, a vertex index out of range or a delta that is not finite")
    return out


def morph_targets_from_dense(deltas):
    """Dense targets [T,V,3] -> (target_first int32 [T+1], vert_idx uint32 [E], deltas float32 [E,3]), the sparse form morph_positions and
    Renderer.mesh_morph_upload take: per target its vertices in ascending order, without the rows whose three components are all +-0."""
    d = _f32(deltas)
    if d.ndim != 3 or d.shape[2] != 3:
        raise RtError(RT_ERR_INVALID, "morph_targets_from_dense: deltas must be [targets, vertices, 3]")
    keep = (d != 0).any(axis=2)
    t, v = np.nonzero(keep)   # row-major: ascending target, then ascending vertex
    first = np.zeros(d.shape[0] + 1, dtype=np.int32)
    np.cumsum(keep.sum(axis=1), out=first[1:])
    return first, v.astype(np.uint32), np.ascontiguousarray(d[t, v])


def debug_morph_pack(n_verts, target_first, vert_idx, deltas) -> dict:
    """What Renderer.mesh_morph_upload would put on the device, without one (rt_debug_morph_pack): "slice_first" uint32 [nSlices+1], "entries" uint32
    [paddedEntries,4] (the delta's float bits and the target; MORPH_PAD_TARGET marks a pad record) and "info", an RtMorphInfo."""
    tf, vi, d = _morph_targets("debug_morph_pack", target_first, vert_idx, deltas)
    args = (int(n_verts), tf.ctypes.data_as(_I32P), vi.ctypes.data_as(_U32P), _fp(d), tf.size - 1)

    def read(which):
        size = C.c_size_t()
        rc = lib().rt_debug_morph_pack(*args, which, None, 0, C.byref(size))
        out = np.zeros(size.value, dtype=np.uint8)
        if rc == RT_OK and size.value:
            rc = lib().rt_debug_morph_pack(*args, which, C.c_void_p(out.ctypes.data), out.size, C.byref(size))
        if rc != RT_OK:
            raise RtError(rc, "rt_debug_morph_pack: targets rt_mesh_morph_upload would refuse" if rc == RT_ERR_INVALID else
                          "rt_debug_morph_pack: the padded entry records reach 2^31")
        return out

    info = RtMorphInfo.from_buffer_copy(read(RT_MORPH_ARRAY_INFO).tobytes())
    return {"info": info, "slice_first": read(RT_MORPH_ARRAY_SLICE_FIRST).view(np.uint32), "entries": read(RT_MORPH_ARRAY_ENTRIES).view(np.uint32).reshape(-1, 4)}


def _normal_mesh(who, tris12, order, indices):
    """tris12 / order / indices as contiguous float32 [T,12] / int32 [T] / uint32 [3T]; what a cast would hide is refused here."""
    t = _f32(tris12).reshape(-1, 12)
    o, ix = np.asarray(order).reshape(-1), np.asarray(indices).reshape(-1)
    if o.size != t.shape[0] or ix.size != 3 * t.shape[0]:
        raise RtError(RT_ERR_INVALID, f"{who}: {t.shape[0]} rows, {o.size} order entries and {ix.size} indices")
    if (o.size and (o.min() < -2 ** 31 or o.max() >= 2 ** 31)) or (ix.size and (ix.min() < 0 or ix.max() >= 2 ** 32)):
        raise RtError(RT_ERR_INVALID, f"{who}: order must fit int32 and indices uint32")
    return t, np.ascontiguousarray(o, dtype=np.int32), np.ascontiguousarray(ix, dtype=np.uint32)


def vertex_normals(tris12, order, indices, n_verts) -> np.ndarray:
    """Area-weighted vertex normals on the host (rt_vertex_normals), the definition Renderer.mesh_vertex_normals is tested against: tris12 [T,12] the
    rows of the triangle array, order [T] row -> input triangle (Renderer.mesh_order), indices the 3T indices of the input triangles -> normals
    [n_verts,3] float32; three +0 for a vertex whose face vectors have no sum with a direction."""
    t, o, ix = _normal_mesh("vertex_normals", tris12, order, indices)
    out = np.zeros((max(int(n_verts), 0), 3), np.float32)
    rc = lib().rt_vertex_normals(_fp(t), o.ctypes.data_as(_I32P), t.shape[0], ix.ctypes.data_as(_U32P), int(n_verts), _fp(out))
    if rc != RT_OK:
        raise RtError(rc, "rt_vertex_normals: no triangles, no vertices, an index out of range or an order entry outside the triangles")
    return out


def hit_normals(tris12, order, indices, normals, hits) -> np.ndarray:
    """Shading normals of hits on the dynamic mesh on the host (rt_hit_normals), the definition Renderer.mesh_hit_normals and the frames' GNRM target
    are tested against: tris12 / order / indices as for vertex_normals, normals [V,3] (or [V,4], the device layout) the vertex normals, hits a
    RayHits / SceneHits or its [N,4] float32 record array -> [N,3] float32; zeros for a prim outside the triangles."""
    rec = np.ascontiguousarray(hits.record if isinstance(hits, RayHits) else hits)
    if rec.dtype != np.float32 or rec.ndim != 2 or rec.shape[1] != 4:
        raise RtError(RT_ERR_INVALID, f"hit_normals: records must be float32 [N,4], got {rec.dtype} {rec.shape}")
    t, o, ix = _normal_mesh("hit_normals", tris12, order, indices)
    nv = _f32(normals)
    if nv.ndim != 2 or nv.shape[1] not in (3, 4):
        raise RtError(RT_ERR_INVALID, f"hit_normals: normals must be [V,3] or [V,4], got {nv.shape}")
    nv = np.ascontiguousarray(nv[:, :3])
    out = np.zeros((rec.shape[0], 3), np.float32)
    rc = lib().rt_hit_normals(_fp(t), o.ctypes.data_as(_I32P), t.shape[0], ix.ctypes.data_as(_U32P), _fp(nv), nv.shape[0], C.c_void_p(rec.ctypes.data),
                              rec.shape[0], _fp(out))
    if rc != RT_OK:
        raise RtError(rc, "rt_hit_normals: no triangles, no vertices, or a hit row whose order entry or indices are out of range")
    return out


def debug_normal_pack(indices, n_verts) -> dict:
    """What Renderer.mesh_normals_enable would put on the device for this index buffer, without one (rt_debug_normal_pack): "slice_first" uint32
    [nSlices+1] in entries, "entries" int32 [paddedEntries] (NORMAL_PAD_ENTRY marks no incidence) and "info", an RtNormalInfo."""
    ix = np.asarray(indices).reshape(-1)
    if ix.size and (ix.min() < 0 or ix.max() >= 2 ** 32):
        raise RtError(RT_ERR_INVALID, "debug_normal_pack: indices must fit uint32")
    ix = np.ascontiguousarray(ix, dtype=np.uint32)
    args = (ix.ctypes.data_as(_U32P), ix.size, int(n_verts))

    def read(which):
        size = C.c_size_t()
        rc = lib().rt_debug_normal_pack(*args, which, None, 0, C.byref(size))
        out = np.zeros(size.value, dtype=np.uint8)
        if rc == RT_OK and size.value:
            rc = lib().rt_debug_normal_pack(*args, which, C.c_void_p(out.ctypes.data), out.size, C.byref(size))
        if rc != RT_OK:
            raise RtError(rc, "rt_debug_normal_pack: an index buffer rt_mesh_normals_enable would refuse" if rc == RT_ERR_INVALID else
                          "rt_debug_normal_pack: the padded adjacency reaches 2^31 entries")
        return out

    info = RtNormalInfo.from_buffer_copy(read(RT_NORMAL_ARRAY_INFO).tobytes())
    return {"info": info, "slice_first": read(RT_NORMAL_ARRAY_SLICE_FIRST).view(np.uint32), "entries": read(RT_NORMAL_ARRAY_ENTRIES).view(np.int32)}


def _color_mesh(who, order, indices, colors):
    """order / indices / colors as contiguous int32 [T] / uint32 [3T] / float32 [V,3] ([V,4], the device layout, is cut); what a cast would hide is
    refused here."""
    o, ix = np.asarray(order).reshape(-1), np.asarray(indices).reshape(-1)
    if ix.size != 3 * o.size:
        raise RtError(RT_ERR_INVALID, f"{who}: {o.size} order entries and {ix.size} indices")
    if (o.size and (o.min() < -2 ** 31 or o.max() >= 2 ** 31)) or (ix.size and (ix.min() < 0 or ix.max() >= 2 ** 32)):
        raise RtError(RT_ERR_INVALID, f"{who}: order must fit int32 and indices uint32")
    cv = _f32(colors)
    if cv.ndim != 2 or cv.shape[1] not in (3, 4):
        raise RtError(RT_ERR_INVALID, f"{who}: colors must be [V,3] or [V,4], got {cv.shape}")
    return np.ascontiguousarray(o, dtype=np.int32), np.ascontiguousarray(ix, dtype=np.uint32), np.ascontiguousarray(cv[:, :3])


def hit_colors(tris12, order, indices, colors, hits) -> np.ndarray:
    """Colours of hits on the dynamic mesh on the host (rt_hit_colors), the definition Renderer.mesh_hit_colors and the frames' albedo are tested
    against: order [T] row -> input triangle (Renderer.mesh_order), indices the 3T indices of the input triangles, colors [V,3] (or [V,4], the device
    layout) the vertex colours, hits a RayHits / SceneHits or its [N,4] float32 record array -> [N,3] float32; zeros for a prim outside the
    triangles.  tris12 (the rows of the triangle array) is not read -- the barycentrics come with the hits -- and may be None."""
    rec = np.ascontiguousarray(hits.record if isinstance(hits, RayHits) else hits)
    if rec.dtype != np.float32 or rec.ndim != 2 or rec.shape[1] != 4:
        raise RtError(RT_ERR_INVALID, f"hit_colors: records must be float32 [N,4], got {rec.dtype} {rec.shape}")
    o, ix, cv = _color_mesh("hit_colors", order, indices, colors)
    t = None if tris12 is None else _f32(tris12).reshape(-1, 12)
    if t is not None and t.shape[0] != o.size:
        raise RtError(RT_ERR_INVALID, f"hit_colors: {t.shape[0]} rows and {o.size} order entries")
    out = np.zeros((rec.shape[0], 3), np.float32)
    rc = lib().rt_hit_colors(None if t is None else _fp(t), o.size, o.ctypes.data_as(_I32P), ix.ctypes.data_as(_U32P), _fp(cv), cv.shape[0],
                             C.c_void_p(rec.ctypes.data), rec.shape[0], _fp(out))
    if rc != RT_OK:
        raise RtError(rc, "rt_hit_colors: no triangles, no vertices, or a hit row whose order entry or indices are out of range")
    return out


def color_rows(order, indices, colors) -> np.ndarray:
    """The device row array of the vertex colours on the host (rt_color_rows), the definition Renderer.mesh_color_rows is tested against -> float32
    [T,12], three (r, g, b, 0) per row; row i holds the corner colours of input triangle order[i]."""
    o, ix, cv = _color_mesh("color_rows", order, indices, colors)
    out = np.zeros((o.size, 12), np.float32)
    rc = lib().rt_color_rows(o.ctypes.data_as(_I32P), ix.ctypes.data_as(_U32P), _fp(cv), o.size, cv.shape[0], _fp(out))
    if rc != RT_OK:
        raise RtError(rc, "rt_color_rows: no triangles, no vertices, an index out of range or an order entry outside the triangles")
    return out


def _uv_mesh(who, order, indices, uvs):
    """order / indices / uvs as contiguous int32 [T] / uint32 [3T] / float32 [V,2]; what a cast would hide is refused here."""
    o, ix = np.asarray(order).reshape(-1), np.asarray(indices).reshape(-1)
    if ix.size != 3 * o.size:
        raise RtError(RT_ERR_INVALID, f"{who}: {o.size} order entries and {ix.size} indices")
    if (o.size and (o.min() < -2 ** 31 or o.max() >= 2 ** 31)) or (ix.size and (ix.min() < 0 or ix.max() >= 2 ** 32)):
        raise RtError(RT_ERR_INVALID, f"{who}: order must fit int32 and indices uint32")
    uv = _f32(uvs)
    if uv.ndim != 2 or uv.shape[1] != 2:
        raise RtError(RT_ERR_INVALID, f"{who}: uvs must be [V,2], got {uv.shape}")
    return np.ascontiguousarray(o, dtype=np.int32), np.ascontiguousarray(ix, dtype=np.uint32), np.ascontiguousarray(uv)


def uv_rows(order, indices, uvs) -> np.ndarray:
    """The device row array of the vertex UVs on the host (rt_uv_rows), the definition Renderer.mesh_uv_rows is tested against -> float32 [T,8],
    (u0, v0, u1, v1), (u2, v2, 0, 0) per row; row i holds the corner UVs of input triangle order[i]."""
    o, ix, uv = _uv_mesh("uv_rows", order, indices, uvs)
    out = np.zeros((o.size, 8), np.float32)
    rc = lib().rt_uv_rows(o.ctypes.data_as(_I32P), ix.ctypes.data_as(_U32P), _fp(uv), o.size, uv.shape[0], _fp(out))
    if rc != RT_OK:
        raise RtError(rc, "rt_uv_rows: no triangles, no vertices, an index out of range or an order entry outside the triangles")
    return out


def hit_uvs(order, indices, uvs, hits) -> np.ndarray:
    """UVs of hits on the dynamic mesh on the host (rt_hit_uvs), the definition Renderer.mesh_hit_uvs is tested against: order [T] row -> input
    triangle (Renderer.mesh_order), indices the 3T indices of the input triangles, uvs [V,2], hits a RayHits / SceneHits or its [N,4] float32 record
    array -> [N,2] float32; zeros for a prim outside the triangles."""
    rec = np.ascontiguousarray(hits.record if isinstance(hits, RayHits) else hits)
    if rec.dtype != np.float32 or rec.ndim != 2 or rec.shape[1] != 4:
        raise RtError(RT_ERR_INVALID, f"hit_uvs: records must be float32 [N,4], got {rec.dtype} {rec.shape}")
    o, ix, uv = _uv_mesh("hit_uvs", order, indices, uvs)
    out = np.zeros((rec.shape[0], 2), np.float32)
    rc = lib().rt_hit_uvs(C.c_void_p(rec.ctypes.data), rec.shape[0], o.ctypes.data_as(_I32P), ix.ctypes.data_as(_U32P), _fp(uv), o.size, uv.shape[0], _fp(out))
    if rc != RT_OK:
        raise RtError(rc, "rt_hit_uvs: no triangles, no vertices, or a hit row whose order entry or indices are out of range")
    return out


def srgb_table() -> np.ndarray:
    """The sRGB decode of the 256 texel codes (rt_srgb_table): the table of an RT_TEX_SRGB texture."""
    out = np.zeros(256, np.float32)
    rc = lib().rt_srgb_table(_fp(out))
    if rc != RT_OK:
        raise RtError(rc, "rt_srgb_table")
    return out


def _texels(who, texels):
    """texels as a contiguous uint8 [H,W,4] array; what a cast would hide is refused here."""
    t = np.asarray(texels)
    if t.dtype != np.uint8 or t.ndim != 3 or t.shape[2] != 4:
        raise RtError(RT_ERR_INVALID, f"{who}: texels must be uint8 [H,W,4] (row 0 at v = 0), got {t.dtype} {t.shape}")
    return np.ascontiguousarray(t)


def sample_texture(texels, flags, uvs) -> np.ndarray:
    """The texture sample on the host (rt_sample_texture), the definition Renderer.mesh_hit_texels and the frames' texel are tested against: texels
    uint8 [H,W,4] with row 0 at v = 0, flags TEX_* or'ed, uvs [N,2] -> float32 [N,3], the decoded RGB."""
    t = _texels("sample_texture", texels)
    uv = _f32(uvs)
    if uv.ndim != 2 or uv.shape[1] != 2:
        raise RtError(RT_ERR_INVALID, f"sample_texture: uvs must be [N,2], got {uv.shape}")
    uv = np.ascontiguousarray(uv)
    out = np.zeros((uv.shape[0], 3), np.float32)
    rc = lib().rt_sample_texture(C.c_void_p(t.ctypes.data), t.shape[1], t.shape[0], int(flags), _fp(uv), uv.shape[0], _fp(out))
    if rc != RT_OK:
        raise RtError(rc, f"rt_sample_texture: a size outside 1 .. {TEX_MAX_SIZE} or unknown flag bits")
    return out


def vertex_colors_from_parts(indices, part_first, rgb, n_verts) -> np.ndarray:
    """Vertex colours [n_verts,3] float32 from one colour per part (pure numpy), the bridge from rt_raster_part_colors' table: part p owns input
    triangles part_first[p] .. part_first[p+1] (Renderer.mesh_upload_parts' table) and every vertex they name gets rgb[p]; on a vertex that parts
    share the later part wins; a vertex no triangle names keeps MESH_GREY."""
    ix = np.asarray(indices).reshape(-1, 3)
    pf = np.asarray(part_first).reshape(-1)
    col = _f32(rgb).reshape(-1, 3)
    if pf.size != col.shape[0] + 1 or pf[0] != 0 or pf[-1] != ix.shape[0] or np.any(np.diff(pf) < 0):
        raise RtError(RT_ERR_INVALID, f"vertex_colors_from_parts: {col.shape[0]} colours, a part table of {pf.size} entries over {ix.shape[0]} triangles")
    if ix.size and (ix.min() < 0 or ix.max() >= int(n_verts)):
        raise RtError(RT_ERR_INVALID, "vertex_colors_from_parts: an index outside the vertices")
    out = np.full((int(n_verts), 3), MESH_GREY, np.float32)
    for p in range(col.shape[0]):
        out[ix[int(pf[p]):int(pf[p + 1])].reshape(-1)] = col[p]
    return out


def bvh_layout(n_tris: int) -> RtBvhLayout:
    """What the triangle count alone determines of the BVH scene (rt_bvh_layout): node / record counts, stack need, array sizes."""
    out = RtBvhLayout()
    rc = lib().rt_bvh_layout(int(n_tris), C.byref(out))
    if rc != RT_OK:
        raise RtError(rc, (lib().rt_last_error(None) or b"").decode())
    return out


def build_bvh(tris9):
    """-> (nodes12 [nNodes,12], tris12 [nTris,12]) in the reference's texture-buffer layout."""
    t = _f32(tris9).reshape(-1, 9)
    n = t.shape[0]
    nodes = np.zeros((max(2 * n, 1), 12), np.float32)
    tris = np.zeros((max(n, 1), 12), np.float32)
    k = lib().rt_build_bvh(_fp(t), n, _fp(nodes), _fp(tris))
    if k < 0:
        raise RtError(k, "rt_build_bvh")
    return nodes[:k].copy(), tris[:n].copy()


def build_bvh_order(tris9):
    """-> (nodes12, tris12, order): build_bvh's arrays (bit for bit) and order[i] = the input triangle that became row i of tris12, so that a
    ray query's prim maps back to the mesh (order[prim])."""
    t = _f32(tris9).reshape(-1, 9)
    n = t.shape[0]
    nodes = np.zeros((max(2 * n, 1), 12), np.float32)
    tris = np.zeros((max(n, 1), 12), np.float32)
    order = np.zeros(max(n, 1), np.int32)
    k = lib().rt_build_bvh_order(_fp(t), n, _fp(nodes), _fp(tris), order.ctypes.data_as(C.POINTER(C.c_int32)))
    if k < 0:
        raise RtError(k, "rt_build_bvh_order")
    return nodes[:k].copy(), tris[:n].copy(), order[:n].copy()


def refit_bvh(nodes12, tris12, order, tris9):
    """-> (nodes12, tris12) of the same tree over new triangles (rt_refit_bvh): tris9 in input order, order as build_bvh_order or Renderer.mesh_order
    gave it.  Row i of tris12 comes from triangle order[i]; every node's box is recomputed from its range; links, first and count stay.  The inputs
    are not modified."""
    n = np.array(_f32(nodes12).reshape(-1, 12), copy=True)
    t = np.array(_f32(tris12).reshape(-1, 12), copy=True)
    o = np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
    t9 = _f32(tris9).reshape(-1, 9)
    if o.size != t.shape[0] or t9.shape[0] != t.shape[0]:
        raise RtError(RT_ERR_INVALID, f"refit_bvh: {t.shape[0]} rows of tris12, {o.size} entries of order, {t9.shape[0]} triangles")
    rc = lib().rt_refit_bvh(_fp(t9), t9.shape[0], o.ctypes.data_as(C.POINTER(C.c_int32)), _fp(n), n.shape[0], _fp(t))
    if rc != RT_OK:
        raise RtError(rc, "rt_refit_bvh: order is not a permutation or the nodes are not a tree over the rows" if rc == RT_ERR_INVALID else "rt_refit_bvh")
    return n, t


def bvh_cost(nodes12) -> RtBvhCost:
    """The quality metric of a tree (rt_bvh_cost): the surface-area heuristic with both unit costs 1, in units of the root's area, summed as integers
    (innerQ, leafQ) so that Renderer.mesh_quality reproduces it bit for bit.  nodes12 as build_bvh / build_bvh_gpu / refit_bvh return them."""
    n = _f32(nodes12).reshape(-1, 12)
    out = RtBvhCost()
    rc = lib().rt_bvh_cost(_fp(n) if n.shape[0] else None, n.shape[0], C.byref(out))
    if rc != RT_OK:
        raise RtError(rc, "rt_bvh_cost: no nodes, a negative count, a non-finite bound or a max below its min")
    return out


def pack_scene(nodes12, tris12, **options) -> dict:
    """What upload_bvh would put on the device, without one (rt_debug_pack_scene): name -> bytes (uint8, padding included; empty: no such array) for
    every name of SCENE_ARRAYS and SCENE_ARRAYS_OPTIONAL, and "info" -> the scalars of RtPackInfo as a namespace (nNodes .. rootMax).  options: qnodes
    (-1 by size, 0 never, > 0 always), fused, implicit, anyhit_sah, sparse_leaf_boxes; with none given the options come from the environment, as an
    upload reads them."""
    n, t = _f32(nodes12).reshape(-1, 12), _f32(tris12).reshape(-1, 12)
    opt = None
    if options:     # RtPackOptions: qnodes, fused, implicit, anyhitSah, sparseLeafBoxes, reserved[3]
        opt = np.array([options.pop("qnodes", -1), options.pop("fused", False), options.pop("implicit", False), options.pop("anyhit_sah", False),
                        options.pop("sparse_leaf_boxes", False), 0, 0, 0], np.int32)
        if options:
            raise TypeError(f"pack_scene: unknown options {sorted(options)}")

    def read(which):
        size = C.c_size_t()
        args = (_fp(n), n.shape[0], _fp(t), t.shape[0], None if opt is None else C.c_void_p(opt.ctypes.data), which)
        rc = lib().rt_debug_pack_scene(*args, None, 0, C.byref(size))
        out = np.zeros(size.value, np.uint8)
        if rc == RT_OK and size.value:
            rc = lib().rt_debug_pack_scene(*args, C.c_void_p(out.ctypes.data), out.size, C.byref(size))
        if rc != RT_OK:
            raise RtError(rc, (lib().rt_last_error(None) or b"").decode())
        return out

    out = {name: read(which) for name, which in {**SCENE_ARRAYS, **SCENE_ARRAYS_OPTIONAL}.items()}
    raw = read(RT_SCENE_ARRAY_PACK_INFO)      # RtPackInfo: seventeen 32-bit words, two float[3], one reserved word
    names = ("nNodes", "nTris", "nInner", "treeDepth", "nWide4", "nPairs", "nFused", "flags", "implicitDepth", "implicitRecords", "rootRef", "rootRefW",
             "rootRef4", "anyStack", "leafBoxMagic", "nLeafBoxes", "collapsed4")
    info = dict(zip(names, raw.view(np.int32)[:17].tolist()))
    info["leafBoxMagic"] = int(raw.view(np.uint32)[14])
    info["rootMin"], info["rootMax"] = raw.view(np.float32)[17:20].copy(), raw.view(np.float32)[20:23].copy()
    out["info"] = types.SimpleNamespace(**info)
    return out


@functools.lru_cache(maxsize=None)
def _wave_plan_types():
    """RtWaveOptions and RtWavePlan, declared at the first rt.wave_plan call and not at import: bench.py's short run is sensitive to what importing the
    package allocates (profiles/r14_scene_pack.txt 3)."""
    class RtWaveOptions(_Struct):
        _fields_ = [("budgetBytes", C.c_uint64), ("q2Cap", C.c_uint64)] + \
                   [(n, i32) for n in ("q2CapSet", "q2Predict", "binGi", "packetAO", "chunksFromSlots", "probeMode", "cuSplit", "shadePrioritySet",
                                       "shadePriority", "skipTraversalSet", "skipTraversal", "gridPct", "gridPctPrimary", "chunkPrimarySet", "chunkPrimary",
                                       "traceStatsSet", "traceStats", "traceTimingSet", "traceTiming", "reserved")]

    class RtWavePlanArray(_Struct):
        _fields_ = [("name", C.c_char * 16), ("offset", C.c_uint64), ("bytes", C.c_uint64)]

    class RtWavePlanArena(_Struct):
        _fields_ = [("bytes", C.c_uint64), ("allocBytes", C.c_uint64), ("nArrays", i32), ("reserved", i32), ("arrays", RtWavePlanArray * 9)]

    class RtWavePlan(_Struct):
        _fields_ = [("options", RtWaveOptions)] + [(n, C.c_uint64) for n in ("slots", "perHit", "chBudget", "ch", "room", "q2Entries")] + \
                   [(n, i32) for n in ("spp", "ao", "S1", "S2", "L1", "deferred", "nChunks", "reserved")] + \
                   [(n, RtWavePlanArena) for n in ("frame", "rays", "results")]

    return RtWaveOptions, RtWavePlan


def wave_plan(slots, spp, ao_rays=0, *, hits=None, share=0.0, **options):
    """The ray-queue plan of one launch set of the wavefront pipeline, without a context or a GPU (rt_debug_wave_plan).  slots: pixel slots
    (tiles x 256 x frames of the batch); ao_rays: AO rays per hit, 0 = AO off; hits: the hit count once it is known (None: before); share: the share of
    (hit, sample) pairs whose bounce ray hit in earlier launch sets.  options: fields of RtWaveOptions by name (budget_mb for budgetBytes; q2_cap sets
    q2Cap and q2CapSet) over the defaults; with none given the options come from the environment, as a lane reads them when the context is created.
    -> namespace of the plan's scalars, `options` (dict) and, per arena (frame, rays, results), bytes, allocBytes and arrays = [(name, offset, bytes)]
    with offset None for a span that is reserved but not handed out.  RtError(RT_ERR_UNSUPPORTED) for a chunk of 2^31 queue entries or more."""
    RtWaveOptions, RtWavePlan = _wave_plan_types()
    opt = None
    if options:
        opt = RtWaveOptions(budgetBytes=16 << 30, q2Predict=1, probeMode=-1)
        if "budget_mb" in options:
            opt.budgetBytes = int(options.pop("budget_mb")) << 20
        if "q2_cap" in options:
            opt.q2CapSet, opt.q2Cap = 1, int(options.pop("q2_cap"))
        names = {n for n, _ in RtWaveOptions._fields_} - {"reserved"}
        for k, v in options.items():
            if k not in names:
                raise TypeError(f"wave_plan: unknown option {k}")
            setattr(opt, k, int(v))
    out = RtWavePlan()
    rc = lib().rt_debug_wave_plan(int(slots), int(spp), int(ao_rays), None if opt is None else C.byref(opt), -1 if hits is None else int(hits), float(share),
                                  C.byref(out))
    if rc != RT_OK:
        raise RtError(rc, (lib().rt_last_error(None) or b"").decode() or "rt_debug_wave_plan")

    def arena(a):
        arrays = [(x.name.decode(), None if x.offset == 2**64 - 1 else int(x.offset), int(x.bytes)) for x in a.arrays[:a.nArrays]]
        return types.SimpleNamespace(bytes=int(a.bytes), allocBytes=int(a.allocBytes), arrays=arrays)

    scalars = {n: int(getattr(out, n)) for n in ("slots", "perHit", "chBudget", "ch", "room", "q2Entries", "spp", "ao", "S1", "S2", "L1", "nChunks")}
    return types.SimpleNamespace(**scalars, deferred=bool(out.deferred), options={n: int(getattr(out.options, n)) for n, _ in RtWaveOptions._fields_ if n != "reserved"},
                                 frame=arena(out.frame), rays=arena(out.rays), results=arena(out.results))


# ---- the k_trace build a traversal launch chooses (no context, no GPU; csrc/rt_trace_build.cpp) ----

TRACE_OPTIONS = ("timing", "coop", "nearFirst", "qnodes", "fused", "impl", "leafb", "leafbClosest")   # RtTraceOptions
TRACE_FORMS = ("q4", "wF", "iN2", "iN4", "iQ4")                                                        # the optional record forms of a scene (RtTraceCase)
TRACE_NODES = ("wnodesW", "wF", "iN2", "w4", "q4", "iN4", "iQ4")                                       # RT_TRACE_NODES_*


@functools.lru_cache(maxsize=None)
def _trace_build_types():
    """RtTraceCase and RtTraceBuild as numpy record types, declared at the first call and not at import (see _wave_plan_types)."""
    case = np.dtype([(n, np.int32) for n in TRACE_OPTIONS + ("any", "stats", "depth", "anyStack") + TRACE_FORMS + ("reserved",)])
    build = np.dtype([("opt", np.uint32), ("nodes", np.int32), ("implPairs", np.int32), ("implLeafBoxes", np.int32), ("stack", np.int32), ("reserved", np.int32),
                      ("ldsBytes", np.uint64)])
    assert case.itemsize == 72 and build.itemsize == 32
    return case, build


def trace_options() -> dict:
    """The switches of the environment that choose a k_trace build, as a context reads them (rt_debug_trace_options)."""
    out = np.zeros(len(TRACE_OPTIONS), np.int32)
    rc = lib().rt_debug_trace_options(out.ctypes.data)
    if rc != RT_OK:
        raise RtError(rc, "rt_debug_trace_options")
    return dict(zip(TRACE_OPTIONS, (int(v) for v in out)))


def trace_builds_kept(any_hit) -> tuple:
    """The k_trace builds the library holds for closest-hit (any_hit false) or any-hit launches: their option bits, unshifted (rt_debug_trace_builds)."""
    out = np.zeros(64, np.uint32)
    n = lib().rt_debug_trace_builds(1 if any_hit else 0, out.ctypes.data_as(_U32P), out.size)
    return tuple(int(v) for v in out[:n])


def trace_build_cases(cases) -> np.ndarray:
    """rt_debug_trace_build over an array of RtTraceCase records (dtype: _trace_build_types()[0]) -> the RtTraceBuild records, one per case."""
    case, build = _trace_build_types()
    cases = np.ascontiguousarray(cases, dtype=case)
    out = np.zeros(cases.shape[0], build)
    rc = lib().rt_debug_trace_build(cases.ctypes.data, cases.shape[0], out.ctypes.data)
    if rc != RT_OK:
        raise RtError(rc, "rt_debug_trace_build")
    return out


def trace_build(any_hit, *, depth, stats=False, any_stack=0, forms=(), **options):
    """The k_trace build a traversal launch chooses, without a context or a GPU (rt_debug_trace_build).  any_hit: an any-hit launch; depth: the
    binary tree's depth; stats: the launch adds to diagnostic sums (a frame's under RT_TRACE_STATS / RT_TRACE_TIMING); any_stack: RtPackInfo.anyStack; forms:
    the optional record forms the scene has, names of TRACE_FORMS; options: fields of RtTraceOptions by name over the defaults -- with none given the
    options come from the environment, as a context reads them.
    -> namespace: opt (RT_BUILD_* bits, unshifted), bits (their names, as Renderer.debug_builds spells them), nodes (the array walked, a name of
    TRACE_NODES), implPairs, implLeafBoxes, stack, ldsBytes."""
    case, _ = _trace_build_types()
    c = np.zeros(1, case)
    opt = {**dict(timing=0, coop=0, nearFirst=0, qnodes=-1, fused=0, impl=0, leafb=2, leafbClosest=2), **options} if options else trace_options()
    if set(opt) != set(TRACE_OPTIONS):
        raise TypeError(f"trace_build: unknown option {sorted(set(opt) - set(TRACE_OPTIONS))}")
    if set(forms) - set(TRACE_FORMS):
        raise TypeError(f"trace_build: unknown record form {sorted(set(forms) - set(TRACE_FORMS))}")
    for k, v in opt.items():
        c[k] = int(v)
    for k in forms:
        c[k] = 1
    c["any"], c["stats"], c["depth"], c["anyStack"] = bool(any_hit), bool(stats), int(depth), int(any_stack)
    b = trace_build_cases(c)[0]
    return types.SimpleNamespace(opt=int(b["opt"]), bits=frozenset(n for n, v in RT_BUILD_BITS.items() if int(b["opt"]) & v), nodes=TRACE_NODES[int(b["nodes"])],
                                 implPairs=bool(b["implPairs"]), implLeafBoxes=bool(b["implLeafBoxes"]), stack=int(b["stack"]), ldsBytes=int(b["ldsBytes"]))


# ---- the shading stages' division-free arithmetic, as the host compiles it (no context, no GPU) ----

class RtFrameGeomInfo(_Struct):   # rt_debug_frame_geom
    _fields_ = [("tilesX", C.c_int32), ("tilesY", C.c_int32), ("nTiles", C.c_int32), ("nLocalTiles", C.c_int32),
                ("rcpLocalTiles", C.c_uint32), ("rcpTilesX", C.c_uint32), ("rcpWorld", C.c_uint32)]


def texel_unorm8() -> np.ndarray:
    """The cube-map lookup's value for each of the 256 texel codes (rt_debug_texel_unorm8)."""
    out = np.zeros(256, np.float32)
    rc = lib().rt_debug_texel_unorm8(_fp(out))
    if rc != RT_OK:
        raise RtError(rc, "rt_debug_texel_unorm8")
    return out


def halton_pairs(frame0, count) -> np.ndarray:
    """[count, 2] float32: the (halton(f + 1, 2), halton(f + 1, 3)) the host writes into the frame descriptor for uFrameIndex f = frame0 + i."""
    out = np.zeros((int(count), 2), np.float32)
    rc = lib().rt_debug_halton_pairs(int(frame0), int(count), _fp(out))
    if rc != RT_OK:
        raise RtError(rc, "rt_debug_halton_pairs")
    return out


def div_reciprocal(d, n_max) -> int:
    """The reciprocal word the host stores for divisor d and largest dividend n_max; 0 = the kernels divide (rt_debug_div_reciprocal)."""
    return int(lib().rt_debug_div_reciprocal(int(d), int(n_max)))


def div_by(d, rcp, n):
    """(n // d, n % d) as the kernels compute them from the divisor and its reciprocal word (rt_debug_div_by); n: uint32 array."""
    n = np.ascontiguousarray(n, np.uint32).reshape(-1)
    q, r = np.zeros_like(n), np.zeros_like(n)
    rc = lib().rt_debug_div_by(int(d), int(rcp), n.ctypes.data_as(_U32P), n.size, q.ctypes.data_as(_U32P), r.ctypes.data_as(_U32P))
    if rc != RT_OK:
        raise RtError(rc, "rt_debug_div_by")
    return q, r


def frame_geom(w, h, rank=0, world=1, batch=1, reciprocals=True, slots=False):
    """rt_debug_frame_geom: (RtFrameGeomInfo, xy) -- the tile geometry rt_resize sets up, with its reciprocal words for batches of `batch` frames, and with
    slots=True an int32 [nLocalTiles * batch * 256, 3] array of (x, y, sub-frame) per pixel slot, -1 for padding (else None)."""
    info = RtFrameGeomInfo()
    rc = lib().rt_debug_frame_geom(int(w), int(h), int(rank), int(world), int(batch), int(bool(reciprocals)), C.byref(info), None)
    if rc != RT_OK:
        raise RtError(rc, "rt_debug_frame_geom")
    xy = None
    if slots:
        xy = np.zeros((info.nLocalTiles * int(batch) * 256, 3), np.int32)
        rc = lib().rt_debug_frame_geom(int(w), int(h), int(rank), int(world), int(batch), int(bool(reciprocals)), C.byref(info),
                                       xy.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc != RT_OK:
            raise RtError(rc, "rt_debug_frame_geom")
    return info, xy


def batch_tiles(batch, n_local_tiles) -> np.ndarray:
    """rt_debug_batch_tiles: int32 [batch * n_local_tiles], the local tile index (k * n_local_tiles + lt) each iteration of k_primary_interleaved's grid handles in a
    batch of frames: the frames of a spatial tile follow each other."""
    out = np.zeros(int(batch) * int(n_local_tiles), np.int32)
    rc = lib().rt_debug_batch_tiles(int(batch), int(n_local_tiles), out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != RT_OK:
        raise RtError(rc, "rt_debug_batch_tiles")
    return out


def batch_order(ballots) -> np.ndarray:
    """rt_debug_batch_order: ballots uint64 [n, waves] (bit l of [k, w]: lane l of wave w has a candidate in iteration k) -> uint32 [n, waves, 64], each
    candidate's position relative to the workgroup's first (0xffffffff: none) in k_primary_interleaved's order for a batch of frames."""
    b = np.ascontiguousarray(ballots, dtype=np.uint64)
    n, waves = b.shape
    out = np.zeros((n, waves, 64), np.uint32)
    rc = lib().rt_debug_batch_order(b.ctypes.data_as(C.POINTER(C.c_uint64)), n, waves, out.ctypes.data_as(_U32P))
    if rc != RT_OK:
        raise RtError(rc, "rt_debug_batch_order")
    return out


class RtBeamCullStats(_Struct):   # rt_debug_beam_cull / rt_debug_beam_cull_stats: the beam cull of a batch's primary stage (RT_BEAM_CULL)
    _fields_ = [("tiles", C.c_uint64), ("deadTiles", C.c_uint64), ("overflowTiles", C.c_uint64), ("levels", C.c_uint64)]


def beam_cull(u, nodes12, tris12, jitters=None, rank=0, world=1, rays=False, packed=None):
    """rt_debug_beam_cull: the dead flags of the frame shape of `u` on the host -> (dead uint8 [nLocalTiles], RtBeamCullStats[, rd_inv float32 [K, H, W, 3]
    with rays=True]).  dead[lt] = 1: every primary ray of local tile lt, in each of the K frames whose jitters are `jitters` ([K, 2]; None: the one frame of
    u.jitter), surely misses the mesh.  packed: a pack_scene result for (nodes12, tris12) to use instead of packing them here."""
    jit = None if jitters is None else _f32(jitters).reshape(-1, 2)
    K = 1 if jit is None else jit.shape[0]
    W, H = int(u.resolution[0]), int(u.resolution[1])
    info, _ = frame_geom(W, H, rank, world)
    p = packed if packed is not None else pack_scene(nodes12, tris12)
    rec = np.ascontiguousarray(p["nodes2w"]).view(np.float32)
    n_inner = int(p["info"].nInner)
    lo, hi = _f32(p["info"].rootMin), _f32(p["info"].rootMax)
    dead = np.zeros(info.nLocalTiles, np.uint8)
    stats = RtBeamCullStats()
    rd = np.zeros((K, H, W, 3), np.float32) if rays else None
    rc = lib().rt_debug_beam_cull(C.byref(u), None if jit is None else _fp(jit), K, int(rank), int(world), _fp(rec) if rec.size else None, n_inner,
                                  int(p["info"].rootRefW), _fp(lo), _fp(hi), dead.ctypes.data_as(_U8P), info.nLocalTiles, C.byref(stats),
                                  None if rd is None else _fp(rd))
    if rc != RT_OK:
        raise RtError(rc, "rt_debug_beam_cull")
    return (dead, stats, rd) if rays else (dead, stats)


def beam_walk(ro, L, H, nodes12=None, tris12=None, packed=None):
    """rt_debug_beam_walk: beams [n, 3] float32 (L, H: per axis the least and largest reciprocal direction) from the one origin ro against the tree ->
    (verdict uint8 [n]: 0 dead, 1 alive, 2 kept because a level of the walk overflowed; levels int32 [n])."""
    p = packed if packed is not None else pack_scene(nodes12, tris12)
    rec = np.ascontiguousarray(p["nodes2w"]).view(np.float32)
    lo, hi, o = _f32(p["info"].rootMin), _f32(p["info"].rootMax), _f32(ro).reshape(3)
    l, h = _f32(L).reshape(-1, 3), _f32(H).reshape(-1, 3)
    if l.shape != h.shape:
        raise ValueError("beam_walk: L and H of different shapes")
    verdict, levels = np.zeros(l.shape[0], np.uint8), np.zeros(l.shape[0], np.int32)
    rc = lib().rt_debug_beam_walk(l.shape[0], _fp(o), _fp(l), _fp(h), _fp(rec) if rec.size else None, int(p["info"].nInner), int(p["info"].rootRefW),
                                  _fp(lo), _fp(hi), verdict.ctypes.data_as(_U8P), levels.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != RT_OK:
        raise RtError(rc, "rt_debug_beam_walk")
    return verdict, levels


def beam_slab(ro, lo, hi, L, H):
    """rt_debug_beam_slab over [n, 3] float32 arrays -> (fails uint8 [n], bounds float32 [n, 4] = tminLo, tminHi, tmaxLo, tmaxHi; NaN where the argument does
    not apply)."""
    a = [_f32(x).reshape(-1, 3) for x in (ro, lo, hi, L, H)]
    n = a[0].shape[0]
    if any(x.shape[0] != n for x in a):
        raise ValueError("beam_slab: arrays of different lengths")
    fails, bounds = np.zeros(n, np.uint8), np.zeros((n, 4), np.float32)
    rc = lib().rt_debug_beam_slab(n, *[_fp(x) for x in a], fails.ctypes.data_as(_U8P), _fp(bounds))
    if rc != RT_OK:
        raise RtError(rc, "rt_debug_beam_slab")
    return fails, bounds


def load_obj(path):
    pos, idx = _FP(), _U32P()
    nv, ni = C.c_int(), C.c_int()
    rc = lib().rt_load_obj(str(path).encode(), C.byref(pos), C.byref(nv), C.byref(idx), C.byref(ni))
    if rc != RT_OK:
        raise RtError(rc, f"rt_load_obj({path})")
    p = np.ctypeslib.as_array(pos, shape=(max(nv.value * 3, 1),))[: nv.value * 3].copy().reshape(-1, 3)
    i = np.ctypeslib.as_array(idx, shape=(max(ni.value, 1),))[: ni.value].copy()
    lib().rt_free(pos)
    lib().rt_free(idx)
    return p, i


def load_obj_uv(path):
    """rt_load_obj_uv: positions [V,3], uvs [V,2], indices [3T] of a .obj with vt records -- one vertex per distinct (v, vt) pair, in order of first
    use by the faces; a corner without vt gets (0, 0)."""
    pos, uv, idx = _FP(), _FP(), _U32P()
    nv, ni = C.c_int(), C.c_int()
    rc = lib().rt_load_obj_uv(str(path).encode(), C.byref(pos), C.byref(uv), C.byref(nv), C.byref(idx), C.byref(ni))
    if rc != RT_OK:
        raise RtError(rc, f"rt_load_obj_uv({path})")
    p = np.ctypeslib.as_array(pos, shape=(max(nv.value * 3, 1),))[: nv.value * 3].copy().reshape(-1, 3)
    t = np.ctypeslib.as_array(uv, shape=(max(nv.value * 2, 1),))[: nv.value * 2].copy().reshape(-1, 2)
    i = np.ctypeslib.as_array(idx, shape=(max(ni.value, 1),))[: ni.value].copy()
    lib().rt_free(pos)
    lib().rt_free(uv)
    lib().rt_free(idx)
    return p, t, i


def load_png(path) -> np.ndarray:
    pix = _U8P()
    w, h, ch = C.c_int(), C.c_int(), C.c_int()
    rc = lib().rt_load_png(str(path).encode(), C.byref(pix), C.byref(w), C.byref(h), C.byref(ch))
    if rc != RT_OK:
        raise RtError(rc, f"rt_load_png({path})")
    a = np.ctypeslib.as_array(pix, shape=(h.value * w.value * ch.value,)).copy().reshape(h.value, w.value, ch.value)
    lib().rt_free(pix)
    return a


def save_png(path, img, flip_y=False):
    a = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = a.shape[:2]
    ch = 1 if a.ndim == 2 else a.shape[2]
    rc = lib().rt_save_png(str(path).encode(), a.ctypes.data_as(_U8P), w, h, ch, int(flip_y))
    if rc != RT_OK:
        raise RtError(rc, f"rt_save_png({path})")


def cubemap_from_cross(img) -> np.ndarray:
    """HxWxC uint8 4x3 cross -> [6, N, N, C] faces in GL order (src/render/cubemap.cpp:86-91)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w, ch = img.shape
    n = h // 3 if h % 3 == 0 else 0
    faces = np.zeros((6, max(n, 1), max(n, 1), ch), np.uint8)
    got = lib().rt_cubemap_from_cross(img.ctypes.data_as(_U8P), w, h, ch, faces.ctypes.data_as(_U8P))
    if got == 0:
        raise RtError(RT_ERR_INVALID, f"not a 4x3 cube-map cross: {w}x{h}")
    return faces


def load_cubemap_cross(path) -> np.ndarray:
    return cubemap_from_cross(load_png(path))


ASSET_DIR = _PKG_DIR.parent / "assets"


# ------------------------------------------------------------------------------------ device side
def _prim_view(record):
    """The prim column of RtHit records [...,4] float32 as int32, a view: numpy or torch, as the records are."""
    if isinstance(record, np.ndarray):
        return record.view(np.int32)[..., 1]
    import torch
    return record.view(torch.int32)[..., 1]


class RayHits:
    """Closest-hit answers of Renderer.trace_rays: `record` [N,4] float32 (one RtHit per ray) and views of it -- t [N], prim [N] int32 (row of
    the uploaded tris12, -1 on a miss), uv [N,2] -- plus normal [N,3] when asked for.  numpy arrays or torch tensors, as the rays were."""

    def __init__(self, record, normal=None):
        self.record = record
        self.t = record[:, 0]
        self.prim = _prim_view(record)
        self.uv = record[:, 2:4]
        self.normal = normal

    @property
    def hit(self):
        return self.prim >= 0

    def __len__(self):
        return self.record.shape[0]


class SceneHits(RayHits):
    """Closest-hit answers of Renderer.trace_scene_rays / Renderer.pick: RayHits (prim -1 on an analytic hit) plus object [N] int32
    (RT_OBJECT_*, RT_OBJECT_NONE on a miss) and, when asked for, normal [N,3] and point [N,3]."""

    def __init__(self, record, obj, normal=None, point=None):
        super().__init__(record, normal)
        self.object = obj
        self.point = point

    @property
    def hit(self):
        return self.object >= 0


def _query_invalid(msg):
    return RtError(RT_ERR_INVALID, f"trace_rays: {msg}")


# ---- the checks every query shares: what kind of arrays, their rows, their limits; and the two ways of handing them to C
def _device_of(index, named, dtype, own=False):
    """The tensors `named` = ((name, tensor or None), ...) are of `dtype` and on cuda:index -> that device.  own: trace_rays names the argument
    in its refusals, every later query does not."""
    import torch
    dev = torch.device("cuda", index)
    for name, a in named:
        if a is None:
            continue
        if a.dtype != dtype:
            raise _query_invalid(f"{name} must be float32, got {a.dtype}" if own else f"expected {dtype}, got {a.dtype}")
        if a.device != dev:
            raise _query_invalid(f"{name} is on {a.device}, the context on {dev}" if own else f"a tensor is on {a.device}, the context on {dev}")
    return dev


def _query_arrays(named, ren=None, own=False):
    """The kind of the float32 arrays of a query, `named` = ((name, array or None), ...) -> None: numpy arrays; a torch device: tensors on it.
    ren None is a host definition, which takes numpy alone; else the Renderer asked, and the arrays may all be numpy or all torch on its device
    (read only then: numpy arguments are refused without a context)."""
    given = [(name, a) for name, a in named if a is not None]
    if ren is not None and not all(isinstance(a, np.ndarray) for _, a in given):
        import torch
        if not all(isinstance(a, torch.Tensor) for _, a in given):
            names = [name for name, _ in named]
            raise _query_invalid(f"{', '.join(names[:-1])} and {names[-1]} must all be numpy arrays or all torch tensors" if len(names) > 1 else
                                 f"{names[0]} must be a numpy array or a torch tensor")
        return _device_of(ren.device, given, torch.float32, own)
    for name, a in given:
        if not isinstance(a, np.ndarray):
            raise _query_invalid(f"{name} must be a numpy array")
        if a.dtype != np.float32:
            raise _query_invalid(f"{name} must be float32, got {a.dtype}")
    return None


def _layout(a):
    """(shape, itemsize, strides) as _rows takes them: of a numpy array in bytes, of a tensor in elements."""
    return (a.shape, a.itemsize, a.strides) if isinstance(a, np.ndarray) else (tuple(a.shape), 1, a.stride())


# the arrays of query rows: noun, least k, layout words, and the [N,a,b] form: ((a, b), what its a * b floats are) or None
_BOXES = ("boxes", 6, " (lo.xyz, hi.xyz)", None)
_QTRIS = ("qtris", 9, " (p0.xyz, p1.xyz, p2.xyz) or [N,3,3]", ((3, 3), "nine floats of a triangle"))
_HULLS = ("hulls", 24, " (c0.xyz .. c7.xyz) or [N,8,3]", ((8, 3), "24 floats of a hull"))
_RECTS = ("rects", 4, " (x0, y0, x1, y1)", None)


def _rows(noun, k, layout, cell, shape, itemsize, strides, n=None):
    """The one row check: an array of query rows is [N,j] with j >= k -- or [N,a,b], cell = ((a, b), words), with the a * b floats of a row
    contiguous --, its floats adjacent within a row and its rows at least k floats apart; n: the row count it must have (dirs) -> the row
    stride in floats.  A single row has no stride to go by: its length stands in."""
    shape = tuple(shape)
    if cell and len(shape) == 3 and shape[1:] == cell[0]:
        (a, b), words = cell
        if strides[1] != b * itemsize or strides[2] != itemsize:
            raise _query_invalid(f"{noun} [N,{a},{b}]: the {words} must be contiguous")
        shape, strides = (shape[0], a * b), (strides[0], itemsize)
    if len(shape) != 2 or shape[1] < k:
        raise _query_invalid(f"{noun} must be [N,k] with k >= {k}{layout}, got shape {shape}")
    if n is not None and shape[0] != n:
        raise _query_invalid(f"{noun} has {shape[0]} rows, origins {n}")
    row, col = strides
    if col != itemsize or row % itemsize or (shape[0] > 1 and row // itemsize < k):
        raise _query_invalid(f"{noun} must have unit stride along its last dimension and rows at least {k} floats apart")
    return max(row // itemsize, k) if shape[0] > 1 else max(shape[1], k)


def _row_array(family, a, ren=None):
    """One array of query rows, family one of _BOXES .. _RECTS: its kind (_query_arrays), then its rows -> (torch device or None, n, row stride)."""
    dev = _query_arrays(((family[0], a),), ren)
    if family is _RECTS and dev is None and a.ndim != 2:
        raise _query_invalid("rects must be [N,k]")          # (numpy rects have words of their own here)
    return dev, a.shape[0], _rows(*family, *_layout(a))


def _limit(name, a, n, dev):
    """tmax / max_dist: [n]; a numpy array is made contiguous, a tensor must be -> the array to pass, or None."""
    if a is None:
        return None
    if dev is None:
        if a.shape != (n,):
            raise _query_invalid(f"{name} must be [{n}], got shape {a.shape}")
        return np.ascontiguousarray(a)
    if tuple(a.shape) != (n,) or (n > 1 and a.stride(0) != 1):
        raise _query_invalid(f"{name} must be a contiguous [{n}] tensor, got shape {tuple(a.shape)}")
    return a


def _ray_check(origins, dirs, tmax, ren=None, own=False):
    """The checks of Renderer.trace_rays on its rays -> (torch device or None for numpy, n, origin stride, dir stride, tmax to pass)."""
    dev = _query_arrays((("origins", origins), ("dirs", dirs), ("tmax", tmax)), ren, own)
    n = origins.shape[0] if len(origins.shape) == 2 else -1
    os_ = _rows("origins", 3, "", None, *_layout(origins))
    ds = _rows("dirs", 3, "", None, *_layout(dirs), n)
    return dev, n, os_, ds, _limit("tmax", tmax, n, dev)


def _point_check(points, max_dist, ren=None):
    """The checks of the nearest-point queries on their points -> (torch device or None for numpy, n, stride, max_dist to pass)."""
    dev = _query_arrays((("points", points), ("max_dist", max_dist)), ren)
    stride = _rows("points", 3, "", None, *_layout(points))
    n = points.shape[0]
    return dev, n, stride, _limit("max_dist", max_dist, n, dev)


def _ptr(a, null_if_empty=False):
    """A numpy array or a tensor as a void * argument; None stays None.  null_if_empty: an empty array goes as NULL, which the multi-hit, nearest
    and overlap queries do on both paths.  rt_trace_rays and rt_trace_scene_rays get the address as it is -- an empty numpy array has one, an
    empty tensor has none -- and that is observable: they refuse an any-hit query with a NULL tMax before they look at n."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data) if a.size or not null_if_empty else None
    return C.c_void_p(a.data_ptr()) if a.numel() or not null_if_empty else None


def _ptr0(a):
    return _ptr(a, True)


def _new(dev, shape, dtype=np.float32, zero=False):
    """An output of a query: a zero-filled numpy array for dev None, else a tensor on dev -- torch.empty unless `zero` says that the fill is
    counted on (the any-hit `occluded` flags, the marquee's corners)."""
    if dev is None:
        return np.zeros(shape, dtype)
    import torch
    return (torch.zeros if zero else torch.empty)(shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)


def _as_bool(occluded):
    """The uint8 flags of an any-hit query as the bool array the caller gets, a view."""
    if isinstance(occluded, np.ndarray):
        return occluded.view(bool)
    import torch
    return occluded.view(torch.bool)


class MultiHits:
    """Answers of multi_hits, Renderer.trace_rays_multi and Renderer.pick_multi: `hits` [N,K,4] float32 -- K RtHit records per ray,
    nearest first, the miss record {inf, -1, 0, 0} past the ray's last hit -- with the views t [N,K], prim [N,K] int32 and uv [N,K,2], and `count`
    [N] int32, the number of all the ray's hits, which may exceed K.  hits.reshape(-1, 4) is an input of the mesh_hit_* queries as it stands.
    numpy arrays or torch tensors, as the rays were."""

    def __init__(self, hits, count):
        self.hits = hits
        self.count = count
        self.t = hits[:, :, 0]
        self.prim = _prim_view(hits)
        self.uv = hits[:, :, 2:4]

    def __len__(self):
        return self.hits.shape[0]


def _multi_k(max_hits):
    k = int(max_hits)
    if not 0 <= k <= RT_MULTI_HIT_MAX:
        raise _query_invalid(f"max_hits = {k} (0 .. RT_MULTI_HIT_MAX = {RT_MULTI_HIT_MAX})")
    return k


def multi_hits(nodes12, tris12, origins, dirs, tmax=None, max_hits=4, eps=1e-4, inf=1e30) -> MultiHits:
    """The definition of the multi-hit query (rt_multi_hits), on the host and without a context: per ray the max_hits nearest of
    the triangles traceBVHShadow's walk of (nodes12, tris12) would accept up to tmax[i] (inf without tmax), ordered by (t, prim), and the count of
    all of them.  Rays as Renderer.trace_rays takes them (numpy); tmax[i] < 0 marks an empty slot."""
    k = _multi_k(max_hits)
    nodes = _f32(nodes12).reshape(-1, 12)
    tris = _f32(tris12).reshape(-1, 12)
    _, n, os_, ds, tmax = _ray_check(origins, dirs, tmax)
    hits, count = np.zeros((n, k, 4), np.float32), np.zeros(n, np.int32)
    p = _ptr0
    rc = lib().rt_multi_hits(p(nodes), nodes.shape[0], p(tris), tris.shape[0], p(origins), os_, p(dirs), ds, p(tmax), eps, inf, n, k, p(hits), _ptr(count))
    if rc != RT_OK:
        raise RtError(rc, "rt_multi_hits: the nodes are not a tree over the rows of tris12" if rc == RT_ERR_INVALID else "rt_multi_hits")
    return MultiHits(hits, count)


class NearestPoints:
    """Answers of nearest_points and Renderer.nearest_points: `hits` [N,4] float32 -- one RtHit record {e, prim, u, v} per point, the
    miss record {+inf, -1, 0, 0} where no triangle lies within the limit -- with the views dist2 [N] (e: the squared distance), prim [N] int32 and
    uv [N,2]; `points` [N,3], the nearest surface point v0 + u e1 + v e2 (zeros for a miss); `visits` [N] int32 or None.  hits is an input of the
    mesh_hit_* queries as it stands.  numpy arrays or torch tensors, as the points were."""

    def __init__(self, hits, points, visits=None):
        self.hits = hits
        self.points = points
        self.visits = visits
        self.dist2 = hits[:, 0]
        self.prim = _prim_view(hits)
        self.uv = hits[:, 2:4]

    def __len__(self):
        return self.hits.shape[0]


def nearest_points(nodes12, tris12, points, max_dist=None) -> NearestPoints:
    """The definition of the nearest-point query (rt_nearest_points), on the host and without a context: per point the triangle of
    (nodes12, tris12) least under (e, prim) with e <= max_dist[i]^2 (no limit without max_dist).  points: float32 [N,k], k >= 3, rows may be
    strided (numpy); max_dist[i] < 0 or a non-finite coordinate marks an empty slot."""
    nodes = _f32(nodes12).reshape(-1, 12)
    tris = _f32(tris12).reshape(-1, 12)
    _, n, stride, max_dist = _point_check(points, max_dist)
    hits, closest = np.zeros((n, 4), np.float32), np.zeros((n, 3), np.float32)
    p = _ptr0
    rc = lib().rt_nearest_points(p(nodes), nodes.shape[0], p(tris), tris.shape[0], p(points), stride, p(max_dist), n, p(hits), p(closest))
    if rc != RT_OK:
        raise RtError(rc, "rt_nearest_points: the nodes are not a tree over the rows of tris12" if rc == RT_ERR_INVALID else "rt_nearest_points")
    return NearestPoints(hits, closest)


class NearestMulti:
    """Answers of nearest_points_multi and Renderer.nearest_points_multi: `hits` [N,K,4] float32 -- K RtHit records {e, prim, u, v} per
    point, nearest first under (e, prim), the miss record {+inf, -1, 0, 0} past the point's last row within its limit -- with the views dist2 [N,K],
    prim [N,K] int32 and uv [N,K,2]; `points` [N,K,3], the surface point of each record (zeros for a miss); `count` [N] int32 or None, the number of
    all the rows within the limit, which may exceed K; `visits` [N] int32 or None.  hits.reshape(-1, 4) is an input of the mesh_hit_* queries as it
    stands.  numpy arrays or torch tensors, as the points were."""

    def __init__(self, hits, points, count=None, visits=None):
        self.hits = hits
        self.points = points
        self.count = count
        self.visits = visits
        self.dist2 = hits[:, :, 0]
        self.prim = _prim_view(hits)
        self.uv = hits[:, :, 2:4]

    def __len__(self):
        return self.hits.shape[0]


def _nearest_multi_k(max_hits, counts):
    k = int(max_hits)
    if not 0 <= k <= RT_NEAREST_MULTI_MAX:
        raise _query_invalid(f"max_hits = {k} (0 .. RT_NEAREST_MULTI_MAX = {RT_NEAREST_MULTI_MAX})")
    if k == 0 and not counts:
        raise _query_invalid("max_hits = 0 asks for the counts alone and needs counts")
    return k


def nearest_points_multi(nodes12, tris12, points, max_hits, max_dist=None) -> NearestMulti:
    """The definition of the proximity query (rt_nearest_points_multi), on the host and without a context: per point the max_hits rows of
    (nodes12, tris12) least under (e, prim) among those with e <= max_dist[i]^2 (no limit without max_dist), and the count of all of them.  Points and
    max_dist as nearest_points takes them; max_hits = 0 asks for the counts alone."""
    k = _nearest_multi_k(max_hits, True)
    nodes = _f32(nodes12).reshape(-1, 12)
    tris = _f32(tris12).reshape(-1, 12)
    _, n, stride, max_dist = _point_check(points, max_dist)
    hits, closest, count = np.zeros((n, k, 4), np.float32), np.zeros((n, k, 3), np.float32), np.zeros(n, np.int32)
    p = _ptr0
    rc = lib().rt_nearest_points_multi(p(nodes), nodes.shape[0], p(tris), tris.shape[0], p(points), stride, p(max_dist), n, k, p(hits),
                                       _ptr(count), p(closest))
    if rc != RT_OK:
        raise RtError(rc, "rt_nearest_points_multi: the nodes are not a tree over the rows of tris12" if rc == RT_ERR_INVALID else "rt_nearest_points_multi")
    return NearestMulti(hits, closest, count)


def nearest_multi_block(stack_entries, max_hits):
    """(threads per block, LDS bytes per block) of rt_query_nearest_multi's launch for a stack of stack_entries per lane and max_hits records
    (rt_debug_nearest_multi_block).  No GPU."""
    threads, lds = C.c_int(0), C.c_int64(0)
    rc = lib().rt_debug_nearest_multi_block(int(stack_entries), int(max_hits), C.byref(threads), C.byref(lds))
    if rc != RT_OK:
        raise RtError(rc, "rt_debug_nearest_multi_block")
    return threads.value, lds.value


class BoxOverlaps:
    """Answers of box_overlaps and Renderer.box_overlaps: `count` [N] int32, the number of rows overlapping each box; `offsets` [N+1]
    int32 and `prims` flat int32 -- the list of box i is prims[offsets[i] : offsets[i] + min(count[i], offsets[i+1] - offsets[i])], in walk order
    (ascending for the trees the library builds).  With cap=None the slots are exact; with cap=k every slot holds k entries, those past the list are
    -1, and count[i] > k says that box i overflowed.  `visits` [N] int32 or None.  numpy arrays or torch tensors, as the boxes were."""

    def __init__(self, count, offsets, prims, visits=None):
        self.count = count
        self.offsets = offsets
        self.prims = prims
        self.visits = visits

    def hits(self):
        """The flat list as RtHit records {0, prim, 1/3, 1/3} [len(prims),4] float32 (prim -1: the miss record's prim): an input of the mesh_hit_*
        queries as it stands -- the part, colour or normal at the centroid of every listed triangle."""
        third = np.float32(1.0) / np.float32(3.0)
        if isinstance(self.prims, np.ndarray):
            rec = np.zeros((self.prims.shape[0], 4), np.float32)
        else:
            import torch
            rec = torch.zeros((self.prims.shape[0], 4), dtype=torch.float32, device=self.prims.device)
        _prim_view(rec)[:] = self.prims
        rec[:, 2:4] = float(third)
        return rec

    def __len__(self):
        return self.count.shape[0]


def _box_cap(cap):
    if cap is None:
        return None
    k = int(cap)
    if k < 0:
        raise _query_invalid(f"cap = {k}")
    return k


def _numpy_box_query(call, result, boxes, n, stride, cap, visits):
    """Both forms on host arrays, for the n checked query rows `boxes`, `stride` floats apart: call(boxes, stride, n, offsets, cap, prims, counts,
    visits) -> rc, checked by the caller's wrapper.  result: the answers' class."""
    p = _ptr0
    count = np.zeros(n, np.int32)
    vis = np.zeros(n, np.int32) if visits else None
    if cap is not None:
        if n * cap > 2 ** 31 - 1:
            raise _query_invalid(f"{n} boxes x cap {cap} exceed INT32_MAX entries")
        offsets = (np.arange(n + 1, dtype=np.int64) * cap).astype(np.int32)
        prims = np.full(n * cap, -1, np.int32)
        if n:
            call(p(boxes), stride, n, None, cap, p(prims), p(count), p(vis))
        return result(count, offsets, prims, vis)
    offsets = np.zeros(n + 1, np.int32)
    if n:
        call(p(boxes), stride, n, None, 0, None, p(count), p(vis))
        total = np.cumsum(count, dtype=np.int64)
        if total[-1] > 2 ** 31 - 1:
            raise _query_invalid(f"the lists hold {int(total[-1])} entries, beyond INT32_MAX")
        offsets[1:] = total
    prims = np.full(int(offsets[-1]), -1, np.int32)
    if prims.size:
        call(p(boxes), stride, n, p(offsets), 0, p(prims), None, None)
    return result(count, offsets, prims, vis)


def box_overlaps(nodes12, tris12, boxes, cap=None) -> BoxOverlaps:
    """The definition of the box query (rt_box_overlaps), on the host and without a context: per closed box [lo, hi] the rows of
    (nodes12, tris12) that lie under overlapping node boxes and that the 13-axis separating-axis test cannot part from it, in walk order, and their
    count.  boxes: float32 [N,k], k >= 6 (lo.xyz, hi.xyz), rows may be strided (numpy); a NaN component or lo > hi marks an empty slot.  cap=None:
    the exact lists in two passes (count, scan, list); cap=k: one pass into k entries per box."""
    return _host_overlaps("rt_box_overlaps", BoxOverlaps, _BOXES, nodes12, tris12, boxes, cap)


def _host_overlaps(entry, result, family, nodes12, tris12, queries, cap):
    """box_overlaps, tri_overlaps and hull_overlaps: the C definition `entry` over the checked arrays -> result."""
    cap = _box_cap(cap)
    nodes = _f32(nodes12).reshape(-1, 12)
    tris = _f32(tris12).reshape(-1, 12)
    _, n, stride = _row_array(family, queries)

    def call(q, stride_, n_, offsets, cap_, prims, counts, _visits):
        rc = getattr(lib(), entry)(_ptr0(nodes), nodes.shape[0], _ptr0(tris), tris.shape[0], q, stride_, n_, offsets, cap_, prims, counts)
        if rc != RT_OK:
            raise RtError(rc, f"{entry}: the nodes are not a tree over the rows of tris12" if rc == RT_ERR_INVALID else entry)

    return _numpy_box_query(call, result, queries, n, stride, cap, False)


class TriOverlaps(BoxOverlaps):
    """Answers of tri_overlaps and Renderer.tri_overlaps: `count`, `offsets`, `prims`, `visits` and `.hits()` as BoxOverlaps, per query
    triangle; `.pairs()` is the list as (query, prim) rows."""

    def pairs(self):
        """[M,2] int32: one row (query, prim) per written list entry, queries ascending and each query's prims in list order -- the form a collision
        response wants.  Entries no list reaches (cap form: the -1 entries) are left out."""
        if isinstance(self.prims, np.ndarray):
            start = self.offsets[:-1].astype(np.int64)
            k = np.clip(np.minimum(self.count.astype(np.int64), self.offsets[1:].astype(np.int64) - start), 0, None)
            query = np.repeat(np.arange(k.size, dtype=np.int64), k)
            within = np.arange(query.size, dtype=np.int64) - np.repeat(np.cumsum(k) - k, k)
            return np.stack([query.astype(np.int32), self.prims[np.repeat(start, k) + within]], 1) if query.size else np.zeros((0, 2), np.int32)
        import torch
        start = self.offsets[:-1].to(torch.int64)
        k = torch.clamp(torch.minimum(self.count.to(torch.int64), self.offsets[1:].to(torch.int64) - start), min=0)
        query = torch.repeat_interleave(torch.arange(k.numel(), dtype=torch.int64, device=k.device), k)
        within = torch.arange(query.numel(), dtype=torch.int64, device=k.device) - torch.repeat_interleave(torch.cumsum(k, 0) - k, k)
        return torch.stack([query.to(torch.int32), self.prims[torch.repeat_interleave(start, k) + within]], 1)


def tri_overlaps(nodes12, tris12, qtris, cap=None) -> TriOverlaps:
    """The definition of the triangle query (rt_tri_overlaps), on the host and without a context: per query triangle (p0, p1, p2) the
    rows of (nodes12, tris12) that lie under node boxes overlapping the box of its points and that the 20-axis separating-axis test cannot part from
    it, in walk order, and their count.  qtris: float32 [N,9], [N,3,3] or [N,k], k >= 9, rows may be strided (numpy); a NaN component marks an empty
    slot.  cap=None: the exact lists in two passes (count, scan, list); cap=k: one pass into k entries per query."""
    return _host_overlaps("rt_tri_overlaps", TriOverlaps, _QTRIS, nodes12, tris12, qtris, cap)


class HullOverlaps(TriOverlaps):
    """Answers of hull_overlaps, Renderer.hull_overlaps and Renderer.pick_rects: `count`, `offsets`, `prims`, `visits`, `.hits()` and
    `.pairs()` as TriOverlaps, per hull; `corners` [N,24] float32 -- the hulls pick_rects made of its rects, eight corners each, ready to draw -- or
    None where the caller brought the hulls."""

    def __init__(self, count, offsets, prims, visits=None, corners=None):
        super().__init__(count, offsets, prims, visits)
        self.corners = corners


def hull_overlaps(nodes12, tris12, hulls, cap=None) -> HullOverlaps:
    """The definition of the hull query (rt_hull_overlaps), on the host and without a context: per convex hexahedron (eight corners, corner
    k with bit 0 / 1 / 2 for the high end along the shape's first / second / third parameter) the rows of (nodes12, tris12) that lie under nodes that
    its box and its six face normals cannot part from it and that the 46-axis separating-axis test cannot part from it, in walk order, and their
    count.  hulls: float32 [N,24], [N,8,3] or [N,k], k >= 24, rows may be strided (numpy); a NaN among the 24 floats marks an empty slot.  cap=None:
    the exact lists in two passes (count, scan, list); cap=k: one pass into k entries per hull."""
    return _host_overlaps("rt_hull_overlaps", HullOverlaps, _HULLS, nodes12, tris12, hulls, cap)


def box_corners(boxes, M=None):
    """The hulls [N,24] float32 of the boxes [N,k], k >= 6 (lo.xyz, hi.xyz; numpy float32, rows may be strided) under M (rt_box_corners, DESIGN.md
    26.2): None, the identity, which copies; 16 floats, one column-major matrix for all boxes; or [N,16], one per box -- rows of
    mesh_part_matrices().  A NaN component or lo > hi gives 24 NaNs, an empty slot of the hull query."""
    _, n, stride = _row_array(_BOXES, boxes)
    m, mat_stride = None, 0
    if M is not None:
        m = _f32(M).reshape(-1, 16)
        if m.shape[0] not in (1, n):
            raise _query_invalid(f"M must hold one matrix or one per box, got {m.shape[0]} for {n} boxes")
        mat_stride = 16 if m.shape[0] == n and n > 1 else 0
    out = np.zeros((n, 24), np.float32)
    if n:
        rc = lib().rt_box_corners(C.c_void_p(boxes.ctypes.data), stride, n, C.c_void_p(m.ctypes.data) if m is not None else None, mat_stride,
                                  C.c_void_p(out.ctypes.data))
        if rc != RT_OK:
            raise RtError(rc, "rt_box_corners")
    return out


def rect_frusta(u, root_min, root_max, rects, t_near=0.0, t_far=None):
    """The hulls [N,24] float32 behind the rects [N,k], k >= 4 (x0, y0, x1, y1 in pixel-corner coordinates of u's frame, row 0 at the bottom; numpy
    float32) between the depths t_near and t_far along the view direction (rt_rect_frusta).  t_near=0: the pyramid from the eye.
    t_far=None: to the far side of the box [root_min, root_max] -- node 0's box of the scene.  A NaN, x1 < x0 or y1 < y0 gives 24 NaNs."""
    _, n, stride = _row_array(_RECTS, rects)
    lo, hi = _f32(root_min).reshape(3), _f32(root_max).reshape(3)
    out = np.zeros((n, 24), np.float32)
    rc = lib().rt_rect_frusta(C.byref(u) if u is not None else None, C.c_void_p(lo.ctypes.data), C.c_void_p(hi.ctypes.data),
                              C.c_void_p(rects.ctypes.data) if n else None, stride, n, float(t_near), -1.0 if t_far is None else float(t_far),
                              C.c_void_p(out.ctypes.data) if n else None)
    if rc != RT_OK:
        raise RtError(rc, "rt_rect_frusta")
    return out


def rows_as_tris(tris12):
    """The points of each row of tris12 as query triangles [N,9] float32: a = v0, b = v0 + e1, c = v0 + e2 by the definition's float32 adds (DESIGN.md
    24.1) -- the very floats the triangle test forms, so a query made of them shares its points with the row bit for bit.  numpy or torch."""
    if isinstance(tris12, np.ndarray):
        t = _f32(tris12).reshape(-1, 12)
        with np.errstate(all="ignore"):
            return np.concatenate([t[:, 0:3], t[:, 0:3] + t[:, 4:7], t[:, 0:3] + t[:, 8:11]], 1)
    import torch
    t = tris12.reshape(-1, 12)
    return torch.cat([t[:, 0:3], t[:, 0:3] + t[:, 4:7], t[:, 0:3] + t[:, 8:11]], 1)


def _model16(who, model):
    """A model matrix argument: None, or 16 floats (column-major, or a 4x4 array as default_bvh_transform returns it) -> None or float32 [16]."""
    m = None if model is None else _f32(model).reshape(-1)
    if m is not None and m.size != 16:
        raise RtError(RT_ERR_INVALID, f"{who}: model must have 16 floats")
    return m


def _wants_torch(as_torch):
    """as_torch of the device-array accessors: None stands for "when torch imports"."""
    if as_torch is None:
        try:
            import torch  # noqa: F401
            return True
        except ImportError:
            return False
    return as_torch


# ------------------------------------------------------------------------------------ device side
class Renderer:
    """One RtContext.  Mirrors the reference's per-frame call sequence."""

    def __init__(self, device=0, rank=0, world_size=1, pipeline=RT_PIPELINE_AUTO, count_work=False):
        self._h = C.c_void_p()
        cfg = RtDeviceConfig(device=device, rank=rank, worldSize=world_size, pipeline=pipeline, countWork=int(count_work))
        rc = lib().rt_create(C.byref(cfg), C.byref(self._h))
        if rc != RT_OK:
            raise RtError(rc, (lib().rt_last_error(None) or b"").decode())
        self.rank, self.world_size = rank, world_size
        self.device = device
        self.width = self.height = 0
        self.n_nodes = self.n_tris = 0
        self.env_loaded = True  # the dummy cube map counts (application.cpp:281)

    def _check(self, rc):
        if rc != RT_OK:
            raise RtError(rc, (lib().rt_last_error(self._h) or b"").decode())

    def close(self):
        if self._h:
            lib().rt_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def upload_bvh(self, nodes12, tris12):
        n, t = _f32(nodes12).reshape(-1, 12), _f32(tris12).reshape(-1, 12)
        self._check(lib().rt_upload_bvh(self._h, _fp(n), n.shape[0], _fp(t), t.shape[0]))
        self.n_nodes, self.n_tris = n.shape[0], t.shape[0]

    # ---- dynamic mesh: the BVH scene rebuilt on the device
    def mesh_upload(self, positions, indices):
        """Positions [V,3] float32 and triangle indices to the device, topology tables and every scene array allocated (rt_mesh_upload).  Installs no
        scene: mesh_rebuild does.  indices=None or empty releases the mesh."""
        idx = np.zeros(0, np.uint32) if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        v = _f32(positions).reshape(-1, 3)
        self._check(lib().rt_mesh_upload(self._h, _fp(v), v.shape[0], idx.ctypes.data_as(_U32P), idx.size))
        self.n_nodes = self.n_tris = 0
        self._mesh_verts = v.shape[0] if idx.size else 0

    def mesh_positions(self, as_torch=None):
        """The device array of object-space positions.  With torch (as_torch=None: when it imports) a float32 [V,3] tensor that aliases it, zero-copy;
        writes to it must be ordered on stream() (run them under torch.cuda.stream(torch.cuda.ExternalStream(ren.stream()))).  Else (pointer, bytes)."""
        return self._device_array("rt_mesh_positions", 3, as_torch)

    def mesh_set_positions(self, positions):
        v = _f32(positions).reshape(-1, 3)
        if v.shape[0] != getattr(self, "_mesh_verts", 0):
            raise RtError(RT_ERR_INVALID, f"mesh_set_positions: {v.shape[0]} vertices, the mesh has {getattr(self, '_mesh_verts', 0)}")
        self._check(lib().rt_mesh_set_positions(self._h, _fp(v)))   # pageable memory: staged before the call returns, as a frame's uniforms are

    def _sync_scene_counts(self):
        i = self.scene_info()
        self.n_nodes, self.n_tris = i.nNodes, i.nTris

    def mesh_rebuild(self, model=None):
        """Gather with the model matrix (column-major 16 floats or a 4x4 array as default_bvh_transform returns it; None: identity), build the BVH and
        every device record form on the device, install (rt_mesh_rebuild).  Asynchronous; no host wait unless the quantised any-hit form is in use."""
        m = _model16("mesh_rebuild", model)
        self._check(lib().rt_mesh_rebuild(self._h, None if m is None else _fp(m)))
        self._sync_scene_counts()

    def mesh_refit(self, model=None):
        """Keep the tree of the last mesh_rebuild and recompute what depends on coordinates -- triangles, every box, every record form -- from the
        current device positions and the model matrix (None: identity) (rt_mesh_refit).  Asynchronous like mesh_rebuild, at a fraction of its cost.
        Exact for any deformation; the tree gets slower to walk as triangles move apart: mesh_measure / mesh_quality measure that, and mesh_update
        refits or rebuilds by it."""
        m = _model16("mesh_refit", model)
        self._check(lib().rt_mesh_refit(self._h, None if m is None else _fp(m)))

    def mesh_measure(self):
        """Enqueue the measurement of the current tree's quality on stream() (rt_mesh_measure): no host wait, no allocation.  When every result slot is
        still in flight nothing is measured and mesh_quality().skipped counts it."""
        self._check(lib().rt_mesh_measure(self._h))

    def mesh_quality(self, which="latest", wait=True) -> RtMeshQuality:
        """which="latest": the newest measurement that has arrived; "baseline": the one of the current tree as its last rebuild left it.  wait=False
        never blocks and raises RtError(RT_ERR_STATE) when no such result has arrived; wait=True waits for the newest enqueued measurement first.
        .cost equals bvh_cost of the host route's nodes bit for bit (rt_mesh_quality)."""
        w = {"latest": RT_MESH_QUALITY_LATEST, "baseline": RT_MESH_QUALITY_BASELINE}.get(which)
        if w is None:
            raise RtError(RT_ERR_INVALID, f"mesh_quality: which must be 'latest' or 'baseline', got {which!r}")
        out = RtMeshQuality()
        self._check(lib().rt_mesh_quality(self._h, w, int(bool(wait)), C.byref(out)))
        return out

    def mesh_update(self, model=None, parts=False, *, rebuild_above):
        """One animation step (rt_mesh_update): refit, or rebuild when the newest arrived measurement of the current tree costs more than rebuild_above
        times what the tree cost as its rebuild left it; then enqueue a measurement of the result.  parts=True gathers under the device matrix table
        (model must be None).  Never waits, so the decision rests on the previous step's tree at the latest.  rebuild_above has no default: what ratio
        is worth a rebuild depends on the scene.  -> "refit" or "rebuild"."""
        m = _model16("mesh_update", model)
        action = C.c_int(-1)
        self._check(lib().rt_mesh_update(self._h, RT_MESH_UPDATE_PARTS if parts else RT_MESH_UPDATE_SINGLE, None if m is None else _fp(m), float(rebuild_above),
                                         C.byref(action)))
        if action.value == RT_MESH_DID_REBUILD:
            self._sync_scene_counts()
        return "rebuild" if action.value == RT_MESH_DID_REBUILD else "refit"

    def mesh_refit_count(self):
        """-> (refits since mesh_upload, refits since the last mesh_rebuild)"""
        total, since = C.c_uint64(), C.c_uint64()
        self._check(lib().rt_mesh_refit_count(self._h, C.byref(total), C.byref(since)))
        return total.value, since.value

    def mesh_order(self, as_torch=None):
        """order[i] = the input triangle that is row i of the device triangle array since the last mesh_rebuild, so order[prim] maps a hit back to the
        index buffer.  With torch (as_torch=None: when it imports) an int32 [nTris] tensor that aliases the device array, zero-copy, valid until the
        next mesh_rebuild and written on stream(): read it there.  Else a numpy array (rt_mesh_order: copies and synchronises)."""
        if not _wants_torch(as_torch):
            out = np.zeros(max(self.mesh_info().nTris, 1), np.int32)
            self._check(lib().rt_mesh_order(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
            return out[:self.mesh_info().nTris]
        ptr, n = C.c_void_p(), C.c_size_t()
        self._check(lib().rt_mesh_order_device(self._h, C.byref(ptr), C.byref(n)))
        return self._alias(ptr.value, (n.value // 4,), "<i4")

    # ---- parts: one model matrix per part, on the device, and hit -> (part, triangle of the part)
    def mesh_upload_parts(self, positions, indices, part_first):
        """mesh_upload for a mesh of parts (rt_mesh_upload_parts): part_first holds nParts + 1 boundaries in triangle units, from 0 to the triangle
        count, non-decreasing; empty parts are legal.  Every part's matrix starts as the identity."""
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        v = _f32(positions).reshape(-1, 3)
        pf = np.ascontiguousarray(part_first, dtype=np.int32).reshape(-1)
        self._check(lib().rt_mesh_upload_parts(self._h, _fp(v), v.shape[0], idx.ctypes.data_as(_U32P), idx.size, pf.ctypes.data_as(C.POINTER(C.c_int32)),
                                               pf.size - 1))
        self.n_nodes = self.n_tris = 0
        self._mesh_verts = v.shape[0] if idx.size else 0

    def mesh_parts(self) -> np.ndarray:
        """The part_first array of the current mesh (int32, nParts + 1 entries); [0, nTris] after mesh_upload."""
        n = C.c_int()
        self._check(lib().rt_mesh_parts(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value + 1, np.int32)
        self._check(lib().rt_mesh_parts(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size, C.byref(n)))
        return out

    def mesh_part_matrices(self, as_torch=None):
        """The device table of model matrices, one per part, column-major.  With torch (as_torch=None: when it imports) a float32 [nParts,16] tensor
        that aliases it, zero-copy; writes to it must be ordered on stream(), as for mesh_positions.  Else (pointer, bytes)."""
        return self._device_array("rt_mesh_part_matrices", 16, as_torch)

    def mesh_set_part_matrices(self, models, first=0):
        """Matrices [count,16] (or [count,4,4] as default_bvh_transform lays one out: column-major) from host memory into entries first .. of the
        table, copied on stream() (rt_mesh_set_part_matrices)."""
        m = _f32(models)
        if m.size % 16:
            raise RtError(RT_ERR_INVALID, "mesh_set_part_matrices: models must hold 16 floats per matrix")
        m = m.reshape(-1, 16)
        self._check(lib().rt_mesh_set_part_matrices(self._h, int(first), m.shape[0], _fp(m)))   # pageable memory: staged before the call returns

    def mesh_rebuild_parts(self):
        """mesh_rebuild with every part gathered under its own matrix of the device table (rt_mesh_rebuild_parts)."""
        self._check(lib().rt_mesh_rebuild_parts(self._h))
        self._sync_scene_counts()

    def mesh_refit_parts(self):
        """mesh_refit with every part gathered under its own matrix of the device table (rt_mesh_refit_parts)."""
        self._check(lib().rt_mesh_refit_parts(self._h))

    def mesh_hit_parts(self, hits):
        """Closest-hit answers -> (parts, tris): int32 [N] each, the part a hit's triangle belongs to and the triangle's index within the part;
        (-1, -1) for a miss, an analytic hit or a prim outside the mesh.  hits: a RayHits / SceneHits or its [N,4] float32 record array.  numpy in,
        numpy out (rt_mesh_hit_parts_host: synchronises); a torch tensor on this context's device takes the zero-copy path of trace_rays: enqueued
        on the library stream, ordered against torch's current stream, no host wait."""
        return tuple(self._mesh_hit_query("mesh_hit_parts", hits, None, [(0, np.int32), (0, np.int32)]))

    # ---- skinning: the positions rewritten on the device from rest positions and a bone table
    def _device_view(self, ptr, nbytes, cols, as_torch):
        """A float32 [nbytes / (4 * cols), cols] tensor that aliases library memory, zero-copy (as_torch=None: when torch imports), else (pointer, bytes)."""
        return self._alias(ptr, (nbytes // (4 * cols), cols), "<f4") if _wants_torch(as_torch) else (ptr, nbytes)

    def _alias(self, ptr, shape, typestr):
        """A tensor of `shape` and `typestr` over device memory at `ptr` that the library owns, zero-copy."""
        import torch

        class _View:   # __cuda_array_interface__: the library owns the memory, the tensor only views it
            __cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}
        return torch.as_tensor(_View(), device=torch.device("cuda", self.device))

    def _device_array(self, entry, cols, as_torch):
        """_device_view of what the (context, void **devPtr, size_t *bytes) accessor `entry` names."""
        ptr, n = C.c_void_p(), C.c_size_t()
        self._check(getattr(lib(), entry)(self._h, C.byref(ptr), C.byref(n)))
        return self._device_view(ptr.value, n.value, cols, as_torch)

    def _mesh_hit_query(self, name, hits, extra, outputs):
        """The mesh_hit_* methods: hits a RayHits / SceneHits or its [N,4] float32 record array; extra None or (name, [N,3] array), a second
        input; outputs (columns, dtype) per answer, columns 0: [N].  numpy in, numpy out through rt_<name>_host, which synchronises; torch tensors on
        this context's device through rt_<name>: zero-copy, enqueued on the library stream, ordered against torch's current stream, no host wait.
        -> the list of answers."""
        rec = hits.record if isinstance(hits, RayHits) else hits
        if isinstance(rec, np.ndarray):
            dev = None
            if rec.dtype != np.float32 or rec.ndim != 2 or rec.shape[1] != 4:
                raise RtError(RT_ERR_INVALID, f"{name}: records must be float32 [N,4], got {rec.dtype} {rec.shape}")
            n = rec.shape[0]
            ins = [np.ascontiguousarray(rec)]
            if extra is not None:
                x = _f32(extra[1]).reshape(-1, 3)
                if x.shape[0] != n:
                    raise RtError(RT_ERR_INVALID, f"{name}: {n} hits and {x.shape[0]} {extra[0]}")
                ins.append(x)
        else:
            import torch
            dev = torch.device("cuda", self.device)
            if not isinstance(rec, torch.Tensor) or rec.dtype != torch.float32 or rec.dim() != 2 or rec.shape[1] != 4 or rec.device != dev:
                raise RtError(RT_ERR_INVALID, f"{name}: records must be a numpy array or a float32 [N,4] tensor on {dev}")
            n = rec.shape[0]
            ins = [rec.contiguous()]
            if extra is not None:
                x = extra[1]
                if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.numel() != 3 * n or x.device != dev:
                    raise RtError(RT_ERR_INVALID, f"{name}: {extra[0]} must be a float32 [N,3] tensor on {dev}")
                ins.append(x.contiguous())
        outs = [_new(dev, (n, cols) if cols else n, dt) for cols, dt in outputs]
        self._query(dev, f"rt_{name}", ins, *(_ptr(a) for a in ins), n, *(_ptr(o) for o in outs))
        return outs

    def mesh_skin_upload(self, bone_idx, weights, n_bones, rest=None):
        """The skin of the current mesh (rt_mesh_skin_upload): bone_idx / weights [V,4], four influences per vertex; rest [V,3] rest positions, None: a
        device-to-device snapshot of mesh_positions() as it stands.  Allocates the bone table with every matrix the identity.  May synchronise;
        n_bones=0 releases the skin."""
        nv = getattr(self, "_mesh_verts", 0)
        if int(n_bones) == 0:
            self._check(lib().rt_mesh_skin_upload(self._h, None, None, None, 0))
            return
        bi, w = _skin_tables("mesh_skin_upload", nv, bone_idx, weights)
        r = None if rest is None else _f32(rest).reshape(-1, 3)
        if r is not None and r.shape[0] != nv:
            raise RtError(RT_ERR_INVALID, f"mesh_skin_upload: {r.shape[0]} rest positions, the mesh has {nv} vertices")
        self._check(lib().rt_mesh_skin_upload(self._h, None if r is None else _fp(r), bi.ctypes.data_as(C.POINTER(C.c_uint16)), _fp(w), int(n_bones)))

    def mesh_bones(self, as_torch=None):
        """The device table of bone matrices, column-major.  With torch (as_torch=None: when it imports) a float32 [nBones,16] tensor that aliases it,
        zero-copy; writes to it must be ordered on stream(), as for mesh_part_matrices.  Else (pointer, bytes)."""
        return self._device_array("rt_mesh_bones", 16, as_torch)

    def mesh_set_bones(self, models, first=0):
        """Matrices [count,16] (or [count,4,4], column-major) from host memory into entries first .. of the bone table, copied on stream() in call
        order with skins, updates, frames and queries (rt_mesh_set_bones)."""
        m = _f32(models)
        if m.size % 16:
            raise RtError(RT_ERR_INVALID, "mesh_set_bones: models must hold 16 floats per matrix")
        m = m.reshape(-1, 16)
        self._check(lib().rt_mesh_set_bones(self._h, int(first), m.shape[0], _fp(m)))   # pageable memory: staged before the call returns

    def mesh_rest_positions(self, as_torch=None):
        """The device array of rest positions the skin reads: a float32 [V,3] tensor that aliases it (as mesh_positions), else (pointer, bytes).
        mesh_morph(to="rest") blends morph targets into it; a caller with a deformer of its own writes it on stream() before mesh_skin."""
        return self._device_array("rt_mesh_rest_positions", 3, as_torch)

    def mesh_skin(self):
        """Enqueue positions := skin(rest, tables, bone table) on stream() (rt_mesh_skin): what skin_positions computes, bit for bit, under the bone
        table as it stands when the kernel runs.  No host wait, no allocation; follow it with mesh_refit / mesh_rebuild / mesh_update."""
        self._check(lib().rt_mesh_skin(self._h))

    # ---- previous pose and object motion: the rows before the most recent update, kept on the device beside the current ones
    def mesh_motion_enable(self, on=True):
        """Keep the previous pose of the dynamic mesh (rt_mesh_motion_enable): every update then moves it, and frames of the mesh's scene with
        useBVH == 1 write object motion at primary hits.  Allocates two arrays of nTris rows and latches if there is a tree; may synchronise.
        on=False releases them.  Off until asked for."""
        self._check(lib().rt_mesh_motion_enable(self._h, 1 if on else 0))

    def mesh_motion_latch(self):
        """previous pose := current pose, enqueued in call order with updates, frames and queries (rt_mesh_motion_latch): no host wait."""
        self._check(lib().rt_mesh_motion_latch(self._h))

    def mesh_prev_tris(self) -> np.ndarray:
        """The previous pose as float32 [nTris,12] rows of the tris12 layout (rt_debug_read_scene: synchronises); empty while motion is not enabled
        or before the first rebuild.  Row i belongs to input triangle mesh_order()[i], as row i of debug_read_scene("tris")."""
        return self.debug_read_scene(RT_SCENE_ARRAY_PREV_TRIS).view(np.float32).reshape(-1, 12)

    def mesh_hit_prev_points(self, hits, points):
        """Where each hit point was in the previous pose: float32 [N,3], hit_motion's prev_points bit for bit; zeros for a miss, an analytic hit or
        a prim outside the mesh.  hits: a RayHits / SceneHits or its [N,4] float32 record array; points [N,3] the hit points (SceneHits.points, or
        origin + dir * t).  numpy in, numpy out (rt_mesh_hit_prev_points_host: synchronises); torch tensors on this context's device take the
        zero-copy path of mesh_hit_parts: enqueued on the library stream, ordered against torch's current stream, no host wait."""
        return self._mesh_hit_query("mesh_hit_prev_points", hits, ("points", points), [(3, np.float32)])[0]

    # ---- smooth vertex normals: recomputed on the device behind every update, blended at mesh hits by frames and by mesh_hit_normals
    def mesh_normals_enable(self, on=True):
        """Keep area-weighted vertex normals of the dynamic mesh (rt_mesh_normals_enable): every update then recomputes them from its new rows, and
        frames of the mesh's scene with useBVH == 1 shade mesh hits with the smooth normal.  Packs the adjacency on the host, allocates five arrays and
        computes the normals if there is a tree; may synchronise.  on=False releases them.  Off until asked for."""
        self._check(lib().rt_mesh_normals_enable(self._h, 1 if on else 0))

    def mesh_vertex_normals(self, as_torch=None):
        """The device array of vertex normals: a float32 [V,4] tensor (nx, ny, nz, 0) that aliases it (as mesh_positions; written on stream() by the
        update calls), else (pointer, bytes).  vertex_normals of debug_read_scene("tris"), mesh_order() and the indices, bit for bit."""
        return self._device_array("rt_mesh_vertex_normals", 4, as_torch)

    def mesh_normal_rows(self) -> np.ndarray:
        """The corner normals as float32 [nTris,12] rows, three (nx, ny, nz, 0) per row (rt_debug_read_scene: synchronises); empty while normals are
        not enabled or before the first rebuild.  Row i belongs to input triangle mesh_order()[i], as row i of debug_read_scene("tris")."""
        return self.debug_read_scene(RT_SCENE_ARRAY_NORMAL_ROWS).view(np.float32).reshape(-1, 12)

    def mesh_hit_normals(self, hits):
        """The shading normal of each hit: float32 [N,3], hit_normals bit for bit -- on a pixel's pick, that pixel's GNRM before the conversion to half;
        zeros for a miss, an analytic hit or a prim outside the mesh.  hits: a RayHits / SceneHits or its [N,4] float32 record array.  numpy in, numpy
        out (rt_mesh_hit_normals_host: synchronises); a torch tensor on this context's device takes the zero-copy path of mesh_hit_parts: enqueued
        on the library stream, ordered against torch's current stream, no host wait."""
        return self._mesh_hit_query("mesh_hit_normals", hits, None, [(3, np.float32)])[0]

    # ---- per-vertex colours: kept on the device beside the triangle array, the albedo of mesh hits in frames and in mesh_hit_colors
    def mesh_colors_enable(self, on=True):
        """Keep one colour per vertex of the dynamic mesh (rt_mesh_colors_enable), every one MESH_GREY at first: every update then gathers the corner
        colours beside its new rows, and frames of the mesh's scene with useBVH == 1 shade mesh hits with them.  Allocates two arrays and fills the
        rows if there is a tree; may synchronise.  on=False releases them.  Off until asked for."""
        self._check(lib().rt_mesh_colors_enable(self._h, 1 if on else 0))

    def mesh_colors(self, as_torch=None):
        """The device array of vertex colours: a float32 [V,4] tensor (r, g, b, 0) that aliases it (as mesh_positions; the caller may write it on
        stream()), else (pointer, bytes).  The rows follow at the next update or mesh_colors_refresh."""
        return self._device_array("rt_mesh_colors", 4, as_torch)

    def mesh_set_colors(self, rgb, first=0):
        """Colours [count,3] from host memory for vertices first .., copied on stream() in call order with updates, frames and queries
        (rt_mesh_set_colors); a non-finite or negative component is refused.  The rows follow at the next update or mesh_colors_refresh."""
        c = _f32(rgb)
        if c.size % 3:
            raise RtError(RT_ERR_INVALID, "mesh_set_colors: rgb must hold 3 floats per vertex")
        c = c.reshape(-1, 3)
        self._check(lib().rt_mesh_set_colors(self._h, _fp(c), int(first), c.shape[0]))   # pageable memory: staged before the call returns

    def mesh_colors_refresh(self):
        """The corner colours gathered again from the vertex colours, for colours that changed under positions that did not; enqueued in call order
        with updates, frames and queries (rt_mesh_colors_refresh): no host wait."""
        self._check(lib().rt_mesh_colors_refresh(self._h))

    def mesh_color_rows(self) -> np.ndarray:
        """The corner colours as float32 [nTris,12] rows, three (r, g, b, 0) per row (rt_debug_read_scene: synchronises); empty while colours are not
        enabled or before the first rebuild.  Row i belongs to input triangle mesh_order()[i], as row i of debug_read_scene("tris")."""
        return self.debug_read_scene(RT_SCENE_ARRAY_COLOR_ROWS).view(np.float32).reshape(-1, 12)

    def mesh_hit_colors(self, hits):
        """The colour of each hit: float32 [N,3], hit_colors bit for bit -- on a pixel's pick, the albedo that pixel's frame shades with; zeros for a
        miss, an analytic hit or a prim outside the mesh.  hits: a RayHits / SceneHits or its [N,4] float32 record array.  numpy in, numpy out
        (rt_mesh_hit_colors_host: synchronises); a torch tensor on this context's device takes the zero-copy path of mesh_hit_normals: enqueued on
        the library stream, ordered against torch's current stream, no host wait."""
        return self._mesh_hit_query("mesh_hit_colors", hits, None, [(3, np.float32)])[0]

    # ---- UVs and the albedo texture: corner UVs beside the triangle array, a texture the albedo of mesh hits is multiplied by
    def mesh_uvs_enable(self, on=True):
        """Keep one UV per vertex of the dynamic mesh (rt_mesh_uvs_enable), zeros at first: every update then gathers the corner UVs beside its new
        rows.  Allocates two arrays and fills the rows if there is a tree; may synchronise.  on=False releases them.  Off until asked for."""
        self._check(lib().rt_mesh_uvs_enable(self._h, 1 if on else 0))

    def mesh_uvs(self, as_torch=None):
        """The device array of vertex UVs: a float32 [V,2] tensor that aliases it (the caller may write it on stream()), else (pointer, bytes).  The
        rows follow at the next update or mesh_uvs_refresh."""
        return self._device_array("rt_mesh_uvs", 2, as_torch)

    def mesh_set_uvs(self, uv, first=0):
        """UVs [count,2] from host memory for vertices first .., copied on stream() in call order with updates, frames and queries (rt_mesh_set_uvs);
        a non-finite component is refused.  The rows follow at the next update or mesh_uvs_refresh."""
        c = _f32(uv)
        if c.size % 2:
            raise RtError(RT_ERR_INVALID, "mesh_set_uvs: uv must hold 2 floats per vertex")
        c = np.ascontiguousarray(c.reshape(-1, 2))
        self._check(lib().rt_mesh_set_uvs(self._h, _fp(c), int(first), c.shape[0]))   # pageable memory: staged before the call returns

    def mesh_uvs_refresh(self):
        """The corner UVs gathered again from the vertex UVs; enqueued in call order with updates, frames and queries (rt_mesh_uvs_refresh): no host
        wait."""
        self._check(lib().rt_mesh_uvs_refresh(self._h))

    def mesh_uv_rows(self) -> np.ndarray:
        """The corner UVs as float32 [nTris,8] rows, (u0, v0, u1, v1), (u2, v2, 0, 0) (rt_debug_read_scene: synchronises); empty while UVs are not
        enabled or before the first rebuild.  Row i belongs to input triangle mesh_order()[i]."""
        return self.debug_read_scene(RT_SCENE_ARRAY_UV_ROWS).view(np.float32).reshape(-1, 8)

    def mesh_texture_upload(self, texels, flags=0):
        """The mesh's albedo texture (rt_mesh_texture_upload): texels uint8 [H,W,4] with row 0 at v = 0, flags TEX_* or'ed; None releases it.  With
        UVs enabled, frames of the mesh's scene with useBVH == 1 multiply the albedo of mesh hits by its sample.  May allocate and synchronise."""
        if texels is None:
            self._check(lib().rt_mesh_texture_upload(self._h, None, 0, 0, 0))
            return
        t = _texels("mesh_texture_upload", texels)
        self._check(lib().rt_mesh_texture_upload(self._h, C.c_void_p(t.ctypes.data), t.shape[1], t.shape[0], int(flags)))

    def mesh_texture(self, as_torch=None):
        """The device texels: a uint8 [H,W,4] tensor that aliases them (the caller may write it on stream(); frames and queries read the texels as
        they stand in stream order), else (pointer, bytes, W, H)."""
        ptr, n, w, h = C.c_void_p(), C.c_size_t(), C.c_int(), C.c_int()
        self._check(lib().rt_mesh_texture(self._h, C.byref(ptr), C.byref(n), C.byref(w), C.byref(h)))
        if not _wants_torch(as_torch):
            return ptr.value, n.value, w.value, h.value
        return self._alias(ptr.value, (h.value, w.value, 4), "|u1")

    def mesh_hit_uvs(self, hits):
        """The UV of each hit: float32 [N,2], hit_uvs bit for bit; zeros for a miss, an analytic hit or a prim outside the mesh.  Arguments and
        paths as mesh_hit_colors."""
        return self._mesh_hit_query("mesh_hit_uvs", hits, None, [(2, np.float32)])[0]

    def mesh_hit_texels(self, hits):
        """The texture's sample at each hit's UV: float32 [N,3], sample_texture(hit_uvs) bit for bit, not multiplied by the colour; zeros for a prim
        outside the mesh.  Arguments and paths as mesh_hit_colors."""
        return self._mesh_hit_query("mesh_hit_texels", hits, None, [(3, np.float32)])[0]

    # ---- morph targets: sparse deltas blended on the device under a weight table, before the skin or straight into the positions
    def mesh_morph_upload(self, target_first, vert_idx, deltas, base=None):
        """The morph targets of the current mesh (rt_mesh_morph_upload), in morph_positions' sparse form (morph_targets_from_dense makes it from dense
        deltas); base [V,3] base positions, None: a device-to-device snapshot of the rest array when the mesh has a skin, else of mesh_positions(),
        as it stands.  Allocates the weight table, all zero.  May synchronise; target_first=None releases the morph."""
        if target_first is None:
            self._check(lib().rt_mesh_morph_upload(self._h, None, None, None, None, 0))
            return
        nv = getattr(self, "_mesh_verts", 0)
        tf, vi, d = _morph_targets("mesh_morph_upload", target_first, vert_idx, deltas)
        b = None if base is None else _f32(base).reshape(-1, 3)
        if b is not None and b.shape[0] != nv:
            raise RtError(RT_ERR_INVALID, f"mesh_morph_upload: {b.shape[0]} base positions, the mesh has {nv} vertices")
        self._check(lib().rt_mesh_morph_upload(self._h, None if b is None else _fp(b), tf.ctypes.data_as(_I32P), vi.ctypes.data_as(_U32P), _fp(d), tf.size - 1))

    def mesh_morph_base(self, as_torch=None):
        """The device array of base positions the morph reads: a float32 [V,3] tensor that aliases it (as mesh_positions), else (pointer, bytes)."""
        return self._device_array("rt_mesh_morph_base", 3, as_torch)

    def mesh_morph_weights(self, as_torch=None):
        """The device table of target weights, zero after the upload.  With torch (as_torch=None: when it imports) a float32 [nTargets,1] tensor that
        aliases it, zero-copy; writes to it must be ordered on stream(), as for mesh_bones.  Else (pointer, bytes)."""
        return self._device_array("rt_mesh_morph_weights", 1, as_torch)

    def mesh_set_morph_weights(self, weights, first=0):
        """Weights [count] from host memory into entries first .. of the weight table, copied on stream() in call order with morphs, skins, updates,
        frames and queries (rt_mesh_set_morph_weights)."""
        w = _f32(weights).reshape(-1)
        self._check(lib().rt_mesh_set_morph_weights(self._h, int(first), w.size, _fp(w)))   # pageable memory: staged before the call returns

    def mesh_morph(self, to="positions"):
        """Enqueue dst := morph(base, targets, weight table) on stream() (rt_mesh_morph): what morph_positions computes, bit for bit, under the weight
        table as it stands when the kernel runs.  to="positions" writes mesh_positions(): follow it with mesh_refit / mesh_rebuild / mesh_update;
        to="rest" writes mesh_rest_positions(): follow it with mesh_skin.  No host wait, no allocation."""
        dst = {"positions": RT_MORPH_TO_POSITIONS, "rest": RT_MORPH_TO_REST}.get(to, to)
        if not isinstance(dst, int):
            raise RtError(RT_ERR_INVALID, f"mesh_morph: to={to!r} (\"positions\" or \"rest\")")
        self._check(lib().rt_mesh_morph(self._h, dst))

    def mesh_morph_info(self) -> RtMorphInfo:
        i = RtMorphInfo()
        self._check(lib().rt_mesh_morph_info(self._h, C.byref(i)))
        return i

    def mesh_info(self) -> RtMeshInfo:
        i = RtMeshInfo()
        self._check(lib().rt_get_mesh_info(self._h, C.byref(i)))
        return i

    def debug_read_scene(self, which) -> np.ndarray:
        """One device scene array as bytes (uint8), padding included; empty when the scene has no such array.  which: RT_SCENE_ARRAY_* or its name."""
        which = {**SCENE_ARRAYS, **SCENE_ARRAYS_OPTIONAL, **SCENE_ARRAYS_MESH}[which] if isinstance(which, str) else int(which)
        n = C.c_size_t()
        self._check(lib().rt_debug_read_scene(self._h, which, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint8)
        if n.value:
            self._check(lib().rt_debug_read_scene(self._h, which, C.c_void_p(out.ctypes.data), out.size, C.byref(n)))
        return out

    def build_bvh_gpu(self, tris9):
        """Median-split BVH built on this context's GPU -> (nodes12, tris12); build_bvh's tree wherever no median ties, and fully specified where
        one does: a stable sort per level from input order, which also fixes the order of the rows inside a leaf."""
        t = _f32(tris9).reshape(-1, 9)
        n = t.shape[0]
        nodes = np.zeros((max(2 * n, 1), 12), np.float32)
        tris = np.zeros((max(n, 1), 12), np.float32)
        k = lib().rt_build_bvh_gpu(self._h, _fp(t), n, _fp(nodes), _fp(tris))
        if k < 0:
            self._check(k)
        return nodes[:k].copy(), tris[:n].copy()

    def upload_env(self, faces):
        if faces is None:
            self._check(lib().rt_upload_env(self._h, None, 0, 0))
            return
        f = np.ascontiguousarray(faces, dtype=np.uint8)
        self._check(lib().rt_upload_env(self._h, f.ctypes.data_as(_U8P), f.shape[1], f.shape[3]))

    def resize(self, w, h):
        self._check(lib().rt_resize(self._h, w, h))
        self.width, self.height = w, h

    def reset_accum(self):
        self._check(lib().rt_reset_accum(self._h))

    @property
    def frame_index(self):
        return lib().rt_frame_index(self._h)

    def render_frame(self, u: RtUniforms):
        self._check(lib().rt_render_frame(self._h, C.byref(u)))

    def render_frames(self, us):
        """Consecutive frames, batched into as few launches as possible (rt_render_frames); us: sequence of RtUniforms."""
        arr = (RtUniforms * len(us))(*us)
        self._check(lib().rt_render_frames(self._h, arr, len(us)))

    def render_ray(self, params, cam, use_bvh=False, show_motion=False, view=None, proj=None):
        v = None if view is None else _f32(view)
        p = None if proj is None else _f32(proj)
        self._check(lib().rt_render_ray(self._h, C.byref(params), C.byref(cam), int(use_bvh), int(show_motion),
                                        None if v is None else _fp(v), None if p is None else _fp(p)))

    def set_extension(self, gi_bounces=1, env_filter=0):
        """gi_bounces: EXTENSION (not in the reference), bounces of the analytic / hybrid GI path.  env_filter: cube-map filter model
        (0 = bilinear weights in exact fp32, the default; 1 = texel coordinates rounded to 1/256 texel first)."""
        e = RtExtension(giBounces=int(gi_bounces), envFilter=int(env_filter))
        self._check(lib().rt_set_extension(self._h, C.byref(e)))

    def render_ray_frames(self, params, cam, count, use_bvh=False, show_motion=False):
        self._check(lib().rt_render_ray_frames(self._h, C.byref(params), C.byref(cam), int(use_bvh), int(show_motion), int(count)))

    def synchronize(self):
        self._check(lib().rt_synchronize(self._h))

    def read_target(self, which, fmt=RT_FORMAT_F16) -> np.ndarray:
        ch = TARGET_CHANNELS[which]
        out = np.zeros((self.height, self.width, ch), np.uint16 if fmt == RT_FORMAT_F16 else np.float32)
        self._check(lib().rt_read_target(self._h, which, out.ctypes.data_as(C.c_void_p), fmt))
        return out

    def write_target(self, which, image) -> None:
        """Overwrite a target of the last frame from an [H, W, channels] uint16 (half bits) image; COLOR = the history."""
        a = np.ascontiguousarray(image, np.uint16)
        if a.shape != (self.height, self.width, TARGET_CHANNELS[which]):
            raise ValueError(f"write_target: expected {(self.height, self.width, TARGET_CHANNELS[which])}, got {a.shape}")
        self._check(lib().rt_write_target(self._h, which, a.ctypes.data_as(C.c_void_p), RT_FORMAT_F16))

    def present(self, params, show_motion=False) -> np.ndarray:
        """Present pass over the last frame -> [H, W, 4] uint8 (row 0 = bottom)."""
        pp = make_present_params(params, show_motion, self.width, self.height)
        out = np.zeros((self.height, self.width, 4), np.uint8)
        self._check(lib().rt_present(self._h, C.byref(pp), out.ctypes.data_as(_U8P)))
        return out

    def present_with(self, pp: RtPresentParams) -> np.ndarray:
        """Present pass with an explicit rt_present.frag uniform block."""
        out = np.zeros((self.height, self.width, 4), np.uint8)
        self._check(lib().rt_present(self._h, C.byref(pp), out.ctypes.data_as(_U8P)))
        return out

    def history_exchange_buffer(self):
        """(device pointer, bytes) of the buffer the ranks' COLOR0 blocks of the last frame are all-gathered into (moving camera)."""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(lib().rt_history_exchange_buffer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def history_exchanged(self):
        self._check(lib().rt_history_exchanged(self._h))

    def present_gathered(self, pp: RtPresentParams, color_ptr, motion_ptr, gpos_ptr, gnrm_ptr) -> np.ndarray:
        """Present pass on the gathering rank over four device arrays of gathered blocks -> [H, W, 4] uint8."""
        out = np.zeros((self.height, self.width, 4), np.uint8)
        self._check(lib().rt_present_gathered(self._h, C.byref(pp), C.c_void_p(color_ptr), C.c_void_p(motion_ptr), C.c_void_p(gpos_ptr),
                                              C.c_void_p(gnrm_ptr), out.ctypes.data_as(_U8P)))
        return out

    def read_all(self):
        return [self.read_target(i) for i in range(4)]

    # ---- tile-parallel exchange owned by the library (RCCL behind the C ABI)
    def comm_init(self, comm_id: bytes):
        """Collective over the ranks of the frame.  comm_id: the 128 bytes rank 0 got from comm_unique_id()."""
        buf = C.create_string_buffer(bytes(comm_id), RT_COMM_ID_BYTES)
        self._check(lib().rt_comm_init(self._h, buf, RT_COMM_ID_BYTES))

    def comm_destroy(self):
        self._check(lib().rt_comm_destroy(self._h))

    def gather_frame(self, which=RT_TARGET_COLOR):
        """Enqueue the gather of the last frame's target to rank 0 (+ un-tiling there) on that frame's stream."""
        self._check(lib().rt_gather_frame(self._h, which))

    def gathered_frame_ptr(self, which=RT_TARGET_COLOR):
        p, n = C.c_void_p(), C.c_size_t()
        self._check(lib().rt_gathered_frame(self._h, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    def read_gathered(self, which=RT_TARGET_COLOR) -> np.ndarray:
        """Rank 0: the frame of the last gather_frame(which) as half bit patterns [H, W, C] (synchronises)."""
        out = np.zeros((self.height, self.width, TARGET_CHANNELS[which]), np.uint16)
        self._check(lib().rt_read_gathered(self._h, which, out.ctypes.data_as(C.c_void_p)))
        return out

    def present_last_gathered(self, pp: RtPresentParams) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), np.uint8)
        self._check(lib().rt_present_last_gathered(self._h, C.byref(pp), out.ctypes.data_as(_U8P)))
        return out

    def exchange_history(self):
        """All-gather of the last frame's COLOR0 blocks so that the next frame may reproject across tiles (moving camera)."""
        self._check(lib().rt_exchange_history(self._h))

    def comm_info(self) -> RtCommInfo:
        """What the RCCL communicator reports about itself (commWorld / commRank, -1 without one) + gather counts and bytes of this context."""
        i = RtCommInfo()
        self._check(lib().rt_comm_info(self._h, C.byref(i)))
        return i

    def local_target(self, which):
        p, n = C.c_void_p(), C.c_size_t()
        self._check(lib().rt_local_target(self._h, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    def gather_block_bytes(self, which):
        n = C.c_size_t()
        self._check(lib().rt_gather_block_bytes(self._h, which, C.byref(n)))
        return n.value

    def assemble_gathered(self, which, gathered_ptr, dst_ptr):
        self._check(lib().rt_assemble_gathered(self._h, which, C.c_void_p(gathered_ptr), C.c_void_p(dst_ptr)))

    def stream(self):
        s = C.c_void_p()
        self._check(lib().rt_stream(self._h, C.byref(s)))
        return s.value

    def counters(self) -> RtCounters:
        c = RtCounters()
        self._check(lib().rt_get_counters(self._h, C.byref(c)))
        return c

    def reset_counters(self):
        self._check(lib().rt_reset_counters(self._h))

    def scene_info(self) -> RtSceneInfo:
        i = RtSceneInfo()
        self._check(lib().rt_get_scene_info(self._h, C.byref(i)))
        return i

    def memory_info(self) -> RtMemoryInfo:
        i = RtMemoryInfo()
        self._check(lib().rt_get_memory_info(self._h, C.byref(i)))
        return i

    def traced_rays(self, reset=False) -> RtTracedRays:
        t = RtTracedRays()
        self._check(lib().rt_get_traced_rays(self._h, C.byref(t), int(reset)))
        return t

    def enable_stage_timing(self, on=True):
        self._check(lib().rt_enable_stage_timing(self._h, int(on)))

    def stage_times(self):
        t = RtStageTimes()
        self._check(lib().rt_get_stage_times(self._h, C.byref(t)))
        return {"frames": t.frames,
                "stages": {lib().rt_stage_name(i).decode(): {"ms": t.ms[i], "launches": t.launches[i]}
                           for i in range(t.nStages) if t.launches[i]}}

    def debug_eval(self, op, a, b=None, c=None) -> np.ndarray:
        a = _f32(a).reshape(-1)
        b = None if b is None else _f32(b).reshape(-1)
        c = None if c is None else _f32(c).reshape(-1)
        out = np.zeros(a.size, np.uint32)
        self._check(lib().rt_debug_eval(self._h, op, _fp(a), None if b is None else _fp(b), None if c is None else _fp(c),
                                        out.ctypes.data_as(_U32P), a.size))
        return out

    def debug_trace(self, kind, origins, dirs, tmax=None, eps=1e-4, inf=1e30) -> np.ndarray:
        o, d = _f32(origins).reshape(-1, 3), _f32(dirs).reshape(-1, 3)
        t = np.full(o.shape[0], inf, np.float32) if tmax is None else _f32(tmax).reshape(-1)
        out = np.zeros((o.shape[0], 7), np.float32)
        self._check(lib().rt_debug_trace(self._h, kind, _fp(o), _fp(d), _fp(t), eps, inf, _fp(out), o.shape[0]))
        return out

    def trace_rays(self, origins, dirs, tmax=None, any_hit=False, eps=1e-4, inf=1e30, normals=False):
        """Ray queries against the uploaded BVH (rt_trace_rays).  origins / dirs: float32 [N,k] with k >= 3 (ray i in row i; rows
        may be strided, e.g. the two halves of one [N,8] array), tmax: float32 [N] or None (closest hit; tmax[i] < 0 marks an empty slot).
        eps / inf are uEPS / uINF (rt_make_uniforms' defaults).  Closest hit -> RayHits; any hit (tmax required) -> occluded [N] bool.
        numpy arrays go through rt_trace_rays_host and come back as numpy arrays.  torch tensors on this context's device take the zero-copy
        path: the library stream waits for torch's current stream, torch's current stream waits for the query, no host synchronisation; the
        answers are allocated on torch's current stream."""
        kind = RT_QUERY_ANY if any_hit else RT_QUERY_CLOSEST
        if any_hit and tmax is None:
            raise _query_invalid("any-hit queries need tmax")
        dev, n, os_, ds, tmax_ = _ray_check(origins, dirs, tmax, self, own=True)
        rays = (_ptr(origins), os_, _ptr(dirs), ds, _ptr(tmax_), eps, inf, n)
        if any_hit:
            occ = _new(dev, n, np.uint8, zero=True)
            self._query(dev, "rt_trace_rays", (origins, dirs, tmax), kind, *rays, None, None, _ptr(occ))
            return _as_bool(occ)
        rec = _new(dev, (n, 4))
        nrm = _new(dev, (n, 3)) if normals else None
        self._query(dev, "rt_trace_rays", (origins, dirs, tmax), kind, *rays, _ptr(rec), _ptr(nrm), None)
        return RayHits(rec, nrm)

    @contextlib.contextmanager
    def _library_stream(self, dev, inputs):
        """The stream protocol of every zero-copy torch path, here and nowhere else: `with ... as run`, and each run(entry, *args)
        is one pass -- the library stream waits for torch's current stream, so the inputs and the outputs, allocated and filled before the first
        pass, are ready; the C call entry(context, *args), checked; torch's current stream waits for the library stream, so the work behind it
        sees the answers.  At the end the input tensors are recorded on torch's current stream.
        Lifetimes: a block freed on torch's current stream is reused only by work queued behind the second wait, i.e. behind the query; input
        tensors of other streams are tied to the current stream by the record.  Never to the library stream: it dies with the context, before
        the tensors may, and the allocator would record an event on it when they are freed -- so nothing is recorded where the caller runs the
        query under torch.cuda.stream(ExternalStream(self.stream()))."""
        import torch
        ext = torch.cuda.ExternalStream(self.stream(), device=dev)
        cur = torch.cuda.current_stream(dev)

        def run(entry, *args):
            ext.wait_stream(cur)
            self._check(entry(self._h, *args))
            cur.wait_stream(ext)

        yield run
        if cur.cuda_stream == ext.cuda_stream:      # the caller made the library stream torch's current one: a record would tie the tensors to it
            return
        for a in inputs:
            if a is not None:
                a.record_stream(cur)

    def _query(self, dev, name, inputs, *args):
        """One query call on the arrays `inputs`: the C entry `name`_host for numpy arrays (dev None), which synchronises; `name` on the library
        stream for tensors on dev, ordered against torch's current stream and without a host wait."""
        if dev is None:
            self._check(getattr(lib(), name + "_host")(self._h, *args))
            return
        with self._library_stream(dev, inputs) as run:
            run(getattr(lib(), name), *args)

    def trace_scene_rays(self, u, origins, dirs, tmax=None, any_hit=False, skip_glass=False, skip_marker=False, normals=False, points=False):
        """Ray queries against the scene a frame rendered with uniforms `u` shows (rt_trace_scene_rays): u.useBVH picks the analytic
        scene, the uploaded BVH or the hybrid scene; u.eps / u.inf, the marker and u.nodeCount / u.triCount come from u.  Rays and tmax as trace_rays.
        Closest hit -> SceneHits; any hit (tmax required) -> occluded [N] bool.  numpy arrays go through rt_trace_scene_rays_host, torch tensors
        on this context's device take the zero-copy path of trace_rays."""
        kind = RT_QUERY_ANY if any_hit else RT_QUERY_CLOSEST
        flags = (RT_QUERY_SKIP_GLASS if skip_glass else 0) | (RT_QUERY_SKIP_MARKER if skip_marker else 0)
        if any_hit and tmax is None:
            raise _query_invalid("any-hit queries need tmax")
        dev, n, os_, ds, tmax_ = _ray_check(origins, dirs, tmax, self)
        rays = (C.byref(u), kind, flags, _ptr(origins), os_, _ptr(dirs), ds, _ptr(tmax_), n)
        if any_hit:
            occ = _new(dev, n, np.uint8, zero=True)
            self._query(dev, "rt_trace_scene_rays", (origins, dirs, tmax), *rays, None, None, None, None, _ptr(occ))
            return _as_bool(occ)
        ans = self._scene_hits(dev, n, normals, points)
        self._query(dev, "rt_trace_scene_rays", (origins, dirs, tmax), *rays, *(_ptr(a) for a in ans), None)
        return SceneHits(*ans)

    def _scene_hits(self, dev, n, normals, points):
        """The outputs of a closest-hit scene query: (record, object, normal or None, point or None), as SceneHits takes them."""
        return _new(dev, (n, 4)), _new(dev, n, np.int32), _new(dev, (n, 3)) if normals else None, _new(dev, (n, 3)) if points else None

    def _pixels(self, xy):
        """The pixel check of pick and pick_multi: int32 [N,2]; a numpy array is made contiguous, a tensor must be -> (torch device or None for
        numpy, n, xy to pass)."""
        if isinstance(xy, np.ndarray):
            if xy.dtype != np.int32 or xy.ndim != 2 or xy.shape[1] != 2:
                raise _query_invalid(f"xy must be int32 [N,2], got {xy.dtype} {xy.shape}")
            return None, xy.shape[0], np.ascontiguousarray(xy)
        import torch
        if not isinstance(xy, torch.Tensor) or xy.dtype != torch.int32 or xy.dim() != 2 or xy.shape[1] != 2 or not xy.is_contiguous():
            raise _query_invalid("xy must be an int32 [N,2] numpy array or contiguous torch tensor")
        return _device_of(self.device, (("xy", xy),), torch.int32), xy.shape[0], xy

    def pick(self, u, xy, normals=True, points=True):
        """What pixels (x, y) (int32 [N,2], row 0 = bottom) of a frame rendered with uniforms `u` show (rt_pick_pixels): each is traced
        along the frame's own primary ray (jitter included) through the frame's scene -> SceneHits.  numpy or torch, as trace_scene_rays."""
        dev, n, xy = self._pixels(xy)
        ans = self._scene_hits(dev, n, normals, points)
        self._query(dev, "rt_pick_pixels", (xy,), C.byref(u), _ptr(xy), n, *(_ptr(a) for a in ans))
        return SceneHits(*ans)

    def trace_rays_multi(self, origins, dirs, tmax=None, max_hits=4, eps=1e-4, inf=1e30) -> MultiHits:
        """The max_hits nearest hits and the hit count of every ray against the uploaded BVH (rt_trace_rays_multi) -> MultiHits, equal
        to multi_hits on the uploaded arrays bit for bit.  Rays, tmax, eps / inf and the numpy / torch paths (stream ordering and lifetimes included)
        as trace_rays.  The walk visits every box along the ray up to tmax: bound the work with tmax.  max_hits = 0 asks for the counts alone."""
        k = _multi_k(max_hits)
        dev, n, os_, ds, tmax_ = _ray_check(origins, dirs, tmax, self)
        hits, count = _new(dev, (n, k, 4)), _new(dev, n, np.int32)
        p = _ptr0
        self._query(dev, "rt_trace_rays_multi", (origins, dirs, tmax), p(origins), os_, p(dirs), ds, p(tmax_), eps, inf, n, k, p(hits), p(count))
        return MultiHits(hits, count)

    def pick_multi(self, u, xy, max_hits=4) -> MultiHits:
        """The max_hits nearest hits and the hit count under pixels (x, y) (int32 [N,2], row 0 = bottom) of a BVH frame rendered with uniforms `u`
        (rt_pick_pixels_multi): each along the frame's own primary ray, jitter included, up to u.inf -> MultiHits.  numpy or torch, as pick."""
        k = _multi_k(max_hits)
        dev, n, xy = self._pixels(xy)
        hits, count = _new(dev, (n, k, 4)), _new(dev, n, np.int32)
        self._query(dev, "rt_pick_pixels_multi", (xy,), C.byref(u), _ptr0(xy), n, k, _ptr0(hits), _ptr0(count))
        return MultiHits(hits, count)

    def nearest_points(self, points, max_dist=None, visits=False) -> NearestPoints:
        """The nearest surface point of the uploaded BVH or the dynamic mesh for every point (rt_query_nearest) -> NearestPoints, equal
        to nearest_points on the same arrays bit for bit.  points: float32 [N,k], k >= 3, rows may be strided; max_dist: float32 [N] or None
        (max_dist[i] < 0 marks an empty slot).  An unbounded query far from the mesh costs more than one near it: give max_dist where a bound is
        known.  visits=True also returns the number of boxes tested per point (a diagnostic).  numpy / torch paths, stream ordering and lifetimes
        as trace_rays_multi."""
        dev, n, stride, limit = _point_check(points, max_dist, self)
        hits, closest = _new(dev, (n, 4)), _new(dev, (n, 3))
        vis = _new(dev, n, np.int32) if visits else None
        p = _ptr0
        self._query(dev, "rt_query_nearest", (points, max_dist), p(points), stride, p(limit), n, p(hits), p(closest), p(vis))
        return NearestPoints(hits, closest, vis)

    def nearest_points_multi(self, points, max_hits, max_dist=None, counts=True, visits=False) -> NearestMulti:
        """The max_hits nearest rows of the uploaded BVH or the dynamic mesh for every point, and the count of all the rows within its limit
        (rt_query_nearest_multi) -> NearestMulti, equal to nearest_points_multi on the same arrays bit for bit.  Points, max_dist,
        visits, the numpy / torch paths, stream ordering and lifetimes as nearest_points.  counts=False leaves the count out and lets the walk cull
        against its max_hits-th best; with counts it visits every box within max_dist, so give max_dist.  max_hits = 0 asks for the counts alone."""
        k = _nearest_multi_k(max_hits, counts)
        dev, n, stride, limit = _point_check(points, max_dist, self)
        hits, closest = _new(dev, (n, k, 4)), _new(dev, (n, k, 3))
        count = _new(dev, n, np.int32) if counts else None
        vis = _new(dev, n, np.int32) if visits else None
        p = _ptr0
        self._query(dev, "rt_query_nearest_multi", (points, max_dist), p(points), stride, p(limit), n, k, p(hits), p(count), p(closest), p(vis))
        return NearestMulti(hits, closest, count, vis)

    def box_overlaps(self, boxes, cap=None, visits=False) -> BoxOverlaps:
        """The rows of the uploaded BVH or the dynamic mesh that overlap each axis-aligned box (rt_query_boxes) -> BoxOverlaps, equal to
        box_overlaps on the same arrays bit for bit.  boxes: float32 [N,k], k >= 6 (lo.xyz, hi.xyz), rows may be strided; a NaN component or lo > hi
        marks an empty slot.  cap=None: the exact lists in two passes -- count, an exclusive scan (torch.cumsum on the device), allocate, list: the
        allocation waits for the total.  cap=k: one call into k entries per box, no host wait; count[i] > k says that box i overflowed.  visits=True
        also returns the number of boxes tested per box.  One lane walks one box: few boxes that each list very many rows run serially.  numpy /
        torch paths, stream ordering and lifetimes as nearest_points."""
        return self._overlap_query("rt_query_boxes", BoxOverlaps, _BOXES, boxes, cap, visits)

    def _overlap_query(self, name, result, family, queries, cap, visits):
        """box_overlaps, tri_overlaps and hull_overlaps: the checks, then _overlaps."""
        cap = _box_cap(cap)
        dev, n, stride = _row_array(family, queries, self)
        return self._overlaps(name, result, dev, n, stride, queries, cap, visits)

    def _overlaps(self, name, result, dev, n, stride, queries, cap, visits, adapt=lambda entry: entry):
        """Both forms of an overlap query over n checked query rows through the C entry `name` (numpy, dev None: `name`_host) -> result(count,
        offsets, prims, visits).  adapt wraps the entry where its arguments are not (context, queries, stride, n, offsets, cap, prims, counts,
        visits) as they stand."""
        if dev is None:
            entry = adapt(getattr(lib(), name + "_host"))
            return _numpy_box_query(lambda *a: self._check(entry(self._h, *a)), result, queries, n, stride, cap, visits)
        return self._device_overlaps(adapt(getattr(lib(), name)), result, queries, stride, dev, cap, visits)

    def _device_overlaps(self, entry, result, boxes, stride, dev, cap, visits):
        """Both forms of an overlap query on a torch device tensor of queries (`boxes`, rows `stride` floats apart), through the C entry `entry`
        -> result(count, offsets, prims, visits).  One pass of the stream protocol per call, the queries recorded once."""
        import torch
        n = boxes.shape[0]
        if cap is not None and n * cap > 2 ** 31 - 1:
            raise _query_invalid(f"{n} boxes x cap {cap} exceed INT32_MAX entries")
        count = torch.zeros(n, dtype=torch.int32, device=dev)
        vis = torch.zeros(n, dtype=torch.int32, device=dev) if visits else None
        p = _ptr0
        with self._library_stream(dev, (boxes,)) as run:
            if cap is not None:
                offsets = (torch.arange(n + 1, dtype=torch.int64, device=dev) * cap).to(torch.int32)
                prims = torch.full((n * cap,), -1, dtype=torch.int32, device=dev)
                if n:
                    run(entry, p(boxes), stride, n, None, cap, p(prims), p(count), p(vis))          # (cap = 0: no prims, the counts alone)
            else:
                offsets = torch.zeros(n + 1, dtype=torch.int32, device=dev)
                total = 0
                if n:
                    run(entry, p(boxes), stride, n, None, 0, None, p(count), p(vis))
                    scan = torch.cumsum(count, 0, dtype=torch.int64)
                    total = int(scan[-1])        # (the one host wait of the exact form: the list's allocation needs the total)
                    if total > 2 ** 31 - 1:
                        raise _query_invalid(f"the lists hold {total} entries, beyond INT32_MAX")
                    offsets[1:] = scan.to(torch.int32)
                prims = torch.full((total,), -1, dtype=torch.int32, device=dev)
                if total:
                    run(entry, p(boxes), stride, n, p(offsets), 0, p(prims), None, None)
        return result(count, offsets, prims, vis)

    def tri_overlaps(self, qtris, cap=None, visits=False) -> TriOverlaps:
        """The rows of the uploaded BVH or the dynamic mesh that each query triangle intersects (rt_query_tris) -> TriOverlaps, equal to
        tri_overlaps on the same arrays bit for bit.  qtris: float32 [N,9], [N,3,3] or [N,k], k >= 9 (p0.xyz, p1.xyz, p2.xyz), rows may be strided; a
        NaN component marks an empty slot.  cap, visits, the numpy / torch paths, stream ordering and lifetimes as box_overlaps; visits equals
        box_overlaps' for the boxes of the queries' points.  A self query lists every neighbour that shares a vertex: filter `.pairs()` by the index
        buffer.  One lane walks one query."""
        return self._overlap_query("rt_query_tris", TriOverlaps, _QTRIS, qtris, cap, visits)

    def hull_overlaps(self, hulls, cap=None, visits=False) -> HullOverlaps:
        """The rows of the uploaded BVH or the dynamic mesh that overlap each convex hexahedron (rt_query_hulls) -> HullOverlaps, equal
        to hull_overlaps on the same arrays bit for bit.  hulls: float32 [N,24], [N,8,3] or [N,k], k >= 24 (c0.xyz .. c7.xyz), rows may be strided; a
        NaN among the 24 floats marks an empty slot.  box_corners and rect_frusta make hulls of boxes under matrices and of rects of the frame.  cap,
        visits, the numpy / torch paths, stream ordering and lifetimes as box_overlaps; visits never exceeds box_overlaps' for the boxes of the
        hulls' corners.  One lane walks one hull."""
        return self._overlap_query("rt_query_hulls", HullOverlaps, _HULLS, hulls, cap, visits)

    def pick_rects(self, u, rects, t_near=0.0, t_far=None, cap=None, visits=False) -> HullOverlaps:
        """Marquee picking (rt_pick_rects): the rows of the uploaded BVH or the dynamic mesh inside the frustum behind each rect of u's
        frame, hidden ones included -> HullOverlaps whose `corners` [N,24] are the frusta, equal to rect_frusta bit for bit, and whose lists equal
        hull_overlaps on them.  rects: float32 [N,k], k >= 4 (x0, y0, x1, y1 in pixel-corner coordinates, row 0 at the bottom: pixel (x, y) covers
        [x, x+1] x [y, y+1]); t_near, t_far as rect_frusta, the root box the scene's own as it stands on the device.  cap, visits, the numpy / torch
        paths, stream ordering and lifetimes as box_overlaps."""
        cap = _box_cap(cap)
        if not isinstance(u, RtUniforms):
            raise _query_invalid("u must be an RtUniforms")
        tn, tf = float(t_near), -1.0 if t_far is None else float(t_far)
        dev, n, stride = _row_array(_RECTS, rects, self)
        corners = _new(dev, (n, 24), zero=True)
        pc = _ptr0(corners)
        adapt = lambda entry: lambda h, r, stride_, n_, *a: entry(h, C.byref(u), r, stride_, n_, tn, tf, pc, *a)
        ans = self._overlaps("rt_pick_rects", HullOverlaps, dev, n, stride, rects, cap, visits, adapt)
        ans.corners = corners
        return ans

    def raster_mesh(self, slot, positions, indices=None):
        """Upload one mesh for the raster preview (Mesh::setupMesh); positions [N,3] float32, indices uint32 triples.  None frees the slot."""
        if positions is None:
            self._check(lib().rt_raster_mesh(self._h, slot, None, 0, None, 0))
            return
        p = _f32(positions).reshape(-1, 3)
        i = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        self._check(lib().rt_raster_mesh(self._h, slot, _fp(p), p.shape[0], i.ctypes.data_as(_U32P), i.size))

    def raster_mesh_dynamic(self, slot, parts=False, colors=None):
        """Bind a raster mesh slot to the dynamic mesh (rt_raster_mesh_dynamic): draws naming it read mesh_positions() and the
        uploaded indices where they lie.  parts=False: the draw's model for every triangle; parts=True: draw.model times each part's matrix of
        mesh_part_matrices().  colors ([nParts,3], parts=True only): a flat colour per part instead of the draw's.  The binding follows later
        mesh_upload / mesh_upload_parts calls; raster_mesh(slot, None) unbinds."""
        self._check(lib().rt_raster_mesh_dynamic(self._h, int(slot), RT_RASTER_BIND_PARTS if parts else RT_RASTER_BIND_SINGLE))
        if colors is not None:
            self.raster_part_colors(slot, colors)

    def raster_part_colors(self, slot, colors):
        """A flat colour per part ([nParts,3] floats, packed as a draw's colour is) for a slot bound with parts=True; None returns to the draw's
        colour (rt_raster_part_colors).  The count must equal the mesh's part count when a draw uses the table."""
        if colors is None:
            self._check(lib().rt_raster_part_colors(self._h, int(slot), None, 0))
            return
        c = _f32(colors)
        if c.size % 3:
            raise RtError(RT_ERR_INVALID, "raster_part_colors: colors must hold 3 floats per part")
        c = c.reshape(-1, 3)
        self._check(lib().rt_raster_part_colors(self._h, int(slot), _fp(c), c.shape[0]))

    def raster_targets(self, as_torch=None):
        """(rgba8 [H,W,4] uint8, prim_id [H,W], depth24 [H,W]) of the last raster frame, row 0 = bottom (rt_raster_targets).  With torch
        (as_torch=None: when it imports) tensors that alias the device buffers, zero-copy and without a host wait: torch's current stream is made to
        wait for the library stream, as trace_rays does it; prim_id and depth24 are int32 views of the uint32 words (the background id reads -1).
        They are valid until a raster call grows the buffers or resize().  Else numpy copies (read_raster)."""
        a, b, c, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        self._check(lib().rt_raster_targets(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        if not _wants_torch(as_torch):
            return self.read_raster()
        import torch
        dev = torch.device("cuda", self.device)
        h, w = self.height, self.width
        out = self._alias(a.value, (h, w, 4), "|u1"), self._alias(b.value, (h, w), "<i4"), self._alias(c.value, (h, w), "<i4")
        torch.cuda.current_stream(dev).wait_stream(torch.cuda.ExternalStream(self.stream(), device=dev))   # torch's reads see the raster frame
        return out

    def render_raster_async(self, draws, view, proj):
        arr = (RtRasterDraw * max(len(draws), 1))(*draws)
        v, p = _f32(view).reshape(-1), _f32(proj).reshape(-1)
        self._check(lib().rt_render_raster(self._h, arr, len(draws), _fp(v), _fp(p)))

    def read_raster(self):
        """(rgba8 [H,W,4] uint8, prim_id [H,W] uint32, depth24 [H,W] uint32) of the last raster frame, row 0 = bottom."""
        rgba = np.zeros((self.height, self.width, 4), np.uint8)
        prim = np.zeros((self.height, self.width), np.uint32)
        depth = np.zeros((self.height, self.width), np.uint32)
        self._check(lib().rt_read_raster(self._h, rgba.ctypes.data_as(_U8P), prim.ctypes.data_as(_U32P), depth.ctypes.data_as(_U32P)))
        return rgba, prim, depth

    def render_raster(self, draws, view, proj):
        """renderRaster: clear + draws (RtRasterDraw list) with currView / currProj -> read_raster()."""
        self.render_raster_async(draws, view, proj)
        return self.read_raster()

    def debug_raster_bin_capacity(self, pairs):
        """Diagnostics: bin arrays of exactly `pairs` pairs for the following raster calls (0: automatic)."""
        self._check(lib().rt_debug_raster_bin_capacity(self._h, int(pairs)))

    def raster_stats(self) -> RtRasterStats:
        s = RtRasterStats()
        self._check(lib().rt_get_raster_stats(self._h, C.byref(s)))
        return s

    def bounce_probe(self, reset=False) -> RtBounceProbe:
        """Counts of the bounce probe (RT_BOUNCE_PROBE) since the last reset: rays walked any-hit first, rays re-traced closest-hit, bounce
        launches with / without the probe (rt_debug_bounce_probe)."""
        b = RtBounceProbe()
        self._check(lib().rt_debug_bounce_probe(self._h, C.byref(b), int(reset)))
        return b

    def disk_skip(self, reset=False) -> RtDiskSkip:
        """Counts of the disk-light skip since the last reset, for k_gen_direct and k_gen_gi: (hit, sample) pairs shaded, pairs proved unlit, pairs whose
        wave skipped the disk loop, waves, waves that skipped (rt_debug_disk_skip).  The kernels count from the first call on: call once with reset first."""
        b = RtDiskSkip()
        self._check(lib().rt_debug_disk_skip(self._h, C.byref(b), int(reset)))
        return b

    def gi_list(self, reset=False) -> RtGiList:
        """Counts of the bounce-hit generator since the last reset: (hit, sample) pairs visited, pairs shaded, launches over the bounce probe's hit list /
        over every pair (rt_debug_gi_list).  The kernels count from the first call on: call once with reset first."""
        b = RtGiList()
        self._check(lib().rt_debug_gi_list(self._h, C.byref(b), int(reset)))
        return b

    def light_masks(self, reset=False) -> RtLightMasks:
        """Counts of the light-slot liveness masks since the last reset: bits set for shadow queue 1 / 2, mask words the any-hit launches scanned, their
        masked refill passes, mask words of the last chunk (rt_debug_light_masks).  The kernels count from the first call on: call once with reset first."""
        b = RtLightMasks()
        self._check(lib().rt_debug_light_masks(self._h, C.byref(b), int(reset)))
        return b

    def beam_cull_stats(self, reset=False) -> RtBeamCullStats:
        """Counts of the beam cull since the last reset: tiles walked, dead tiles, tiles kept because a level of the walk overflowed, levels walked
        (rt_debug_beam_cull_stats).  The kernel counts from the first call on: call once with reset first."""
        b = RtBeamCullStats()
        self._check(lib().rt_debug_beam_cull_stats(self._h, C.byref(b), int(reset)))
        return b

    def beam_cull_flags(self, n_local_tiles) -> np.ndarray:
        """uint8 [n_local_tiles] (frame_geom(...).nLocalTiles of this rank): the dead flags of the launch set rendered last (rt_debug_beam_cull_flags:
        synchronises); RtError(RT_ERR_STATE) when that set was not culled."""
        out = np.zeros(int(n_local_tiles), np.uint8)
        self._check(lib().rt_debug_beam_cull_flags(self._h, out.ctypes.data_as(_U8P), out.size))
        return out

    def debug_disk_unlit(self, u, hp, normals, seeds=64):
        """rt_debug_disk_unlit: (unlit, lit, maxDot) arrays for n (hp, normal) pairs -- the per-hit test, whether any of the four disk samples of `seeds`
        seeds had geom != 0, and the largest dot(N, L) they computed."""
        hp = np.ascontiguousarray(hp, dtype=np.float32).reshape(-1, 3)
        nr = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        n = hp.shape[0]
        if nr.shape[0] != n:
            raise ValueError("hp and normals differ in length")
        flags = np.zeros(n, dtype=np.uint8)
        md = np.zeros(n, dtype=np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        self._check(lib().rt_debug_disk_unlit(self._h, C.byref(u), fp(hp), fp(nr), n, int(seeds), flags.ctypes.data_as(C.POINTER(C.c_uint8)), fp(md)))
        return (flags & 1) != 0, (flags & 2) != 0, md

    def debug_build_bits(self, reset=False) -> int:
        """rt_debug_builds as the raw RT_BUILD_* word (closest-hit half, any-hit half << RT_BUILD_ANY_SHIFT)."""
        v = C.c_uint32(0)
        self._check(lib().rt_debug_builds(self._h, C.byref(v), 1 if reset else 0))
        return v.value

    def debug_builds(self, reset=True) -> dict:
        """The traversal kernel builds launched since the last reset (frames and debug_trace kinds 2 - 4), as
        {"closest": frozenset of RT_BUILD_BITS names, "any": ...}."""
        v = C.c_uint32(0)
        self._check(lib().rt_debug_builds(self._h, C.byref(v), 1 if reset else 0))
        half = lambda b: frozenset(n for n, m in RT_BUILD_BITS.items() if b & m)
        return {"closest": half(v.value & 0xFFFF), "any": half(v.value >> RT_BUILD_ANY_SHIFT)}


def frame_uniforms(params, cam, w, h, frame_index, use_bvh, node_count=0, tri_count=0, prev_vp=None, env_loaded=True,
                   show_motion=False) -> RtUniforms:
    """Static-camera convenience: the uniform block mainLoop would hand renderRay for this frame."""
    view, proj = camera_view(cam), camera_proj(cam)
    vp = mat4_mul(proj, view)
    prev = vp if prev_vp is None else prev_vp
    moved = camera_moved(vp, prev)
    return make_uniforms(params, cam, view, vp, prev, w, h, frame_index, moved, use_bvh, show_motion, node_count, tri_count, env_loaded)
