"""The refusals of the C API outside the dynamic mesh, as one table shared by tests/golden/make_api_golden.py, which recorded them on the
commit before csrc/rt_api.hip was split into rt_api_exchange.hip, rt_api_query.hip and rt_api_debug.hip, and tests/test_gpu_api_contract.py, which
holds the library to that record.  The mechanism is that of tests/mesh_api_cases.py.

A case is a context state, a raw ctypes call of an exported entry point and what came back: the return code and rt_last_error's text when the call
was refused.  Every call here is refused before any device work, or (n = 0) does none; the device entries are nevertheless given real device memory
of eight records, so that a library that failed to refuse would do no harm.  No output may be written."""
import ctypes as C

import numpy as np

import opengl_raytracing_amd as rt
import scenes

f32 = np.float32
W, H = 32, 16
N_REC = 8
SENTINEL = 0x5A

STATES = ("fresh", "fresh_raster", "sized", "rendered", "rank0of2", "rank1of2")
ALL = STATES
SIZED = ("sized", "rendered", "rank0of2", "rank1of2")
RANKS = ("rank0of2", "rank1of2")
NO_BVH = tuple(s for s in STATES if s != "rendered")


def uniforms(use_bvh=False, nodes=0, tris=0, w=W, h=H):
    return rt.frame_uniforms(rt.default_render_params(), rt.default_camera(), w, h, 0, use_bvh, nodes, tris)


def make(state, device=0):
    """A fresh Renderer brought into `state`.  fresh_raster: a rasteriser, no framebuffer; rendered: a BVH of two triangles, one frame, its COLOR
    target gathered (and no other); rank r of 2: a tile-parallel context without a communicator, one analytic frame rendered."""
    r = rt.Renderer(device=device, rank=1 if state == "rank1of2" else 0, world_size=2 if state in RANKS else 1)
    if state == "fresh_raster":
        assert rt.lib().rt_debug_raster_bin_capacity(r._h, 0) == rt.RT_OK
    if state in SIZED:
        r.resize(W, H)
    if state == "rendered":
        nodes, tris = scenes.one_leaf_mesh()
        r.upload_bvh(nodes, tris)
        r.render_frame(uniforms(True, nodes.shape[0], tris.shape[0]))
        r.gather_frame(rt.RT_TARGET_COLOR)
    if state in RANKS:
        r.render_frame(uniforms())
    r.synchronize()
    return r


class Buffers:
    """Host and device memory for the calls: eight rays, pixels and records; every output pre-filled with SENTINEL bytes."""
    IN = {"origins": (N_REC * 3, f32), "dirs": (N_REC * 3, f32), "tmax": (N_REC, f32), "xy": (N_REC * 2, np.int32)}
    OUT = {"hits": N_REC * 16, "objects": N_REC * 4, "normals": N_REC * 12, "points": N_REC * 12, "occluded": N_REC, "image": W * H * 16}

    def __init__(self, device):
        import torch
        dev = torch.device("cuda", device)
        self.h = {k: np.ones(n, t) for k, (n, t) in self.IN.items()}
        self.d = {k: torch.from_numpy(v).to(dev) for k, v in self.h.items()}
        self.h.update({k: np.full(n, SENTINEL, np.uint8) for k, n in self.OUT.items()})
        self.d.update({k: torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev) for k, n in self.OUT.items()})
        torch.cuda.synchronize(dev)

    def ptr(self, host, name):
        return self.h[name].ctypes.data if host else self.d[name].data_ptr()

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool((self.h[k] == SENTINEL).all()) and bool((self.d[k] == SENTINEL).all().item()) for k in self.OUT)


# ---------------------------------------------------------------- the six query entries
RAY_VARIANTS = ("kind_7", "n_negative", "stride_2", "null_rays", "any_without_tmax", "closest_without_hits", "any_without_occluded", "past_2_32_floats",
                "n_zero", "no_bvh", "rays_misaligned", "hits_misaligned")
SCENE_VARIANTS = ("null_uniforms", "flags_8", "more_nodes_than_uploaded")
PICK_VARIANTS = ("null_xy", "n_negative", "null_uniforms", "closest_without_hits", "more_nodes_than_uploaded", "n_zero", "xy_misaligned", "hits_misaligned")
_MORE = uniforms(True, 1 << 20, 1 << 20)
_ANALYTIC = uniforms()


def _ray_call(family, host, variant):
    """family: "rays" (rt_trace_rays) or "scene" (rt_trace_scene_rays); host: the _host entry."""
    def call(L, h, b):
        p = lambda name: b.ptr(host, name)
        kind, flags, n, os_, ds, u = rt.RT_QUERY_CLOSEST, 0, N_REC, 3, 3, _ANALYTIC
        o, d, tm, hits, occ = p("origins"), p("dirs"), None, p("hits"), None
        if variant == "kind_7":
            kind = 7
        elif variant == "n_negative":
            n = -1
        elif variant == "stride_2":
            os_ = 2
        elif variant == "null_rays":
            o = None
        elif variant == "any_without_tmax":
            kind, hits, occ = rt.RT_QUERY_ANY, None, p("occluded")
        elif variant == "closest_without_hits":
            hits = None
        elif variant == "any_without_occluded":
            kind, tm, hits = rt.RT_QUERY_ANY, p("tmax"), None
        elif variant == "past_2_32_floats":
            n = 2 ** 31 - 1
        elif variant == "n_zero":
            n = 0
        elif variant == "rays_misaligned":                          # inside the buffer: seven rays from 2 bytes in
            o, n = o + 2, N_REC - 1
        elif variant == "hits_misaligned":
            hits, n = hits + 4, N_REC - 1
        elif variant == "null_uniforms":
            u = None
        elif variant == "flags_8":
            flags = 8
        elif variant == "more_nodes_than_uploaded":
            u = _MORE
        if family == "rays":
            fn = L.rt_trace_rays_host if host else L.rt_trace_rays
            rc = fn(h, kind, o, os_, d, ds, tm, 1e-4, 1e30, n, hits, p("normals"), occ)
        else:
            fn = L.rt_trace_scene_rays_host if host else L.rt_trace_scene_rays
            rc = fn(h, None if u is None else C.byref(u), kind, flags, o, os_, d, ds, tm, n, hits, p("objects"), p("normals"), p("points"), occ)
        return rc, {}
    return call


def _pick_call(host, variant):
    def call(L, h, b):
        p = lambda name: b.ptr(host, name)
        u, xy, n, hits = _ANALYTIC, p("xy"), N_REC, p("hits")
        if variant == "null_xy":
            xy = None
        elif variant == "n_negative":
            n = -1
        elif variant == "null_uniforms":
            u = None
        elif variant == "closest_without_hits":
            hits = None
        elif variant == "more_nodes_than_uploaded":
            u = _MORE
        elif variant == "n_zero":
            n = 0
        elif variant == "xy_misaligned":
            xy, n = xy + 2, N_REC - 1
        elif variant == "hits_misaligned":
            hits, n = hits + 4, N_REC - 1
        fn = L.rt_pick_pixels_host if host else L.rt_pick_pixels
        return fn(h, None if u is None else C.byref(u), xy, n, hits, p("objects"), p("normals"), p("points")), {}
    return call


CALLS = {}
for _host in (False, True):
    _sfx = "_host" if _host else ""
    for _v in RAY_VARIANTS:
        if _host and _v.endswith("misaligned"):
            continue
        # rt_trace_rays: without a BVH every call ends at "no BVH uploaded" at the latest; with one, "no_bvh" is a valid query and is left out
        CALLS[f"rt_trace_rays{_sfx}/{_v}"] = (_ray_call("rays", _host, _v), NO_BVH if _v == "no_bvh" else ALL)
        if _v != "no_bvh":
            CALLS[f"rt_trace_scene_rays{_sfx}/{_v}"] = (_ray_call("scene", _host, _v), ALL)
    for _v in SCENE_VARIANTS:
        CALLS[f"rt_trace_scene_rays{_sfx}/{_v}"] = (_ray_call("scene", _host, _v), ALL)
    for _v in PICK_VARIANTS:
        if _host and _v.endswith("misaligned"):
            continue
        CALLS[f"rt_pick_pixels{_sfx}/{_v}"] = (_pick_call(_host, _v), ALL)


# ---------------------------------------------------------------- everything else
def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


_PARAMS, _CAM = rt.default_render_params(), rt.default_camera()
_PRESENT = rt.make_present_params(_PARAMS, False, W, H)
_PRESENT_64 = rt.make_present_params(_PARAMS, False, 64, 64)
_U64 = uniforms(w=64, h=64)
_EYE = np.eye(4, dtype=f32).reshape(-1)
_FACES = np.zeros(6 * 2, np.uint8)
_NODES, _TRIS = (np.ascontiguousarray(a, f32) for a in scenes.one_leaf_mesh())
_RAYS = np.ones((4, 3), f32)
_OUT7 = np.full((4, 7), 7.0, f32)
_U8P, _U32P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)


def _img(b, host=True):
    return b.ptr(host, "image")


def _ptr_and_size(name, *args):
    def call(L, h, b):
        ptr, n = C.c_void_p(0xDEAD0), C.c_size_t(12345)
        return getattr(L, name)(h, *args, C.byref(ptr), C.byref(n)), {"outputs": [ptr.value, n.value]}
    return call


def _raster_targets(L, h, b):
    p = [C.c_void_p(0xDEAD0) for _ in range(3)]
    n = C.c_size_t(12345)
    return L.rt_raster_targets(h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(n)), {"outputs": [q.value for q in p] + [n.value]}


def _read_scene(which, room):
    def call(L, h, b):
        n = C.c_size_t(12345)
        return L.rt_debug_read_scene(h, which, _img(b), room, C.byref(n)), {"bytes": n.value}
    return call


def _pack_scene(L, h, b):
    n = C.c_size_t(12345)
    rc = L.rt_debug_pack_scene(_fp(_NODES), _NODES.shape[0], _fp(_TRIS), _TRIS.shape[0], None, 99, _img(b), 64, C.byref(n))
    return rc, {"bytes": n.value, "error": L.rt_last_error(None).decode()}   # no context: the text is the thread's


def _debug_trace_wave(L, h, b):
    rc = L.rt_debug_trace(h, 2, _fp(_RAYS), _fp(_RAYS), _fp(_RAYS), 1e-4, 1e30, _fp(_OUT7), 4)
    return rc, {"out7_untouched": bool((_OUT7 == 7.0).all())}


CALLS.update({
    # before rt_resize
    "rt_reset_accum/before_resize": (lambda L, h, b: (L.rt_reset_accum(h), {}), ("fresh", "fresh_raster")),
    "rt_render_frame/before_resize": (lambda L, h, b: (L.rt_render_frame(h, C.byref(_ANALYTIC)), {}), ("fresh", "fresh_raster")),
    "rt_render_frames/before_resize": (lambda L, h, b: (L.rt_render_frames(h, C.byref(_ANALYTIC), 1), {}), ("fresh", "fresh_raster")),
    "rt_render_ray/before_resize": (lambda L, h, b: (L.rt_render_ray(h, C.byref(_PARAMS), C.byref(_CAM), 0, 0, None, None), {}), ("fresh", "fresh_raster")),
    "rt_render_ray_frames/before_resize": (lambda L, h, b: (L.rt_render_ray_frames(h, C.byref(_PARAMS), C.byref(_CAM), 0, 0, 2), {}), ("fresh", "fresh_raster")),
    "rt_read_target/before_resize": (lambda L, h, b: (L.rt_read_target(h, 0, _img(b), rt.RT_FORMAT_F16), {}), ("fresh", "fresh_raster")),
    "rt_write_target/before_resize": (lambda L, h, b: (L.rt_write_target(h, 0, _img(b), rt.RT_FORMAT_F16), {}), ("fresh", "fresh_raster")),
    "rt_present/before_resize": (lambda L, h, b: (L.rt_present(h, C.byref(_PRESENT), C.cast(_img(b), _U8P)), {}), ("fresh", "fresh_raster")),
    "rt_present_gathered/before_resize": (lambda L, h, b: (L.rt_present_gathered(h, C.byref(_PRESENT), *[_img(b, False)] * 4, C.cast(_img(b), _U8P)), {}),
                                          ("fresh", "fresh_raster")),
    "rt_history_exchange_buffer/before_resize": (_ptr_and_size("rt_history_exchange_buffer"), ("fresh", "fresh_raster")),
    "rt_history_exchanged/before_resize": (lambda L, h, b: (L.rt_history_exchanged(h), {}), ("fresh", "fresh_raster")),
    "rt_local_target/before_resize": (_ptr_and_size("rt_local_target", 0), ("fresh", "fresh_raster")),
    "rt_assemble_gathered/before_resize": (lambda L, h, b: (L.rt_assemble_gathered(h, 0, _img(b, False), _img(b, False)), {}), ("fresh", "fresh_raster")),
    "rt_gather_frame/before_resize": (lambda L, h, b: (L.rt_gather_frame(h, 0), {}), ("fresh", "fresh_raster")),
    "rt_exchange_history/before_resize": (lambda L, h, b: (L.rt_exchange_history(h), {}), ("fresh", "fresh_raster")),
    "rt_render_raster/before_resize": (lambda L, h, b: (L.rt_render_raster(h, None, 0, _fp(_EYE), _fp(_EYE)), {}), ("fresh", "fresh_raster")),
    "rt_raster_targets/before_resize": (_raster_targets, ("fresh_raster",)),
    "rt_read_raster/before_resize": (lambda L, h, b: (L.rt_read_raster(h, C.cast(_img(b), _U8P), None, None), {}), ("fresh_raster",)),
    # frames
    "rt_render_frame/resolution_64x64": (lambda L, h, b: (L.rt_render_frame(h, C.byref(_U64)), {}), SIZED),
    "rt_render_frame/more_nodes_than_uploaded": (lambda L, h, b: (L.rt_render_frame(h, C.byref(uniforms(True, 1 << 20, 1 << 20))), {}), SIZED),
    "rt_set_extension/gi_bounces_0": (lambda L, h, b: (L.rt_set_extension(h, C.byref(rt.RtExtension(giBounces=0, envFilter=0))), {}), ALL),
    "rt_set_extension/env_filter_2": (lambda L, h, b: (L.rt_set_extension(h, C.byref(rt.RtExtension(giBounces=1, envFilter=2))), {}), ALL),
    "rt_upload_env/two_channels": (lambda L, h, b: (L.rt_upload_env(h, _FACES.ctypes.data_as(_U8P), 1, 2), {}), ALL),
    "rt_upload_bvh/null_nodes": (lambda L, h, b: (L.rt_upload_bvh(h, None, 1, _fp(_TRIS), 1), {}), ALL),
    "rt_get_counters/without_count_work": (lambda L, h, b: (L.rt_get_counters(h, C.byref(rt.RtCounters())), {}), ALL),
    # targets and present
    "rt_read_target/which_9": (lambda L, h, b: (L.rt_read_target(h, 9, _img(b), rt.RT_FORMAT_F16), {}), SIZED),
    "rt_read_target/format_7": (lambda L, h, b: (L.rt_read_target(h, 0, _img(b), 7), {}), SIZED),
    "rt_write_target/which_9": (lambda L, h, b: (L.rt_write_target(h, 9, _img(b), rt.RT_FORMAT_F16), {}), SIZED),
    "rt_write_target/format_f32": (lambda L, h, b: (L.rt_write_target(h, 0, _img(b), rt.RT_FORMAT_F32), {}), SIZED),
    "rt_local_target/which_9": (_ptr_and_size("rt_local_target", 9), SIZED),
    "rt_present/world_2": (lambda L, h, b: (L.rt_present(h, C.byref(_PRESENT), C.cast(_img(b), _U8P)), {}), RANKS),
    "rt_present/resolution_64x64": (lambda L, h, b: (L.rt_present(h, C.byref(_PRESENT_64), C.cast(_img(b), _U8P)), {}), ("sized", "rendered")),
    "rt_present_gathered/resolution_64x64": (lambda L, h, b: (L.rt_present_gathered(h, C.byref(_PRESENT_64), *[_img(b, False)] * 4, C.cast(_img(b), _U8P)), {}), SIZED),
    # the exchange
    "rt_history_exchanged/without_its_buffer": (lambda L, h, b: (L.rt_history_exchanged(h), {}), SIZED),
    "rt_gather_frame/before_the_first_frame": (lambda L, h, b: (L.rt_gather_frame(h, 0), {}), ("sized",)),
    "rt_gather_frame/without_communicator": (lambda L, h, b: (L.rt_gather_frame(h, 0), {}), RANKS),
    "rt_gather_frame/which_9": (lambda L, h, b: (L.rt_gather_frame(h, 9), {}), ("rendered",)),
    "rt_gathered_frame/rank_1": (_ptr_and_size("rt_gathered_frame", 0), ("rank1of2",)),
    "rt_gathered_frame/no_gather": (_ptr_and_size("rt_gathered_frame", 1), ("fresh", "fresh_raster", "sized", "rendered", "rank0of2")),
    "rt_present_last_gathered/incomplete_gather": (lambda L, h, b: (L.rt_present_last_gathered(h, C.byref(_PRESENT), C.cast(_img(b), _U8P)), {}), ALL),
    "rt_exchange_history/without_communicator": (lambda L, h, b: (L.rt_exchange_history(h), {}), RANKS),
    # the raster preview
    "rt_raster_targets/before_render": (_raster_targets, tuple(s for s in STATES if s != "fresh_raster")),
    "rt_read_raster/before_render": (lambda L, h, b: (L.rt_read_raster(h, C.cast(_img(b), _U8P), None, None), {}), tuple(s for s in STATES if s != "fresh_raster")),
    "rt_render_raster/null_view": (lambda L, h, b: (L.rt_render_raster(h, None, 0, None, _fp(_EYE)), {}), ALL),
    "rt_render_raster/draws_without_array": (lambda L, h, b: (L.rt_render_raster(h, None, 2, _fp(_EYE), _fp(_EYE)), {}), ALL),
    "rt_render_raster/world_2": (lambda L, h, b: (L.rt_render_raster(h, None, 0, _fp(_EYE), _fp(_EYE)), {}), RANKS),
    "rt_debug_raster_bin_capacity/above_2_31": (lambda L, h, b: (L.rt_debug_raster_bin_capacity(h, (1 << 31) + 1), {}), ALL),
    # debug entries
    "rt_debug_read_scene/array_99": (_read_scene(99, 64), ALL),
    "rt_debug_read_scene/room_for_4_bytes": (_read_scene(rt.SCENE_ARRAYS["tris"], 4), ("rendered",)),
    "rt_debug_pack_scene/array_99": (_pack_scene, ALL),
    "rt_debug_trace/kind_2_without_bvh": (_debug_trace_wave, NO_BVH),
})
QUIET = tuple(n for n in CALLS if n.endswith("/n_zero"))            # calls that may succeed: they do no device work


def run(state, device=0):
    """{call name: {"rc", "error", ...}} of every call of the table that belongs to `state`, on one fresh context brought into it."""
    out = {}
    L = rt.lib()
    with make(state, device) as r:
        b = Buffers(device)
        for name, (call, states) in CALLS.items():
            if state not in states:
                continue
            rc, seen = call(L, r._h, b)
            rec = {"rc": int(rc), "error": None if rc == rt.RT_OK else L.rt_last_error(r._h).decode(), "untouched": b.untouched()}
            rec.update(seen)
            out[name] = rec
    return out


# ---------------------------------------------------------------- the lane-summed getters on one fixed render
def lane_sums(device=0):
    """{getter: {field: count}} of rt_get_traced_rays, rt_debug_bounce_probe, rt_debug_disk_skip and rt_debug_gi_list after three frames of the bunny
    stand-in at 32 x 16 and 1 spp (the wavefront pipeline; the counts start at a reset before the first frame)."""
    nodes, tris = scenes.bunny_bvh(3)
    p = rt.default_render_params()
    p.sppPerFrame = 1
    cam = scenes.camera("closeup", aspect=W / H)
    with rt.Renderer(device=device) as r:
        r.upload_bvh(nodes, tris)
        r.upload_env(scenes.tiny_env(8))
        r.resize(W, H)
        getters = {"rt_get_traced_rays": r.traced_rays, "rt_debug_bounce_probe": r.bounce_probe, "rt_debug_disk_skip": r.disk_skip, "rt_debug_gi_list": r.gi_list}
        for get in getters.values():
            get(reset=True)
        for frame in range(3):
            r.render_frame(rt.frame_uniforms(p, cam, W, H, frame, True, nodes.shape[0], tris.shape[0]))
        r.synchronize()
        out = {}
        for name, get in getters.items():
            s = get()
            out[name] = {f: getattr(s, f) for f, *_ in s._fields_ if isinstance(getattr(s, f), int)}   # (reserved words are arrays)
        return out
