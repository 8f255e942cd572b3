"""The refusals of the dynamic-mesh C API, as one table shared by tests/golden/make_mesh_api_golden.py, which recorded them on the commit
before the API moved to csrc/rt_api_mesh.hip -- and the UV and texture cases on the commit before colours and UVs became one corner-attribute path --
and tests/test_gpu_mesh_api_contract.py, which holds the library to that record.

A case is a context state, a raw ctypes call of an exported entry point and what came back: the return code, rt_last_error's text when the call was
refused, and for the device-pointer accessors what they left in their outputs.  Every call here is refused before any device work, or (n = 0, the
accessors) does none; the device entries are nevertheless given real device memory of eight records, so that a library that failed to refuse would do
no harm."""
import ctypes as C

import numpy as np

import opengl_raytracing_amd as rt

f32 = np.float32
N_TRIS, PART_FIRST, N_BONES, N_TARGETS = 65, (0, 30, 65), 2, 3   # 65 triangles: more than one wave, more than the 8-triangle leaf
N_REC = 8                                                         # records in every hit buffer
SENTINEL = 0x5A

STATES = ("no_mesh", "mesh_no_tree", "tree_features_off", "features_no_tree", "morph_no_skin", "all_on", "released", "uvs_no_texture")
ALL = STATES


def mesh():
    """A strip of 65 triangles over 67 random vertices, every vertex used, in two parts."""
    rng = np.random.default_rng(65)
    nv = N_TRIS + 2
    v = rng.normal(0, 1, (nv, 3)).astype(f32)
    f = np.stack([np.arange(nv - 2), np.arange(1, nv - 1), np.arange(2, nv)], axis=1).astype(np.uint32).reshape(-1)
    return v, f


def skin(nv):
    """Two bones: the first half of the vertices follows bone 0, the second half both."""
    bi = np.zeros((nv, 4), np.uint16)
    w = np.zeros((nv, 4), f32)
    w[:, 0] = 1.0
    bi[nv // 2:, 1] = 1
    w[nv // 2:, 0], w[nv // 2:, 1] = 0.5, 0.5
    return bi, w


def morph(nv):
    d = np.zeros((N_TARGETS, nv, 3), f32)
    for t in range(N_TARGETS):
        d[t, t::N_TARGETS, t] = 0.25
    return rt.morph_targets_from_dense(d)


def texture():
    """3 x 5 texels, every byte its own."""
    return np.random.default_rng(35).integers(0, 256, (5, 3, 4)).astype(np.uint8)


def enter(r, state):
    """Brings the fresh Renderer r into `state`."""
    v, f = mesh()
    nv = v.shape[0]
    if state == "no_mesh":
        return
    r.mesh_upload_parts(v, f, PART_FIRST)
    if state in ("features_no_tree", "all_on", "released"):
        r.mesh_skin_upload(*skin(nv), N_BONES, rest=v)
    if state in ("features_no_tree", "morph_no_skin", "all_on", "released"):
        r.mesh_morph_upload(*morph(nv), base=v)
    if state in ("features_no_tree", "all_on", "released"):
        r.mesh_motion_enable()
        r.mesh_normals_enable()
        r.mesh_colors_enable()
        r.mesh_uvs_enable()
        r.mesh_texture_upload(texture())
    if state == "uvs_no_texture":                                   # a tree and UVs: what rt_mesh_hit_texels still lacks is the texture
        r.mesh_uvs_enable()
    if state in ("tree_features_off", "all_on", "released", "uvs_no_texture"):
        r.mesh_rebuild_parts()
    if state == "released":
        r.upload_bvh(np.zeros((0, 12), f32), np.zeros((0, 12), f32))
    r.synchronize()


class Buffers:
    """Host and device memory for the calls: eight hit records (all misses), eight points, outputs pre-filled with SENTINEL bytes."""

    def __init__(self, device):
        import torch
        rec = np.zeros((N_REC, 4), f32)
        rec.view(np.int32)[:, 1] = -1
        self.h_hits, self.h_points = rec, np.zeros((N_REC, 3), f32)
        self.h_out = [np.full(N_REC * 12, SENTINEL, np.uint8) for _ in range(2)]
        dev = torch.device("cuda", device)
        self.d_hits, self.d_points = torch.from_numpy(rec).to(dev), torch.zeros((N_REC, 3), dtype=torch.float32, device=dev)
        self.d_out = [torch.full((N_REC * 12,), SENTINEL, dtype=torch.uint8, device=dev) for _ in range(2)]
        torch.cuda.synchronize(dev)

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool((o == SENTINEL).all()) for o in self.h_out) and all(bool((o == SENTINEL).all().item()) for o in self.d_out)


QUERIES = ("parts", "prev_points", "normals", "colors", "uvs", "texels")
HIT_VARIANTS = ("n_negative", "null_hits", "null_outputs", "null_points", "n_zero", "hits_misaligned", "output_misaligned")


def _hit_call(query, host, variant):
    def call(L, h, b):
        hits = b.h_hits.ctypes.data if host else b.d_hits.data_ptr()
        points = b.h_points.ctypes.data if host else b.d_points.data_ptr()
        outs = [o.ctypes.data for o in b.h_out] if host else [o.data_ptr() for o in b.d_out]
        n = N_REC
        if variant == "n_negative":
            n = -1
        elif variant == "null_hits":
            hits = None
        elif variant == "null_outputs":
            outs = [None, None]
        elif variant == "null_points":
            points = None
        elif variant == "n_zero":
            n = 0
        elif variant == "hits_misaligned":   # inside the buffer: seven records from 2 (parts) or 4 bytes in
            hits, n = hits + (2 if query == "parts" else 4), N_REC - 1
        elif variant == "output_misaligned":
            outs, n = [outs[0] + 2, outs[1]], N_REC - 1
        fn = getattr(L, f"rt_mesh_hit_{query}" + ("_host" if host else ""))
        if query == "parts":
            rc = fn(h, hits, n, outs[0], outs[1])
        elif query == "prev_points":
            rc = fn(h, hits, points, n, outs[0])
        else:
            rc = fn(h, hits, n, outs[0])
        return rc, {"untouched": b.untouched()}
    return call


ACCESSORS = ("rt_mesh_part_matrices", "rt_mesh_positions", "rt_mesh_vertex_normals", "rt_mesh_colors", "rt_mesh_uvs", "rt_mesh_bones",
             "rt_mesh_rest_positions", "rt_mesh_morph_base", "rt_mesh_morph_weights")
QUIET = ACCESSORS + ("rt_mesh_texture",)                          # calls that succeed where there is something to hand out: they do no device work


def _accessor(name):
    def call(L, h, b):
        ptr, n = C.c_void_p(0xDEAD0), C.c_size_t(12345)
        rc = getattr(L, name)(h, C.byref(ptr), C.byref(n))
        if rc == rt.RT_OK:
            return rc, {"null": not ptr.value, "bytes": n.value}
        return rc, {"cleared": [not ptr.value, n.value == 0]}
    return call


def _texture(L, h, b):
    ptr, n, w, t = C.c_void_p(0xDEAD0), C.c_size_t(12345), C.c_int(77), C.c_int(88)
    rc = L.rt_mesh_texture(h, C.byref(ptr), C.byref(n), C.byref(w), C.byref(t))
    if rc == rt.RT_OK:
        return rc, {"null": not ptr.value, "bytes": n.value, "size": [w.value, t.value]}
    return rc, {"cleared": [not ptr.value, n.value == 0, w.value == 0, t.value == 0]}


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


_M = np.tile(np.eye(4, dtype=f32).reshape(-1), 4)
_ONES = np.ones(64, f32)
_NEGATIVE = np.array([0.5, -0.25, 0.5], f32)                      # one colour, its green negative
_NOT_FINITE = np.array([0.5, 0.25, 0.5, np.inf], f32)             # two UVs, the second one's v infinite
_TEXELS = texture()
_NOT_TREE = ("no_mesh", "mesh_no_tree", "features_no_tree", "morph_no_skin", "released")
_NOT_ALL_ON = tuple(s for s in STATES if s != "all_on")

# name -> (call, states): the states in which the call is refused (the hit queries with n = 0 and the accessors: every state, they do no device work)
CALLS = {}
for _q in QUERIES:
    for _host in (False, True):
        for _v in HIT_VARIANTS:
            if (_v == "null_points" and _q != "prev_points") or (_host and _v.endswith("misaligned")):
                continue
            CALLS[f"rt_mesh_hit_{_q}{'_host' if _host else ''}/{_v}"] = (_hit_call(_q, _host, _v), ALL)
for _a in ACCESSORS:
    CALLS[_a] = (_accessor(_a), ALL)
CALLS.update({
    "rt_mesh_order_device": (_accessor("rt_mesh_order_device"), _NOT_TREE),
    "rt_mesh_set_bones/past_the_table": (lambda L, h, b: (L.rt_mesh_set_bones(h, 1, N_BONES, _fp(_M)), {}), ALL),
    "rt_mesh_set_morph_weights/past_the_table": (lambda L, h, b: (L.rt_mesh_set_morph_weights(h, N_TARGETS + 1, 0, _fp(_ONES)), {}), ALL),
    "rt_mesh_set_colors/past_the_table": (lambda L, h, b: (L.rt_mesh_set_colors(h, _fp(_ONES), N_TRIS + 2, 1), {}), ALL),
    "rt_mesh_set_colors/negative": (lambda L, h, b: (L.rt_mesh_set_colors(h, _fp(_NEGATIVE), 5, 1), {}), ALL),
    "rt_mesh_set_uvs/past_the_table": (lambda L, h, b: (L.rt_mesh_set_uvs(h, _fp(_ONES), N_TRIS + 2, 1), {}), ALL),
    "rt_mesh_set_uvs/not_finite": (lambda L, h, b: (L.rt_mesh_set_uvs(h, _fp(_NOT_FINITE), 3, 2), {}), ALL),
    "rt_mesh_set_part_matrices/past_the_table": (lambda L, h, b: (L.rt_mesh_set_part_matrices(h, 1, len(PART_FIRST) - 1, _fp(_M)), {}), ALL),
    "rt_mesh_motion_latch": (lambda L, h, b: (L.rt_mesh_motion_latch(h), {}), _NOT_ALL_ON),
    "rt_mesh_colors_refresh": (lambda L, h, b: (L.rt_mesh_colors_refresh(h), {}), _NOT_ALL_ON),
    "rt_mesh_uvs_refresh": (lambda L, h, b: (L.rt_mesh_uvs_refresh(h), {}), tuple(s for s in _NOT_ALL_ON if s != "uvs_no_texture")),
    "rt_mesh_texture": (_texture, ALL),
    "rt_mesh_texture_upload/zero_width": (lambda L, h, b: (L.rt_mesh_texture_upload(h, _TEXELS.ctypes.data, 0, 5, 0), {}), ALL),
    "rt_mesh_texture_upload/unknown_flags": (lambda L, h, b: (L.rt_mesh_texture_upload(h, _TEXELS.ctypes.data, 3, 5, 8), {}), ALL),
    "rt_mesh_skin": (lambda L, h, b: (L.rt_mesh_skin(h), {}), ("no_mesh", "mesh_no_tree", "tree_features_off", "morph_no_skin", "released")),
    "rt_mesh_morph/destination_7": (lambda L, h, b: (L.rt_mesh_morph(h, 7), {}), ALL),
    "rt_mesh_morph/to_rest": (lambda L, h, b: (L.rt_mesh_morph(h, rt.RT_MORPH_TO_REST), {}), ("no_mesh", "mesh_no_tree", "tree_features_off", "morph_no_skin", "released")),
    "rt_mesh_update/rebuild_above_half": (lambda L, h, b: (L.rt_mesh_update(h, rt.RT_MESH_UPDATE_SINGLE, None, 0.5, None), {}), ALL),
    "rt_mesh_update/matrix_with_parts": (lambda L, h, b: (L.rt_mesh_update(h, rt.RT_MESH_UPDATE_PARTS, _fp(_M), 2.0, None), {}), ALL),
    "rt_mesh_measure": (lambda L, h, b: (L.rt_mesh_measure(h), {}), _NOT_TREE),
    "rt_mesh_quality/which_9": (lambda L, h, b: (L.rt_mesh_quality(h, 9, 0, C.byref(rt.RtMeshQuality())), {}), ALL),
    "rt_mesh_quality/nothing_measured": (lambda L, h, b: (L.rt_mesh_quality(h, rt.RT_MESH_QUALITY_LATEST, 0, C.byref(rt.RtMeshQuality())), {}), ALL),
})


def run(state, device=0):
    """{call name: {"rc", "error", ...}} of every call of the table that belongs to `state`, on one fresh context brought into it."""
    out = {}
    L = rt.lib()
    with rt.Renderer(device=device) as r:
        enter(r, state)
        b = Buffers(device)
        for name, (call, states) in CALLS.items():
            if state not in states:
                continue
            rc, seen = call(L, r._h, b)
            rec = {"rc": int(rc), "error": None if rc == rt.RT_OK else L.rt_last_error(r._h).decode()}
            rec.update(seen)
            out[name] = rec
    return out
