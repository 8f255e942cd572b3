"""The Python half of the device queries, once per Renderer method and on both of its paths (numpy through the *_host entries, torch zero-copy):
what the binding refuses, by full message text; what N = 0 gives -- a result of recorded type, shapes and dtypes, or a recorded error; the torch
answers against the numpy answers bit for bit, for one row and for four rows strided out of a wider array; and the torch call from a side stream,
its input produced by the op before it and its answer consumed by the op after it.  The texts and the N = 0 outcomes are recorded here literally:
they are the binding's contract, not recomputed from it.  The scene is the two-triangle quad of test_query_binding_host.py, N <= 4 throughout."""
import numpy as np
import pytest

import opengl_raytracing_amd as rt
import test_query_binding_host as host
from test_query_binding_host import BOXES, DIRS, HULLS, MAX_DIST, NODES, ORIGINS, POINTS, PREFIX, QTRIS, RECTS, TMAX, TRIS, UNIT, U

pytestmark = pytest.mark.gpu

f32 = np.float32
XY = np.array([[8, 8], [4, 11], [0, 0], [15, 15]], np.int32)                 # pixels of U's 16 x 16 frame
DEV = "cuda:0"
MIXED = "{} must all be numpy arrays or all torch tensors"
XY_WORDS = "xy must be an int32 [N,2] numpy array or contiguous torch tensor"

INPUTS = {"rays": (ORIGINS, DIRS, TMAX), "xy": (XY,), "points": (POINTS, MAX_DIST), "boxes": (BOXES,), "qtris": (QTRIS,), "hulls": (HULLS,),
          "rects": (RECTS,)}

# method -> (its input family, the call)
METHODS = {
    "trace_rays": ("rays", lambda r, o, d, t: r.trace_rays(o, d, t, normals=True)),
    "trace_rays_any": ("rays", lambda r, o, d, t: r.trace_rays(o, d, t, any_hit=True)),
    "trace_scene_rays": ("rays", lambda r, o, d, t: r.trace_scene_rays(U, o, d, t, normals=True, points=True)),
    "trace_scene_rays_any": ("rays", lambda r, o, d, t: r.trace_scene_rays(U, o, d, t, any_hit=True)),
    "pick": ("xy", lambda r, xy: r.pick(U, xy)),
    "trace_rays_multi": ("rays", lambda r, o, d, t: r.trace_rays_multi(o, d, t, max_hits=2)),
    "pick_multi": ("xy", lambda r, xy: r.pick_multi(U, xy, max_hits=2)),
    "nearest_points": ("points", lambda r, p, m: r.nearest_points(p, m, visits=True)),
    "nearest_points_multi": ("points", lambda r, p, m: r.nearest_points_multi(p, 2, m, visits=True)),
    "box_overlaps": ("boxes", lambda r, b: r.box_overlaps(b, visits=True)),
    "box_overlaps_cap2": ("boxes", lambda r, b: r.box_overlaps(b, cap=2)),
    "tri_overlaps": ("qtris", lambda r, q: r.tri_overlaps(q, visits=True)),
    "tri_overlaps_cap2": ("qtris", lambda r, q: r.tri_overlaps(q, cap=2)),
    "hull_overlaps": ("hulls", lambda r, h: r.hull_overlaps(h, visits=True)),
    "hull_overlaps_cap2": ("hulls", lambda r, h: r.hull_overlaps(h, cap=2)),
    "pick_rects": ("rects", lambda r, x: r.pick_rects(U, x, visits=True)),
    "pick_rects_cap2": ("rects", lambda r, x: r.pick_rects(U, x, cap=2)),
}
FIELDS = {"RayHits": ("record", "normal"), "SceneHits": ("record", "object", "normal", "point"), "MultiHits": ("hits", "count"),
          "NearestPoints": ("hits", "points", "visits"), "NearestMulti": ("hits", "points", "count", "visits"),
          "BoxOverlaps": ("count", "offsets", "prims", "visits"), "TriOverlaps": ("count", "offsets", "prims", "visits"),
          "HullOverlaps": ("count", "offsets", "prims", "visits", "corners")}

# ---- what N = 0 gives, as _describe() states it.  One entry where the two paths agree, else {"numpy": ..., "torch": ...}.
_F, _I = "float32", "int32"
_OVERLAPS0 = (("count", (_I, (0,))), ("offsets", (_I, (1,))), ("prims", (_I, (0,))))
N0 = {
    "trace_rays": ("RayHits", (("record", (_F, (0, 4))), ("normal", (_F, (0, 3))))),
    "trace_rays_any": {"numpy": ("bool", (0,)), "torch": "rt_mi355 error -1: rt_trace_rays: any-hit queries need tMax"},
    "trace_scene_rays": ("SceneHits", (("record", (_F, (0, 4))), ("object", (_I, (0,))), ("normal", (_F, (0, 3))), ("point", (_F, (0, 3))))),
    "trace_scene_rays_any": {"numpy": ("bool", (0,)), "torch": "rt_mi355 error -1: rt_trace_scene_rays: any-hit queries need tMax"},
    "pick": ("SceneHits", (("record", (_F, (0, 4))), ("object", (_I, (0,))), ("normal", (_F, (0, 3))), ("point", (_F, (0, 3))))),
    "trace_rays_multi": ("MultiHits", (("hits", (_F, (0, 2, 4))), ("count", (_I, (0,))))),
    "pick_multi": ("MultiHits", (("hits", (_F, (0, 2, 4))), ("count", (_I, (0,))))),
    "nearest_points": ("NearestPoints", (("hits", (_F, (0, 4))), ("points", (_F, (0, 3))), ("visits", (_I, (0,))))),
    "nearest_points_multi": ("NearestMulti", (("hits", (_F, (0, 2, 4))), ("points", (_F, (0, 2, 3))), ("count", (_I, (0,))), ("visits", (_I, (0,))))),
    "box_overlaps": ("BoxOverlaps", _OVERLAPS0 + (("visits", (_I, (0,))),)),
    "box_overlaps_cap2": ("BoxOverlaps", _OVERLAPS0 + (("visits", None),)),
    "tri_overlaps": ("TriOverlaps", _OVERLAPS0 + (("visits", (_I, (0,))),)),
    "tri_overlaps_cap2": ("TriOverlaps", _OVERLAPS0 + (("visits", None),)),
    "hull_overlaps": ("HullOverlaps", _OVERLAPS0 + (("visits", (_I, (0,))), ("corners", None))),
    "hull_overlaps_cap2": ("HullOverlaps", _OVERLAPS0 + (("visits", None), ("corners", None))),
    "pick_rects": ("HullOverlaps", _OVERLAPS0 + (("visits", (_I, (0,))), ("corners", (_F, (0, 24))))),
    "pick_rects_cap2": ("HullOverlaps", _OVERLAPS0 + (("visits", None), ("corners", (_F, (0, 24))))),
    "mesh_hit_parts": {"numpy": ((_I, (0,)), (_I, (0,))),
                       "torch": "rt_mi355 error -1: rt_mesh_hit_parts: bad arguments (n = 0; hits and one of parts / tris are needed)"},
}


@pytest.fixture(scope="module")
def ren():
    with rt.Renderer() as r:
        r.upload_bvh(NODES, TRIS)
        yield r


def _torch():
    import torch
    return torch


def _to(a):
    return _torch().from_numpy(np.array(a, copy=True, order="C")).to(DEV)      # (the shared inputs stay as they are)


def _wide(a):
    """The rows of the 2-D array `a` strided out of an array four columns wider -> (numpy view, torch view of the same floats)."""
    w = np.full((a.shape[0], a.shape[1] + 4), 7, a.dtype)
    w[:, 1:1 + a.shape[1]] = a
    return w[:, 1:1 + a.shape[1]], _to(w)[:, 1:1 + a.shape[1]]


def _parts(r):
    """The arrays of an answer, in a fixed order; None where the answer has none."""
    if isinstance(r, tuple):
        return list(r)
    if type(r).__name__ in FIELDS:
        return [getattr(r, f) for f in FIELDS[type(r).__name__]]
    return [r]


def _describe(r):
    if r is None:
        return None
    if isinstance(r, tuple):
        return tuple(_describe(x) for x in r)
    if type(r).__name__ in FIELDS:
        return type(r).__name__, tuple((f, _describe(getattr(r, f))) for f in FIELDS[type(r).__name__])
    return str(r.dtype).replace("torch.", ""), tuple(r.shape)


def _outcome(fn):
    try:
        return _describe(fn())
    except rt.RtError as e:
        return str(e)


def _bits(a):
    if a is None:
        return None
    if not isinstance(a, np.ndarray):
        a = a.cpu().numpy()
    return a.dtype, a.shape, np.ascontiguousarray(a).tobytes()


def _same(got, want, what, kind=None):
    assert type(got).__name__ not in FIELDS or type(got) is type(want), what
    for i, (g, w) in enumerate(zip(_parts(got), _parts(want))):
        assert _bits(g) == _bits(w), (what, i)
        if kind is not None and g is not None:
            assert isinstance(g, kind), (what, i)


def _refused(text, fn, *args, prefix=PREFIX, **kw):
    with pytest.raises(rt.RtError) as e:
        fn(*args, **kw)
    assert str(e.value) == prefix + text, str(e.value)
    assert e.value.code == rt.RT_ERR_INVALID


def _empty(a, path):
    if path == "numpy":
        return a[:0]
    torch = _torch()
    return torch.empty((0,) + a.shape[1:], dtype=getattr(torch, a.dtype.name), device=DEV)


# ---------------------------------------------------------------- N = 0

@pytest.mark.parametrize("path", ["numpy", "torch"])
@pytest.mark.parametrize("name", list(METHODS))
def test_no_queries(ren, name, path):
    family, call = METHODS[name]
    want = N0[name][path] if isinstance(N0[name], dict) else N0[name]
    args = [_empty(a, path) for a in INPUTS[family]]
    got = _outcome(lambda: call(ren, *args))
    print(name, path, repr(got))
    assert got == want
    if not isinstance(want, str):
        kind = np.ndarray if path == "numpy" else _torch().Tensor
        assert all(isinstance(a, kind) for a in _parts(call(ren, *args)) if a is not None)


# ---------------------------------------------------------------- numpy against torch, and the side stream

@pytest.mark.parametrize("name", list(METHODS))
def test_torch_equals_numpy(ren, name):
    torch = _torch()
    family, call = METHODS[name]
    full = INPUTS[family]
    want = call(ren, *full)
    _same(call(ren, *[_to(a) for a in full]), want, (name, "contiguous"), torch.Tensor)
    for i in (0, 1, 3):                                                          # N = 1: the stride comes from the shape
        one = [a[i:i + 1] for a in full]
        got = call(ren, *one)
        for g, w in zip(_parts(got), _parts(want)):
            if g is not None and family in ("rays", "xy", "points"):              # (every array of these answers has one row per query)
                assert _bits(g) == _bits(w[i:i + 1]), (name, i)
        _same(call(ren, *[_to(a) for a in one]), got, (name, "N = 1", i), torch.Tensor)
        if full[0].dtype == f32:
            w_np, w_t = _wide(full[0])
            _same(call(ren, w_np[i:i + 1], *one[1:]), got, (name, "N = 1 of a wider array, numpy", i))
            _same(call(ren, w_t[i:i + 1], *[_to(a) for a in one[1:]]), got, (name, "N = 1 of a wider array, torch", i), torch.Tensor)
    if full[0].dtype == f32:                                                     # N = 4 as strided rows of wider arrays
        wide = [_wide(a) if a.ndim == 2 else (a, _to(a)) for a in full]
        _same(call(ren, *[w[0] for w in wide]), want, (name, "strided, numpy"))
        _same(call(ren, *[w[1] for w in wide]), want, (name, "strided, torch"), torch.Tensor)
    if family in ("qtris", "hulls"):                                             # the [N,3,3] / [N,8,3] forms
        cell = (4, 3, 3) if family == "qtris" else (4, 8, 3)
        _same(call(ren, full[0].reshape(cell)), want, (name, "cells, numpy"))
        _same(call(ren, _to(full[0]).reshape(cell)), want, (name, "cells, torch"), torch.Tensor)
        _same(call(ren, _wide(full[0])[1].unflatten(1, cell[1:])), want, (name, "strided cells, torch"), torch.Tensor)
    if family == "xy":                                                           # numpy pixels are made contiguous
        _same(call(ren, np.asfortranarray(XY)), want, (name, "Fortran order"))
    if family in ("rays", "points"):                                             # ... and so is a numpy tmax / max_dist
        _same(call(ren, *full[:-1], np.repeat(full[-1], 2)[::2]), want, (name, "strided limit"))


def _from_side_stream(ren, call, full, want, what):
    """The torch call inside torch.cuda.stream(side): inputs made by an op on that stream, the answer read by the next op on it."""
    torch = _torch()
    base = [_to(a) for a in full]
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = call(ren, *[b.clone() for b in base])
        copies = [None if a is None else a.clone() for a in _parts(got)]
    side.synchronize()
    for i, (g, w) in enumerate(zip(copies, _parts(want))):
        assert _bits(g) == _bits(w), (what, i)


@pytest.mark.parametrize("name", list(METHODS))
def test_from_a_side_stream(ren, name):
    family, call = METHODS[name]
    _from_side_stream(ren, call, INPUTS[family], call(ren, *INPUTS[family]), name)


# ---------------------------------------------------------------- what the answers are (so that the comparisons above compare something)

def test_the_answers_are_the_quads(ren):
    hits = ren.trace_rays(ORIGINS, DIRS)
    assert hits.hit.tolist() == [True, True, True, False] and hits.prim[:3].tolist() == [0, 1, hits.prim[2]] and hits.t[:2].tolist() == [1, 1]
    assert ren.trace_rays(ORIGINS, DIRS, TMAX, any_hit=True).tolist() == [True, True, False, False]
    assert ren.trace_scene_rays(U, ORIGINS, DIRS).object[:3].tolist() == [rt.RT_OBJECT_MESH] * 3
    assert ren.pick(U, XY).hit[0] and ren.pick_multi(U, XY).count[0] == 1
    for name, fn in (("box", rt.box_overlaps), ("tri", rt.tri_overlaps), ("hull", rt.hull_overlaps)):
        q = INPUTS[{"box": "boxes", "tri": "qtris", "hull": "hulls"}[name]][0]
        _same(getattr(ren, name + "_overlaps")(q), fn(NODES, TRIS, q), name)
    _same(ren.trace_rays_multi(ORIGINS, DIRS, TMAX, max_hits=4), rt.multi_hits(NODES, TRIS, ORIGINS, DIRS, TMAX), "multi")
    got, want = ren.nearest_points(POINTS, MAX_DIST), rt.nearest_points(NODES, TRIS, POINTS, MAX_DIST)
    assert _bits(got.hits) == _bits(want.hits) and _bits(got.points) == _bits(want.points)
    marquee = ren.pick_rects(U, RECTS)
    assert _bits(marquee.corners) == _bits(rt.rect_frusta(U, host.LO, host.HI, RECTS)) and marquee.count[0] == 2
    _same(ren.hull_overlaps(marquee.corners), rt.hull_overlaps(NODES, TRIS, marquee.corners), "marquee")


# ---------------------------------------------------------------- refusals

RAY_METHODS = [n for n, (f, _) in METHODS.items() if f == "rays"]
POINT_METHODS = [n for n, (f, _) in METHODS.items() if f == "points"]
XY_METHODS = [n for n, (f, _) in METHODS.items() if f == "xy"]
OVERLAP_METHODS = [n for n, (f, _) in METHODS.items() if f in ("boxes", "qtris", "hulls", "rects")]


@pytest.mark.parametrize("name", RAY_METHODS)
def test_ray_refusals(ren, name):
    torch = _torch()
    call = lambda *a: METHODS[name][1](ren, *a)
    o, d, t = ORIGINS, DIRS, TMAX
    mixed = MIXED.format("origins, dirs and tmax")
    _refused("origins must be float32, got float64", call, o.astype(np.float64), d, t)
    _refused("dirs must be float32, got float64", call, o, d.astype(np.float64), t)
    _refused("tmax must be float32, got float64", call, o, d, t.astype(np.float64))
    _refused("origins must be float32, got float64", call, o.astype(np.float64).reshape(-1), d, t)            # dtype before shape
    _refused("origins must be [N,k] with k >= 3, got shape (12,)", call, o.reshape(-1), d, t)
    _refused("origins must be [N,k] with k >= 3, got shape (4, 2)", call, o[:, :2], d, t)
    _refused("dirs must be [N,k] with k >= 3, got shape (4, 2)", call, o, d[:, :2], t)
    _refused("dirs has 3 rows, origins 4", call, o, d[:3], t)
    _refused("tmax must be [4], got shape (3,)", call, o, d, t[:3])
    _refused(UNIT.format("origins", 3), call, np.asfortranarray(o), d, t)
    _refused(UNIT.format("dirs", 3), call, o, np.zeros((4, 8), f32)[:, ::2], t)
    _refused(mixed, call, o.tolist(), d, t)
    _refused(mixed, call, o, d, t.tolist())
    if name.endswith("_any"):
        _refused("any-hit queries need tmax", call, o, d, None)
        _refused("any-hit queries need tmax", call, o.tolist(), _to(d), None)                                 # ... before the arrays
    if name == "trace_rays_multi":
        _refused("max_hits = 33 (0 .. RT_MULTI_HIT_MAX = 32)", ren.trace_rays_multi, o.tolist(), d, max_hits=33)   # max_hits before the arrays
        _refused("max_hits = -1 (0 .. RT_MULTI_HIT_MAX = 32)", ren.trace_rays_multi, o, d, max_hits=-1)
    # torch
    O, D, T = _to(o), _to(d), _to(t)
    own = name in ("trace_rays", "trace_rays_any")                                                           # (these two name the argument)
    f64 = lambda n: f"{n} must be float32, got torch.float64" if own else "expected torch.float32, got torch.float64"
    cpu = lambda n: f"{n} is on cpu, the context on cuda:0" if own else "a tensor is on cpu, the context on cuda:0"
    _refused(cpu("origins"), call, O.cpu(), D, T)
    _refused(cpu("dirs"), call, O, D.cpu(), T)
    _refused(cpu("tmax"), call, O, D, T.cpu())
    _refused(f64("origins"), call, O.double(), D, T)
    _refused(f64("tmax"), call, O, D, T.double())
    _refused(f64("origins"), call, O.double().cpu(), D, T)                                                   # dtype before device
    _refused(cpu("origins"), call, O.cpu().reshape(-1), D, T)                                                # device before shape
    _refused(UNIT.format("origins", 3), call, _to(np.ascontiguousarray(o.T)).T, D, T)                        # a transposed tensor
    _refused(UNIT.format("dirs", 3), call, O, torch.zeros((4, 8), device=DEV)[:, ::2], T)
    _refused("origins must be [N,k] with k >= 3, got shape (12,)", call, O.reshape(-1), D, T)
    _refused("dirs must be [N,k] with k >= 3, got shape (4, 2)", call, O, D[:, :2], T)
    _refused("dirs has 3 rows, origins 4", call, O, D[:3], T)
    _refused("tmax must be a contiguous [4] tensor, got shape (3,)", call, O, D, T[:3])
    _refused("tmax must be a contiguous [4] tensor, got shape (4,)", call, O, D, torch.zeros(8, device=DEV)[::2])
    _refused(mixed, call, o, D, T)
    _refused(mixed, call, O, D, t)


@pytest.mark.parametrize("name", POINT_METHODS)
def test_point_refusals(ren, name):
    torch = _torch()
    call = lambda *a: METHODS[name][1](ren, *a)
    p, m = POINTS, MAX_DIST
    mixed = MIXED.format("points and max_dist")
    _refused("points must be float32, got float64", call, p.astype(np.float64), m)
    _refused("max_dist must be float32, got float64", call, p, m.astype(np.float64))
    _refused("points must be [N,k] with k >= 3, got shape (12,)", call, p.reshape(-1), m)
    _refused("points must be [N,k] with k >= 3, got shape (4, 2)", call, p[:, :2], m)
    _refused("max_dist must be [4], got shape (3,)", call, p, m[:3])
    _refused(UNIT.format("points", 3), call, np.asfortranarray(p), m)
    _refused(mixed, call, p.tolist(), m)
    _refused(mixed, call, p, m.tolist())
    if name == "nearest_points_multi":
        _refused("max_hits = 33 (0 .. RT_NEAREST_MULTI_MAX = 32)", ren.nearest_points_multi, p.tolist(), 33)        # max_hits before the arrays
        _refused("max_hits = -1 (0 .. RT_NEAREST_MULTI_MAX = 32)", ren.nearest_points_multi, p, -1)
        _refused("max_hits = 0 asks for the counts alone and needs counts", ren.nearest_points_multi, p, 0, counts=False)
    P, M = _to(p), _to(m)
    _refused("a tensor is on cpu, the context on cuda:0", call, P.cpu(), M)
    _refused("a tensor is on cpu, the context on cuda:0", call, P, M.cpu())
    _refused("expected torch.float32, got torch.float64", call, P.double(), M)
    _refused("expected torch.float32, got torch.float64", call, P.double().cpu(), M)                          # dtype before device
    _refused("a tensor is on cpu, the context on cuda:0", call, P.cpu().reshape(-1), M)                       # device before shape
    _refused(UNIT.format("points", 3), call, _to(np.ascontiguousarray(p.T)).T, M)                             # a transposed tensor
    _refused("points must be [N,k] with k >= 3, got shape (4, 2)", call, P[:, :2], M)
    _refused("max_dist must be a contiguous [4] tensor, got shape (3,)", call, P, M[:3])
    _refused("max_dist must be a contiguous [4] tensor, got shape (4,)", call, P, torch.zeros(8, device=DEV)[::2])
    _refused(mixed, call, p, M)
    _refused(mixed, call, P, m)


@pytest.mark.parametrize("name", XY_METHODS)
def test_pixel_refusals(ren, name):
    torch = _torch()
    call = lambda xy: METHODS[name][1](ren, xy)
    _refused("xy must be int32 [N,2], got int64 (4, 2)", call, XY.astype(np.int64))
    _refused("xy must be int32 [N,2], got int32 (4, 3)", call, np.zeros((4, 3), np.int32))
    _refused("xy must be int32 [N,2], got int32 (8,)", call, XY.reshape(-1))
    _refused(XY_WORDS, call, XY.tolist())
    if name == "pick_multi":
        _refused("max_hits = 33 (0 .. RT_MULTI_HIT_MAX = 32)", ren.pick_multi, U, XY.tolist(), max_hits=33)        # max_hits before the array
    X = _to(XY)
    _refused(XY_WORDS, call, X.long())
    _refused(XY_WORDS, call, X.reshape(-1))
    _refused(XY_WORDS, call, torch.zeros((4, 4), dtype=torch.int32, device=DEV)[:, ::2])                      # not contiguous
    _refused(XY_WORDS, call, _to(np.ascontiguousarray(XY.T)).T)                                               # a transposed tensor
    _refused("a tensor is on cpu, the context on cuda:0", call, X.cpu())


OVERLAP_WORDS = {"boxes": (6, "[N,k] with k >= 6 (lo.xyz, hi.xyz)", None, None),
                 "qtris": (9, "[N,k] with k >= 9 (p0.xyz, p1.xyz, p2.xyz) or [N,3,3]", (3, 3), "qtris [N,3,3]: the nine floats of a triangle must be contiguous"),
                 "hulls": (24, "[N,k] with k >= 24 (c0.xyz .. c7.xyz) or [N,8,3]", (8, 3), "hulls [N,8,3]: the 24 floats of a hull must be contiguous"),
                 "rects": (4, "[N,k] with k >= 4 (x0, y0, x1, y1)", None, None)}


@pytest.mark.parametrize("name", OVERLAP_METHODS)
def test_overlap_refusals(ren, name):
    torch = _torch()
    noun = METHODS[name][0]
    call = lambda q: METHODS[name][1](ren, q)
    method = getattr(ren, name.replace("_cap2", ""))
    capped = (lambda q, cap: method(U, q, cap=cap)) if noun == "rects" else (lambda q, cap: method(q, cap=cap))
    k, layout, cell, broken = OVERLAP_WORDS[noun]
    q = INPUTS[noun][0]
    _refused(f"{noun} must be float32, got float64", call, q.astype(np.float64))
    _refused(f"{noun} must be float32, got float64", call, q.astype(np.float64).reshape(-1))                 # dtype before shape
    _refused("rects must be [N,k]" if noun == "rects" else f"{noun} must be {layout}, got shape ({4 * k},)", call, q.reshape(-1))
    _refused(f"{noun} must be {layout}, got shape (4, {k - 1})", call, q[:, :k - 1])
    _refused(UNIT.format(noun, k), call, np.asfortranarray(q))
    _refused(f"{noun} must be a numpy array or a torch tensor", call, q.tolist())
    _refused("cap = -1", capped, q, -1)
    _refused("cap = -1", capped, q.tolist(), -1)                                                             # cap before the array's type
    if noun == "rects":
        _refused("u must be an RtUniforms", ren.pick_rects, None, q)
        _refused("cap = -1", ren.pick_rects, None, q, cap=-1)                                                # cap before u
    Q = _to(q)
    _refused("a tensor is on cpu, the context on cuda:0", call, Q.cpu())
    _refused("expected torch.float32, got torch.float64", call, Q.double())
    _refused("expected torch.float32, got torch.float64", call, Q.double().cpu())                            # dtype before device
    _refused("a tensor is on cpu, the context on cuda:0", call, Q.cpu().reshape(-1))                         # device before shape
    _refused(f"{noun} must be {layout}, got shape ({4 * k},)", call, Q.reshape(-1))
    _refused(f"{noun} must be {layout}, got shape (4, {k - 1})", call, Q[:, :k - 1])
    _refused(UNIT.format(noun, k), call, _to(np.ascontiguousarray(q.T)).T)                                   # a transposed tensor
    _refused(UNIT.format(noun, k), call, torch.zeros((4, 2 * k), device=DEV)[:, ::2])
    if cell:
        _refused(broken, call, np.zeros((4,) + cell[::-1], f32).transpose(0, 2, 1))
        _refused(broken, call, torch.zeros((4,) + cell[::-1], device=DEV).transpose(1, 2))
        _refused(broken, call, torch.zeros((4, cell[0], 4), device=DEV)[:, :, :3])


# ---------------------------------------------------------------- mesh_hit_parts, after a rebuild of the same quad as a dynamic mesh

def test_mesh_hit_parts(ren):
    torch = _torch()
    words = "rt_mi355 error -1: mesh_hit_parts: "
    try:
        ren.mesh_upload(np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], f32), np.array([0, 1, 2, 0, 2, 3], np.uint32))
        ren.mesh_rebuild()
        rec = ren.trace_rays(ORIGINS, DIRS).record
        want = ren.mesh_hit_parts(rec)
        assert [a.tolist() for a in want] == [[0, 0, 0, -1], [0, 1, want[1][2], -1]] and want[0].dtype == want[1].dtype == np.int32
        R = _to(rec)
        _same(ren.mesh_hit_parts(R), want, "torch", torch.Tensor)
        _same(ren.mesh_hit_parts(rt.RayHits(R)), want, "RayHits", torch.Tensor)
        wide_np, wide_t = _wide(rec)
        _same(ren.mesh_hit_parts(wide_np), want, "strided, numpy")                   # records are made contiguous on both paths
        _same(ren.mesh_hit_parts(wide_t), want, "strided, torch", torch.Tensor)
        _same(ren.mesh_hit_parts(_to(np.ascontiguousarray(rec.T)).T), want, "transposed, torch", torch.Tensor)
        for i in (0, 3):
            _same(ren.mesh_hit_parts(R[i:i + 1]), tuple(a[i:i + 1] for a in want), ("N = 1", i), torch.Tensor)
            _same(ren.mesh_hit_parts(rec[i:i + 1]), tuple(a[i:i + 1] for a in want), ("N = 1, numpy", i))
        for path in ("numpy", "torch"):
            got = _outcome(lambda: ren.mesh_hit_parts(_empty(rec, path)))
            print("mesh_hit_parts", path, repr(got))
            assert got == N0["mesh_hit_parts"][path], path
        _from_side_stream(ren, lambda r, x: r.mesh_hit_parts(x), (rec,), want, "mesh_hit_parts")
        _refused("records must be float32 [N,4], got float64 (4, 4)", ren.mesh_hit_parts, rec.astype(np.float64), prefix=words)
        _refused("records must be float32 [N,4], got float32 (16,)", ren.mesh_hit_parts, rec.reshape(-1), prefix=words)
        _refused("records must be float32 [N,4], got float32 (4, 3)", ren.mesh_hit_parts, rec[:, :3], prefix=words)
        tensor = "records must be a numpy array or a float32 [N,4] tensor on cuda:0"
        for bad in (rec.tolist(), R.cpu(), R.double(), R.reshape(-1), R[:, :3]):
            _refused(tensor, ren.mesh_hit_parts, bad, prefix=words)
    finally:
        ren.upload_bvh(NODES, TRIS)                                                  # takes the scene over again and releases the mesh
