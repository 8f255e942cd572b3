"""The Python half of the host queries (multi_hits, nearest_points, nearest_points_multi, box_overlaps, tri_overlaps, hull_overlaps, box_corners,
rect_frusta), no GPU: what the binding refuses, by full message text, and the query layouts it accepts, against the contiguous [N,k] call bit for
bit.  The texts and the N = 0 outcomes are recorded here literally -- they are the binding's contract, not recomputed from it -- so that a change of
the shared row / ray / point checks that moves a word, an order of refusals or a stride shows."""
import numpy as np
import pytest

import opengl_raytracing_amd as rt

f32 = np.float32
PREFIX = "rt_mi355 error -1: trace_rays: "
UNIT = "{} must have unit stride along its last dimension and rows at least {} floats apart"

QUAD = np.array([[0, 0, 0, 1, 0, 0, 1, 1, 0], [0, 0, 0, 1, 1, 0, 0, 1, 0]], f32)            # two triangles of the unit square in z = 0
NODES, TRIS = rt.build_bvh(QUAD)
ORIGINS = np.array([[0.75, 0.25, 1], [0.25, 0.75, 1], [0.6, 0.5, 2], [3, 3, 1]], f32)        # ray 3 misses
DIRS = np.array([[0, 0, -1]] * 4, f32)
TMAX = np.array([5, 5, 1.5, 5], f32)                                                         # ray 2 stops short
POINTS = np.array([[0.75, 0.25, 0.5], [0.25, 0.75, -1], [2, 0.5, 0], [-1, -1, 3]], f32)
MAX_DIST = np.array([1, 2, 0.5, 9], f32)                                                     # point 2 finds nothing within its limit
BOXES = np.array([[0.6, 0.1, -1, 0.9, 0.3, 1], [-1, -1, -1, 2, 2, 2], [0.1, 0.6, 0.5, 0.3, 0.9, 1], [0.4, 0.4, -0.1, 0.6, 0.6, 0.1]], f32)
QTRIS = np.array([[0.7, 0.2, -1, 0.7, 0.2, 1, 0.8, 0.3, 1], [0, 0.5, -1, 1, 0.5, -1, 0.5, 0.5, 1], [0, 0, 1, 1, 0, 1, 0, 1, 1],
                  [0.2, 0.7, -0.5, 0.2, 0.8, 0.5, 0.3, 0.8, 0.5]], f32)
HULLS = rt.box_corners(BOXES)
RECTS = np.array([[0, 0, 16, 16], [4, 4, 9, 7], [7.5, 7.5, 8.5, 8.5], [0, 0, 1, 1]], f32)


def _uniforms():
    cam = rt.default_camera()
    cam.pos[0], cam.pos[1], cam.pos[2] = 0.5, 0.5, 3.0
    cam.yaw, cam.pitch, cam.aspect = -90.0, 0.0, 1.0
    return rt.frame_uniforms(rt.default_render_params(), cam, 16, 16, 0, True, NODES.shape[0], TRIS.shape[0])


U = _uniforms()
LO, HI = NODES[0, 0:3], NODES[0, 4:7]


def _refused(text, fn, *args, **kw):
    with pytest.raises(rt.RtError) as e:
        fn(*args, **kw)
    assert str(e.value) == PREFIX + text, str(e.value)
    assert e.value.code == rt.RT_ERR_INVALID


def _bits(a):
    return (a.dtype, a.shape, np.ascontiguousarray(a).tobytes())


def _same(got, want, fields):
    assert type(got) is type(want)
    for f in fields:
        assert _bits(getattr(got, f)) == _bits(getattr(want, f)), f


def _wide(a, cols, at=0):
    """The rows of `a` as a view into a wider array of `cols` columns, NaN around them."""
    w = np.full((a.shape[0], cols), np.nan, f32)
    w[:, at:at + a.shape[1]] = a
    return w[:, at:at + a.shape[1]]


def _fortran(a):
    out = np.asfortranarray(a)
    assert out.strides[-1] != 4 or a.shape[0] == 1
    return out


# ---------------------------------------------------------------- rays: multi_hits

def _multi(o, d, t=None, k=4):
    return rt.multi_hits(NODES, TRIS, o, d, t, max_hits=k)


def test_multi_hits_refusals():
    o, d, t = ORIGINS, DIRS, TMAX
    _refused("origins must be float32, got float64", _multi, o.astype(np.float64), d)
    _refused("dirs must be float32, got float64", _multi, o, d.astype(np.float64))
    _refused("tmax must be float32, got float64", _multi, o, d, t.astype(np.float64))
    _refused("origins must be float32, got float64", _multi, o.astype(np.float64).reshape(-1), d)          # dtype before shape
    _refused("origins must be [N,k] with k >= 3, got shape (12,)", _multi, o.reshape(-1), d)
    _refused("dirs must be [N,k] with k >= 3, got shape (12,)", _multi, o, d.reshape(-1))
    _refused("origins must be [N,k] with k >= 3, got shape (4, 2)", _multi, o[:, :2], d)
    _refused("dirs must be [N,k] with k >= 3, got shape (4, 2)", _multi, o, d[:, :2])
    _refused("dirs has 3 rows, origins 4", _multi, o, d[:3])
    _refused("tmax must be [4], got shape (3,)", _multi, o, d, t[:3])
    _refused("tmax must be [4], got shape (4, 1)", _multi, o, d, t.reshape(4, 1))
    _refused(UNIT.format("origins", 3), _multi, _fortran(o), d)
    _refused(UNIT.format("dirs", 3), _multi, o, _fortran(d))
    _refused(UNIT.format("origins", 3), _multi, np.zeros((4, 8), f32)[:, ::2], d)
    _refused("origins must be a numpy array", _multi, o.tolist(), d)
    _refused("dirs must be a numpy array", _multi, o, d.tolist())
    _refused("tmax must be a numpy array", _multi, o, d, t.tolist())
    _refused("max_hits = 33 (0 .. RT_MULTI_HIT_MAX = 32)", _multi, o, d, k=33)
    _refused("max_hits = -1 (0 .. RT_MULTI_HIT_MAX = 32)", _multi, o, d, k=-1)
    _refused("max_hits = 33 (0 .. RT_MULTI_HIT_MAX = 32)", _multi, o.tolist(), d, k=33)                    # max_hits before the arrays


def test_multi_hits_layouts():
    want = _multi(ORIGINS, DIRS, TMAX)
    assert want.count.tolist() == [1, 1, 0, 0] and want.hits.shape == (4, 4, 4) and want.prim[:2, 0].tolist() == [0, 1]
    fields = ("hits", "count")
    halves = np.full((4, 8), np.nan, f32)
    halves[:, 0:3], halves[:, 4:7] = ORIGINS, DIRS
    _same(_multi(halves[:, 0:4], halves[:, 4:8], TMAX), want, fields)                  # the two halves of one [N,8] array
    _same(_multi(halves[:, 0:3], halves[:, 4:7], TMAX), want, fields)
    _same(_multi(_wide(ORIGINS, 5, 1), _wide(DIRS, 7, 2), TMAX), want, fields)
    _same(_multi(ORIGINS, DIRS, np.repeat(TMAX, 2)[::2]), want, fields)                # a strided tmax is made contiguous
    one = _multi(ORIGINS[1:2], DIRS[1:2], TMAX[1:2])
    assert _bits(one.hits) == _bits(want.hits[1:2]) and _bits(one.count) == _bits(want.count[1:2])
    _same(_multi(halves[1:2, 0:4], halves[1:2, 4:8], TMAX[1:2]), one, fields)          # one row of a wider array: the stride is shape[1]
    _same(_multi(halves[1:2], halves[1:2, 4:8], TMAX[1:2]), one, fields)
    none = _multi(ORIGINS[:0], DIRS[:0], TMAX[:0])
    assert _bits(none.hits) == (np.dtype(f32), (0, 4, 4), b"") and _bits(none.count) == (np.dtype(np.int32), (0,), b"")
    _same(_multi(ORIGINS[:0], DIRS[:0]), none, fields)
    zero = _multi(ORIGINS, DIRS, TMAX, k=0)                                           # the counts alone
    assert zero.hits.shape == (4, 0, 4) and _bits(zero.count) == _bits(want.count)


# ---------------------------------------------------------------- points: nearest_points, nearest_points_multi

def _near(p, m=None):
    return rt.nearest_points(NODES, TRIS, p, m)


def _near_multi(p, m=None, k=2):
    return rt.nearest_points_multi(NODES, TRIS, p, k, m)


@pytest.mark.parametrize("fn", [_near, _near_multi])
def test_nearest_refusals(fn):
    p, m = POINTS, MAX_DIST
    _refused("points must be float32, got float64", fn, p.astype(np.float64))
    _refused("max_dist must be float32, got float64", fn, p, m.astype(np.float64))
    _refused("points must be float32, got float64", fn, p.astype(np.float64).reshape(-1))                 # dtype before shape
    _refused("points must be [N,k] with k >= 3, got shape (12,)", fn, p.reshape(-1))
    _refused("points must be [N,k] with k >= 3, got shape (4, 2)", fn, p[:, :2])
    _refused("max_dist must be [4], got shape (3,)", fn, p, m[:3])
    _refused("max_dist must be [4], got shape (4, 1)", fn, p, m.reshape(4, 1))
    _refused(UNIT.format("points", 3), fn, _fortran(p))
    _refused("points must be a numpy array", fn, p.tolist())
    _refused("max_dist must be a numpy array", fn, p, m.tolist())


def test_nearest_multi_max_hits():
    _refused("max_hits = 33 (0 .. RT_NEAREST_MULTI_MAX = 32)", _near_multi, POINTS, k=33)
    _refused("max_hits = -1 (0 .. RT_NEAREST_MULTI_MAX = 32)", _near_multi, POINTS, k=-1)
    _refused("max_hits = 33 (0 .. RT_NEAREST_MULTI_MAX = 32)", _near_multi, POINTS.tolist(), k=33)       # max_hits before the arrays


@pytest.mark.parametrize("fn,fields,tail", [(_near, ("hits", "points"), (4,)), (_near_multi, ("hits", "points", "count"), (2, 4))])
def test_nearest_layouts(fn, fields, tail):
    want = fn(POINTS, MAX_DIST)
    assert want.hits.shape == (4,) + tail and np.isinf(want.dist2.reshape(4, -1)[2]).all() and (want.prim.reshape(4, -1)[:, 0] >= 0).tolist() == [True, True, False, True]
    halves = np.full((4, 8), np.nan, f32)
    halves[:, 4:7] = POINTS
    _same(fn(halves[:, 4:7], MAX_DIST), want, fields)
    _same(fn(halves[:, 4:8], MAX_DIST), want, fields)
    _same(fn(_wide(POINTS, 5, 1), np.repeat(MAX_DIST, 2)[::2]), want, fields)
    one = fn(POINTS[1:2], MAX_DIST[1:2])
    for f in fields:
        assert _bits(getattr(one, f)) == _bits(getattr(want, f)[1:2]), f
    _same(fn(halves[1:2, 4:8], MAX_DIST[1:2]), one, fields)                            # one row of a wider array: the stride is shape[1]
    none = fn(POINTS[:0], MAX_DIST[:0])
    assert none.hits.shape == (0,) + tail and none.hits.dtype == f32 and none.points.shape == (0,) + tail[:-1] + (3,) and none.visits is None
    _same(fn(POINTS[:0]), none, fields)
    assert fn is _near or _bits(none.count) == (np.dtype(np.int32), (0,), b"")


# ---------------------------------------------------------------- boxes, triangles, hulls: the overlap queries

def _boxes(b, cap=None):
    return rt.box_overlaps(NODES, TRIS, b, cap)


def _tris(q, cap=None):
    return rt.tri_overlaps(NODES, TRIS, q, cap)


def _hulls(h, cap=None):
    return rt.hull_overlaps(NODES, TRIS, h, cap)


FAMILIES = [
    # call, noun, the queries, least k, layout words, 3-D cell, the words of a broken cell
    (_boxes, "boxes", BOXES, 6, "[N,k] with k >= 6 (lo.xyz, hi.xyz)", None, None),
    (_tris, "qtris", QTRIS, 9, "[N,k] with k >= 9 (p0.xyz, p1.xyz, p2.xyz) or [N,3,3]", (3, 3), "qtris [N,3,3]: the nine floats of a triangle must be contiguous"),
    (_hulls, "hulls", HULLS, 24, "[N,k] with k >= 24 (c0.xyz .. c7.xyz) or [N,8,3]", (8, 3), "hulls [N,8,3]: the 24 floats of a hull must be contiguous"),
]


@pytest.mark.parametrize("fn,noun,q,k,layout,cell,broken", FAMILIES)
def test_overlap_refusals(fn, noun, q, k, layout, cell, broken):
    _refused(f"{noun} must be float32, got float64", fn, q.astype(np.float64))
    _refused(f"{noun} must be float32, got float64", fn, q.astype(np.float64).reshape(-1))              # dtype before shape
    _refused(f"{noun} must be {layout}, got shape ({4 * k},)", fn, q.reshape(-1))
    _refused(f"{noun} must be {layout}, got shape (4, {k - 1})", fn, q[:, :k - 1])
    _refused(f"{noun} must be {layout}, got shape (4, 2, 2)", fn, np.zeros((4, 2, 2), f32))
    _refused(UNIT.format(noun, k), fn, _fortran(q))
    _refused(UNIT.format(noun, k), fn, np.zeros((4, 2 * k), f32)[:, ::2])
    _refused(f"{noun} must be a numpy array", fn, q.tolist())
    _refused("cap = -1", fn, q, cap=-1)
    _refused("cap = -1", fn, q.tolist(), cap=-1)                                                         # cap before the array's type
    if cell:
        _refused(broken, fn, np.zeros((4,) + cell[::-1], f32).transpose(0, 2, 1))
        _refused(broken, fn, np.zeros((4, cell[0], 4), f32)[:, :, :3])


@pytest.mark.parametrize("fn,noun,q,k,layout,cell,broken", FAMILIES)
def test_overlap_layouts(fn, noun, q, k, layout, cell, broken):
    fields = ("count", "offsets", "prims")
    want = fn(q)
    assert want.count.sum() == want.prims.size > 0 and want.count.min() == 0 and want.count.max() == 2 and want.visits is None
    capped = fn(q, cap=1)
    assert capped.offsets.tolist() == [0, 1, 2, 3, 4] and _bits(capped.count) == _bits(want.count)
    for cap, ans in ((None, want), (1, capped)):
        _same(fn(_wide(q, 32), cap), ans, fields)                                      # rows strided out of a wider array
        _same(fn(_wide(q, k + 1, 1), cap), ans, fields)
        if cell:
            _same(fn(q.reshape((4,) + cell), cap), ans, fields)
            _same(fn(np.lib.stride_tricks.as_strided(_wide(q, 32), (4,) + cell, (128, 12, 4)), cap), ans, fields)
        one = fn(q[1:2], cap)
        assert one.count.tolist() == [2] and one.prims.tolist() == ([0, 1] if cap is None else ans.prims[1:2].tolist())
        _same(fn(_wide(q, 32)[1:2], cap), one, fields)                                 # one row of a wider array: the stride is shape[1]
        _same(fn(np.pad(q[1:2], ((0, 0), (0, 32 - k))), cap), one, fields)             # ... and a [1,32] array as it stands
        none = fn(q[:0], cap)
        assert _bits(none.count) == (np.dtype(np.int32), (0,), b"") and none.offsets.tolist() == [0] and none.offsets.dtype == np.int32
        assert _bits(none.prims) == (np.dtype(np.int32), (0,), b"") and none.visits is None and (not cell or none.pairs().shape == (0, 2))
        if cell:
            _same(fn(q[:0].reshape((0,) + cell), cap), none, fields)


# ---------------------------------------------------------------- the corner makers: box_corners, rect_frusta

def test_box_corners_refusals_and_layouts():
    _refused("boxes must be float32, got float64", rt.box_corners, BOXES.astype(np.float64))
    _refused("boxes must be [N,k] with k >= 6 (lo.xyz, hi.xyz), got shape (24,)", rt.box_corners, BOXES.reshape(-1))
    _refused("boxes must be [N,k] with k >= 6 (lo.xyz, hi.xyz), got shape (4, 5)", rt.box_corners, BOXES[:, :5])
    _refused(UNIT.format("boxes", 6), rt.box_corners, _fortran(BOXES))
    _refused("boxes must be a numpy array", rt.box_corners, BOXES.tolist())
    _refused("M must hold one matrix or one per box, got 2 for 4 boxes", rt.box_corners, BOXES, np.zeros((2, 16), f32))
    assert HULLS.shape == (4, 24) and HULLS.dtype == f32
    assert _bits(HULLS[:, 0:3]) == _bits(BOXES[:, 0:3]) and _bits(HULLS[:, 21:24]) == _bits(BOXES[:, 3:6])
    assert _bits(rt.box_corners(_wide(BOXES, 8, 1))) == _bits(HULLS)
    assert _bits(rt.box_corners(BOXES[1:2])) == _bits(HULLS[1:2]) and _bits(rt.box_corners(_wide(BOXES, 8)[1:2])) == _bits(HULLS[1:2])
    assert _bits(rt.box_corners(BOXES[:0])) == (np.dtype(f32), (0, 24), b"")
    M = np.eye(4, dtype=f32)
    M[3, :3] = (1, 2, 3)                                                               # column-major: a translation
    moved = rt.box_corners(BOXES, M)
    assert np.array_equal(moved, (HULLS.reshape(4, 8, 3) + f32([1, 2, 3])).reshape(4, 24))
    assert _bits(rt.box_corners(_wide(BOXES, 8, 1), np.tile(M.reshape(1, 16), (4, 1)))) == _bits(moved)


def test_rect_frusta_refusals_and_layouts():
    fr = lambda r: rt.rect_frusta(U, LO, HI, r)
    _refused("rects must be float32, got float64", fr, RECTS.astype(np.float64))
    _refused("rects must be [N,k]", fr, RECTS.reshape(-1))
    _refused("rects must be [N,k] with k >= 4 (x0, y0, x1, y1), got shape (4, 3)", fr, RECTS[:, :3])
    _refused(UNIT.format("rects", 4), fr, _fortran(RECTS))
    _refused("rects must be a numpy array", fr, RECTS.tolist())
    want = fr(RECTS)
    assert want.shape == (4, 24) and want.dtype == f32 and np.isfinite(want).all()
    assert _bits(fr(_wide(RECTS, 8, 2))) == _bits(want)
    assert _bits(fr(RECTS[1:2])) == _bits(want[1:2]) and _bits(fr(_wide(RECTS, 8)[1:2])) == _bits(want[1:2])
    assert _bits(fr(RECTS[:0])) == (np.dtype(f32), (0, 24), b"")
    # the frusta are hulls as the hull query takes them: the whole frame sees both triangles, one pixel off the quad sees none
    got = _hulls(want)
    assert got.count[0] == 2 and _bits(_hulls(want.reshape(4, 8, 3)).prims) == _bits(got.prims)
