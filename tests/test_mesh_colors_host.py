"""rt_hit_colors and rt_color_rows, the host definitions of the dynamic mesh's per-vertex colours, without a GPU: against their
float32 numpy restatement (tests/colors_ref.py) bit for bit, hit records off the triangle and off the mesh, the flat rule (three bit-equal corners hand
their colour back), vertex_colors_from_parts, their refusals, the exports, a null context to every new entry, and their meaning: linear interpolation
reproduces an affine colour field on the icosphere."""
import ctypes as C
import functools

import numpy as np
import pytest

import colors_ref
import opengl_raytracing_amd as rt
from colors_ref import bits, records

f32 = np.float32
IDENT = np.eye(4, dtype=f32).reshape(-1)
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
NEW_SYMBOLS = ("rt_mesh_colors_enable", "rt_mesh_colors", "rt_mesh_set_colors", "rt_mesh_colors_refresh", "rt_mesh_hit_colors", "rt_mesh_hit_colors_host",
               "rt_hit_colors", "rt_color_rows")
FP, U32P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
PART_FIRST = (0, 100, 220, 300)
PART_RGB = np.array([[0.9, 0.1, 0.1], [0.1, 0.8, 0.2], [0.2, 0.3, 0.95]], f32)


def _strip(nv, seed):
    """A triangle strip over nv random vertices: nv - 2 triangles, every vertex used."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (nv, 3)).astype(f32)
    f = np.stack([np.arange(nv - 2), np.arange(1, nv - 1), np.arange(2, nv)], axis=1)
    return v, f.astype(np.uint32).reshape(-1)


def _soup(n, seed=1):
    rng = np.random.default_rng(seed + n)
    nv = max(3, n // 2 + 3)
    return rng.normal(0, 1, (nv, 3)).astype(f32), rng.integers(0, nv, (n, 3)).astype(np.uint32).reshape(-1)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (order [T], indices [3T], colors [V,3]), read only."""
    rng = np.random.default_rng(len(name))
    if name == "1 triangle":
        v, f = np.array([[0, 0, 0], [1, 0, 0.5], [0.2, 1, 0]], f32), np.array([0, 1, 2], np.uint32)
    elif name == "2 triangles":
        v, f = np.array([[0, 0, 0], [1, 0, 0.5], [0.2, 1, 0], [1.1, 0.9, -0.7]], f32), np.array([0, 1, 2, 2, 1, 3], np.uint32)   # share the edge 1 - 2
    elif name in ("63 vertices", "64 vertices", "65 vertices"):
        v, f = _strip(int(name.split()[0]), 7)
    elif name in ("1000 triangles", "3 parts"):
        v, f = _soup(1000 if name == "1000 triangles" else 300)
    else:
        raise KeyError(name)
    n, nv = f.size // 3, v.shape[0]
    if name == "1000 triangles":
        order = rng.permutation(n).astype(np.int32)                              # a shuffled order: the order array matters
    else:
        _, _, order = rt.build_bvh_order(rt.gather_triangles(v, f, IDENT))
        order = np.ascontiguousarray(order, np.int32)
    if name == "3 parts":
        f = f.copy()
        f[3 * 99], f[3 * 100], f[3 * 220] = 7, 7, 7                              # vertex 7 is shared by all three parts: the last one wins
        colors = rt.vertex_colors_from_parts(f, PART_FIRST, PART_RGB, nv)
    else:
        colors = rng.uniform(0, 1, (nv, 3)).astype(f32)
    for a in (order, f, colors):
        a.setflags(write=False)
    return order, f, colors


CASES = ("1 triangle", "2 triangles", "63 vertices", "64 vertices", "65 vertices", "1000 triangles", "3 parts")


def _hits(n_tris, n, seed):
    rng = np.random.default_rng(seed)
    prim = rng.integers(0, n_tris, n).astype(np.int32)
    prim[:min(n, n_tris)] = np.arange(min(n, n_tris))                            # every row at least once where there is room
    a = rng.uniform(0, 1, n).astype(f32)
    b = (rng.uniform(0, 1, n) * (1 - a)).astype(f32)
    a[::11], b[::13] = 0, 0                                                      # corners and edges
    return records(prim, a, b)


@pytest.mark.parametrize("name", CASES)
def test_equals_the_numpy_definition(name):
    order, f, colors = _case(name)
    n, nv = order.size, colors.shape[0]
    rows = rt.color_rows(order, f, colors)
    assert rows.shape == (n, 12) and (bits(rows) == bits(colors_ref.color_rows(order, f, colors))).all()
    assert (bits(rows.reshape(n, 3, 4)[:, :, 3]) == 0).all()
    rec = _hits(n, max(257, 2 * n), 5)
    got = rt.hit_colors(None, order, f, colors, rec)
    want = colors_ref.hit_colors(order, f, colors, rec)
    assert (bits(got) == bits(want)).all(), int((bits(got) != bits(want)).any(axis=1).sum())
    t12 = np.zeros((n, 12), f32)                                                 # the rows are not read: any rows give the same answer
    assert (bits(rt.hit_colors(t12, order, f, colors, rec)) == bits(got)).all()
    four = np.concatenate([colors, np.full((nv, 1), 9, f32)], axis=1)           # the device layout: the fourth float is not a colour's
    assert (bits(rt.hit_colors(None, order, f, four, rec)) == bits(got)).all()
    assert (bits(rt.color_rows(order, f, four)) == bits(rows)).all()
    if name in ("1000 triangles", "3 parts"):
        assert not np.array_equal(order, np.arange(n))
        assert got.min() >= 0 and got.max() <= 1 + 1e-6                          # a convex combination up to rounding
    if name == "3 parts":
        assert (colors[7] == PART_RGB[2]).all()                                  # the shared vertex: the later part wins
        want_c = colors_ref.vertex_colors_from_parts(f, PART_FIRST, PART_RGB, nv)
        assert (bits(colors) == bits(want_c)).all()
        used = np.zeros(nv, bool)
        used[f] = True
        assert (colors[~used] == colors_ref.GREY).all() and rt.MESH_GREY == 0.85


def test_hit_records_off_the_triangle_and_off_the_mesh():
    order, f, colors = _case("1000 triangles")
    n = order.size
    rec = _hits(n, 64, 9)
    rec[0:4, 2] = [np.nan, np.inf, -np.inf, 0.25]                                # NaN and infinite barycentrics: the first corner
    rec[2:6, 3] = [0.5, np.nan, np.inf, -np.inf]
    bad = np.array([-1, n, INT_MAX, INT_MIN], np.int32)
    rec[8:12, 1] = bad.view(f32)
    got = rt.hit_colors(None, order, f, colors, rec)
    assert (bits(got) == bits(colors_ref.hit_colors(order, f, colors, rec))).all()
    c0 = colors[f.reshape(-1, 3)[order[colors_ref.prims(rec)[:6]], 0]]
    assert (bits(got[:6]) == bits(c0)).all()
    assert (bits(got[8:12]) == 0).all() and (bits(got[12:]) != 0).any(axis=1).all()
    # nothing is read out of bounds: the same call on exactly-sized copies, the last row's hit included
    rec[12, 1] = np.array([n - 1], np.int32).view(f32)[0]
    again = rt.hit_colors(None, order.copy(), f.copy(), colors.copy(), rec.copy())
    assert (bits(again) == bits(colors_ref.hit_colors(order, f, colors, rec))).all()


def test_flat_rule():
    """Three bit-equal corners return c0's bits at every (a, b), a + b slightly above 1 included -- where the blend itself would not."""
    order, f, _ = _case("65 vertices")
    n = order.size
    c = np.array([0.85, 0.1, 0.7], f32)
    colors = np.tile(c, (65, 1))
    a = np.array([0, 1, 0, 0.5, 0.5000001, 0.3333333, 0.9999999, 1e-8, 0.25, 0.7, -0.1, 1.5, np.nan], f32)
    b = np.array([0, 0, 1, 0.5, 0.5000001, 0.3333334, 2e-7, 1.0, 0.1, 0.3000001, 0.2, 0.5, 0.5], f32)
    prim = (np.arange(a.size) * 5 % n).astype(np.int32)
    rec = records(prim, a, b)
    got = rt.hit_colors(None, order, f, colors, rec)
    assert (bits(got) == bits(np.tile(c, (a.size, 1)))).all()
    with np.errstate(all="ignore"):
        w = ((f32(1) - a).astype(f32) - b).astype(f32)
        blend = (((c[None] * w[:, None]).astype(f32) + (c[None] * a[:, None]).astype(f32)).astype(f32) + (c[None] * b[:, None]).astype(f32)).astype(f32)
    assert (bits(blend) != bits(got)).any()                                      # the rule is not vacuous: the blend loses bits somewhere
    # the constant the frames replace: 0.85 at every corner is 0.85f to the bit
    grey = rt.hit_colors(None, order, f, np.full((65, 3), 0.85, f32), rec)
    assert (bits(grey) == bits(f32(0.85))).all()
    # channel by channel: a channel pinned over the mesh comes back to the bit whatever the other two do
    rng = np.random.default_rng(8)
    for ch in range(3):
        pinned = rng.uniform(0, 1, (65, 3)).astype(f32)
        pinned[:, ch] = f32(0.85)
        out = rt.hit_colors(None, order, f, pinned, rec)
        assert (bits(out[:, ch]) == bits(f32(0.85))).all(), ch
        assert (bits(out) == bits(colors_ref.hit_colors(order, f, pinned, rec))).all()
    # one corner one ulp away: no longer flat, the blend's bits
    colors2 = colors.copy()
    colors2[f.reshape(-1, 3)[order[prim[3]], 1], 0] = np.nextafter(f32(0.85), f32(1))
    got2 = rt.hit_colors(None, order, f, colors2, rec)
    assert (bits(got2) == bits(colors_ref.hit_colors(order, f, colors2, rec))).all()


# ---------------------------------------------------------------- refusals, exports, a null context
def _hc_raw(t12, n_tris, order, f, colors, nv, rec, n, out):
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)      # noqa: E731
    return rt.lib().rt_hit_colors(p(t12, FP), n_tris, p(order, I32P), p(f, U32P), p(colors, FP), nv, None if rec is None else C.c_void_p(rec.ctypes.data), n,
                                  p(out, FP))


def _cr_raw(order, f, colors, n_tris, nv, out):
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)      # noqa: E731
    return rt.lib().rt_color_rows(p(order, I32P), p(f, U32P), p(colors, FP), n_tris, nv, p(out, FP))


def test_refusals():
    order, f, colors = (np.array(a) for a in _case("65 vertices"))
    n, nv = order.size, colors.shape[0]
    rows = np.zeros((n, 12), f32)
    assert _cr_raw(order, f, colors, n, nv, rows) == rt.RT_OK
    for args in ((None, f, colors, n, nv, rows), (order, None, colors, n, nv, rows), (order, f, None, n, nv, rows), (order, f, colors, n, nv, None),
                 (order, f, colors, 0, nv, rows), (order, f, colors, -1, nv, rows), (order, f, colors, n, 0, rows), (order, f, colors, n, nv - 1, rows)):
        assert _cr_raw(*args) == rt.RT_ERR_INVALID
    for bad in (-1, n, INT_MAX, INT_MIN):
        o2 = order.copy()
        o2[3] = bad
        assert _cr_raw(o2, f, colors, n, nv, rows) == rt.RT_ERR_INVALID            # an order entry outside the triangles
    rec = _hits(n, 9, 2)
    out = np.zeros((9, 3), f32)
    assert _hc_raw(None, n, order, f, colors, nv, rec, 9, out) == rt.RT_OK
    assert _hc_raw(None, n, order, f, colors, nv, rec, 0, out) == rt.RT_OK         # no hits: nothing to do
    assert _hc_raw(None, n, order, f, colors, nv, None, 0, None) == rt.RT_OK
    for args in ((None, n, None, f, colors, nv, rec, 9, out), (None, n, order, None, colors, nv, rec, 9, out), (None, n, order, f, None, nv, rec, 9, out),
                 (None, n, order, f, colors, nv, None, 9, out), (None, n, order, f, colors, nv, rec, 9, None), (None, 0, order, f, colors, nv, rec, 9, out),
                 (None, n, order, f, colors, 0, rec, 9, out), (None, n, order, f, colors, nv, rec, -1, out)):
        assert _hc_raw(*args) == rt.RT_ERR_INVALID
    o2 = order.copy()
    o2[colors_ref.prims(rec)[0]] = n
    assert _hc_raw(None, n, o2, f, colors, nv, rec, 9, out) == rt.RT_ERR_INVALID   # the order entry of a hit row outside the triangles
    assert _hc_raw(None, n, order, f, colors, 1, rec, 9, out) == rt.RT_ERR_INVALID  # ... and a corner outside the colours
    for call in (lambda: rt.hit_colors(None, order[:-1], f, colors, rec), lambda: rt.color_rows(order, f[:-3], colors),
                 lambda: rt.hit_colors(None, order, f, colors, rec[:, :3]), lambda: rt.hit_colors(None, order, f, colors[:, :2], rec),
                 lambda: rt.hit_colors(None, order, f, colors, rec.astype(np.float64)), lambda: rt.hit_colors(np.zeros((n - 1, 12), f32), order, f, colors, rec),
                 lambda: rt.vertex_colors_from_parts(f, (0, 10, n - 1), PART_RGB[:2], nv), lambda: rt.vertex_colors_from_parts(f, (0, n), PART_RGB[:1], nv - 1)):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt.RT_ERR_INVALID


def test_symbols_are_exported_and_declared():
    L = rt.lib()
    for name in NEW_SYMBOLS:
        assert name in rt.SIGNATURES, name
        assert getattr(L, name) is not None, name
    assert rt.RT_SCENE_ARRAY_COLOR_ROWS == 15 and rt.SCENE_ARRAYS_MESH["color rows"] == 15
    for method in ("mesh_colors_enable", "mesh_colors", "mesh_set_colors", "mesh_colors_refresh", "mesh_color_rows", "mesh_hit_colors"):
        assert callable(getattr(rt.Renderer, method)), method
    for fn in ("hit_colors", "color_rows", "vertex_colors_from_parts"):
        assert callable(getattr(rt, fn)), fn


def test_null_context():
    L = rt.lib()
    rec, out, rgb = np.zeros((4, 4), f32), np.zeros((4, 3), f32), np.zeros((4, 3), f32)
    ptr, size = C.c_void_p(), C.c_size_t(1)
    calls = {
        "rt_mesh_colors_enable": lambda: L.rt_mesh_colors_enable(None, 1),
        "rt_mesh_colors": lambda: L.rt_mesh_colors(None, C.byref(ptr), C.byref(size)),
        "rt_mesh_set_colors": lambda: L.rt_mesh_set_colors(None, rgb.ctypes.data_as(FP), 0, 4),
        "rt_mesh_colors_refresh": lambda: L.rt_mesh_colors_refresh(None),
        "rt_mesh_hit_colors": lambda: L.rt_mesh_hit_colors(None, C.c_void_p(rec.ctypes.data), 4, C.c_void_p(out.ctypes.data)),
        "rt_mesh_hit_colors_host": lambda: L.rt_mesh_hit_colors_host(None, C.c_void_p(rec.ctypes.data), 4, C.c_void_p(out.ctypes.data)),
    }
    assert set(calls) == set(NEW_SYMBOLS) - {"rt_hit_colors", "rt_color_rows"}
    for name, call in calls.items():
        assert call() == rt.RT_ERR_INVALID, name
    assert L.rt_debug_read_scene(None, rt.RT_SCENE_ARRAY_COLOR_ROWS, None, 0, C.byref(size)) == rt.RT_ERR_INVALID


# ---------------------------------------------------------------- the meaning: an affine colour field
# Linear interpolation reproduces an affine field.  Every vertex of the 1 280-triangle icosphere gets the colour A p + b of its position p; the colour
# rt_hit_colors gives at a hit is compared with A x + b at the hit point x, found by brute force in float64 for a 48 x 48 grid of parallel rays.
# Largest absolute error over the hits and the three channels, measured on the CPU:
#   1.142e-07  over 1 403 hits
# The test asserts four times the measured value: the margin covers the rays' placement and the float32 hit point.
AFFINE_MEASURED = 1.142e-07
AFFINE_A = np.array([[0.30, 0.05, -0.10], [-0.07, 0.25, 0.12], [0.02, -0.15, 0.28]])
AFFINE_B = np.array([0.5, 0.45, 0.55])


def test_an_affine_field_is_reproduced_on_the_icosphere():
    v, f = rt.meshgen.icosphere(3)
    v = np.ascontiguousarray(v, f32)
    _, t12, order = rt.build_bvh_order(rt.gather_triangles(v, f, IDENT))
    d = np.array([0.13, -0.07, -1.0])
    d /= np.linalg.norm(d)
    g = (np.arange(48) + 0.5) / 48 * 2.1 - 1.05
    ox, oy = np.meshgrid(g, g)
    o = np.stack([ox.reshape(-1), oy.reshape(-1), np.full(ox.size, 3.0)], axis=1)
    hit, prim, a, b, pts = colors_ref.brute_force_hits(t12, o, d)
    assert t12.shape[0] == 1280 and prim.size >= 1200
    colors = (v.astype(np.float64) @ AFFINE_A.T + AFFINE_B).astype(f32)
    assert colors.min() > 0
    got = rt.hit_colors(t12, order, f, colors, records(prim, a, b))
    want = pts @ AFFINE_A.T + AFFINE_B                                           # the yardstick: the field itself, in float64
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"largest absolute error against the affine field: {err:.3e} over {prim.size} hits")
    assert err <= 4 * AFFINE_MEASURED, err
