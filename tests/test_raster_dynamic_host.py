"""The raster preview of the dynamic mesh without a GPU: the new symbols, what they refuse without a context, raster_prim_parts
against searchsorted, and the expansion helper tests/raster_dynamic_ref.py that the GPU tests (tests/test_gpu_raster_dynamic.py) hold the device to.
The soups, splits and matrices defined here are the ones the GPU tests use."""
import ctypes as C

import numpy as np
import pytest

import opengl_raytracing_amd as rt
import raster_dynamic_ref as rd
import raster_ref as rr

NEW_SYMBOLS = ("rt_raster_mesh_dynamic", "rt_raster_part_colors", "rt_raster_targets")
SPLITS = ("one", "singles", "uneven")


def split(name, n):
    """part_first for n triangles, as tests/test_mesh_parts_host.py defines the three splits.  one: a single part.  singles: every triangle its own
    part.  uneven: boundaries at 1, 8, 9, 255, 257 and 1000, clipped to n and deduplicated, with an empty part at the front, one in the middle and
    one at the end."""
    if name == "one":
        return np.array([0, n], np.int32)
    if name == "singles":
        return np.arange(n + 1, dtype=np.int32)
    assert name == "uneven"
    b = sorted({0, n} | {min(x, n) for x in (1, 8, 9, 255, 257, 1000)})
    mid = b[len(b) // 2]
    return np.array(sorted([0] + b + [mid] + [n]), np.int32)


def soup(n, seed=20261017):
    """n compact triangles: centres N(0, 2), corners N(0, 0.3) around the centre, triangle order shuffled; n == 1: one triangle spanning the view.
    -> (positions [3n,3] float32, indices [3n] uint32)"""
    if n == 1:
        return np.array([[-2, -1, 0], [2, -1, 0], [0, 2, 0]], np.float32), np.arange(3, dtype=np.uint32)
    rng = np.random.default_rng(seed + n)
    c = rng.normal(0, 2, (n, 1, 3))
    v = (c + rng.normal(0, 0.3, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    f = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)[rng.permutation(n)]
    return v, np.ascontiguousarray(f).reshape(-1)


def part_model(p):
    """A rotation times a non-uniform scale and a translation, distinct for every part, column-major: small enough that the soup stays in view."""
    M = np.eye(4)
    a = 0.37 * (p + 1)
    c, s = np.cos(a), np.sin(a)
    M[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([1.0 + 0.1 * (p % 7), 1.0 + 0.03 * (p % 3), 1.0 - 0.05 * (p % 11)])
    M[:3, 3] = [0.1 * (p % 13) - 0.6, 0.3 - 0.05 * (p % 17), -0.2 * (p % 5)]
    return np.ascontiguousarray(M.T, dtype=np.float32).reshape(-1)


def part_models(n_parts, shift=0):
    return np.stack([part_model(p + shift) for p in range(n_parts)]).astype(np.float32)


def part_colors(n_parts):
    """Distinct after the unorm8 packing for every part count the tests use (a 16 x 16 x 16 lattice), with values outside [0, 1] to clamp."""
    p = np.arange(n_parts)
    c = np.stack([(p % 16) / 15.0, ((p // 16) % 16) / 15.0, ((p // 256) % 16) / 15.0], 1)
    c[::7, 0] += 1.0     # clamps to 1
    c[3::11, 2] -= 2.0   # clamps to 0
    return c.astype(np.float32)


def test_symbols_are_exported_and_declared():
    L = rt.lib()
    for name in NEW_SYMBOLS:
        assert name in rt.SIGNATURES, name
        assert getattr(L, name) is not None, name
    assert (rt.RT_RASTER_BIND_SINGLE, rt.RT_RASTER_BIND_PARTS) == (0, 1)


def test_null_context():
    L = rt.lib()
    rgb = np.zeros((2, 3), np.float32)
    a, b, c, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert L.rt_raster_mesh_dynamic(None, 0, rt.RT_RASTER_BIND_SINGLE) == rt.RT_ERR_INVALID
    assert L.rt_raster_mesh_dynamic(None, 0, rt.RT_RASTER_BIND_PARTS) == rt.RT_ERR_INVALID
    assert L.rt_raster_part_colors(None, 0, rgb.ctypes.data_as(C.POINTER(C.c_float)), 2) == rt.RT_ERR_INVALID
    assert L.rt_raster_part_colors(None, 0, None, 0) == rt.RT_ERR_INVALID
    assert L.rt_raster_targets(None, C.byref(a), C.byref(b), C.byref(c), C.byref(n)) == rt.RT_ERR_INVALID
    assert L.rt_raster_targets(None, None, None, None, None) == rt.RT_ERR_INVALID


@pytest.mark.parametrize("name", SPLITS)
@pytest.mark.parametrize("n", [1, 9, 100, 1000])
def test_raster_prim_parts_is_searchsorted(n, name):
    pf = split(name, n)
    base = 7
    rng = np.random.default_rng(n)
    prim = np.concatenate([np.arange(0, base + n + 9), rng.integers(0, base + n + 9, 300), [rr.BACKGROUND, 0x7fffffff, base - 1, base, base + n - 1, base + n]])
    prim = prim.astype(np.uint32).reshape(2, -1) if prim.size % 2 == 0 else prim[:-1].astype(np.uint32).reshape(2, -1)
    part, tri = rt.raster_prim_parts(prim, base, pf)
    assert part.shape == prim.shape and tri.shape == prim.shape and part.dtype == np.int32 and tri.dtype == np.int32
    t = prim.astype(np.int64) - base
    inside = (prim != rr.BACKGROUND) & (t >= 0) & (t < n)
    want = np.searchsorted(pf, t, "right") - 1
    assert (part[~inside] == -1).all() and (tri[~inside] == -1).all() and (~inside).sum() >= base + 9
    assert np.array_equal(part[inside], want[inside]) and np.array_equal(tri[inside], (t - pf[np.clip(want, 0, pf.size - 2)])[inside])
    assert (np.diff(pf)[part[inside]] > 0).all()                         # never an empty part
    assert np.array_equal(pf[part[inside]] + tri[inside], t[inside])     # back to the caller's index buffer
    wp, wt = rd.prim_parts(prim, base, pf)
    assert np.array_equal(part, wp) and np.array_equal(tri, wt)
    # base 0 and a scalar
    p0, t0 = rt.raster_prim_parts(np.uint32(n - 1), 0, pf)
    assert int(p0) == int(np.searchsorted(pf, n - 1, "right") - 1) and int(t0) == n - 1 - int(pf[int(p0)])


def _camera(w, h):
    cam = rt.default_camera()
    cam.pos[0], cam.pos[1], cam.pos[2] = 0.0, 0.0, 6.0
    cam.yaw, cam.pitch, cam.fov, cam.aspect = -90.0, 0.0, 60.0, w / h
    return rt.camera_view(cam), rt.camera_proj(cam)


def test_expansion_of_the_uneven_split():
    """Primitive ids of the expanded list are base + input triangle; empty parts add no draw; the draws before and after keep their own ids."""
    W, H, n = 97, 61, 100
    v, f = soup(n)
    pf = split("uneven", n)
    k = pf.size - 1
    assert (np.diff(pf) == 0).sum() >= 3
    table = part_models(k)
    quad = (np.array([[-3, -2, -4], [3, -2, -4], [3, 2, -4], [-3, 2, -4]], np.float32), np.array([0, 1, 2, 0, 2, 3], np.uint32))
    model = rr.mat4_mul(np.eye(4, dtype=np.float32).reshape(-1), part_model(5))
    draws = [(0, np.eye(4, dtype=np.float32).reshape(-1), (0.2, 0.3, 0.4)), (1, model, (1.0, 0.5, 0.25)), (0, part_model(2), (0.9, 0.1, 0.1))]
    bound = {1: rd.Bound(parts=True, colors=part_colors(k))}
    meshes, out, bases = rd.expand({0: quad}, draws, bound, (v, f, pf, table))
    assert bases == [0, 2, 2 + n]
    assert len(out) == 2 + int((np.diff(pf) > 0).sum())                  # one draw per non-empty part
    at = 2
    for slot, m, color in out[1:-1]:
        p = slot[2]
        assert slot[:2] == ("dyn", 1) and pf[p + 1] > pf[p]
        assert np.array_equal(meshes[slot][1], f.reshape(-1, 3)[pf[p]:pf[p + 1]])
        assert np.array_equal(np.asarray(m, np.float32).view(np.uint32), rr.mat4_mul(model, table[p]).view(np.uint32))
        assert list(color) == list(part_colors(k)[p])
        assert at == 2 + pf[p]                                             # the part's first triangle is base + its first input triangle
        at += pf[p + 1] - pf[p]
    assert at == 2 + n
    view, proj = _camera(W, H)
    rgba, prim, depth, stats, bases = rd.render({0: quad}, draws, bound, (v, f, pf, table), view, proj, W, H)
    assert stats["in"] == n + 4
    # every visible pixel of the bound draw: the id names the input triangle, and the pixel has that triangle's part's colour
    part, tri = rd.prim_parts(prim, bases[1], pf)
    vis = part >= 0
    assert vis.sum() > 50 and len(set(part[vis].tolist())) >= 3
    packed = np.array([rr.pack_rgba(c) for c in part_colors(k)], np.uint32)
    assert np.array_equal(rgba.view(np.uint32)[..., 0][vis], packed[part[vis]])
    # and the frame is the one of the whole soup drawn triangle by triangle under its part's matrix (ids base + t by construction)
    singles = {("t", t): (v, f.reshape(-1, 3)[t:t + 1]) for t in range(n)}
    singles[0] = quad
    own = np.searchsorted(pf, np.arange(n), "right") - 1
    per_tri = [draws[0]] + [(("t", t), rr.mat4_mul(model, table[own[t]]), part_colors(k)[own[t]]) for t in range(n)] + [draws[2]]
    want = rr.render(singles, per_tri, view, proj, W, H)
    for g, e in zip((rgba, prim, depth), want):
        assert np.array_equal(g, e)


def test_expansion_single_mode_ignores_the_table():
    v, f = soup(9)
    pf = split("uneven", 9)
    draws = [(3, part_model(4), (0.5, 0.5, 0.5))]
    meshes, out, bases = rd.expand({}, draws, {3: rd.Bound(parts=False)}, (v, f, pf, None))
    assert bases == [0] and len(out) == 1 and np.array_equal(meshes[out[0][0]][1], f.reshape(-1, 3))
    assert np.array_equal(np.asarray(out[0][1]), part_model(4))
