"""rt_uv_rows, rt_hit_uvs, rt_sample_texture, rt_srgb_table and rt_load_obj_uv, the host definitions of the dynamic mesh's UVs and albedo texture
(DESIGN.md 14.15), without a GPU: against their float32 numpy restatement (tests/uvs_ref.py) bit for bit, hit records off the triangle and off the
mesh, every texture size and flag combination on a UV grid with its edge cases, the flat rule (a texture of one value samples as that value), the sRGB
table against the double formula, small .obj texts, their refusals, the exports, a null context to every new entry, and their meaning: a linear ramp
sampled at interpolated UVs reproduces the ramp at the float64 hit point on the icosphere."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import colors_ref
import opengl_raytracing_amd as rt
import uvs_ref
from colors_ref import bits, records
from test_mesh_colors_host import _hits, _soup, _strip

f32 = np.float32
IDENT = np.eye(4, dtype=f32).reshape(-1)
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
MESH_SYMBOLS = ("rt_mesh_uvs_enable", "rt_mesh_uvs", "rt_mesh_set_uvs", "rt_mesh_uvs_refresh", "rt_mesh_texture_upload", "rt_mesh_texture", "rt_mesh_hit_uvs",
                "rt_mesh_hit_uvs_host", "rt_mesh_hit_texels", "rt_mesh_hit_texels_host")
HOST_SYMBOLS = ("rt_uv_rows", "rt_hit_uvs", "rt_srgb_table", "rt_sample_texture", "rt_load_obj_uv")
FP, U32P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
CASES = ("1 triangle", "2 triangles", "63 vertices", "64 vertices", "65 vertices", "1000 triangles")
SIZES = ((1, 1), (2, 2), (3, 5), (1, 7), (64, 64))   # (W, H)
FLAGS = tuple(range(8))


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (order [T], indices [3T], uvs [V,2]), read only."""
    rng = np.random.default_rng(len(name) + 40)
    if name == "1 triangle":
        v, f = np.array([[0, 0, 0], [1, 0, 0.5], [0.2, 1, 0]], f32), np.array([0, 1, 2], np.uint32)
    elif name == "2 triangles":
        v, f = np.array([[0, 0, 0], [1, 0, 0.5], [0.2, 1, 0], [1.1, 0.9, -0.7]], f32), np.array([0, 1, 2, 2, 1, 3], np.uint32)   # share the edge 1 - 2
    elif name in ("63 vertices", "64 vertices", "65 vertices"):
        v, f = _strip(int(name.split()[0]), 7)
    elif name == "1000 triangles":
        v, f = _soup(1000)
    else:
        raise KeyError(name)
    n, nv = f.size // 3, v.shape[0]
    if name == "1000 triangles":
        order = rng.permutation(n).astype(np.int32)                              # a shuffled order: the order array matters
    else:
        _, _, order = rt.build_bvh_order(rt.gather_triangles(v, f, IDENT))
        order = np.ascontiguousarray(order, np.int32)
    uvs = rng.uniform(-1.5, 2.5, (nv, 2)).astype(f32)
    for a in (order, f, uvs):
        a.setflags(write=False)
    return order, f, uvs


@functools.lru_cache(maxsize=None)
def _tables():
    unorm, srgb = rt.texel_unorm8(), rt.srgb_table()
    unorm.setflags(write=False)
    srgb.setflags(write=False)
    return unorm, srgb


def _table(flags):
    return _tables()[1 if flags & rt.TEX_SRGB else 0]


@functools.lru_cache(maxsize=None)
def _texture(w, h):
    t = np.random.default_rng(100 * w + h).integers(0, 256, (h, w, 4)).astype(np.uint8)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _uv_grid():
    """Every pair of the special coordinates, and a random cloud around [-1, 2]^2."""
    special = np.array([0, 1, np.nextafter(f32(0), f32(-1)), -0.25, 3.75, 1e9, -1e9, np.nan, np.inf, -np.inf, 0.5, 0.999999, 1e-7, 0.25, 1 / 3], f32)
    pairs = np.array(list(itertools.product(special, special)), f32)
    cloud = np.random.default_rng(3).uniform(-1, 2, (600, 2)).astype(f32)
    g = np.concatenate([pairs, cloud])
    g.setflags(write=False)
    return g


@pytest.mark.parametrize("name", CASES)
def test_rows_and_hit_uvs_equal_the_numpy_definition(name):
    order, f, uvs = _case(name)
    n = order.size
    rows = rt.uv_rows(order, f, uvs)
    assert rows.shape == (n, 8) and (bits(rows) == bits(uvs_ref.uv_rows(order, f, uvs))).all()
    assert (bits(rows[:, 6:]) == 0).all()
    rec = _hits(n, max(257, 2 * n), 5)
    got = rt.hit_uvs(order, f, uvs, rec)
    want = uvs_ref.hit_uvs(order, f, uvs, rec)
    assert got.shape == (rec.shape[0], 2) and (bits(got) == bits(want)).all(), int((bits(got) != bits(want)).any(axis=1).sum())
    if name == "1000 triangles":
        assert not np.array_equal(order, np.arange(n))


def test_hit_records_off_the_triangle_and_off_the_mesh():
    order, f, uvs = _case("1000 triangles")
    n = order.size
    rec = _hits(n, 64, 9)
    rec[0:4, 2] = [np.nan, np.inf, -np.inf, 0.25]                                # NaN and infinite barycentrics: the first corner
    rec[2:6, 3] = [0.5, np.nan, np.inf, -np.inf]
    rec[8:12, 1] = np.array([-1, n, INT_MAX, INT_MIN], np.int32).view(f32)
    got = rt.hit_uvs(order, f, uvs, rec)
    assert (bits(got) == bits(uvs_ref.hit_uvs(order, f, uvs, rec))).all()
    c0 = uvs[f.reshape(-1, 3)[order[colors_ref.prims(rec)[:6]], 0]]
    assert (bits(got[:6]) == bits(c0)).all()
    assert (bits(got[8:12]) == 0).all()
    # nothing is read out of bounds: the same call on exactly-sized copies, the last row's hit included
    rec[12, 1] = np.array([n - 1], np.int32).view(f32)[0]
    again = rt.hit_uvs(order.copy(), f.copy(), uvs.copy(), rec.copy())
    assert (bits(again) == bits(uvs_ref.hit_uvs(order, f, uvs, rec))).all()
    # three bit-equal corners: the value's bits at every (a, b)
    flat = np.tile(np.array([0.3, -0.7], f32), (uvs.shape[0], 1))
    assert (bits(rt.hit_uvs(order, f, flat, rec)[12:]) == bits(flat[:rec.shape[0] - 12])).all()


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_samples_equal_the_numpy_definition(size, flags):
    tex, uv = _texture(*size), _uv_grid()
    got = rt.sample_texture(tex, flags, uv)
    want = uvs_ref.sample_texture(tex, flags, uv, _table(flags))
    assert got.shape == (uv.shape[0], 3)
    assert (bits(got) == bits(want)).all(), (int((bits(got) != bits(want)).any(axis=1).sum()), uv[(bits(got) != bits(want)).any(axis=1)][:4])
    # alpha is stored and ignored
    other = tex.copy()
    other[:, :, 3] ^= 0xFF
    assert (bits(rt.sample_texture(other, flags, uv)) == bits(got)).all()


def test_nearest_and_texel_centres_name_the_texel():
    """Row 0 is v = 0, column 0 is u = 0: at a texel's centre every filter answers that texel's decoded value."""
    tex = _texture(3, 5)
    jj, ii = np.meshgrid(np.arange(5), np.arange(3), indexing="ij")
    uv = np.stack([(ii.reshape(-1) + 0.5) / 3, (jj.reshape(-1) + 0.5) / 5], axis=1).astype(f32)
    want = _tables()[0][tex[jj.reshape(-1), ii.reshape(-1), :3]]
    for flags in (rt.TEX_NEAREST, rt.TEX_NEAREST | rt.TEX_CLAMP):
        assert (bits(rt.sample_texture(tex, flags, uv)) == bits(want)).all()
    for flags in (rt.TEX_LINEAR, rt.TEX_CLAMP):
        assert np.abs(rt.sample_texture(tex, flags, uv) - want).max() < 1e-5


def test_flat_rule():
    """A texture of one value returns that decoded value bit for bit at every UV; an all-255 texture returns exactly 1.0f: the white anchor."""
    uv = _uv_grid()
    for (w, h), flags in itertools.product(SIZES, FLAGS):
        table = _table(flags)
        for code in ((255, 255, 255, 255), (255, 255, 255, 0), (7, 130, 201, 9)):
            tex = np.tile(np.array(code, np.uint8), (h, w, 1))
            got = rt.sample_texture(tex, flags, uv)
            assert (bits(got) == bits(np.tile(table[list(code[:3])], (uv.shape[0], 1)))).all(), (w, h, flags, code)
            if code[:3] == (255, 255, 255):
                assert (bits(got) == bits(f32(1.0))).all()
    # the rule is not vacuous: the four weights do not sum to 1 in float32 somewhere on the grid
    a = np.random.default_rng(4).uniform(0, 1, (4096, 2)).astype(f32)
    one = f32(1)
    w = [((one - a[:, 0]) * (one - a[:, 1])).astype(f32), (a[:, 0] * (one - a[:, 1])).astype(f32), ((one - a[:, 0]) * a[:, 1]).astype(f32), (a[:, 0] * a[:, 1]).astype(f32)]
    assert ((((w[0] + w[1]).astype(f32) + w[2]).astype(f32) + w[3]).astype(f32) != one).any()


def test_srgb_table():
    got, unorm = rt.srgb_table(), rt.texel_unorm8()
    want = uvs_ref.srgb_table_f64()
    w32 = want.astype(f32)
    ulp = np.spacing(np.maximum(np.abs(w32), np.finfo(f32).tiny))
    assert (np.abs(got.astype(np.float64) - want) <= ulp).all()                  # within 1 float32 ulp of the double formula
    assert (np.diff(got.astype(np.float64)) > 0).all()                           # strictly increasing
    assert bits(got[0]) == 0 and bits(got[255]) == bits(f32(1.0))                # exact ends
    assert (bits(unorm) == bits((np.arange(256, dtype=f32) / f32(255)).astype(f32))).all()   # the UNORM table is c / 255


# ---------------------------------------------------------------- rt_load_obj_uv
def _obj(tmp_path, text):
    p = tmp_path / "m.obj"
    p.write_text(text)
    return rt.load_obj_uv(p)


def test_load_obj_uv(tmp_path):
    # a position shared by two vt: two vertices; vertex k is the k-th distinct pair in order of first use
    pos, uv, idx = _obj(tmp_path, "v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nvt 0.5 0.5\nf 1/1 2/2 3/3\nf 2/4 4/2 3/3\n")
    assert idx.tolist() == [0, 1, 2, 3, 4, 2]
    assert pos.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [1, 1, 0]]
    assert uv.tolist() == [[0, 0], [1, 0], [0, 1], [0.5, 0.5], [1, 0]]
    # a quad: the fan of rt_load_obj; v/vt/vn and v/vt mix
    pos, uv, idx = _obj(tmp_path, "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 0 1\nf 1/1/1 2/2/1 3/3 4/4/1\n")
    assert idx.tolist() == [0, 1, 2, 0, 2, 3] and uv.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]]
    p2, i2 = rt.load_obj(tmp_path / "m.obj")
    assert (p2 == pos).all() and i2.tolist() == idx.tolist()                     # no seam: the same mesh as rt_load_obj's
    # negative indices, for v and for vt
    pos, uv, idx = _obj(tmp_path, "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0.25 0.5\nvt 0.75 0.5\nvt 0.5 1\nf -3/-3 -2/-2 -1/-1\n")
    assert idx.tolist() == [0, 1, 2] and uv.tolist() == [[0.25, 0.5], [0.75, 0.5], [0.5, 1]] and pos[1].tolist() == [1, 0, 0]
    # a face without vt: (0, 0), and it pairs as vt = none -- apart from the same position with a vt
    pos, uv, idx = _obj(tmp_path, "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0.5 0.5\nf 1 2 3\nf 1/1 2//1 3\n")
    assert idx.tolist() == [0, 1, 2, 3, 1, 2]
    assert uv.tolist() == [[0, 0], [0, 0], [0, 0], [0.5, 0.5]] and pos[3].tolist() == [0, 0, 0]
    # refusals: an index outside the records, a missing file
    for text in ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/2 2/1 3/1\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n"):
        with pytest.raises(rt.RtError):
            _obj(tmp_path, text)
    with pytest.raises(rt.RtError):
        rt.load_obj_uv(tmp_path / "absent.obj")


# ---------------------------------------------------------------- refusals, exports, a null context
def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _rows_raw(order, f, uvs, n, nv, out):
    return rt.lib().rt_uv_rows(_p(order, I32P), _p(f, U32P), _p(uvs, FP), n, nv, _p(out, FP))


def _hit_raw(rec, n, order, f, uvs, n_tris, nv, out):
    return rt.lib().rt_hit_uvs(None if rec is None else C.c_void_p(rec.ctypes.data), n, _p(order, I32P), _p(f, U32P), _p(uvs, FP), n_tris, nv, _p(out, FP))


def _sample_raw(tex, w, h, flags, uv, n, out):
    return rt.lib().rt_sample_texture(None if tex is None else C.c_void_p(tex.ctypes.data), w, h, flags, _p(uv, FP), n, _p(out, FP))


def test_refusals():
    order, f, uvs = (np.array(a) for a in _case("65 vertices"))
    n, nv = order.size, uvs.shape[0]
    rows = np.zeros((n, 8), f32)
    assert _rows_raw(order, f, uvs, n, nv, rows) == rt.RT_OK
    for args in ((None, f, uvs, n, nv, rows), (order, None, uvs, n, nv, rows), (order, f, None, n, nv, rows), (order, f, uvs, n, nv, None),
                 (order, f, uvs, 0, nv, rows), (order, f, uvs, -1, nv, rows), (order, f, uvs, n, 0, rows), (order, f, uvs, n, nv - 1, rows)):
        assert _rows_raw(*args) == rt.RT_ERR_INVALID                             # (nv - 1: a corner index outside the vertices is refused, not read)
    for bad in (-1, n, INT_MAX, INT_MIN):
        o2 = order.copy()
        o2[3] = bad
        assert _rows_raw(o2, f, uvs, n, nv, rows) == rt.RT_ERR_INVALID
    rec = _hits(n, 9, 2)
    out = np.zeros((9, 2), f32)
    assert _hit_raw(rec, 9, order, f, uvs, n, nv, out) == rt.RT_OK
    assert _hit_raw(rec, 0, order, f, uvs, n, nv, out) == rt.RT_OK
    assert _hit_raw(None, 0, order, f, uvs, n, nv, None) == rt.RT_OK
    for args in ((rec, 9, None, f, uvs, n, nv, out), (rec, 9, order, None, uvs, n, nv, out), (rec, 9, order, f, None, n, nv, out), (None, 9, order, f, uvs, n, nv, out),
                 (rec, 9, order, f, uvs, n, nv, None), (rec, 9, order, f, uvs, 0, nv, out), (rec, 9, order, f, uvs, n, 0, out), (rec, -1, order, f, uvs, n, nv, out)):
        assert _hit_raw(*args) == rt.RT_ERR_INVALID
    o2 = order.copy()
    o2[colors_ref.prims(rec)[0]] = n
    assert _hit_raw(rec, 9, o2, f, uvs, n, nv, out) == rt.RT_ERR_INVALID
    assert _hit_raw(rec, 9, order, f, uvs, n, 1, out) == rt.RT_ERR_INVALID
    tex, uv, o3 = np.array(_texture(3, 5)), np.zeros((4, 2), f32), np.zeros((4, 3), f32)
    assert _sample_raw(tex, 3, 5, 7, uv, 4, o3) == rt.RT_OK
    assert _sample_raw(tex, 3, 5, 0, uv, 0, o3) == rt.RT_OK and _sample_raw(tex, 3, 5, 0, None, 0, None) == rt.RT_OK
    for args in ((None, 3, 5, 0, uv, 4, o3), (tex, 3, 5, 0, None, 4, o3), (tex, 3, 5, 0, uv, 4, None), (tex, 0, 5, 0, uv, 4, o3), (tex, 3, 0, 0, uv, 4, o3),
                 (tex, -1, 5, 0, uv, 4, o3), (tex, rt.TEX_MAX_SIZE + 1, 1, 0, uv, 4, o3), (tex, 1, rt.TEX_MAX_SIZE + 1, 0, uv, 4, o3), (tex, 3, 5, 8, uv, 4, o3),
                 (tex, 3, 5, -1, uv, 4, o3), (tex, 3, 5, 0x100, uv, 4, o3), (tex, 3, 5, 0, uv, -1, o3)):
        assert _sample_raw(*args) == rt.RT_ERR_INVALID, args[1:4]
    assert rt.lib().rt_srgb_table(None) == rt.RT_ERR_INVALID
    assert rt.lib().rt_load_obj_uv(None, None, None, None, None, None) == rt.RT_ERR_INVALID
    for call in (lambda: rt.uv_rows(order, f[:-3], uvs), lambda: rt.hit_uvs(order[:-1], f, uvs, rec), lambda: rt.hit_uvs(order, f, uvs, rec[:, :3]),
                 lambda: rt.hit_uvs(order, f, np.zeros((nv, 3), f32), rec), lambda: rt.hit_uvs(order, f, uvs, rec.astype(np.float64)),
                 lambda: rt.sample_texture(tex[:, :, :3], 0, uv), lambda: rt.sample_texture(tex.astype(np.float32), 0, uv), lambda: rt.sample_texture(tex, 0, uv[:, :1]),
                 lambda: rt.sample_texture(tex, 8, uv)):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt.RT_ERR_INVALID


def test_symbols_are_exported_and_declared():
    L = rt.lib()
    for name in MESH_SYMBOLS + HOST_SYMBOLS:
        assert name in rt.SIGNATURES, name
        assert getattr(L, name) is not None, name
    assert rt.RT_SCENE_ARRAY_UV_ROWS == 16 and rt.SCENE_ARRAYS_MESH["uv rows"] == 16
    assert (rt.TEX_LINEAR, rt.TEX_NEAREST, rt.TEX_REPEAT, rt.TEX_CLAMP, rt.TEX_UNORM, rt.TEX_SRGB) == (0, 1, 0, 2, 0, 4) and rt.TEX_MAX_SIZE == 16384
    for method in ("mesh_uvs_enable", "mesh_uvs", "mesh_set_uvs", "mesh_uvs_refresh", "mesh_uv_rows", "mesh_texture_upload", "mesh_texture", "mesh_hit_uvs",
                   "mesh_hit_texels"):
        assert callable(getattr(rt.Renderer, method)), method
    for fn in ("uv_rows", "hit_uvs", "sample_texture", "srgb_table", "load_obj_uv"):
        assert callable(getattr(rt, fn)), fn


def test_null_context():
    L = rt.lib()
    rec, out, uv, tex = np.zeros((4, 4), f32), np.zeros((4, 3), f32), np.zeros((4, 2), f32), np.zeros((2, 2, 4), np.uint8)
    ptr, size, w, h = C.c_void_p(), C.c_size_t(1), C.c_int(1), C.c_int(1)
    hits, dst = C.c_void_p(rec.ctypes.data), C.c_void_p(out.ctypes.data)
    calls = {
        "rt_mesh_uvs_enable": lambda: L.rt_mesh_uvs_enable(None, 1),
        "rt_mesh_uvs": lambda: L.rt_mesh_uvs(None, C.byref(ptr), C.byref(size)),
        "rt_mesh_set_uvs": lambda: L.rt_mesh_set_uvs(None, uv.ctypes.data_as(FP), 0, 4),
        "rt_mesh_uvs_refresh": lambda: L.rt_mesh_uvs_refresh(None),
        "rt_mesh_texture_upload": lambda: L.rt_mesh_texture_upload(None, C.c_void_p(tex.ctypes.data), 2, 2, 0),
        "rt_mesh_texture": lambda: L.rt_mesh_texture(None, C.byref(ptr), C.byref(size), C.byref(w), C.byref(h)),
        "rt_mesh_hit_uvs": lambda: L.rt_mesh_hit_uvs(None, hits, 4, dst),
        "rt_mesh_hit_uvs_host": lambda: L.rt_mesh_hit_uvs_host(None, hits, 4, dst),
        "rt_mesh_hit_texels": lambda: L.rt_mesh_hit_texels(None, hits, 4, dst),
        "rt_mesh_hit_texels_host": lambda: L.rt_mesh_hit_texels_host(None, hits, 4, dst),
    }
    assert set(calls) == set(MESH_SYMBOLS)
    for name, call in calls.items():
        assert call() == rt.RT_ERR_INVALID, name
    assert L.rt_debug_read_scene(None, rt.RT_SCENE_ARRAY_UV_ROWS, None, 0, C.byref(size)) == rt.RT_ERR_INVALID


# ---------------------------------------------------------------- the meaning: a ramp texture under affine UVs
# A W = 64 texture whose texel i along u has code i (UNORM, CLAMP, LINEAR) is, between its first and last texel centres, the linear function
# (u W - 0.5) / 255 of u.  Every vertex of the 1 280-triangle icosphere gets a UV that is an affine function of its position and stays inside
# [0.5 / W, 1 - 0.5 / W]; the sample at the UV rt_hit_uvs gives at a hit is compared with (u64 W - 0.5) / 255 at the hit point, found by brute force
# in float64 for a 48 x 48 grid of parallel rays.  Largest absolute error over the hits and the three channels, measured on the CPU:
#   3.290e-08  over 1 403 hits
# The test asserts four times the measured value (the margin of DESIGN.md 14.14, for the same reasons: the rays' placement and the float32 hit point).
RAMP_MEASURED = 3.290e-08
RAMP_W = 64
RAMP_A = np.array([[0.40, 0.05, -0.06], [-0.07, 0.38, 0.08]])
RAMP_B = np.array([0.5, 0.5])


def test_a_ramp_texture_is_reproduced_on_the_icosphere():
    W = RAMP_W
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
    uvs = (v.astype(np.float64) @ RAMP_A.T + RAMP_B).astype(f32)
    assert uvs.min() >= 0.5 / W and uvs.max() <= 1 - 0.5 / W
    tex = np.zeros((2, W, 4), np.uint8)
    tex[:, :, :3] = np.arange(W, dtype=np.uint8)[None, :, None]
    got = rt.sample_texture(tex, rt.TEX_CLAMP, rt.hit_uvs(order, f, uvs, records(prim, a, b)))
    u64 = pts @ RAMP_A[0] + RAMP_B[0]                                            # the yardstick: the field itself, in float64
    want = (u64 * W - 0.5) / 255.0
    err = np.abs(got.astype(np.float64) - want[:, None]).max()
    print(f"largest absolute error against the ramp: {err:.3e} over {prim.size} hits")
    assert err <= 4 * RAMP_MEASURED, err
