"""rt_vertex_normals and rt_hit_normals, the host definitions of the dynamic mesh's smooth normals, and rt_debug_normal_pack, the packed
vertex -> triangle adjacency the device reads, without a GPU: against their float32 numpy restatement (tests/normals_ref.py) bit for bit, their
refusals, the exports, a null context to every new entry, the flat anchor (a flat region shades with exactly the face normal's bits) and their meaning
against an analytic sphere."""
import ctypes as C
import functools

import numpy as np
import pytest

import normals_ref
import opengl_raytracing_amd as rt

f32 = np.float32
IDENT = np.eye(4, dtype=f32).reshape(-1)
INT_MAX = 2 ** 31 - 1
NEW_SYMBOLS = ("rt_mesh_normals_enable", "rt_mesh_vertex_normals", "rt_mesh_hit_normals", "rt_mesh_hit_normals_host", "rt_vertex_normals", "rt_hit_normals",
               "rt_debug_normal_pack")
FP, U32P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def records(prim, u, v):
    rec = np.zeros((len(prim), 4), f32)
    rec[:, 0], rec[:, 2], rec[:, 3] = 1.0, u, v
    rec[:, 1] = np.asarray(prim, np.int32).view(f32)
    return rec


def _turn(k):
    a = 0.7 * k
    c, s = np.cos(a), np.sin(a)
    M = np.eye(4)
    M[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]]) @ np.diag([1.0 + 0.2 * k, 1.0, 0.8])
    M[:3, 3] = [0.3 * k, -0.2, 0.1 * k]
    return np.ascontiguousarray(M.T, f32).reshape(-1)


def _strip(nv, seed):
    """A triangle strip over nv random vertices: nv - 2 triangles, every vertex used."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (nv, 3)).astype(f32)
    f = np.stack([np.arange(nv - 2), np.arange(1, nv - 1), np.arange(2, nv)], axis=1)
    return v, f.astype(np.uint32).reshape(-1)


def _fan(valence=200):
    """A fan of `valence` triangles about vertex 0, every rim triangle with two vertices of its own (valence 1), one of them raised."""
    rng = np.random.default_rng(valence)
    a = np.linspace(0, 2 * np.pi, 2 * valence, endpoint=False)
    rim = np.stack([np.cos(a), 0.2 * rng.normal(0, 1, a.size), np.sin(a)], axis=1)
    v = np.concatenate([[[0.0, 0.5, 0.0]], rim]).astype(f32)
    k = np.arange(valence)
    f = np.stack([np.zeros(valence, np.int64), 1 + 2 * k + 1, 1 + 2 * k], axis=1)
    return v, f.astype(np.uint32).reshape(-1)


def _soup(n, seed=1):
    rng = np.random.default_rng(seed + n)
    nv = max(3, n // 2 + 3)
    return rng.normal(0, 1, (nv, 3)).astype(f32), rng.integers(0, nv, (n, 3)).astype(np.uint32).reshape(-1)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (tris12 [T,12], order [T], indices [3T], n_verts), read only.  The rows and their order are the host builder's."""
    part_first = None
    if name == "1 triangle":
        v, f = np.array([[0, 0, 0], [1, 0, 0.5], [0.2, 1, 0]], f32), np.array([0, 1, 2], np.uint32)
    elif name == "2 triangles":
        v, f = np.array([[0, 0, 0], [1, 0, 0.5], [0.2, 1, 0], [1.1, 0.9, -0.7]], f32), np.array([0, 1, 2, 2, 1, 3], np.uint32)
    elif name in ("63 vertices", "64 vertices", "65 vertices"):
        v, f = _strip(int(name.split()[0]), 7)
    elif name == "fan":
        v, f = _fan()
    elif name == "isolated vertex":
        v, f = _strip(9, 3)
        v = np.concatenate([v[:4], [[5, 5, 5]], v[4:]]).astype(f32)            # vertex 4 is named by nobody
        f = np.where(f >= 4, f + 1, f).astype(np.uint32)
    elif name == "vertex named twice":
        v, f = _strip(7, 4)
        f = np.concatenate([f, [2, 2, 5], [6, 0, 6]]).astype(np.uint32)        # degenerate rows: a zero face vector, counted twice
    elif name == "opposite pair":
        v = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1], [3, 0, 0], [4, 0, 0], [3, 1, 0]], f32)
        f = np.array([0, 1, 2, 0, 2, 1, 3, 4, 5], np.uint32)                   # vertices 0 - 2: two windings of one triangle, the sums are zero
    elif name == "1000 triangles":
        v, f = _soup(1000)
    elif name == "3 parts":
        v, f = _soup(300)
        part_first = [0, 100, 220, 300]
    else:
        raise KeyError(name)
    if part_first is None:
        t9 = rt.gather_triangles(v, f, _turn(1) if name == "1000 triangles" else IDENT)
    else:
        t9 = rt.gather_triangles_parts(v, f, part_first, np.stack([_turn(1), _turn(2), _turn(-1)]))
    _, t12, order = rt.build_bvh_order(t9)
    order = np.ascontiguousarray(order, np.int32)
    for a in (t12, order, f):
        a.setflags(write=False)
    return t12, order, f, v.shape[0]


CASES = ("1 triangle", "2 triangles", "63 vertices", "64 vertices", "65 vertices", "fan", "isolated vertex", "vertex named twice", "opposite pair",
         "1000 triangles", "3 parts")


def _hits(n_tris, n, seed):
    rng = np.random.default_rng(seed)
    prim = rng.integers(0, n_tris, n).astype(np.int32)
    prim[:min(n, n_tris)] = np.arange(min(n, n_tris))                           # every row at least once where there is room
    a = rng.uniform(0, 1, n).astype(f32)
    b = (rng.uniform(0, 1, n) * (1 - a)).astype(f32)
    a[::11], b[::13] = 0, 0                                                     # corners and edges
    return records(prim, a, b)


@pytest.mark.parametrize("name", CASES)
def test_equals_the_numpy_definition(name):
    t12, order, f, nv = _case(name)
    n = t12.shape[0]
    got = rt.vertex_normals(t12, order, f, nv)
    want = normals_ref.vertex_normals(t12, order, f, nv)
    assert (bits(got) == bits(want)).all(), int((bits(got) != bits(want)).any(axis=1).sum())
    rec = _hits(n, max(257, 2 * n), 5)
    hn = rt.hit_normals(t12, order, f, got, rec)
    assert (bits(hn) == bits(normals_ref.hit_normals(t12, order, f, got, rec))).all()
    four = np.concatenate([got, np.full((nv, 1), 9, f32)], axis=1)             # the device layout: the fourth float is not a normal's
    assert (bits(rt.hit_normals(t12, order, f, four, rec)) == bits(hn)).all()
    face = normals_ref.face_normals(t12)[normals_ref.prims(rec)]
    if name == "fan":
        count = np.bincount(f, minlength=nv)
        assert count[0] == 200 and (count[1:] == 1).all()
        assert (bits(hn) != bits(face)).any(axis=1).sum() >= 200                # the pole's normal is not any face's
    if name == "isolated vertex":
        assert (bits(got[4]) == 0).all() and (bits(np.delete(got, 4, axis=0)) != 0).any(axis=1).all()
    if name == "opposite pair":
        assert (bits(got[:3]) == 0).all()                                       # the sums are zero: three +0 ...
        on_pair = np.isin(order[normals_ref.prims(rec)], (0, 1))
        assert on_pair.any() and (bits(hn[on_pair]) == bits(face[on_pair])).all()   # ... and the hit falls back to the face normal
        assert (bits(hn[~on_pair]) == bits(face[~on_pair])).all()               # a triangle of its own: bit-equal corners hand the normal back
    if name in ("1 triangle",):
        assert (bits(hn) == bits(face)).all()
    if name in ("1000 triangles", "3 parts"):
        assert not np.array_equal(order, np.arange(n))                          # the rows are not in input order: the order array matters
        unit = np.linalg.norm(got.astype(np.float64), axis=1)
        assert np.abs(unit[unit > 0] - 1).max() < 1e-6


def test_hit_records_off_the_triangle_and_off_the_mesh():
    t12, order, f, nv = _case("1000 triangles")
    n = t12.shape[0]
    normals = rt.vertex_normals(t12, order, f, nv)
    rec = _hits(n, 64, 9)
    rec[0:4, 2] = [np.nan, np.inf, -np.inf, 0.25]                               # NaN and infinite barycentrics: the face normal
    rec[2:6, 3] = [0.5, np.nan, np.inf, -np.inf]
    bad = np.array([-1, n, INT_MAX, -INT_MAX - 1], np.int32)
    rec[8:12, 1] = bad.view(f32)
    got = rt.hit_normals(t12, order, f, normals, rec)
    assert (bits(got) == bits(normals_ref.hit_normals(t12, order, f, normals, rec))).all()
    face = normals_ref.face_normals(t12)[normals_ref.prims(rec)[:6]]
    assert (bits(got[:6]) == bits(face)).all()
    assert (bits(got[8:12]) == 0).all() and (bits(got[12:]) != 0).any(axis=1).all()
    # nothing is read out of bounds: the same call on exactly-sized copies, the last row's and the last vertex's hits included
    rec[12, 1] = np.array([n - 1], np.int32).view(f32)[0]
    again = rt.hit_normals(t12.copy(), order.copy(), f.copy(), normals.copy(), rec.copy())
    assert (bits(again) == bits(normals_ref.hit_normals(t12, order, f, normals, rec))).all()


# ---------------------------------------------------------------- the packed adjacency
def _info_dict(i):
    return {k: getattr(i, k) for k, _ in rt.RtNormalInfo._fields_}


@pytest.mark.parametrize("nv", [1, 3, 63, 64, 65, 127, 128, 129, 200])
def test_pack_equals_the_numpy_packer(nv):
    rng = np.random.default_rng(nv)
    f = rng.integers(0, nv, 3 * max(1, 2 * nv)).astype(np.uint32)
    f[:6] = nv - 1                                                              # the last vertex, in the last lane of its slice: two triangles, all three corners
    got, want = rt.debug_normal_pack(f, nv), normals_ref.pack(f, nv)
    assert _info_dict(got["info"]) == want["info"]
    assert got["slice_first"].tobytes() == want["slice_first"].tobytes() and got["entries"].tobytes() == want["entries"].tobytes()
    assert got["entries"].size == got["slice_first"][-1] and (got["entries"] == rt.NORMAL_PAD_ENTRY).sum() == got["entries"].size - f.size
    assert C.sizeof(rt.RtNormalInfo) == 40


def test_pack_one_high_valence_vertex_widens_its_own_slice():
    _, _, f, nv = _case("fan")
    got, want = rt.debug_normal_pack(f, nv), normals_ref.pack(f, nv)
    assert got["slice_first"].tobytes() == want["slice_first"].tobytes() and got["entries"].tobytes() == want["entries"].tobytes()
    width = np.diff(got["slice_first"].astype(np.int64)) // 64
    assert width[0] == 200 and (width[1:] == 1).all() and got["info"].maxPerVertex == 200
    lane0 = got["entries"][:200 * 64:64]
    assert (lane0 == np.arange(200)).all()                                      # the pole's incidences, k ascending


def _pack_raw(f, n_idx, nv, which, dst, cap, size):
    return rt.lib().rt_debug_normal_pack(None if f is None else f.ctypes.data_as(U32P), n_idx, nv, which, dst, cap, size)


def test_pack_refusals():
    f = np.array([0, 1, 2, 2, 1, 3], np.uint32)
    size = C.c_size_t(7)
    for which, want in ((rt.RT_NORMAL_ARRAY_SLICE_FIRST, 8), (rt.RT_NORMAL_ARRAY_ENTRIES, 2 * 64 * 4), (rt.RT_NORMAL_ARRAY_INFO, 40)):
        assert _pack_raw(f, 6, 4, which, None, 0, C.byref(size)) == rt.RT_OK and size.value == want             # dst == NULL asks for the size
        buf = np.zeros(want, np.uint8)
        assert _pack_raw(f, 6, 4, which, C.c_void_p(buf.ctypes.data), want - 1, C.byref(size)) == rt.RT_ERR_INVALID
        assert _pack_raw(f, 6, 4, which, C.c_void_p(buf.ctypes.data), want, C.byref(size)) == rt.RT_OK and size.value == want
    assert _pack_raw(f, 6, 4, 2, None, 0, C.byref(size)) == rt.RT_ERR_INVALID and size.value == 0                # an unknown array
    assert _pack_raw(f, 6, 4, rt.RT_NORMAL_ARRAY_INFO, None, 0, None) == rt.RT_ERR_INVALID
    for args in ((None, 6, 4), (f, 0, 4), (f, 5, 4), (f, -3, 4), (f, 6, 0), (f, 6, -1), (f, 6, 3)):             # the last: index 3 of 3 vertices
        assert _pack_raw(*args, rt.RT_NORMAL_ARRAY_INFO, None, 0, C.byref(size)) == rt.RT_ERR_INVALID, args[1:]
    with pytest.raises(rt.RtError) as e:
        rt.debug_normal_pack(f, 3)
    assert e.value.code == rt.RT_ERR_INVALID


def test_pack_refuses_two_to_the_31_entries():
    """One vertex named 2^25 + 1 times sets the width of its slice of 64: 2^31 + 64 padded entries."""
    n_idx = 2 ** 25 + 1
    assert n_idx % 3 == 0
    f = np.zeros(n_idx, np.uint32)
    size = C.c_size_t()
    assert _pack_raw(f, n_idx, 1, rt.RT_NORMAL_ARRAY_INFO, None, 0, C.byref(size)) == rt.RT_ERR_UNSUPPORTED
    assert _pack_raw(f, n_idx - 3, 1, rt.RT_NORMAL_ARRAY_INFO, None, 0, C.byref(size)) == rt.RT_OK               # (2^25 - 2) * 64 < 2^31


# ---------------------------------------------------------------- refusals, exports, a null context
def _vn_raw(t12, order, n_tris, f, nv, out):
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)      # noqa: E731
    return rt.lib().rt_vertex_normals(p(t12, FP), p(order, I32P), n_tris, p(f, U32P), nv, p(out, FP))


def _hn_raw(t12, order, n_tris, f, normals, nv, rec, n, out):
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)      # noqa: E731
    return rt.lib().rt_hit_normals(p(t12, FP), p(order, I32P), n_tris, p(f, U32P), p(normals, FP), nv, None if rec is None else C.c_void_p(rec.ctypes.data), n,
                                   p(out, FP))


def test_refusals():
    t12, order, f, nv = (np.array(a) if isinstance(a, np.ndarray) else a for a in _case("65 vertices"))
    n = t12.shape[0]
    out = np.zeros((nv, 3), f32)
    assert _vn_raw(t12, order, n, f, nv, out) == rt.RT_OK
    for args in ((None, order, n, f, nv, out), (t12, None, n, f, nv, out), (t12, order, n, None, nv, out), (t12, order, n, f, nv, None),
                 (t12, order, 0, f, nv, out), (t12, order, -1, f, nv, out), (t12, order, n, f, 0, out), (t12, order, n, f, nv - 1, out)):
        assert _vn_raw(*args) == rt.RT_ERR_INVALID
    for bad in (-1, n, INT_MAX):
        o2 = order.copy()
        o2[3] = bad
        assert _vn_raw(t12, o2, n, f, nv, out) == rt.RT_ERR_INVALID                # an order entry outside the triangles
    normals = rt.vertex_normals(t12, order, f, nv)
    rec = _hits(n, 9, 2)
    hn = np.zeros((9, 3), f32)
    assert _hn_raw(t12, order, n, f, normals, nv, rec, 9, hn) == rt.RT_OK
    assert _hn_raw(t12, order, n, f, normals, nv, rec, 0, hn) == rt.RT_OK          # no hits: nothing to do
    assert _hn_raw(t12, order, n, f, normals, nv, None, 0, None) == rt.RT_OK
    for args in ((None, order, n, f, normals, nv, rec, 9, hn), (t12, None, n, f, normals, nv, rec, 9, hn), (t12, order, n, None, normals, nv, rec, 9, hn),
                 (t12, order, n, f, None, nv, rec, 9, hn), (t12, order, n, f, normals, nv, None, 9, hn), (t12, order, n, f, normals, nv, rec, 9, None),
                 (t12, order, 0, f, normals, nv, rec, 9, hn), (t12, order, n, f, normals, 0, rec, 9, hn), (t12, order, n, f, normals, nv, rec, -1, hn)):
        assert _hn_raw(*args) == rt.RT_ERR_INVALID
    o2 = order.copy()
    o2[normals_ref.prims(rec)[0]] = n
    assert _hn_raw(t12, o2, n, f, normals, nv, rec, 9, hn) == rt.RT_ERR_INVALID   # the order entry of a hit row outside the triangles
    assert _hn_raw(t12, order, n, f, normals, 1, rec, 9, hn) == rt.RT_ERR_INVALID        # ... and a corner outside the normals (every triangle of the strip has one)
    for call in (lambda: rt.vertex_normals(t12, order[:-1], f, nv), lambda: rt.vertex_normals(t12, order, f[:-3], nv),
                 lambda: rt.hit_normals(t12, order, f, normals, rec[:, :3]), lambda: rt.hit_normals(t12, order, f, normals[:, :2], rec),
                 lambda: rt.hit_normals(t12, order, f, normals, rec.astype(np.float64))):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt.RT_ERR_INVALID


def test_symbols_are_exported_and_declared():
    L = rt.lib()
    for name in NEW_SYMBOLS:
        assert name in rt.SIGNATURES, name
        assert getattr(L, name) is not None, name
    assert rt.RT_SCENE_ARRAY_NORMAL_ROWS == 14 and rt.SCENE_ARRAYS_MESH["normal rows"] == 14
    for method in ("mesh_normals_enable", "mesh_vertex_normals", "mesh_normal_rows", "mesh_hit_normals"):
        assert callable(getattr(rt.Renderer, method)), method
    for fn in ("vertex_normals", "hit_normals", "debug_normal_pack"):
        assert callable(getattr(rt, fn)), fn


def test_null_context():
    L = rt.lib()
    rec, out = np.zeros((4, 4), f32), np.zeros((4, 3), f32)
    ptr, size = C.c_void_p(), C.c_size_t(1)
    calls = {
        "rt_mesh_normals_enable": lambda: L.rt_mesh_normals_enable(None, 1),
        "rt_mesh_vertex_normals": lambda: L.rt_mesh_vertex_normals(None, C.byref(ptr), C.byref(size)),
        "rt_mesh_hit_normals": lambda: L.rt_mesh_hit_normals(None, C.c_void_p(rec.ctypes.data), 4, C.c_void_p(out.ctypes.data)),
        "rt_mesh_hit_normals_host": lambda: L.rt_mesh_hit_normals_host(None, C.c_void_p(rec.ctypes.data), 4, C.c_void_p(out.ctypes.data)),
    }
    assert set(calls) == set(NEW_SYMBOLS) - {"rt_vertex_normals", "rt_hit_normals", "rt_debug_normal_pack"}
    for name, call in calls.items():
        assert call() == rt.RT_ERR_INVALID, name
    assert L.rt_debug_read_scene(None, rt.RT_SCENE_ARRAY_NORMAL_ROWS, None, 0, C.byref(size)) == rt.RT_ERR_INVALID


# ---------------------------------------------------------------- the flat anchor
def flat_grid(nx=5, nz=4):
    """Unit right triangles in the plane y = 0, two per cell: (v0, v0 + z, v0 + x) and its mirror image from the opposite corner, so that every row has
    e1 = (0, 0, +-1), e2 = (+-1, 0, 0) and cross(e1, e2) = (+0, 1, +0) exactly.  -> (positions [V,3], indices)."""
    x, z = np.meshgrid(np.arange(nx + 1), np.arange(nz + 1), indexing="ij")
    v = np.stack([x, np.zeros_like(x), z], axis=-1).reshape(-1, 3).astype(f32)
    at = lambda i, j: i * (nz + 1) + j      # noqa: E731
    f = []
    for i in range(nx):
        for j in range(nz):
            f += [at(i, j), at(i, j + 1), at(i + 1, j), at(i + 1, j + 1), at(i + 1, j), at(i, j + 1)]
    return v, np.array(f, np.uint32)


def test_k_times_its_reciprocal_root_is_one():
    k = np.arange(1, 13).astype(f32)
    with np.errstate(all="ignore"):
        assert ((k * (f32(1.0) / np.sqrt((k * k).astype(f32)).astype(f32)).astype(f32)).astype(f32) == 1).all()


def test_flat_anchor():
    v, f = flat_grid()
    shift = np.array([-2, 0, 3], f32)                                            # small integers: the edges stay exact
    M = np.eye(4, dtype=f32)
    M[3, :3] = shift
    t9 = rt.gather_triangles(v, f, M.reshape(-1))
    _, t12, order = rt.build_bvh_order(t9)
    n, nv = t12.shape[0], v.shape[0]
    up = np.array([0.0, 1.0, 0.0], f32)
    assert (np.abs(t12[:, 4:7]) == [0, 0, 1]).all() and (np.abs(t12[:, 8:11]) == [1, 0, 0]).all()
    assert (bits(normals_ref.face_normals(t12)) == bits(np.tile(up, (n, 1)))).all()
    normals = rt.vertex_normals(t12, order, f, nv)
    assert np.bincount(f, minlength=nv).max() == 6
    assert (bits(normals) == bits(np.tile(up, (nv, 1)))).all()                   # (+0, 1, +0) at every vertex, whatever its valence
    rec = _hits(n, 600, 4)
    rec[::7, 2] = np.nan
    got = rt.hit_normals(t12, order, f, normals, rec)
    assert (bits(got) == bits(normals_ref.face_normals(t12)[normals_ref.prims(rec)])).all()
    assert (bits(got) == bits(np.tile(up, (600, 1)))).all()


# ---------------------------------------------------------------- the meaning: against the analytic sphere
# Largest angle, in radians, between the normal at a hit on the 1 280-triangle icosphere of radius 1 and the analytic normal (p - c) / |p - c| of the
# sphere at the hit point, over the hits of the grid of rays below, measured on the CPU:
#   smooth (rt_hit_normals) 0.011706      face (normalize(cross(e1, e2))) 0.087860      over 1 403 hits
# The test asserts the smooth figure at twice its measured value -- the margin covers the rays' placement -- and below a third of the face figure.
SMOOTH_MEASURED = 0.011706


def sphere_hits():
    """Hits of a 48 x 48 grid of parallel rays on the icosphere, brute force in float64 -> (tris12, order, indices, n_verts, records, points)."""
    v, f = rt.meshgen.icosphere(3)
    v = np.ascontiguousarray(v, f32)
    t9 = rt.gather_triangles(v, f, IDENT)
    _, t12, order = rt.build_bvh_order(t9)
    d = np.array([0.13, -0.07, -1.0])
    d /= np.linalg.norm(d)
    g = (np.arange(48) + 0.5) / 48 * 2.1 - 1.05
    ox, oy = np.meshgrid(g, g)
    o = np.stack([ox.reshape(-1), oy.reshape(-1), np.full(ox.size, 3.0)], axis=1) - 0.0 * d
    T = t12.astype(np.float64)
    v0, e1, e2 = T[:, 0:3], T[:, 4:7], T[:, 8:11]
    pvec = np.cross(d, e2)                                                       # [T,3]
    det = (e1 * pvec).sum(axis=1)
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        tvec = o[:, None, :] - v0[None, :, :]                                    # [R,T,3]
        a = (tvec * pvec[None]).sum(axis=2) * inv
        qvec = np.cross(tvec, e1[None])
        b = (qvec * d).sum(axis=2) * inv
        t = (qvec * e2[None]).sum(axis=2) * inv
    ok = (a >= 0) & (b >= 0) & (a + b <= 1) & (t > 0) & np.isfinite(t)
    t = np.where(ok, t, np.inf)
    prim = t.argmin(axis=1)
    r = np.arange(o.shape[0])
    hit = np.isfinite(t[r, prim])
    rec = records(prim[hit], a[r, prim][hit], b[r, prim][hit])
    pts = o[hit] + d * t[r, prim][hit, None]
    return t12, order, f, v.shape[0], rec, pts


def _angles(n, ref):
    n = n.astype(np.float64)
    c = (n * ref).sum(axis=1) / np.linalg.norm(n, axis=1)
    return np.arccos(np.clip(c, -1, 1))


def test_smooth_normals_against_the_analytic_sphere():
    t12, order, f, nv, rec, pts = sphere_hits()
    assert t12.shape[0] == 1280 and rec.shape[0] >= 1200
    ref = pts / np.linalg.norm(pts, axis=1, keepdims=True)
    normals = rt.vertex_normals(t12, order, f, nv)
    smooth = _angles(rt.hit_normals(t12, order, f, normals, rec), ref).max()
    face = _angles(normals_ref.face_normals(t12)[normals_ref.prims(rec)], ref).max()
    print(f"largest angle to the analytic normal: smooth {smooth:.6f} rad, face {face:.6f} rad, over {rec.shape[0]} hits")
    assert smooth <= 2 * SMOOTH_MEASURED, (smooth, face)
    assert smooth < face / 3, (smooth, face)
