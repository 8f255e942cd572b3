"""Parts of the dynamic mesh without a GPU: rt_gather_triangles_parts, the host definition the device's part-aware gather is held to
(tests/test_gpu_mesh_parts.py), equals the concatenation of per-part rt_gather_triangles_checked calls bit for bit; what it refuses; and the new
symbols.  The splits and matrices defined here are the ones the GPU tests use."""
import ctypes as C

import numpy as np
import pytest

import opengl_raytracing_amd as rt
from test_gpu_dynamic_mesh import _soup

NEW_SYMBOLS = ("rt_gather_triangles_parts", "rt_mesh_upload_parts", "rt_mesh_parts", "rt_mesh_part_matrices", "rt_mesh_set_part_matrices",
               "rt_mesh_rebuild_parts", "rt_mesh_refit_parts", "rt_mesh_hit_parts", "rt_mesh_hit_parts_host")
SPLITS = ("one", "singles", "uneven")


def split(name, n):
    """part_first for n triangles.  one: a single part.  singles: every triangle its own part.  uneven: boundaries at 1, 8, 9, 255, 257 and 1000 --
    inside 8-triangle leaves, inside 64-lane waves, across 256-thread blocks -- clipped to n and deduplicated, with an empty part at the front, one in
    the middle and one at the end."""
    if name == "one":
        return np.array([0, n], np.int32)
    if name == "singles":
        return np.arange(n + 1, dtype=np.int32)
    assert name == "uneven"
    b = sorted({0, n} | {min(x, n) for x in (1, 8, 9, 255, 257, 1000)})
    mid = b[len(b) // 2]
    return np.array(sorted([0] + b + [mid] + [n]), np.int32)


def splits_for(n):
    return [s for s in SPLITS if s != "singles" or n <= 100]


def part_model(p):
    """A rotation times a non-uniform scale and a translation, distinct for every part, column-major; part 0: the default BVH transform."""
    if p == 0:
        return np.ascontiguousarray(rt.default_bvh_transform(), np.float32).reshape(-1)
    M = np.eye(4)
    c, s = np.cos(0.37 * p), np.sin(0.37 * p)
    M[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([1.0 + 0.1 * (p % 7), 1.0 + 0.03 * (p % 3), 1.0 - 0.05 * (p % 11)])
    M[:3, 3] = [0.1 * (p % 13), 0.6 - 0.01 * (p % 17), -0.2 * (p % 5)]
    return np.ascontiguousarray(M.T, dtype=np.float32).reshape(-1)


def part_models(n_parts, shift=0):
    """[n_parts,16]; shift > 0: another set of distinct matrices (part 0 included)."""
    return np.stack([part_model(p + shift) for p in range(n_parts)]).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _per_part(v, f, pf, models):
    """The definition: one rt_gather_triangles_checked call per part, concatenated."""
    f = np.asarray(f).reshape(-1, 3)
    rows = [rt.gather_triangles(v, f[pf[p]:pf[p + 1]].reshape(-1), models[p]) for p in range(pf.size - 1) if pf[p + 1] > pf[p]]
    return np.concatenate(rows) if rows else np.zeros((0, 9), np.float32)


@pytest.mark.parametrize("name", SPLITS)
@pytest.mark.parametrize("n", [1, 9, 100])
def test_equals_the_concatenation_of_per_part_gathers(n, name):
    v, f = _soup(n)
    pf = split(name, n)
    assert pf[0] == 0 and pf[-1] == n and (np.diff(pf) >= 0).all()
    if name == "uneven":
        assert pf[1] == 0 and pf[-2] == n and (np.diff(pf) == 0).sum() >= 3      # the empty parts are there
    models = part_models(pf.size - 1)
    assert len({m.tobytes() for m in models}) == pf.size - 1                     # distinct matrices
    got = rt.gather_triangles_parts(v, f, pf, models)
    want = _per_part(v, f, pf, models)
    assert got.shape == (n, 9) and np.array_equal(_bits(got), _bits(want))
    if pf.size > 2 and n > 1:
        assert not np.array_equal(_bits(got), _bits(rt.gather_triangles(v, f, models[0])))      # the matrices do matter


@pytest.mark.parametrize("name", SPLITS)
@pytest.mark.parametrize("n", [1, 9, 100])
def test_null_matrices_are_identities(n, name):
    v, f = _soup(n)
    pf = split(name, n)
    ident = np.tile(np.eye(4, dtype=np.float32).reshape(-1), (pf.size - 1, 1))
    got = rt.gather_triangles_parts(v, f, pf, None)
    assert np.array_equal(_bits(got), _bits(rt.gather_triangles_parts(v, f, pf, ident)))
    assert np.array_equal(_bits(got), _bits(rt.gather_triangles(v, f, np.eye(4, dtype=np.float32).reshape(-1))))


def _raw(v, f, n_idx, pf, n_parts, n_verts=None):
    """rt_gather_triangles_parts as C sees it -> return code"""
    v = np.ascontiguousarray(v, np.float32)
    f = np.ascontiguousarray(f, np.uint32)
    pf = np.ascontiguousarray(pf, np.int32)
    out = np.zeros((max(f.size // 3, 1) + 1, 9), np.float32)
    return rt.lib().rt_gather_triangles_parts(v.ctypes.data_as(C.POINTER(C.c_float)), v.shape[0] if n_verts is None else n_verts,
                                              f.ctypes.data_as(C.POINTER(C.c_uint32)), n_idx, pf.ctypes.data_as(C.POINTER(C.c_int32)), n_parts, None,
                                              out.ctypes.data_as(C.POINTER(C.c_float)))


def test_refusals():
    n = 100
    v, f = _soup(n)
    pf = split("uneven", n)
    k = pf.size - 1
    assert _raw(v, f, f.size, pf, k) == n                                      # the good call returns the triangle count
    bad = pf.copy(); bad[0] = 1
    assert _raw(v, f, f.size, bad, k) == rt.RT_ERR_INVALID                     # partFirst[0] != 0
    bad = pf.copy(); bad[-1] = n - 1
    assert _raw(v, f, f.size, bad, k) == rt.RT_ERR_INVALID                     # a wrong last entry
    bad = pf.copy(); bad[-1] = n + 1
    assert _raw(v, f, f.size, bad, k) == rt.RT_ERR_INVALID
    bad = pf.copy(); bad[3], bad[4] = 9, 8
    assert _raw(v, f, f.size, bad, k) == rt.RT_ERR_INVALID                     # a decreasing entry
    assert _raw(v, f, f.size, pf, 0) == rt.RT_ERR_INVALID                      # nParts of 0 ...
    big = np.zeros(rt.RT_MAX_MESH_PARTS + 2, np.int32); big[-1] = n
    assert _raw(v, f, f.size, big, rt.RT_MAX_MESH_PARTS + 1) == rt.RT_ERR_INVALID      # ... and of RT_MAX_MESH_PARTS + 1
    assert _raw(v, f, f.size, big[1:], rt.RT_MAX_MESH_PARTS) == n              # the largest count is legal
    idx = f.copy(); idx[22] = v.shape[0]
    assert _raw(v, idx, f.size, pf, k) == rt.RT_ERR_INVALID                    # an index >= nVerts
    assert _raw(v, f, f.size - 1, pf, k) == rt.RT_ERR_INVALID                  # nIdx % 3 != 0
    L = rt.lib()
    fp, u32, i32 = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    out = np.zeros((n, 9), np.float32)
    assert L.rt_gather_triangles_parts(v.ctypes.data_as(fp), v.shape[0], f.ctypes.data_as(u32), f.size, None, k, None, out.ctypes.data_as(fp)) == rt.RT_ERR_INVALID
    with pytest.raises(rt.RtError) as e:
        rt.gather_triangles_parts(v, f, pf, part_models(k + 1))
    assert e.value.code == rt.RT_ERR_INVALID


def test_symbols_are_exported_and_declared():
    L = rt.lib()
    for name in NEW_SYMBOLS:
        assert name in rt.SIGNATURES, name
        assert getattr(L, name) is not None, name
    assert rt.RT_MAX_MESH_PARTS == 65535


def test_null_context():
    L = rt.lib()
    n = C.c_int()
    ptr, size = C.c_void_p(), C.c_size_t()
    v, f = _soup(9)
    pf = split("one", 9)
    m = part_models(1)
    hits = np.zeros((4, 4), np.float32)
    out = np.zeros(4, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    calls = {
        "rt_mesh_upload_parts": lambda: L.rt_mesh_upload_parts(None, v.ctypes.data_as(C.POINTER(C.c_float)), v.shape[0], f.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                               f.size, pf.ctypes.data_as(C.POINTER(C.c_int32)), 1),
        "rt_mesh_parts": lambda: L.rt_mesh_parts(None, None, 0, C.byref(n)),
        "rt_mesh_part_matrices": lambda: L.rt_mesh_part_matrices(None, C.byref(ptr), C.byref(size)),
        "rt_mesh_set_part_matrices": lambda: L.rt_mesh_set_part_matrices(None, 0, 1, m.ctypes.data_as(C.POINTER(C.c_float))),
        "rt_mesh_rebuild_parts": lambda: L.rt_mesh_rebuild_parts(None),
        "rt_mesh_refit_parts": lambda: L.rt_mesh_refit_parts(None),
        "rt_mesh_hit_parts": lambda: L.rt_mesh_hit_parts(None, p(hits), 4, p(out), p(out)),
        "rt_mesh_hit_parts_host": lambda: L.rt_mesh_hit_parts_host(None, p(hits), 4, p(out), p(out)),
    }
    assert set(calls) == set(NEW_SYMBOLS) - {"rt_gather_triangles_parts"}
    for name, call in calls.items():
        assert call() == rt.RT_ERR_INVALID, name
