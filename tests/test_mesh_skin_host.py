"""Skinning of the dynamic mesh without a GPU: rt_skin_positions, the host definition the device's skin is held to
(tests/test_gpu_mesh_skin.py), equals its numpy restatement (tests/skin_ref.py) bit for bit; a skin of one influence of weight 1 is the gather's
transform; what it refuses; and the new symbols.  The rest positions, tables and bone matrices defined here are the ones the GPU tests use."""
import ctypes as C

import numpy as np
import pytest

import opengl_raytracing_amd as rt
from skin_ref import skin_ref
from test_gpu_mesh_refit import COORDS
from test_mesh_parts_host import part_models, split

NEW_SYMBOLS = ("rt_skin_positions", "rt_mesh_skin_upload", "rt_mesh_bones", "rt_mesh_set_bones", "rt_mesh_rest_positions", "rt_mesh_skin")
VERTS = (1, 63, 64, 65, 257, 1000)          # wave and block edges of a one-thread-per-vertex kernel
BONES = (1, 2, 300, 65536)
N_PATTERNS = 9


def bone_mats(n, step=0):
    """[n,16] column-major: a rotation about y times a non-uniform scale and a translation, distinct per bone, another set at every step."""
    b = np.arange(n, dtype=np.float64)
    ang = 0.37 * (b % 97) + 0.011 * b + 0.23 * step
    c, s = np.cos(ang), np.sin(ang)
    M = np.zeros((n, 4, 4))
    M[:, 0, 0], M[:, 0, 2], M[:, 2, 0], M[:, 2, 2], M[:, 1, 1], M[:, 3, 3] = c, s, -s, c, 1.0, 1.0
    M[:, :3, :3] *= np.stack([1.0 + 0.1 * (b % 7), 1.0 + 0.03 * (b % 3), 1.0 - 0.05 * (b % 11)], 1)[:, None, :]
    M[:, 0, 3], M[:, 1, 3], M[:, 2, 3] = 0.1 * (b % 13) + 0.05 * step, 0.6 - 0.01 * (b % 17), -0.2 * (b % 5)
    return np.ascontiguousarray(np.transpose(M, (0, 2, 1)), np.float32).reshape(n, 16)


def rest_positions(nv, seed=0):
    """Random positions in which -0, +0 and the values of test_gpu_mesh_refit.COORDS stand as coordinates here and there."""
    rng = np.random.default_rng(1000 + nv + seed)
    p = rng.normal(0, 1, (nv, 3)).astype(np.float32)
    special = np.array([-0.0, 0.0] + [float(c) for c in COORDS], np.float32)
    flat = p.reshape(-1)
    at = np.arange(0, flat.size, 4)
    flat[at] = special[(np.arange(at.size) + seed) % special.size]
    return p


def skin_tables(nv, nb, offset=0):
    """(bone_idx [nv,4] uint16, weights [nv,4] float32).  Vertex v has weight pattern (v + offset) % N_PATTERNS: all zero; one 1.0; zeros between
    non-zeros (two forms); negative and above one; a sum that is not one; four normalised; -0 between non-zeros; all -0.  Every index is below nb
    whatever its weight, and the last bone is in use with a non-zero weight wherever a pattern has one."""
    rng = np.random.default_rng(7 * nv + nb + offset)
    bi = rng.integers(0, nb, (nv, 4)).astype(np.uint16)
    bi[::3, 3] = nb - 1
    bi[::5, 1] = nb - 1
    r = rng.uniform(0.05, 1.0, (nv, 4)).astype(np.float32)
    w = np.zeros((nv, 4), np.float32)
    pat = (np.arange(nv) + offset) % N_PATTERNS
    v = np.arange(nv)
    m = pat == 1; w[m, v[m] % 4] = 1.0
    m = pat == 2; w[m, 0] = r[m, 0]; w[m, 3] = r[m, 3]
    m = pat == 3; w[m, 1] = r[m, 1]; w[m, 3] = r[m, 3]
    m = pat == 4; w[m] = r[m] * np.array([-1.0, 1.7, -0.4, 2.5], np.float32)
    m = pat == 5; w[m] = r[m]
    m = pat == 6; w[m] = r[m] / r[m].sum(1, keepdims=True)
    m = pat == 7; w[m] = np.array([-0.0, 0.7, -0.0, 0.3], np.float32)
    m = pat == 8; w[m] = np.float32(-0.0)
    return bi, w


def skin_case(nv, nb, offset=0):
    """(rest, bone_idx, weights, bones) of one size"""
    bi, w = skin_tables(nv, nb, offset)
    return rest_positions(nv, offset), bi, w, bone_mats(nb)


def _same(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


@pytest.mark.parametrize("nb", BONES)
@pytest.mark.parametrize("nv", VERTS)
def test_equals_the_numpy_definition(nv, nb):
    for offset in range(N_PATTERNS if nv < N_PATTERNS else 1):      # a single vertex meets every pattern in turn
        rest, bi, w, bones = skin_case(nv, nb, offset)
        assert bi.max() == nb - 1 and bi.dtype == np.uint16
        got = rt.skin_positions(rest, bi, w, bones)
        want = skin_ref(rest, bi, w, bones)
        assert got.dtype == np.float32 and got.shape == (nv, 3) and _same(got, want), (nv, nb, offset)
        none = ~(w != 0).any(1)
        assert _same(got[none], rest[none])                          # nothing unskipped: the rest position's bits, -0 included
        if nv >= 63:
            pat = np.arange(nv) % N_PATTERNS
            assert all((pat == k).any() for k in range(N_PATTERNS)) and none.sum() >= 2 * (nv // N_PATTERNS)
            assert (np.signbit(rest) & (rest == 0)).any() and not _same(got, rest)
            if nb > 1:
                assert (w[bi == nb - 1] != 0).any()                  # the last bone is in use


def test_out_may_be_rest():
    rest, bi, w, bones = skin_case(257, 300)
    want = skin_ref(rest, bi, w, bones)
    buf = rest.copy()
    fp = C.POINTER(C.c_float)
    rc = rt.lib().rt_skin_positions(buf.ctypes.data_as(fp), 257, bi.ctypes.data_as(C.POINTER(C.c_uint16)), w.ctypes.data_as(fp), bones.ctypes.data_as(fp), 300,
                                    buf.ctypes.data_as(fp))
    assert rc == rt.RT_OK and _same(buf, want)


def parts_as_bones(n):
    """n triangles that share no vertex, split into uneven parts, and the skin that gives every vertex its part's matrix with weight 1."""
    v = np.random.default_rng(n).normal(0, 1, (3 * n, 3)).astype(np.float32)
    v[::7, 1] = -0.0
    f = np.arange(3 * n, dtype=np.uint32)
    pf = split("uneven", n)
    models = part_models(pf.size - 1)
    part_of_tri = np.searchsorted(pf, np.arange(n), "right") - 1
    bi = np.zeros((3 * n, 4), np.uint16)
    bi[:, 0] = np.repeat(part_of_tri, 3)
    w = np.zeros((3 * n, 4), np.float32)
    w[:, 0] = 1.0
    return v, f, pf, models, bi, w


@pytest.mark.parametrize("n", [9, 100, 1000])
def test_one_influence_of_weight_one_is_the_gather(n):
    v, f, pf, models, bi, w = parts_as_bones(n)
    skinned = rt.skin_positions(v, bi, w, models)
    got = rt.gather_triangles(skinned, f, np.eye(4, dtype=np.float32).reshape(-1))
    want = rt.gather_triangles_parts(v, f, pf, models)
    assert np.array_equal(got, want)                                 # as floats: an identity gather turns -0 into +0
    assert not np.array_equal(got, rt.gather_triangles(v, f, np.eye(4, dtype=np.float32).reshape(-1)))
    moved = w.copy(); moved[:, [0, 2]] = moved[:, [2, 0]]            # the same influence in the third slot, zeros before it
    bi2 = bi.copy(); bi2[:, [0, 2]] = bi2[:, [2, 0]]
    assert _same(rt.skin_positions(v, bi2, moved, models), skinned)


def _raw(rest, nv, bi, w, bones, nb, out="own"):
    fp, u16 = C.POINTER(C.c_float), C.POINTER(C.c_uint16)
    buf = np.zeros((max(nv, 1), 3), np.float32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    return rt.lib().rt_skin_positions(ptr(rest, fp), nv, ptr(bi, u16), ptr(w, fp), ptr(bones, fp), nb, None if out is None else buf.ctypes.data_as(fp))


def test_refusals():
    nv, nb = 65, 300
    rest, bi, w, bones = skin_case(nv, nb)
    assert _raw(rest, nv, bi, w, bones, nb) == rt.RT_OK
    assert _raw(None, nv, bi, w, bones, nb) == rt.RT_ERR_INVALID                    # a null array, each of the five
    assert _raw(rest, nv, None, w, bones, nb) == rt.RT_ERR_INVALID
    assert _raw(rest, nv, bi, None, bones, nb) == rt.RT_ERR_INVALID
    assert _raw(rest, nv, bi, w, None, nb) == rt.RT_ERR_INVALID
    assert _raw(rest, nv, bi, w, bones, nb, out=None) == rt.RT_ERR_INVALID
    assert _raw(rest, 0, bi, w, bones, nb) == rt.RT_ERR_INVALID                     # nVerts <= 0
    assert _raw(rest, -1, bi, w, bones, nb) == rt.RT_ERR_INVALID
    assert _raw(rest, nv, np.zeros_like(bi), w, bones, 0) == rt.RT_ERR_INVALID      # nBones outside 1 .. RT_MAX_MESH_BONES
    assert _raw(rest, nv, np.zeros_like(bi), w, bones, -3) == rt.RT_ERR_INVALID
    assert _raw(rest, nv, np.zeros_like(bi), w, bones, rt.RT_MAX_MESH_BONES + 1) == rt.RT_ERR_INVALID
    assert _raw(rest, nv, bi, w, bone_mats(rt.RT_MAX_MESH_BONES), rt.RT_MAX_MESH_BONES) == rt.RT_OK      # the largest count is legal
    for slot in range(4):                                                            # an index >= nBones in any slot, whatever its weight
        for weight in (0.0, 0.5):
            b2, w2 = bi.copy(), w.copy()
            b2[40, slot], w2[40, slot] = nb, weight
            assert _raw(rest, nv, b2, w2, bones, nb) == rt.RT_ERR_INVALID, (slot, weight)
    assert _raw(rest, nv, bi, w, bones, nb - 1) == rt.RT_ERR_INVALID                # the same tables against a table one bone short
    for bad in (np.nan, np.inf, -np.inf):                                            # a weight that is not finite
        w2 = w.copy(); w2[64, 3] = bad
        assert _raw(rest, nv, bi, w2, bones, nb) == rt.RT_ERR_INVALID, bad
    nanbones = bones.copy(); nanbones[5] = np.nan                                    # bone matrices are not inspected
    assert _raw(rest, nv, bi, w, nanbones, nb) == rt.RT_OK
    for call in (lambda: rt.skin_positions(rest, bi[:-1], w[:-1], bones), lambda: rt.skin_positions(rest, bi.astype(np.int64) + 70000, w, bones),
                 lambda: rt.skin_positions(rest, bi, w, bones.reshape(-1)[:-1])):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt.RT_ERR_INVALID


def test_symbols_are_exported_and_declared():
    L = rt.lib()
    for name in NEW_SYMBOLS:
        assert name in rt.SIGNATURES, name
        assert getattr(L, name) is not None, name
    assert rt.RT_SKIN_INFLUENCES == 4 and rt.RT_MAX_MESH_BONES == 65536


def test_null_context():
    L = rt.lib()
    ptr, size = C.c_void_p(), C.c_size_t()
    rest, bi, w, bones = skin_case(9, 2)
    fp = C.POINTER(C.c_float)
    calls = {
        "rt_mesh_skin_upload": lambda: L.rt_mesh_skin_upload(None, rest.ctypes.data_as(fp), bi.ctypes.data_as(C.POINTER(C.c_uint16)), w.ctypes.data_as(fp), 2),
        "rt_mesh_bones": lambda: L.rt_mesh_bones(None, C.byref(ptr), C.byref(size)),
        "rt_mesh_set_bones": lambda: L.rt_mesh_set_bones(None, 0, 2, bones.ctypes.data_as(fp)),
        "rt_mesh_rest_positions": lambda: L.rt_mesh_rest_positions(None, C.byref(ptr), C.byref(size)),
        "rt_mesh_skin": lambda: L.rt_mesh_skin(None),
    }
    assert set(calls) == set(NEW_SYMBOLS) - {"rt_skin_positions"}
    for name, call in calls.items():
        assert call() == rt.RT_ERR_INVALID, name
