"""Morph targets of the dynamic mesh without a GPU: rt_morph_positions, the host definition the device's morph is held to
(tests/test_gpu_mesh_morph.py), equals its numpy restatement (tests/morph_ref.py) bit for bit; rt_debug_morph_pack's arrays equal the numpy packer
byte for byte; what both refuse; and the new symbols.  The targets and weights defined here are the ones the GPU tests use."""
import ctypes as C

import numpy as np
import pytest

import opengl_raytracing_amd as rt
from morph_ref import PAD, morph_ref, pack_ref
from test_mesh_skin_host import rest_positions

NEW_SYMBOLS = ("rt_morph_positions", "rt_debug_morph_pack", "rt_mesh_morph_upload", "rt_mesh_morph_base", "rt_mesh_morph_weights",
               "rt_mesh_set_morph_weights", "rt_mesh_morph", "rt_mesh_morph_info")
VERTS = (1, 63, 64, 65, 257, 1000)          # wave and block edges of a one-thread-per-vertex kernel; all but 64 end in a partial slice
TARGETS = (1, 3, 40)
N_PATTERNS = 6                              # weight patterns: +0, -0, 1, negative, above one, inside (0, 1)

FP, I32P, U32P = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)


def _same(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def hub_of(nv):
    """(hub, bare): the vertex every non-empty target names (some of them twice), and its neighbour in the same slice that no target names."""
    return (0, None) if nv < 3 else ((nv // 2) | 1, ((nv // 2) | 1) - 1)


def empty_targets(nv, nt, offset=0):
    """Which targets have no entry: the first, the middle and the last one of 40; one of three, another one per size and offset; none of one."""
    return {0, nt // 2, nt - 1} if nt >= 40 else ({(nv + offset) % 3} if nt == 3 else set())


def morph_targets(nv, nt, offset=0):
    """(target_first int32 [nt+1], vert_idx uint32 [E], deltas float32 [E,3]).  Every non-empty target names about a third of the vertices in shuffled
    order, and the hub; every other one names the hub a second time, as its last entry; the hub's neighbour is named by none.  Deltas have +0 and -0
    as components here and there, and whole rows of them."""
    rng = np.random.default_rng(31 * nv + nt + 7 * offset)
    hub, bare = hub_of(nv)
    empty = empty_targets(nv, nt, offset)
    first, vi, d = [0], [], []
    for t in range(nt):
        if t not in empty:
            v = np.flatnonzero(rng.uniform(0, 1, nv) < 0.3)
            v = v[(v != hub) & (v != (-1 if bare is None else bare))]
            v = rng.permutation(np.concatenate([v, [hub]]))
            if t % 2 == 0:
                v = np.concatenate([v, [hub]])
            vi.append(v)
            d.append(rng.normal(0, 0.1, (v.size, 3)).astype(np.float32))
        first.append(first[-1] + (vi[-1].size if t not in empty else 0))
    vi = np.concatenate(vi).astype(np.uint32) if vi else np.zeros(0, np.uint32)
    d = np.concatenate(d) if d else np.zeros((0, 3), np.float32)
    flat = d.reshape(-1)
    flat[0::5] = np.float32(0.0)
    flat[2::7] = np.float32(-0.0)
    d[3::11] = np.float32(-0.0)
    d[4::13] = np.float32(0.0)
    return np.asarray(first, np.int32), vi, d


def morph_weights(nt, offset=0, step=0):
    """[nt] float32; target t has pattern (t + offset) % N_PATTERNS, other values at every step."""
    rng = np.random.default_rng(5 * nt + offset + 1000 * step)
    r = rng.uniform(0.05, 1.0, nt).astype(np.float32)
    pat = (np.arange(nt) + offset) % N_PATTERNS
    w = np.zeros(nt, np.float32)
    w[pat == 1] = np.float32(-0.0)
    w[pat == 2] = np.float32(1.0)
    w[pat == 3] = -r[pat == 3]
    w[pat == 4] = r[pat == 4] + np.float32(1.0)
    w[pat == 5] = r[pat == 5]
    return w


def morph_case(nv, nt, offset=0):
    """(base, target_first, vert_idx, deltas, weights) of one size"""
    return (rest_positions(nv, offset),) + morph_targets(nv, nt, offset) + (morph_weights(nt, offset),)


@pytest.mark.parametrize("nt", TARGETS)
@pytest.mark.parametrize("nv", VERTS)
def test_equals_the_numpy_definition(nv, nt):
    seen_empty = set()
    for offset in range(N_PATTERNS):                                  # every target, and with it every vertex, meets each weight pattern in turn
        base, tf, vi, d, w = morph_case(nv, nt, offset)
        got = rt.morph_positions(base, tf, vi, d, w)
        want = morph_ref(base, tf, vi, d, w)
        assert got.dtype == np.float32 and got.shape == (nv, 3) and _same(got, want), (nv, nt, offset)
        used = np.zeros(nv, bool)
        used[vi[np.repeat(w, np.diff(tf)) != 0]] = True
        assert _same(got[~used], base[~used])                         # nothing unskipped: the base position's bits, -0 included
        hub, bare = hub_of(nv)
        empty = empty_targets(nv, nt, offset)
        seen_empty |= empty
        count = np.bincount(vi, minlength=nv)
        assert count[hub] == count.max() and count[hub] >= nt - len(empty)      # named by every non-empty target
        assert all(tf[t] == tf[t + 1] for t in empty)
        if nt > 1:
            t = next(t for t in range(nt) if t % 2 == 0 and t not in empty)
            assert (vi[tf[t]:tf[t + 1]] == hub).sum() == 2                      # the same (target, vertex) pair twice
        if bare is not None:
            assert count[bare] == 0 and bare // 64 == hub // 64 and not used[bare]
            assert (d == 0).any() and np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all() and (d == 0).all(1).any()
            assert (np.signbit(base) & (base == 0)).any()
            if used.any():
                assert not _same(got, base)
    if nt == 3:
        assert seen_empty == {0, 1, 2}                                # an empty target first, in the middle and last
    if nt == 40:
        assert seen_empty == {0, 20, 39}
    pats = {(t + o) % N_PATTERNS for t in range(nt) for o in range(N_PATTERNS)}
    assert pats == set(range(N_PATTERNS))
    w = morph_weights(40)
    assert (w == 0).sum() >= 12 and np.signbit(w[w == 0]).any() and (w == 1).any() and (w < 0).any() and (w > 1).any()


def test_out_may_be_base():
    base, tf, vi, d, w = morph_case(257, 40, 2)
    want = morph_ref(base, tf, vi, d, w)
    buf = base.copy()
    rc = rt.lib().rt_morph_positions(buf.ctypes.data_as(FP), 257, tf.ctypes.data_as(I32P), vi.ctypes.data_as(U32P), d.ctypes.data_as(FP), 40,
                                     w.ctypes.data_as(FP), buf.ctypes.data_as(FP))
    assert rc == rt.RT_OK and _same(buf, want) and not _same(buf, base)


def test_a_weight_of_one_adds_the_delta_and_order_matters():
    base = np.array([[1.0, -0.0, 3.0], [-0.0, 0.0, -0.0]], np.float32)
    tf, vi = np.array([0, 2, 3], np.int32), np.array([0, 0, 0], np.uint32)
    d = np.array([[1e8, 0.0, -0.0], [-1e8, 0.0, -0.0], [0.5, -0.0, 0.0]], np.float32)
    got = rt.morph_positions(base, tf, vi, d, np.array([1.0, 1.0], np.float32))
    assert _same(got[0], np.array([0.5, 0.0, 3.0], np.float32))       # (1 + 1e8) - 1e8 = 0 in fp32, then + 0.5; -0 + +0 = +0
    assert _same(got[1], base[1])
    got = rt.morph_positions(base, tf, vi, d, np.array([-0.0, 1.0], np.float32))
    assert _same(got[0], np.array([1.5, -0.0, 3.0], np.float32))      # -0 + -0 = -0: only the third entry is left


# ---------------------------------------------------------------- the packed form
def _assert_pack(nv, tf, vi, d, tag):
    got = rt.debug_morph_pack(nv, tf, vi, d)
    sf, ent, info = pack_ref(nv, tf, vi, d)
    assert got["slice_first"].dtype == np.uint32 and _same(got["slice_first"], sf), tag
    assert got["entries"].shape == ent.shape and _same(got["entries"], ent), tag
    assert {k: getattr(got["info"], k) for k in info} == info, tag
    return got, info


@pytest.mark.parametrize("nt", TARGETS)
@pytest.mark.parametrize("nv", VERTS)
def test_pack_equals_the_numpy_packer(nv, nt):
    _, tf, vi, d, _ = morph_case(nv, nt, 1)
    got, info = _assert_pack(nv, tf, vi, d, (nv, nt))
    ent = got["entries"]
    pad = ent[:, 3] == PAD
    assert (ent[pad, :3] == 0).all() and (~pad).sum() == vi.size      # pad records are {+0, +0, +0, pad}; every entry is there once
    lanes = np.arange(ent.shape[0]) % 64 + 64 * np.searchsorted(got["slice_first"], np.arange(ent.shape[0]) // 64, "right") - 64
    assert pad[lanes >= nv].all()                                     # the lanes of the last slice that have no vertex
    hub, bare = hub_of(nv)
    if bare is not None:
        s = hub // 64
        rows = int(got["slice_first"][s + 1] - got["slice_first"][s])
        assert rows == info["maxPerVertex"] and pad[(int(got["slice_first"][s]) + np.arange(rows)) * 64 + bare % 64].all()


def test_pack_edge_cases():
    z = np.zeros((0, 3), np.float32)
    got, info = _assert_pack(130, np.zeros(4, np.int32), np.zeros(0, np.uint32), z, "all empty")     # no entry at all: every slice has no row
    assert info["paddedEntries"] == 0 and got["entries"].shape == (0, 4) and list(got["slice_first"]) == [0, 0, 0, 0]
    # one entry in the middle slice of three
    got, info = _assert_pack(130, np.array([0, 0, 1], np.int32), np.array([70], np.uint32), np.array([[1, -0.0, 3]], np.float32), "one")
    assert list(got["slice_first"]) == [0, 0, 1, 1] and info["paddedEntries"] == 64 and info["bytes"] == 64 * 16 + 16 + 130 * 12 + 8
    assert list(got["entries"][6]) == [0x3F800000, 0x80000000, 0x40400000, 1]


def test_pack_size_query_convention():
    _, tf, vi, d, _ = morph_case(65, 3)
    L = rt.lib()
    args = (65, tf.ctypes.data_as(I32P), vi.ctypes.data_as(U32P), d.ctypes.data_as(FP), 3)
    size = C.c_size_t(7)
    for which, want in ((rt.RT_MORPH_ARRAY_SLICE_FIRST, 12), (rt.RT_MORPH_ARRAY_INFO, C.sizeof(rt.RtMorphInfo))):
        assert L.rt_debug_morph_pack(*args, which, None, 0, C.byref(size)) == rt.RT_OK and size.value == want      # dst == NULL asks for the size
        buf = np.zeros(want, np.uint8)
        assert L.rt_debug_morph_pack(*args, which, C.c_void_p(buf.ctypes.data), want - 1, C.byref(size)) == rt.RT_ERR_INVALID
        assert L.rt_debug_morph_pack(*args, which, C.c_void_p(buf.ctypes.data), want, C.byref(size)) == rt.RT_OK and size.value == want
    assert C.sizeof(rt.RtMorphInfo) == 40
    assert L.rt_debug_morph_pack(*args, rt.RT_MORPH_ARRAY_ENTRIES, None, 0, C.byref(size)) == rt.RT_OK
    assert size.value == pack_ref(65, tf, vi, d)[2]["paddedEntries"] * 16
    assert L.rt_debug_morph_pack(*args, 2, None, 0, C.byref(size)) == rt.RT_ERR_INVALID and size.value == 0       # an unknown array
    assert L.rt_debug_morph_pack(*args, rt.RT_MORPH_ARRAY_INFO, None, 0, None) == rt.RT_ERR_INVALID


def test_pack_refuses_2_31_records():
    """One vertex named 2^25 times gives its slice 2^25 rows of 64 records.  The entry arrays are untouched zero pages and the refusal comes from the
    counts, before any record is made; one entry fewer is accepted (as a size query, which makes no record either)."""
    n = 1 << 25
    tf = np.array([0, n], np.int32)
    vi, d = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32)
    L = rt.lib()
    size = C.c_size_t()
    call = lambda first, which: L.rt_debug_morph_pack(64, first.ctypes.data_as(I32P), vi.ctypes.data_as(U32P), d.ctypes.data_as(FP), 1, which, None, 0,
                                                     C.byref(size))
    for which in (rt.RT_MORPH_ARRAY_INFO, rt.RT_MORPH_ARRAY_ENTRIES, rt.RT_MORPH_ARRAY_SLICE_FIRST):
        assert call(tf, which) == rt.RT_ERR_UNSUPPORTED and size.value == 0
    with pytest.raises(rt.RtError) as e:
        rt.debug_morph_pack(64, tf, vi, d)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED
    assert call(np.array([0, n - 1], np.int32), rt.RT_MORPH_ARRAY_ENTRIES) == rt.RT_OK and size.value == ((1 << 31) - 64) * 16


def test_targets_from_dense_round_trip():
    rng = np.random.default_rng(3)
    T, V = 5, 130
    dense = rng.normal(0, 1, (T, V, 3)).astype(np.float32)
    dense[rng.uniform(0, 1, (T, V)) < 0.6] = 0.0
    dense[1] = 0.0                                                    # an empty target
    dense[2, 7] = [-0.0, 0.0, -0.0]                                   # dropped: all three components are +-0
    dense[2, 9] = [-0.0, 0.25, 0.0]                                   # kept, signed zeros and all
    tf, vi, d = rt.morph_targets_from_dense(dense)
    assert tf.dtype == np.int32 and vi.dtype == np.uint32 and d.dtype == np.float32 and tf[0] == 0 and tf[-1] == vi.size == d.shape[0]
    assert tf[2] == tf[1] and tf[1] > 0                              # target 1 is empty
    assert (d != 0).any(1).all() and vi.size == int((dense != 0).any(2).sum())
    back = np.zeros_like(dense)
    for t in range(T):
        seg = slice(tf[t], tf[t + 1])
        assert (np.diff(vi[seg].astype(np.int64)) > 0).all()          # ascending, each vertex once
        back[t, vi[seg]] = d[seg]
    assert np.array_equal(back, dense) and _same(back[2, 9], dense[2, 9]) and 7 not in vi[tf[2]:tf[3]]
    base = rest_positions(V)
    w = np.array([0.5, 3.0, -1.0, 0.0, 1.0], np.float32)
    want = base.copy()
    for t in range(T):                                                # the dense blend, target by target, skipping what the sparse form skips
        if w[t] != 0:
            keep = (dense[t] != 0).any(1)
            want[keep] = want[keep] + w[t] * dense[t][keep]
    assert _same(rt.morph_positions(base, tf, vi, d, w), want)
    with pytest.raises(rt.RtError):
        rt.morph_targets_from_dense(dense[0])


# ---------------------------------------------------------------- refusals
def _raw(base, nv, tf, vi, d, nt, w, out="own"):
    buf = np.zeros((max(nv, 1), 3), np.float32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    return rt.lib().rt_morph_positions(ptr(base, FP), nv, ptr(tf, I32P), ptr(vi, U32P), ptr(d, FP), nt, ptr(w, FP), None if out is None else buf.ctypes.data_as(FP))


def _raw_pack(nv, tf, vi, d, nt):
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    size = C.c_size_t()
    return rt.lib().rt_debug_morph_pack(nv, ptr(tf, I32P), ptr(vi, U32P), ptr(d, FP), nt, rt.RT_MORPH_ARRAY_INFO, None, 0, C.byref(size))


def broken_targets(nv, nt, tf, vi, d):
    """name -> (target_first, vert_idx, deltas, nTargets) that every entry point refuses with RT_ERR_INVALID"""
    out = {}
    t2 = tf.copy(); t2[0] = 1; out["targetFirst[0] != 0"] = (t2, vi, d, nt)
    t2 = tf.copy(); t2[2] = t2[1] - 1; out["targetFirst decreases"] = (t2, vi, d, nt)
    v2 = vi.copy(); v2[5] = nv; out["vertIdx == nVerts"] = (tf, v2, d, nt)
    v2 = vi.copy(); v2[-1] = 0xFFFFFFFF; out["vertIdx huge"] = (tf, v2, d, nt)
    for bad in (np.nan, np.inf, -np.inf):
        d2 = d.copy(); d2[-1, 2] = bad; out[f"delta {bad}"] = (tf, vi, d2, nt)
    out["no targets"] = (tf, vi, d, 0)
    out["negative targets"] = (tf, vi, d, -2)
    big = np.zeros(rt.RT_MAX_MORPH_TARGETS + 2, np.int32)
    out["too many targets"] = (big, vi, d, rt.RT_MAX_MORPH_TARGETS + 1)
    return out


def test_refusals():
    nv, nt = 65, 3
    base, tf, vi, d, w = morph_case(nv, nt)
    assert _raw(base, nv, tf, vi, d, nt, w) == rt.RT_OK and _raw_pack(nv, tf, vi, d, nt) == rt.RT_OK
    assert _raw(None, nv, tf, vi, d, nt, w) == rt.RT_ERR_INVALID                     # a null array, each of the six
    assert _raw(base, nv, None, vi, d, nt, w) == rt.RT_ERR_INVALID
    assert _raw(base, nv, tf, None, d, nt, w) == rt.RT_ERR_INVALID
    assert _raw(base, nv, tf, vi, None, nt, w) == rt.RT_ERR_INVALID
    assert _raw(base, nv, tf, vi, d, nt, None) == rt.RT_ERR_INVALID
    assert _raw(base, nv, tf, vi, d, nt, w, out=None) == rt.RT_ERR_INVALID
    assert _raw_pack(nv, None, vi, d, nt) == _raw_pack(nv, tf, None, d, nt) == _raw_pack(nv, tf, vi, None, nt) == rt.RT_ERR_INVALID
    for bad_nv in (0, -1):                                                            # nVerts <= 0
        assert _raw(base, bad_nv, np.zeros(2, np.int32), vi, d, 1, w) == rt.RT_ERR_INVALID
        assert _raw_pack(bad_nv, np.zeros(2, np.int32), vi, d, 1) == rt.RT_ERR_INVALID
    for name, (t2, v2, d2, n2) in broken_targets(nv, nt, tf, vi, d).items():
        assert _raw(base, nv, t2, v2, d2, n2, np.zeros(max(n2, 1) + 1, np.float32)) == rt.RT_ERR_INVALID, name
        assert _raw_pack(nv, t2, v2, d2, n2) == rt.RT_ERR_INVALID, name
    big = np.zeros(rt.RT_MAX_MORPH_TARGETS + 1, np.int32)                            # the largest count is legal (all of them empty)
    assert _raw(base, nv, big, vi, d, rt.RT_MAX_MORPH_TARGETS, np.ones(rt.RT_MAX_MORPH_TARGETS, np.float32)) == rt.RT_OK
    assert _raw_pack(nv, big, vi, d, rt.RT_MAX_MORPH_TARGETS) == rt.RT_OK
    for x in (np.nan, np.inf):                                                        # base and weights are not inspected
        b2 = base.copy(); b2[3, 1] = x
        assert _raw(b2, nv, tf, vi, d, nt, w) == rt.RT_OK
    for call in (lambda: rt.morph_positions(base, tf, vi[:-1], d[:-1], w), lambda: rt.morph_positions(base, tf, vi, d, w[:-1]),
                 lambda: rt.morph_positions(base, tf, -vi.astype(np.int64) - 1, d, w), lambda: rt.morph_positions(base, tf[:1], vi[:0], d[:0], w[:0])):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt.RT_ERR_INVALID


def test_symbols_are_exported_and_declared():
    L = rt.lib()
    for name in NEW_SYMBOLS:
        assert name in rt.SIGNATURES, name
        assert getattr(L, name) is not None, name
    assert rt.RT_MAX_MORPH_TARGETS == 65536 and (rt.RT_MORPH_TO_POSITIONS, rt.RT_MORPH_TO_REST) == (0, 1)
    assert (rt.RT_MORPH_ARRAY_SLICE_FIRST, rt.RT_MORPH_ARRAY_ENTRIES, rt.RT_MORPH_ARRAY_INFO) == (0, 1, 100)


def test_null_context():
    L = rt.lib()
    ptr, size = C.c_void_p(), C.c_size_t()
    base, tf, vi, d, w = morph_case(9, 3)
    info = rt.RtMorphInfo()
    calls = {
        "rt_mesh_morph_upload": lambda: L.rt_mesh_morph_upload(None, base.ctypes.data_as(FP), tf.ctypes.data_as(I32P), vi.ctypes.data_as(U32P), d.ctypes.data_as(FP), 3),
        "rt_mesh_morph_base": lambda: L.rt_mesh_morph_base(None, C.byref(ptr), C.byref(size)),
        "rt_mesh_morph_weights": lambda: L.rt_mesh_morph_weights(None, C.byref(ptr), C.byref(size)),
        "rt_mesh_set_morph_weights": lambda: L.rt_mesh_set_morph_weights(None, 0, 3, w.ctypes.data_as(FP)),
        "rt_mesh_morph": lambda: L.rt_mesh_morph(None, rt.RT_MORPH_TO_POSITIONS),
        "rt_mesh_morph_info": lambda: L.rt_mesh_morph_info(None, C.byref(info)),
    }
    assert set(calls) == set(NEW_SYMBOLS) - {"rt_morph_positions", "rt_debug_morph_pack"}
    for name, call in calls.items():
        assert call() == rt.RT_ERR_INVALID, name
