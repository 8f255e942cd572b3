"""rt_refit_bvh without a GPU: the tree of a build kept -- links, first, count, which input triangle sits in which row -- and the
triangle rows and every node's box recomputed from new triangles.  It is the definition the device refit (tests/test_gpu_mesh_refit.py) is held to."""
import ctypes as C

import numpy as np
import pytest

import opengl_raytracing_amd as rt
from test_dynamic_mesh_host import SIZES

LINKS = [3, 7, 8, 9]          # left, right, first, count
BOX = [0, 1, 2, 4, 5, 6]      # min.xyz, max.xyz


def _soup9(n, seed=None):
    """n small triangles scattered through a cube of half-extent 1.5: (v0, e1, e2) rows."""
    rng = np.random.default_rng(n if seed is None else seed)
    t = np.empty((n, 9), np.float32)
    t[:, :3] = rng.uniform(-1.5, 1.5, (n, 3))
    t[:, 3:] = rng.normal(0, 0.12, (n, 6))
    return t


def _displaced(t9):
    out = t9.copy()
    out[:, :3] = t9[:, :3] + np.float32(0.05) * np.sin(np.float32(3) * t9[:, :3] + np.float32(0.7)).astype(np.float32)
    return out


def _scattered(t9, seed=1):
    out = t9.copy()
    out[:, :3] = t9[:, :3] + np.random.default_rng(seed).uniform(-1.5, 1.5, (t9.shape[0], 3)).astype(np.float32)
    return out


def _subtree_rows(nodes, i):
    """Rows of tris12 under node i, by walking the links."""
    rows, todo = [], [i]
    while todo:
        k = todo.pop()
        if nodes[k, 9] > 0:
            rows.extend(range(int(nodes[k, 8]), int(nodes[k, 8]) + int(nodes[k, 9])))
        else:
            todo += [int(nodes[k, 3]), int(nodes[k, 7])]
    return rows


def _corner_boxes(t12):
    """Per row: min and max over the corners v0, v0 + e1, v0 + e2 (fp32 additions)."""
    v0, v1, v2 = t12[:, 0:3], t12[:, 0:3] + t12[:, 4:7], t12[:, 0:3] + t12[:, 8:11]
    c = np.stack([v0, v1, v2])
    return c.min(0), c.max(0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- identity
@pytest.mark.parametrize("n", SIZES)
def test_identity_refit_returns_the_build(n):
    t9 = np.random.default_rng(n).normal(0, 1, (n, 9)).astype(np.float32)      # the soups of test_dynamic_mesh_host: no mixed-sign zeros
    nodes, tris, order = rt.build_bvh_order(t9)
    n2, t2 = rt.refit_bvh(nodes, tris, order, t9)
    assert np.array_equal(_bits(n2), _bits(nodes)) and np.array_equal(_bits(t2), _bits(tris))
    # from arrays whose coordinates were wiped: nothing of the old boxes or rows survives a refit
    wiped_n, wiped_t = nodes.copy(), np.full_like(tris, 7.0)
    wiped_n[:, BOX] = np.nan
    n3, t3 = rt.refit_bvh(wiped_n, wiped_t, order, t9)
    assert np.array_equal(_bits(n3), _bits(nodes)) and np.array_equal(_bits(t3), _bits(tris))


# ---------------------------------------------------------------- deformed input
@pytest.mark.parametrize("n,deform", [(9, _displaced), (100, _displaced), (1000, _displaced), (1000, _scattered), (5000, _displaced)])
def test_deformed_refit(n, deform):
    t9 = _soup9(n)
    nodes, tris, order = rt.build_bvh_order(t9)
    new9 = deform(t9)
    keep_n, keep_t, keep_o = nodes.copy(), tris.copy(), order.copy()
    n2, t2 = rt.refit_bvh(nodes, tris, order, new9)
    assert np.array_equal(nodes, keep_n) and np.array_equal(tris, keep_t) and np.array_equal(order, keep_o)      # the wrapper works on copies
    assert np.array_equal(_bits(n2[:, LINKS]), _bits(nodes[:, LINKS])) and np.array_equal(_bits(n2[:, 10:]), _bits(nodes[:, 10:]))
    assert np.array_equal(_bits(t2[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]), _bits(new9[order]))
    assert not t2[:, [3, 7, 11]].any()
    lo, hi = _corner_boxes(t2)
    for i in range(n2.shape[0]):
        rows = _subtree_rows(n2, i)
        assert np.array_equal(n2[i, 0:3], lo[rows].min(0)) and np.array_equal(n2[i, 4:7], hi[rows].max(0)), i
    assert sorted(_subtree_rows(n2, 0)) == list(range(n))


def test_one_leaf_tree():
    for n in (1, 5, 8):
        t9 = _soup9(n)
        nodes, tris, order = rt.build_bvh_order(t9)
        assert nodes.shape[0] == 1
        new9 = _scattered(t9)
        n2, t2 = rt.refit_bvh(nodes, tris, order, new9)
        lo, hi = _corner_boxes(t2)
        assert np.array_equal(n2[0, 0:3], lo.min(0)) and np.array_equal(n2[0, 4:7], hi.max(0))
        assert np.array_equal(_bits(n2[0, LINKS]), _bits(nodes[0, LINKS]))


def test_signed_zero_orders_as_the_device_keys():
    """-0 lies below +0 whichever comes first: the min of a box takes -0 if any corner has it, the max takes +0 if any corner has it."""
    nz, pz = np.float32(-0.0), np.float32(0.0)
    base = np.zeros((12, 9), np.float32)
    base[:, 0] = np.arange(12)                     # x sorts the triangles: two leaves of six
    base[:, 3:] = [0.5, 0, 0, 0.25, 0, 0]          # e1, e2 along x only: y and z of every corner are v0's
    nodes, tris, order = rt.build_bvh_order(base + [0, 1, 1, 0, 0, 0, 0, 0, 0])
    assert nodes.shape[0] == 3
    for first, second in ((nz, pz), (pz, nz)):
        new9 = base.copy()
        new9[:, 1] = np.where(np.arange(12) % 2 == 0, first, second)       # y: both zeros in every leaf, in either order
        new9[:, 2] = first                                                 # z: one kind only
        new9[:, 5] = new9[:, 8] = nz                                       # v0.z + e.z: -0 + -0 = -0, +0 + -0 = +0
        n2, t2 = rt.refit_bvh(nodes, tris, order, new9)
        for i in range(3):
            assert _bits(n2[i, 1]) == _bits(nz) and _bits(n2[i, 5]) == _bits(pz), (i, first)
            assert _bits(n2[i, 2]) == _bits(first) and _bits(n2[i, 6]) == _bits(first), (i, first)


# ---------------------------------------------------------------- the oracle walks a refitted tree to the same hits
CASES = [(2000, _displaced), (2000, _scattered), (5000, _displaced)]


@pytest.mark.parametrize("n,deform", CASES)
def test_oracle_trace_on_a_refitted_tree(orc, n, deform):
    """traceBVH on the refitted tree finds the t it finds on a tree built from scratch over the same triangles.  The two trees put a triangle in
    different leaves, so a triangle whose computed t falls a rounding in front of its leaf box may be culled in one and not
    in the other: such rays are counted and capped at 1 % of the hitting rays.  The cap is a bound, not a measurement: a numpy emulation of the
    refit under the oracle's own trace_bvh found 0 of 2 880, 0 of 2 296 and 0 of 2 998 differing rays on soups of this kind."""
    t9 = _soup9(n, seed=100 + n)
    nodes, tris, order = rt.build_bvh_order(t9)
    new9 = deform(t9)
    rn, rtris = rt.refit_bvh(nodes, tris, order, new9)
    bn, btris = rt.build_bvh(new9)
    u = orc.frame_uniforms(orc.default_render_params(), orc.default_camera(), 8, 8, 0, True, rn.shape[0], rtris.shape[0])
    rng = np.random.default_rng(n + 1)
    n_rays = 3000
    org = (rng.normal(0, 1, (n_rays, 3)) * 4).astype(np.float32)
    aim = new9[rng.integers(0, n, n_rays), :3] + rng.normal(0, 0.2, (n_rays, 3)).astype(np.float32)      # into the cloud
    dirs = aim - org
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    hitting = differ = 0
    for i in range(n_rays):
        ha, ta, _, _, _ = orc.trace_bvh(u, rn, rtris, org[i], dirs[i])
        hb, tb, _, _, _ = orc.trace_bvh(u, bn, btris, org[i], dirs[i])
        if ha or hb:
            hitting += 1
            differ += int(ha != hb or np.float32(ta).view(np.uint32) != np.float32(tb).view(np.uint32))
    print(f"refitted vs rebuilt tree, {n} triangles {deform.__name__}: {differ} of {hitting} hitting rays differ")
    assert hitting > 1000
    assert differ < 0.01 * hitting, (differ, hitting)


# ---------------------------------------------------------------- refusals
def test_refusals():
    t9 = _soup9(100)
    nodes, tris, order = rt.build_bvh_order(t9)
    L = rt.lib()
    FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)

    def call(t=t9, o=order, nd=nodes, tr=tris, nt=100, nn=None):
        nd, tr = None if nd is None else nd.copy(), None if tr is None else tr.copy()
        p = lambda a, ty: None if a is None else a.ctypes.data_as(ty)
        return L.rt_refit_bvh(p(t, FP), nt, p(o, IP), p(nd, FP), nodes.shape[0] if nn is None else nn, p(tr, FP))

    assert call() == rt.RT_OK
    for kw in ({"t": None}, {"o": None}, {"nd": None}, {"tr": None}, {"nt": 0}, {"nt": -3}, {"nn": 0}):
        assert call(**kw) == rt.RT_ERR_INVALID, kw
    for bad in (lambda o: o.__setitem__(5, o[6]), lambda o: o.__setitem__(0, 100), lambda o: o.__setitem__(99, -1)):
        o = order.copy()
        bad(o)
        assert call(o=o) == rt.RT_ERR_INVALID
    inner = int(np.flatnonzero(nodes[:, 9] == 0)[1])
    leaf = int(np.flatnonzero(nodes[:, 9] > 0)[0])
    edits = [(inner, 3, float(nodes.shape[0])),      # a child beyond the array
             (inner, 7, float(inner)),               # a node its own child
             (inner, 7, nodes[inner, 3]),            # both links to one child
             (inner, 3, 0.0),                        # back to the root
             (inner, 3, nodes[inner, 3] + 0.5),      # not an integer
             (leaf, 8, 97.0),                        # a range past the last row / overlapping another leaf
             (leaf, 9, nodes[leaf, 9] - 1),          # a row no leaf owns
             (leaf, 9, -2.0), (leaf, 8, np.nan)]
    for i, col, val in edits:
        nd = nodes.copy()
        nd[i, col] = val
        assert call(nd=nd) == rt.RT_ERR_INVALID, (i, col, val)
    assert call(nn=nodes.shape[0] - 1) == rt.RT_ERR_INVALID      # a link beyond the shortened array
    with pytest.raises(rt.RtError) as e:
        rt.refit_bvh(nodes, tris, order[:-1], t9)
    assert e.value.code == rt.RT_ERR_INVALID
    with pytest.raises(rt.RtError) as e:
        rt.refit_bvh(nodes, tris, order[::-1] * 0, t9)
    assert e.value.code == rt.RT_ERR_INVALID


def test_exported_and_null_safe():
    L = rt.lib()
    for name in ("rt_refit_bvh", "rt_mesh_refit", "rt_mesh_refit_count", "rt_mesh_order", "rt_mesh_order_device"):
        assert name in rt.SIGNATURES and hasattr(L, name)
    assert L.rt_mesh_refit(None, None) == rt.RT_ERR_INVALID
    a, b = C.c_uint64(), C.c_uint64()
    assert L.rt_mesh_refit_count(None, C.byref(a), C.byref(b)) == rt.RT_ERR_INVALID
    assert L.rt_mesh_order(None, np.zeros(4, np.int32).ctypes.data_as(C.POINTER(C.c_int32))) == rt.RT_ERR_INVALID
    p, n = C.c_void_p(), C.c_size_t()
    assert L.rt_mesh_order_device(None, C.byref(p), C.byref(n)) == rt.RT_ERR_INVALID
    assert C.sizeof(rt.RtMeshInfo) == 48      # the layout stays; the refit counters have their own entry
