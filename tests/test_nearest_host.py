"""The nearest-point query's host definition (rt_nearest_points, rt.nearest_points) against its numpy restatement (nearest_ref.py),
bit for bit: every shared mesh and point set with and without max_dist, point layouts, the limit exactly at a winner's e and one ulp either side, the
single leaf as a tree, the refusals, the three invariants of the definition, its accuracy against the float64 true distance, and that the fixtures
do exercise the clamp e(t) != d2(t).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import nearest_ref as ref
import opengl_raytracing_amd as rt

f32 = np.float32
bits = ref.bits

# the largest |sqrt(e) - D64| / ulp32(maxAbsCoord + D64) measured over all the fixtures below (on the layer stack).  The test allows
# four times it: the margin covers other point seeds, not other code.
MEASURED_ULPS = 3.654
# points of the fixtures whose winner has e(t) != d2(t), and points where any row has (all on the layer stack)
CLAMPED_WINNERS, CLAMPED_ANY = 8, 13


def _same(got, hits, closest, what):
    bad = np.flatnonzero((bits(got.hits) != bits(hits)).any(1))
    assert bad.size == 0, (what, bad[:8], got.hits[bad[:2]], hits[bad[:2]])
    bad = np.flatnonzero((bits(got.points) != bits(closest)).any(1))
    assert bad.size == 0, (what, bad[:8], got.points[bad[:2]], closest[bad[:2]])


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("mesh", ref.MESHES)
def test_definition_equals_the_numpy_restatement(mesh, limited):
    nodes, tris, pts, md = ref.case(mesh)
    hits, closest, _ = ref.reference(mesh, limited)
    got = rt.nearest_points(nodes, tris, pts, md if limited else None)
    _same(got, hits, closest, (mesh, limited))
    assert got.visits is None and len(got) == pts.shape[0]
    assert np.array_equal(got.dist2, hits[:, 0], equal_nan=True) and np.array_equal(got.prim, hits.view(np.int32)[:, 1]) and got.uv.shape == (len(got), 2)
    miss = got.prim < 0
    assert (got.hits[miss, 0] == np.inf).all() and (bits(got.hits[miss, 2:]) == 0).all() and (bits(got.points[miss]) == 0).all()
    assert miss[~np.isfinite(pts).all(1)].all()
    if limited:
        assert miss[::97].all() and 100 < miss.sum() < len(got) - 100          # empty slots, and limits on both sides of the distances
    else:
        assert miss.sum() == (~np.isfinite(pts).all(1)).sum() == 9
    if mesh in ("one_triangle", "one_leaf"):
        assert nodes.shape[0] == 1                                            # the single leaf as a tree


def test_point_layouts_give_identical_bytes():
    nodes, tris, pts, md = ref.case("bunny")
    hits, closest, _ = ref.reference("bunny", True)
    p4 = np.full((pts.shape[0], 4), np.nan, f32); p4[:, :3] = pts
    p8 = np.full((pts.shape[0], 8), 7.0, f32); p8[:, 2:5] = pts
    for name, p in (("[N,4]", p4), ("[N,8] interleaved", p8[:, 2:5]), ("[N,4] cut", p4[:, :3]), ("one point", pts[5:6])):
        if p.shape[0] == 1:
            _same(rt.nearest_points(nodes, tris, p, md[5:6]), hits[5:6], closest[5:6], name)
        else:
            _same(rt.nearest_points(nodes, tris, p, md), hits, closest, name)
    assert len(rt.nearest_points(nodes, tris, pts[:0])) == 0


def test_the_limit_exactly_at_the_winners_e_and_one_ulp_either_side():
    """An axis-aligned quad at y = 0 and points exactly 0.5 and 2 above it: e = 0.25 and 4, L = max_dist^2 is exact too."""
    nodes, tris = rt.build_bvh(np.array([[-4, 0, -4, 8, 0, 0, 8, 0, 8], [-4, 0, -4, 8, 0, 8, 0, 0, 8]], f32))
    for h in (f32(0.5), f32(2.0)):
        pts = np.array([[1.0, h, -2.0], [-3.0, h, 0.5], [0.25, -h, 0.25]], f32)
        free = rt.nearest_points(nodes, tris, pts)
        assert (free.dist2 == h * h).all() and (free.prim >= 0).all()
        for md, hit in ((h, True), (np.nextafter(h, f32(0)), False), (np.nextafter(h, f32(9)), True)):
            got = rt.nearest_points(nodes, tris, pts, np.full(3, md, f32))
            want = ref.answer(nodes, tris, pts, np.full(3, md, f32))
            _same(got, want[0], want[1], (h, md))
            assert ((got.prim >= 0) == hit).all(), (h, md, got.hits)
            if hit:
                assert np.array_equal(bits(got.hits), bits(free.hits)) and np.array_equal(bits(got.points), bits(free.points))
    nanlimit = rt.nearest_points(nodes, tris, pts, np.full(3, np.nan, f32))                    # a NaN limit accepts nothing
    assert (nanlimit.prim == -1).all()
    assert (rt.nearest_points(nodes, tris, pts, np.full(3, np.inf, f32)).prim >= 0).all()


@pytest.mark.parametrize("mesh", ref.MESHES)
def test_the_three_invariants(mesh):
    nodes, tris, pts, md = ref.case(mesh)
    got = rt.nearest_points(nodes, tris, pts)
    t = ref.reference(mesh, False)[2]
    hit = got.prim >= 0
    assert (got.dist2[hit] >= t.lb_root[hit]).all()                                             # 1: e >= lb(root box)
    with np.errstate(invalid="ignore"):
        assert (~(got.dist2[hit, None] > t.e[hit])).all()                                       # 2: e <= e(t) for every row t (a NaN e(t) is no row's answer)
    v0 = np.ascontiguousarray(tris[:, 0:3])                                                     # 3: a vertex of row r: e == 0 and prim <= r
    at = rt.nearest_points(nodes, tris, v0)
    assert (bits(at.dist2) == 0).all() and (at.prim <= np.arange(tris.shape[0])).all() and (at.prim >= 0).all()
    assert (at.points == v0).all()                                                              # (numerically: a zero's sign is free)


def test_accuracy_against_the_float64_true_distance():
    worst = 0.0
    for mesh in ref.MESHES:
        nodes, tris, pts, md = ref.case(mesh)
        got = rt.nearest_points(nodes, tris, pts)
        ok = got.prim >= 0
        D = ref.true_distance(tris, pts[ok])
        scale = np.maximum(np.abs(pts[ok]).max(1).astype(np.float64), float(np.abs(nodes[0, [0, 1, 2, 4, 5, 6]]).max())) + D
        err = np.abs(np.sqrt(got.dist2[ok].astype(np.float64)) - D) / ref.ulp32(scale)
        print(f"nearest accuracy {mesh}: {err.max():.4f} ulp32(maxAbsCoord + D64) at point {pts[ok][err.argmax()]}")
        worst = max(worst, float(err.max()))
    print(f"nearest accuracy, all fixtures: {worst:.4f}")
    assert worst <= 4 * MEASURED_ULPS, worst


def test_the_fixtures_exercise_the_clamp():
    """Points where rounding made a triangle look nearer than a box around it: e(t) != d2(t), for the winner or a runner-up."""
    winners = any_row = 0
    for mesh in ref.MESHES:
        hits, _, t = ref.reference(mesh, False)
        prim = hits.view(np.int32)[:, 1]
        ok = prim >= 0
        rows = np.arange(prim.size)
        raised = (t.e != t.d2) & ~np.isnan(t.d2)
        winners += int(raised[rows, np.maximum(prim, 0)][ok].sum())
        any_row += int(raised[ok].any(1).sum())
    print(f"clamped winners {winners}, points with a clamped row {any_row}")
    assert winners == CLAMPED_WINNERS and any_row == CLAMPED_ANY and winners > 0


def test_refusals_write_nothing():
    L = rt.lib()
    nodes, tris, pts, md = ref.case("layers")
    pts, md = np.ascontiguousarray(pts[:8]), np.abs(md[:8])
    hits, closest = np.full((8, 4), f32(-7.5), f32), np.full((8, 3), f32(-7.5), f32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(nodes_=nodes, tris_=tris, n_nodes=None, n_tris=None, pts_=pts, stride=3, n=8, hits_=hits):
        return L.rt_nearest_points(p(nodes_), nodes.shape[0] if n_nodes is None else n_nodes, p(tris_), tris.shape[0] if n_tris is None else n_tris,
                                   p(pts_), stride, p(md), n, p(hits_), p(closest))

    assert call(n=-1) == rt.RT_ERR_INVALID
    assert call(stride=2) == rt.RT_ERR_INVALID
    assert call(pts_=None) == rt.RT_ERR_INVALID
    assert call(hits_=None) == rt.RT_ERR_INVALID
    assert call(nodes_=None) == rt.RT_ERR_INVALID and call(tris_=None) == rt.RT_ERR_INVALID
    assert call(n_nodes=-1) == rt.RT_ERR_INVALID and call(n_tris=-1) == rt.RT_ERR_INVALID
    assert call(n=1 << 30, stride=8) == rt.RT_ERR_INVALID                                       # beyond 2^32 floats
    for link in (-1.0, 1e9, np.nan, float(nodes.shape[0]), 0.0):                                # no tree over the rows
        bad = nodes.copy()
        bad[0, 3] = link
        assert call(nodes_=bad) == rt.RT_ERR_INVALID, link
    leaf = ref.one_triangle()[0].copy()
    leaf[0, 9] = 3.0
    assert L.rt_nearest_points(p(leaf), 1, p(tris), 1, p(pts), 3, None, 8, p(hits), p(closest)) == rt.RT_ERR_INVALID
    assert (hits == f32(-7.5)).all() and (closest == f32(-7.5)).all()
    assert call(n=0, pts_=None, hits_=None) == rt.RT_OK and (hits == f32(-7.5)).all()            # n == 0: a no-op
    # no scene: every point a miss; closest may be null
    assert L.rt_nearest_points(None, 0, None, 0, p(pts), 3, None, 8, p(hits), None) == rt.RT_OK
    assert (hits[:, 0] == np.inf).all() and (hits.view(np.int32)[:, 1] == -1).all() and (closest == f32(-7.5)).all()
    # Python: refused before any call into the library
    with pytest.raises(rt.RtError, match="float32"):
        rt.nearest_points(nodes, tris, pts.astype(np.float64))
    with pytest.raises(rt.RtError, match=r"k >= 3"):
        rt.nearest_points(nodes, tris, pts[:, :2])
    with pytest.raises(rt.RtError, match="max_dist must be"):
        rt.nearest_points(nodes, tris, pts, md[:-1])
    bad = nodes.copy()
    bad[0, 3] = 1000.0
    with pytest.raises(rt.RtError, match="not a tree") as e:
        rt.nearest_points(bad, tris, pts)
    assert e.value.code == rt.RT_ERR_INVALID


def test_exports_signatures_and_null_contexts():
    L = rt.lib()
    for name in ("rt_nearest_points", "rt_query_nearest", "rt_query_nearest_host"):
        assert name in rt.SIGNATURES and hasattr(L, name), name
    for name in ("nearest_points", "NearestPoints"):
        assert hasattr(rt, name)
    assert callable(rt.Renderer.nearest_points)
    pts, hit = np.zeros((1, 3), f32), np.zeros((1, 4), f32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    for fn in (L.rt_query_nearest, L.rt_query_nearest_host):
        assert fn(None, p(pts), 3, None, 1, p(hit), None, None) == rt.RT_ERR_INVALID
    assert not hit.any()
