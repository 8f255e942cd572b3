"""The proximity query's host definition (rt_nearest_points_multi, rt.nearest_points_multi) against its numpy restatement
(nearest_multi_ref.py), bit for bit: every shared mesh and point set at K = 0, 1, 2, 3, 4, 8, 32 with and without max_dist, point layouts, NaN,
infinite and huge points, the limit exactly at the K-th winner's e and one ulp either side, the two consistency rules against rt.nearest_points, the
refusals, the block size of the device launch, and that the fixtures do hold the cases where a wrong cull or a wrong tie-break shows.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import nearest_multi_ref as mref
import nearest_ref as ref
import opengl_raytracing_amd as rt

f32 = np.float32
bits = ref.bits


def _same(got, want, what):
    hits, closest, count = want
    assert got.hits.shape == hits.shape and got.points.shape == closest.shape, what
    bad = np.flatnonzero((bits(got.hits) != bits(hits)).any((1, 2)))
    assert bad.size == 0, (what, bad[:8], got.hits[bad[:2]], hits[bad[:2]])
    bad = np.flatnonzero((bits(got.points) != bits(closest)).any((1, 2)))
    assert bad.size == 0, (what, bad[:8], got.points[bad[:2]], closest[bad[:2]])
    if got.count is not None:
        bad = np.flatnonzero(got.count != count)
        assert bad.size == 0, (what, bad[:8], got.count[bad[:8]], count[bad[:8]])


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("K", mref.KS)
@pytest.mark.parametrize("mesh", mref.MESHES)
def test_definition_equals_the_numpy_restatement(mesh, K, limited):
    nodes, tris, pts, _ = ref.case(mesh)
    md = mref.limit(mesh) if limited else None
    want = mref.reference(mesh, limited, K)
    got = rt.nearest_points_multi(nodes, tris, pts, K, md)
    _same(got, want, (mesh, K, limited))
    assert got.visits is None and len(got) == pts.shape[0] and got.count.dtype == np.int32
    assert got.hits.shape == (pts.shape[0], K, 4) and got.dist2.shape == got.prim.shape == (pts.shape[0], K) and got.uv.shape == (pts.shape[0], K, 2)
    miss = got.prim < 0
    assert np.array_equal(miss, np.arange(K)[None, :] >= got.count[:, None])                   # the first min(K, count) slots hold records, the rest misses
    assert (got.hits[miss, 0] == np.inf).all() and (bits(got.hits[miss][:, 2:]) == 0).all() and (bits(got.points[miss]) == 0).all()
    empty = ~np.isfinite(pts).all(1)
    if limited:
        empty[::97] = True
    assert (got.count[empty] == 0).all()
    if not limited:
        e = ref.reference(mesh, False)[2].e                                                   # no limit: every row whose e is no NaN is accepted
        assert np.array_equal(got.count[~empty], (~np.isnan(e)).sum(1)[~empty]) and (got.count[~empty] >= tris.shape[0] - 1).all()
    with np.errstate(invalid="ignore"):
        d = got.dist2
        assert (d[:, 1:] >= d[:, :-1]).all()                                                   # ascending, misses (+inf) last
        tie = (d[:, 1:] == d[:, :-1]) & ~miss[:, 1:]
        assert (got.prim[:, 1:][tie] > got.prim[:, :-1][tie]).all()                            # equal e: prim ascending


def test_point_layouts_and_strange_points_give_identical_bytes():
    nodes, tris, pts, _ = ref.case("bunny")
    md = mref.limit("bunny")
    want = mref.reference("bunny", True, 4)
    p4 = np.full((pts.shape[0], 4), np.nan, f32); p4[:, :3] = pts
    p8 = np.full((pts.shape[0], 8), 7.0, f32); p8[:, 2:5] = pts
    for name, p in (("[N,4]", p4), ("[N,8] interleaved", p8[:, 2:5]), ("[N,4] cut", p4[:, :3])):
        _same(rt.nearest_points_multi(nodes, tris, p, 4, md), want, name)
    one = rt.nearest_points_multi(nodes, tris, pts[5:6], 4, md[5:6])
    _same(one, tuple(a[5:6] for a in want), "one point")
    assert len(rt.nearest_points_multi(nodes, tris, pts[:0], 4)) == 0
    # NaN, infinite, huge and denormal coordinates, and limits of every kind (NaN: accepts nothing; +inf; huge; 0)
    sp = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-41, 3.0, 3e38, -3e38, 1e19], f32)
    strange = np.stack(np.meshgrid(sp, sp, sp, indexing="ij"), -1).reshape(-1, 3)
    lim = np.resize(np.array([np.nan, np.inf, 3e38, 0.0, 1e19, 2.0, -1.0, -np.inf], f32), strange.shape[0])
    for mesh in ("layers", "one_leaf"):
        nodes, tris = ref.mesh(mesh)
        table = ref.Table(nodes, tris, strange)
        for m in (None, lim):
            for K in (0, 2, 32):
                _same(rt.nearest_points_multi(nodes, tris, strange, K, m), mref.answer(tris, mref.Sorted(table, m), K), (mesh, K, m is not None))
        got = rt.nearest_points_multi(nodes, tris, strange, 2, lim)
        assert (got.count[np.isnan(lim)] == 0).all() and (got.count[~np.isfinite(strange).all(1)] == 0).all() and got.count.max() > 0
        assert not np.isnan(got.dist2).any()                                                   # a NaN e is never accepted


def _exact_layers():
    """Twelve large triangles in the planes y = 0, -1, ..., -11 and points 0.5 above the interior of the first: e of the k-th nearest row is
    (k - 0.5)^2 exactly, and max_dist = k - 0.5 squares to exactly that."""
    t9 = np.array([[-40, -k, -40, 120, 0, 0, 0, 0, 120] for k in range(12)], f32)
    nodes, tris = rt.build_bvh(t9)
    assert tris.shape[0] == 12 and nodes.shape[0] > 1
    pts = np.array([[1.0, 0.5, -2.0], [-3.0, 0.5, 0.5], [0.25, 0.5, 0.25]], f32)
    return nodes, tris, pts


@pytest.mark.parametrize("K", [1, 2, 3, 4, 8])
def test_the_limit_exactly_at_the_kth_winners_e_and_one_ulp_either_side(K):
    nodes, tris, pts = _exact_layers()
    table = ref.Table(nodes, tris, pts)
    free = rt.nearest_points_multi(nodes, tris, pts, K)
    assert (free.dist2 == ((np.arange(K) + 0.5) ** 2).astype(f32)[None, :]).all() and (free.count == 12).all()
    at = f32(K - 0.5)
    for md, count in ((at, K), (np.nextafter(at, f32(0)), K - 1), (np.nextafter(at, f32(99)), K)):
        m = np.full(3, md, f32)
        got = rt.nearest_points_multi(nodes, tris, pts, K, m)
        _same(got, mref.answer(tris, mref.Sorted(table, m), K), (K, md))
        assert (got.count == count).all(), (K, md, got.count)
        assert np.array_equal(bits(got.hits[:, :count]), bits(free.hits[:, :count])) and (got.prim[:, count:] == -1).all()
    nanlimit = rt.nearest_points_multi(nodes, tris, pts, K, np.full(3, np.nan, f32))            # a NaN limit accepts nothing
    assert (nanlimit.prim == -1).all() and (nanlimit.count == 0).all()
    assert (rt.nearest_points_multi(nodes, tris, pts, K, np.full(3, np.inf, f32)).count == 12).all()


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("mesh", mref.MESHES)
def test_the_two_consistency_rules(mesh, limited):
    """1: with K = 1 the records and points are rt.nearest_points' bit for bit.  2: count > 0 exactly where rt.nearest_points answers."""
    nodes, tris, pts, case_md = ref.case(mesh)
    for md in ((mref.limit(mesh), case_md) if limited else (None,)):                           # the fixed limit, and nearest_ref's own random limits
        one = rt.nearest_points(nodes, tris, pts, md)
        got = rt.nearest_points_multi(nodes, tris, pts, 1, md)
        assert np.array_equal(bits(got.hits[:, 0]), bits(one.hits)) and np.array_equal(bits(got.points[:, 0]), bits(one.points))
        assert np.array_equal(got.count > 0, one.prim >= 0)
        assert np.array_equal(rt.nearest_points_multi(nodes, tris, pts, 0, md).count, got.count)
        assert 0 < (got.count > 0).sum() < len(got)


def test_the_fixtures_hold_the_cases_where_a_wrong_cull_or_tie_break_shows():
    """Conditions on the fixtures, not measurements.  Counts that no limit can produce are left out, with the reason: K = 1 has no count between 0 and
    K; a mesh of T rows has no count above K >= T; every row of the layer stack has two coincident copies, so its counts there are multiples of 3."""
    for mesh in mref.MESHES:
        T = ref.mesh(mesh)[1].shape[0]
        count = mref.ordered(mesh, True).count
        for K in (1, 2, 3, 4, 8):
            more, fewer, none = int((count > K).sum()), int(((count > 0) & (count < K)).sum()), int((count == 0).sum())
            print(f"{mesh} K={K}: count > K at {more} points, 0 < count < K at {fewer}, count == 0 at {none}")
            assert none > 0
            assert more > 0 or T <= K, (mesh, K)
            assert fewer > 0 or K == 1 or (mesh == "layers" and K <= 3), (mesh, K)
    assert ((mref.ordered("layers", True).count % 3) == 0).all()
    # the layer stack: the K-th and (K+1)-th accepted rows have equal e, so prim alone decides who is kept
    for limited in (False, True):
        srt = mref.ordered("layers", limited)
        e = srt.table.e
        rows = np.arange(e.shape[0])
        for K in (1, 2, 4):
            ok = srt.count > K
            ties = int((e[rows, srt.order[:, K - 1]] == e[rows, srt.order[:, K]])[ok].sum())
            print(f"layers {'limited' if limited else 'unlimited'} K={K}: K-th and (K+1)-th rows tie in e at {ties} points")
            assert ties > 0
    # 21.2's clamp: a record among the winners whose e(t) != d2(t)
    clamped = {}
    for K in (1, 2, 4, 8, 32):
        n = 0
        for mesh in mref.MESHES:
            srt = mref.ordered(mesh, False)
            t = srt.table
            k = min(K, t.e.shape[1])
            rows = np.arange(t.e.shape[0])[:, None]
            raised = ((t.e != t.d2) & ~np.isnan(t.d2))[rows, srt.order[:, :k]] & (np.arange(k)[None, :] < srt.count[:, None])
            n += int(raised.any(1).sum())
        clamped[K] = n
    print(f"points with a clamped row among their K winners: {clamped}")
    assert all(v > 0 for v in clamped.values())


def test_block_size_of_the_device_launch():
    """Every legal (stack depth, K) gets 64, 128 or 256 threads whose LDS -- 8 bytes per stack entry and per record, per thread -- fits gfx950's
    160 KiB per workgroup, and 256 wherever 256 fit."""
    LDS = 160 << 10
    seen = set()
    for depth in range(1, 65):
        for K in range(0, 33):
            threads, lds = rt.nearest_multi_block(depth, K)
            assert threads in (64, 128, 256) and lds == threads * 8 * (depth + K) and lds <= LDS, (depth, K, threads, lds)
            assert threads == 256 or 256 * 8 * (depth + K) > LDS, (depth, K, threads)
            assert threads >= 128 or 128 * 8 * (depth + K) > LDS, (depth, K, threads)
            seen.add(threads)
    assert rt.nearest_multi_block(64, 32) == (128, 98304) and rt.nearest_multi_block(64, 16) == (256, 163840) and seen == {128, 256}
    for bad in ((0, 4), (65, 4), (8, -1), (8, 33)):
        with pytest.raises(rt.RtError):
            rt.nearest_multi_block(*bad)


def test_refusals_write_nothing():
    L = rt.lib()
    nodes, tris, pts, md = ref.case("layers")
    pts, md = np.ascontiguousarray(pts[:8]), np.abs(md[:8])
    K = 4
    hits, closest, counts = np.full((8, K, 4), f32(-7.5), f32), np.full((8, K, 3), f32(-7.5), f32), np.full(8, -77, np.int32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(nodes_=nodes, tris_=tris, n_nodes=None, n_tris=None, pts_=pts, stride=3, n=8, k=K, hits_=hits, counts_=counts):
        return L.rt_nearest_points_multi(p(nodes_), nodes.shape[0] if n_nodes is None else n_nodes, p(tris_), tris.shape[0] if n_tris is None else n_tris,
                                         p(pts_), stride, p(md), n, k, p(hits_), p(counts_), p(closest))

    assert call(k=-1) == rt.RT_ERR_INVALID and call(k=rt.RT_NEAREST_MULTI_MAX + 1) == rt.RT_ERR_INVALID
    assert call(k=0, counts_=None) == rt.RT_ERR_INVALID                                         # K = 0 without counts
    assert call(n=(1 << 31) // K + 1) == rt.RT_ERR_INVALID                                      # n * K beyond INT32_MAX
    assert call(n=-1) == rt.RT_ERR_INVALID
    assert call(stride=2) == rt.RT_ERR_INVALID
    assert call(pts_=None) == rt.RT_ERR_INVALID
    assert call(hits_=None) == rt.RT_ERR_INVALID
    assert call(nodes_=None) == rt.RT_ERR_INVALID and call(tris_=None) == rt.RT_ERR_INVALID
    assert call(n_nodes=-1) == rt.RT_ERR_INVALID and call(n_tris=-1) == rt.RT_ERR_INVALID
    assert call(n=1 << 28, stride=32, k=1) == rt.RT_ERR_INVALID                                 # beyond 2^32 floats
    for link in (-1.0, 1e9, np.nan, float(nodes.shape[0]), 0.0):                                # no tree over the rows
        bad = nodes.copy()
        bad[0, 3] = link
        assert call(nodes_=bad) == rt.RT_ERR_INVALID, link
    assert (hits == f32(-7.5)).all() and (closest == f32(-7.5)).all() and (counts == -77).all()
    assert call(n=0, pts_=None, hits_=None, counts_=None) == rt.RT_OK and (hits == f32(-7.5)).all()          # n == 0: a no-op
    # K = 0 with counts: the counts alone, hits may be null
    assert call(k=0, hits_=None) == rt.RT_OK and (counts >= 0).all() and (hits == f32(-7.5)).all() and (closest == f32(-7.5)).all()
    assert np.array_equal(counts, rt.nearest_points_multi(nodes, tris, pts, 0, md).count)
    # no scene: every slot a miss, every count 0; counts and closest may be null
    assert L.rt_nearest_points_multi(None, 0, None, 0, p(pts), 3, None, 8, K, p(hits), None, None) == rt.RT_OK
    assert (hits[:, :, 0] == np.inf).all() and (hits.view(np.int32)[:, :, 1] == -1).all() and (closest == f32(-7.5)).all()
    # Python: refused before any call into the library
    with pytest.raises(rt.RtError, match="float32"):
        rt.nearest_points_multi(nodes, tris, pts.astype(np.float64), 2)
    with pytest.raises(rt.RtError, match=r"k >= 3"):
        rt.nearest_points_multi(nodes, tris, pts[:, :2], 2)
    with pytest.raises(rt.RtError, match="max_dist must be"):
        rt.nearest_points_multi(nodes, tris, pts, 2, md[:-1])
    with pytest.raises(rt.RtError, match="max_hits = 33"):
        rt.nearest_points_multi(nodes, tris, pts, 33)
    bad = nodes.copy()
    bad[0, 3] = 1000.0
    with pytest.raises(rt.RtError, match="not a tree") as e:
        rt.nearest_points_multi(bad, tris, pts, 2)
    assert e.value.code == rt.RT_ERR_INVALID


def test_exports_signatures_and_null_contexts():
    L = rt.lib()
    for name in ("rt_nearest_points_multi", "rt_query_nearest_multi", "rt_query_nearest_multi_host", "rt_debug_nearest_multi_block"):
        assert name in rt.SIGNATURES and hasattr(L, name), name
    for name in ("nearest_points_multi", "NearestMulti", "nearest_multi_block"):
        assert hasattr(rt, name)
    assert callable(rt.Renderer.nearest_points_multi) and rt.RT_NEAREST_MULTI_MAX == 32
    pts, hit, cnt = np.zeros((1, 3), f32), np.zeros((1, 4), f32), np.zeros(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    for fn in (L.rt_query_nearest_multi, L.rt_query_nearest_multi_host):
        assert fn(None, p(pts), 3, None, 1, 1, p(hit), p(cnt), None, None) == rt.RT_ERR_INVALID
    assert not hit.any() and not cnt.any()
