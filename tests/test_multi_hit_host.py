"""Multi-hit queries, host side (no GPU): rt_multi_hits -- the definition -- against the plain-Python restatement over the oracle's
aabbHit / triHit (tests/multi_hit_ref.py), bit for bit on hits and counts; the conditions that make the comparison mean something (the walk is what
is matched, not brute force; overflowing K-buffers; equal-t pairs; triangles in front of their leaf's slab entry); the invariants that tie the
query to traceBVHShadow and traceBVH; tMax at a hit's t and one ulp either side; eps = 0; NaN and infinite rays; every refusal; the exports."""
import ctypes as C

import numpy as np
import pytest

import multi_hit_ref as ref
import opengl_raytracing_amd as rt
import scenes

f32 = np.float32
bits = ref.bits
LAYER_STRIDE = 10   # of the 3 000 layer rays: the first 300 all go straight down (none has a hit in front of its leaf's slab entry); every 10th mixes both kinds


def _same(got, lists, tris, o, d, K, what, inf=1e30):
    wh, wc = ref.answer(lists, tris, o, d, K, inf)
    assert np.array_equal(got.count, wc), (what, K, np.flatnonzero(got.count != wc)[:8])
    bad = np.flatnonzero((bits(got.hits) != bits(wh)).reshape(len(lists), -1).any(1))
    assert bad.size == 0, (what, K, bad[:8], got.hits[bad[:1]], wh[bad[:1]])
    assert got.hits.shape == (len(lists), K, 4) and got.hits.dtype == f32 and got.count.dtype == np.int32


# ---------------------------------------------------------------- 1: the definition against the restatement, three meshes

@pytest.fixture(scope="module")
def bunny():
    nodes, tris, o, d, tm = ref.bunny_rays()
    return nodes, tris, o, d, tm, ref.all_hits(nodes, tris, o, d), ref.all_hits(nodes, tris, o, d, tm)


@pytest.fixture(scope="module")
def layers():
    nodes, tris = ref.layer_stack()
    o, d = ref.layer_rays()
    o, d = np.ascontiguousarray(o[::LAYER_STRIDE]), np.ascontiguousarray(d[::LAYER_STRIDE])
    return nodes, tris, o, d, ref.all_hits(nodes, tris, o, d)


@pytest.mark.parametrize("K", [0, 1, 2, 4, 32])
def test_one_leaf_matches_the_restatement(K):
    nodes, tris, o, d, tm = ref.one_leaf_rays()
    _same(rt.multi_hits(nodes, tris, o, d, max_hits=K), ref.all_hits(nodes, tris, o, d), tris, o, d, K, "one_leaf")
    with_tm = ref.all_hits(nodes, tris, o, d, tm)
    assert max(len(l) for l in with_tm) >= 1 and not with_tm[0] and not with_tm[97]
    _same(rt.multi_hits(nodes, tris, o, d, tm, max_hits=K), with_tm, tris, o, d, K, "one_leaf tmax")


@pytest.mark.parametrize("K", [0, 1, 2, 4, 32])
def test_bunny_adversarial_rays_match_the_restatement(bunny, K):
    nodes, tris, o, d, tm, free, bounded = bunny
    _same(rt.multi_hits(nodes, tris, o, d, max_hits=K), free, tris, o, d, K, "bunny")
    _same(rt.multi_hits(nodes, tris, o, d, tm, max_hits=K), bounded, tris, o, d, K, "bunny tmax")
    got = rt.multi_hits(nodes, tris, o, d, tm, max_hits=K)
    assert not got.count[::97].any() and (got.hits.view(np.int32)[::97, :, 1] == -1).all()      # the empty slots


def test_bunny_rays_are_the_hard_ones(bunny):
    """The conditions of the comparison above: the walk differs from brute force, K-buffers overflow, equal-t pairs exist."""
    nodes, tris, o, d, tm, free, _ = bunny
    counts = np.array([len(l) for l in free])
    assert (counts > 2).sum() >= 5 and (counts > 1).sum() >= 100 and counts.max() >= 5
    ties = sum(any(bits(l[j][0]) == bits(l[j + 1][0]) for j in range(len(l) - 1)) for l in free)
    assert ties >= 3
    # brute force over all triangles accepts more than the walk on axis-parallel rays lying in box planes and on corner grazes (rays 150 .. 899)
    sel = np.arange(150, 900)
    more = sum(len(b) > len(free[i]) for i, b in zip(sel, ref.brute(tris, o[sel], d[sel], f32(1e30), 1e-4)))
    assert more >= 50, more
    got = rt.multi_hits(nodes, tris, o, d, max_hits=0)
    assert np.array_equal(got.count, counts)                # ... and the walk is what is matched


@pytest.mark.parametrize("K", [1, 2, 4, 17, 18, 19, 32])
def test_layer_stack_matches_the_restatement(layers, K):
    nodes, tris, o, d, lists = layers
    got = rt.multi_hits(nodes, tris, o, d, max_hits=K)
    _same(got, lists, tris, o, d, K, "layers")
    # ties come out in ascending prim
    t, prim = bits(got.t).astype(np.int64), got.prim.astype(np.int64)
    valid = prim[:, 1:] >= 0
    tie = valid & (t[:, 1:] == t[:, :-1])
    assert (prim[:, 1:] > prim[:, :-1])[tie].all()
    if K > 1:
        assert tie.any(1).all()                             # every ray has equal-t pairs
    assert (ref.key(got.t[:, 1:])[valid] >= ref.key(got.t[:, :-1])[valid]).all()


def test_layer_rays_hit_in_front_of_their_leaf(layers):
    """Distance culling against a found hit is not exact: accepted triangles whose leaf's slab entry exceeds their own t."""
    nodes, tris, o, d, lists = layers
    counts = np.array([len(l) for l in lists])
    assert set(np.unique(counts)) <= {18, 36} and (counts == 18).sum() >= 250
    flush = sum(any(f[2] > f[0] for f in l) for l in lists)
    assert flush >= 20, flush


# ---------------------------------------------------------------- 2: the invariants that tie it to what exists

@pytest.mark.parametrize("subdiv,n", [(2, 150), (3, 300)])
def test_invariants_against_the_oracles_walks(orc, subdiv, n):
    nodes, tris, o, d, tm = ref.bunny_rays(subdiv, n)
    u = rt.frame_uniforms(rt.default_render_params(), rt.default_camera(), 64, 64, 0, True, nodes.shape[0], tris.shape[0])
    free = rt.multi_hits(nodes, tris, o, d, max_hits=1, eps=u.eps, inf=u.inf)
    bounded = rt.multi_hits(nodes, tris, o, d, tm, max_hits=0, eps=u.eps, inf=u.inf)
    for i in range(o.shape[0]):
        occ = tm[i] >= 0 and orc.trace_bvh_shadow(u, nodes, tris, o[i], d[i], tm[i])
        assert (bounded.count[i] > 0) == occ, i                                   # the same walk
        prim, t = orc.trace_bvh_prim(u, nodes, tris, o[i], d[i])
        assert (free.count[i] > 0) == (prim >= 0), i
        if prim >= 0:
            assert ref.key(free.t[i, 0]) <= ref.key(f32(t)), i                       # the closest answer is an element of S


# ---------------------------------------------------------------- 3: limits, eps, degenerate rays

def test_tmax_at_a_hit_and_one_ulp_either_side(bunny, layers):
    for name, (nodes, tris, o, d, lists) in (("bunny", bunny[:4] + (bunny[5],)), ("layers", layers)):
        rays = [i for i, l in enumerate(lists) if len(l) >= 2][:24]
        assert len(rays) >= 10
        O, D, TM = [], [], []
        for i in rays:
            for j in sorted({0, 1, len(lists[i]) - 1}):
                t = lists[i][j][0]
                for tm in (t, np.nextafter(t, f32(-np.inf)), np.nextafter(t, f32(np.inf))):
                    O.append(o[i]); D.append(d[i]); TM.append(tm)
        O, D, TM = np.array(O, f32), np.array(D, f32), np.array(TM, f32)
        want = ref.all_hits(nodes, tris, O, D, TM)
        for K in (0, 2, 32):
            _same(rt.multi_hits(nodes, tris, O, D, TM, max_hits=K), want, tris, O, D, K, name)
        assert len({len(w) for w in want}) > 2              # the limit bites


def test_eps_zero(bunny):
    nodes, tris, o, d = bunny[:4]
    sel = np.arange(600, 750)                               # rays that start on triangle vertices and edge midpoints
    o, d = np.ascontiguousarray(o[sel]), np.ascontiguousarray(d[sel])
    zero = ref.all_hits(nodes, tris, o, d, eps=0.0)
    _same(rt.multi_hits(nodes, tris, o, d, max_hits=4, eps=0.0), zero, tris, o, d, 4, "eps 0")
    assert sum(len(l) for l in zero) > sum(len(l) for l in bunny[5][600:750])      # the hits at the start count now


def _sentinel_call(nodes, tris, o, d, tm, K, eps=1e-4, inf=1e30):
    """rt_multi_hits straight through ctypes on outputs filled with a sentinel -> (hits, counts, rc)."""
    n = o.shape[0]
    hits, counts = np.full((n, K, 4), f32(-7.5), f32), np.full(n, -77, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    rc = rt.lib().rt_multi_hits(p(nodes), nodes.shape[0], p(tris), tris.shape[0], p(o), o.strides[0] // 4, p(d), d.strides[0] // 4, p(tm), eps, inf, n, K,
                                p(hits), p(counts))
    return hits, counts, rc


def test_nan_and_infinite_rays_answer_what_the_restatement_says(bunny):
    nodes, tris, o, d, tm = bunny[:5]
    rng = np.random.default_rng(3)
    sel = rng.choice(o.shape[0], 96, replace=False)
    O, D, TM = o[sel].copy(), d[sel].copy(), np.abs(tm[sel]).copy()
    special = [f32(np.nan), f32(np.inf), f32(-np.inf), f32(0.0), f32(-0.0)]
    for k in range(96):
        which = (O, D, O, D, TM, D)[k % 6]
        if which is TM:
            TM[k] = special[(k // 6) % 3]
        else:
            which[k, rng.integers(0, 3)] = special[(k // 6) % 5]
            if k % 12 >= 6:
                which[k, rng.integers(0, 3)] = special[(k // 12) % 5]
    want = ref.all_hits(nodes, tris, O, D, TM)
    for K in (1, 4):
        hits, counts, rc = _sentinel_call(nodes, tris, O, D, TM, K)
        assert rc == rt.RT_OK
        wh, wc = ref.answer(want, tris, O, D, K)
        assert np.array_equal(counts, wc)
        assert np.array_equal(bits(hits[:, :, 0:2]), bits(wh[:, :, 0:2]))          # t and prim, NaN t included
        # u, v: the bits, or a NaN on both sides (which NaN an operation hands on is no part of the float model)
        assert (np.equal(bits(hits[:, :, 2:4]), bits(wh[:, :, 2:4])) | (np.isnan(hits[:, :, 2:4]) & np.isnan(wh[:, :, 2:4]))).all()
        assert not (hits == f32(-7.5)).all(2).any()         # no slot is left unwritten


# ---------------------------------------------------------------- 4: refusals, exports

def test_every_refusal_of_the_definition_leaves_the_outputs_alone():
    nodes, tris, o, d, tm = ref.one_leaf_rays()
    L = rt.lib()
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    hits, counts = np.full((o.shape[0], 4, 4), f32(-7.5), f32), np.full(o.shape[0], -77, np.int32)

    def call(nodes=nodes, nn=None, tris=tris, nt=None, o=o, os_=3, d=d, ds=3, n=o.shape[0], K=4, hits=hits, counts=counts):
        return L.rt_multi_hits(p(nodes), nodes.shape[0] if nn is None else nn, p(tris), tris.shape[0] if nt is None else nt, p(o), os_, p(d), ds, None, 1e-4, 1e30,
                               n, K, p(hits), p(counts))

    assert call(K=-1) == rt.RT_ERR_INVALID and call(K=rt.RT_MULTI_HIT_MAX + 1) == rt.RT_ERR_INVALID
    assert call(n=-1) == rt.RT_ERR_INVALID
    assert call(os_=2) == rt.RT_ERR_INVALID and call(ds=2) == rt.RT_ERR_INVALID
    assert call(o=None) == rt.RT_ERR_INVALID and call(d=None) == rt.RT_ERR_INVALID
    assert call(hits=None) == rt.RT_ERR_INVALID and call(K=0, counts=None) == rt.RT_ERR_INVALID
    assert call(n=1 << 27, K=32) == rt.RT_ERR_INVALID                              # n * maxHits beyond INT32_MAX, refused before a ray is read
    assert call(nn=-1) == rt.RT_ERR_INVALID and call(nt=-1) == rt.RT_ERR_INVALID
    bn, bt = scenes.bunny_bvh(2)
    for edit in ((0, 3, 1000.0), (0, 7, 0.0), (1, 3, 0.0)):                       # a child off the array, a node that is its own child, a cycle
        bad = bn.copy()
        inner = np.flatnonzero(bad[:, 9] == 0)
        bad[inner[edit[0]], edit[1]] = edit[2]
        assert call(nodes=bad, tris=bt) == rt.RT_ERR_INVALID
    bad = bn.copy()
    leaf = np.flatnonzero(bad[:, 9] > 0)[-1]
    bad[leaf, 8] = bt.shape[0] - 1
    bad[leaf, 9] = 2                                                               # a range that ends beyond the rows
    assert call(nodes=bad, tris=bt) == rt.RT_ERR_INVALID
    assert (hits == f32(-7.5)).all() and (counts == -77).all()
    assert call(n=0, o=None, d=None, hits=None, counts=None) == rt.RT_OK           # n == 0 is a no-op
    assert call(hits=hits, counts=None) == rt.RT_OK and not (hits == f32(-7.5)).all(2).any()
    # an empty scene has no occluders: every count 0
    h2, c2, rc = _sentinel_call(nodes[:0], tris[:0], o, d, None, 2)
    assert rc == rt.RT_OK and not c2.any() and (h2.view(np.int32)[:, :, 1] == -1).all() and (h2[:, :, 0] == f32(1e30)).all()


def test_python_refusals_carry_their_text():
    nodes, tris, o, d, tm = ref.one_leaf_rays()
    for bad in (-1, 33):
        with pytest.raises(rt.RtError, match="max_hits = .* RT_MULTI_HIT_MAX = 32") as e:
            rt.multi_hits(nodes, tris, o, d, max_hits=bad)
        assert e.value.code == rt.RT_ERR_INVALID
    with pytest.raises(rt.RtError, match="float32"):
        rt.multi_hits(nodes, tris, o.astype(np.float64), d)
    with pytest.raises(rt.RtError, match=r"k >= 3"):
        rt.multi_hits(nodes, tris, o[:, :2], d)
    with pytest.raises(rt.RtError, match="rows"):
        rt.multi_hits(nodes, tris, o, d[:-1])
    with pytest.raises(rt.RtError, match="tmax must be"):
        rt.multi_hits(nodes, tris, o, d, tm[:-1])
    bad = scenes.bunny_bvh(2)[0].copy()
    bad[0, 3] = 1000.0
    with pytest.raises(rt.RtError, match="not a tree") as e:
        rt.multi_hits(bad, scenes.bunny_bvh(2)[1], o, d)
    assert e.value.code == rt.RT_ERR_INVALID


def test_ray_layouts_give_identical_bytes():
    nodes, tris, o, d, tm = ref.bunny_rays()
    want = rt.multi_hits(nodes, tris, o, d, tm, max_hits=4)
    o4, d4 = np.zeros((o.shape[0], 4), f32), np.full((o.shape[0], 4), f32(np.nan))
    o4[:, :3], d4[:, :3] = o, d
    both = np.concatenate([o4, d4], 1)
    for oo, dd in ((o4, d4), (both[:, 0:4], both[:, 4:8]), (both[:, 0:3], both[:, 4:7])):
        got = rt.multi_hits(nodes, tris, oo, dd, tm, max_hits=4)
        assert np.array_equal(bits(got.hits), bits(want.hits)) and np.array_equal(got.count, want.count)


def test_exports_signatures_and_null_contexts():
    L = rt.lib()
    names = ("rt_multi_hits", "rt_trace_rays_multi", "rt_trace_rays_multi_host", "rt_pick_pixels_multi", "rt_pick_pixels_multi_host")
    for name in names:
        assert name in rt.SIGNATURES and hasattr(L, name), name
    assert rt.RT_MULTI_HIT_MAX == 32
    for name in ("multi_hits", "MultiHits"):
        assert hasattr(rt, name)
    for name in ("trace_rays_multi", "pick_multi"):
        assert callable(getattr(rt.Renderer, name))
    o = np.zeros((1, 3), f32)
    hit, cnt = np.zeros((1, 4), f32), np.zeros(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    u = rt.RtUniforms()
    xy = np.zeros((1, 2), np.int32)
    for fn in (L.rt_trace_rays_multi, L.rt_trace_rays_multi_host):
        assert fn(None, p(o), 3, p(o), 3, None, 1e-4, 1e30, 1, 1, p(hit), p(cnt)) == rt.RT_ERR_INVALID
    for fn in (L.rt_pick_pixels_multi, L.rt_pick_pixels_multi_host):
        assert fn(None, C.byref(u), p(xy), 1, 1, p(hit), p(cnt)) == rt.RT_ERR_INVALID
    assert not hit.any() and not cnt.any()
