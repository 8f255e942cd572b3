"""The triangle query's definition on the host (rt_tri_overlaps), no GPU: rt.tri_overlaps against the numpy float32 restatement
(tri_query_ref.py) bit for bit -- counts and lists, exact CSR slots and fixed capacities, strided and [N,3,3] queries, counts alone and lists alone --,
the entries no list reaches left as they were, every refusal writing nothing, the properties of library-built trees (the path mask removes nothing,
every list ascends), the shared-point property, walk order on a hand-made tree with its children swapped, what the fixtures must hold for a wrong
test to show, and the float64 test."""
import ctypes as C

import numpy as np
import pytest

import opengl_raytracing_amd as rt
import tri_query_ref as ref

f32 = np.float32
SENTINEL = -77
CAPS = (0, 1, 3, 8)


def _raw(nodes, tris, qtris, stride, n, offsets, cap, prims, counts):
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    return rt.lib().rt_tri_overlaps(p(nodes), nodes.shape[0], p(tris), tris.shape[0], p(qtris), stride, n, p(offsets), cap, p(prims), p(counts))


def _lists_of(got):
    return [got.prims[got.offsets[i]:got.offsets[i] + min(got.count[i], got.offsets[i + 1] - got.offsets[i])] for i in range(len(got))]


# ---------------------------------------------------------------- 1: against the numpy definition

@pytest.mark.parametrize("mesh", ref.MESHES)
def test_counts_and_lists_equal_the_numpy_definition(mesh):
    nodes, tris, q = ref.case(mesh)
    want = ref.reference(mesh)
    assert q.shape[0] >= 2049
    got = rt.tri_overlaps(nodes, tris, q)
    bad = np.flatnonzero(got.count != want.count)
    assert bad.size == 0, (mesh, bad[:8], got.count[bad[:8]], want.count[bad[:8]], q[bad[:2]])
    assert isinstance(got, rt.TriOverlaps) and np.array_equal(got.offsets, want.offsets()) and got.prims.dtype == np.int32
    assert np.array_equal(got.prims, want.filled(want.offsets())), mesh
    pairs = got.pairs()
    assert pairs.dtype == np.int32 and np.array_equal(pairs, want.pairs())
    for cap in CAPS:
        got = rt.tri_overlaps(nodes, tris, q, cap=cap)
        assert np.array_equal(got.count, want.count) and np.array_equal(got.offsets, np.arange(q.shape[0] + 1) * cap)
        assert np.array_equal(got.prims, want.filled(cap=cap, sentinel=-1)), (mesh, cap)
        kept = got.pairs()                                             # the written entries alone: the first min(cap, count) of every list
        assert np.array_equal(kept, np.array([(i, t) for i, rows in enumerate(want.lists) for t in rows[:cap]], np.int32).reshape(-1, 2))
    hits = rt.tri_overlaps(nodes, tris, q[:65], cap=3).hits()
    assert hits.shape == (195, 4) and np.array_equal(hits.view(np.int32)[:, 1], want.filled(cap=3, sentinel=-1)[:195])
    assert (hits[:, 0] == 0).all() and (hits[:, 2:4] == f32(1) / f32(3)).all()
    assert np.array_equal(rt.rows_as_tris(tris), ref.rows_as_tris(tris)) and rt.rows_as_tris(tris).dtype == f32


@pytest.mark.parametrize("stride", [9, 10, 12])
def test_strided_queries_counts_alone_lists_alone_and_sentinels(stride):
    nodes, tris, q = ref.case("bunny")
    want = ref.reference("bunny")
    N = q.shape[0]
    wide = np.full((N, stride), np.nan, f32)
    wide[:, :9] = q
    flat = np.ascontiguousarray(wide.reshape(-1)[:(N - 1) * stride + 9])          # exactly as long as a call may read
    view = np.lib.stride_tricks.as_strided(flat, (N, 9), (4 * stride, 4))
    got = rt.tri_overlaps(nodes, tris, view)
    assert np.array_equal(got.count, want.count) and np.array_equal(got.prims, want.filled(want.offsets()))
    if stride == 9:
        got = rt.tri_overlaps(nodes, tris, flat.reshape(N, 3, 3))                 # [N,3,3]
    else:
        got = rt.tri_overlaps(nodes, tris, np.lib.stride_tricks.as_strided(flat, (N, 3, 3), (4 * stride, 12, 4)))
    assert np.array_equal(got.count, want.count) and np.array_equal(got.prims, want.filled(want.offsets()))
    # counts alone
    counts = np.full(N, SENTINEL, np.int32)
    assert _raw(nodes, tris, flat, stride, N, None, 0, None, counts) == rt.RT_OK and np.array_equal(counts, want.count)
    # lists alone: exact slots with a guard word behind the last, slots one short, and fixed capacities
    off = want.offsets()
    prims = np.full(off[-1] + 1, SENTINEL, np.int32)
    assert _raw(nodes, tris, flat, stride, N, off, 0, prims, None) == rt.RT_OK
    assert np.array_equal(prims[:-1], want.filled(off)) and prims[-1] == SENTINEL
    short = np.concatenate([[0], np.cumsum(np.maximum(want.count - 1, 0))]).astype(np.int32)
    prims = np.full(short[-1], SENTINEL, np.int32)
    counts[:] = SENTINEL
    assert _raw(nodes, tris, flat, stride, N, short, 0, prims, counts) == rt.RT_OK
    assert np.array_equal(prims, want.filled(short)) and np.array_equal(counts, want.count)
    for cap in CAPS:
        prims = np.full(N * cap, SENTINEL, np.int32)
        assert _raw(nodes, tris, flat, stride, N, None, cap, prims if cap else np.zeros(1, np.int32), None) == rt.RT_OK
        filled = want.filled(cap=cap, sentinel=SENTINEL)
        assert np.array_equal(prims, filled), cap
        if cap:
            assert (filled == SENTINEL).any() and ((prims == SENTINEL) == (np.arange(N * cap) % cap >= np.repeat(want.count, cap))).all()
    # a slot of negative length, and one with a negative start, hold nothing
    odd = np.array([3, 1, 1, -5, 2, 2], np.int32)
    prims = np.full(8, SENTINEL, np.int32)
    counts = np.full(5, SENTINEL, np.int32)
    assert _raw(nodes, tris, flat, stride, 5, odd, 0, prims, counts) == rt.RT_OK
    assert np.array_equal(counts, want.count[:5]) and (prims == SENTINEL).all()


def test_every_refusal_writes_nothing():
    nodes, tris, q = ref.case("layers")
    q = np.array(q[:4])
    prims, counts = np.full(32, SENTINEL, np.int32), np.full(4, SENTINEL, np.int32)
    off = np.array([0, 8, 16, 24, 32], np.int32)
    ok = dict(nodes=nodes, tris=tris, qtris=q, stride=9, n=4, offsets=off, cap=0, prims=prims, counts=counts)
    call = lambda **kw: _raw(**dict(ok, **kw))
    assert call(n=-1) == rt.RT_ERR_INVALID
    assert call(stride=8) == rt.RT_ERR_INVALID
    assert call(qtris=None) == rt.RT_ERR_INVALID
    assert call(prims=None, counts=None) == rt.RT_ERR_INVALID
    assert call(offsets=None, cap=-1) == rt.RT_ERR_INVALID
    assert call(offsets=None, cap=(1 << 31) // 4 + 1) == rt.RT_ERR_INVALID                   # n * cap beyond INT32_MAX
    for link in (-1.0, 1e9, np.nan, float(nodes.shape[0]), 0.0):                             # nodes that are no tree over the rows
        bad = nodes.copy()
        bad[0, 3] = link
        assert call(nodes=bad) == rt.RT_ERR_INVALID, link
    bad = nodes.copy()
    leaf = [k for k in range(nodes.shape[0]) if nodes[k, 9] > 0][0]
    bad[leaf, 8] = 2e9
    assert call(nodes=bad) == rt.RT_ERR_INVALID
    assert (prims == SENTINEL).all() and (counts == SENTINEL).all()
    assert _raw(nodes, tris, None, 9, 0, None, 0, None, None) == rt.RT_OK                     # n == 0: a no-op
    assert call() == rt.RT_OK and (counts != SENTINEL).all()
    for bad_call in (lambda: rt.tri_overlaps(nodes, tris, q[:, :8]), lambda: rt.tri_overlaps(nodes, tris, q.astype(np.float64)),
                     lambda: rt.tri_overlaps(nodes, tris, q, cap=-1), lambda: rt.tri_overlaps(nodes, tris, list(q)),
                     lambda: rt.tri_overlaps(nodes, tris, q.reshape(4, 3, 3).transpose(0, 2, 1)), lambda: rt.tri_overlaps(nodes, tris, q.reshape(2, 2, 9))):
        with pytest.raises(rt.RtError) as e:
            bad_call()
        assert e.value.code == rt.RT_ERR_INVALID
    empty = rt.tri_overlaps(nodes, tris, q[:0])
    assert len(empty) == 0 and empty.prims.size == 0 and np.array_equal(empty.offsets, [0]) and empty.pairs().shape == (0, 2)


# ---------------------------------------------------------------- 2: the properties of library-built trees, the shared point, and walk order

@pytest.mark.parametrize("mesh", ref.MESHES)
def test_the_path_mask_removes_nothing_and_every_list_ascends(mesh):
    """Node boxes are the float min / max of exactly a, b, c of their rows, the box axes of the triangle test compare the same values with the same
    [qlo, qhi] and comparisons do not round: a row the triangle test accepts lies under overlapping boxes all the way up.  And the right-first walk
    of rt_build_bvh's trees meets the rows in ascending order."""
    want = ref.reference(mesh)
    assert not (want.sat.accept & ~want.walk.path).any()
    assert np.array_equal(want.walk.order, np.arange(want.walk.order.size))
    assert all((np.diff(rows) > 0).all() for rows in want.lists)


@pytest.mark.parametrize("mesh", ref.MESHES)
def test_a_pair_that_shares_a_point_is_accepted_and_a_self_query_lists_its_row(mesh):
    """Derived from 24.1, not from the code: if a query point equals one of the row's a, b, c in all three floats, then on every projected axis the
    same dot on the same operands yields the same float, which lies in both intervals, and on the box axes the comparisons are exact -- no axis
    separates.  It holds for b and c as for a, since all three row points are projected on every axis."""
    nodes, tris, q = ref.case(mesh)
    want = ref.reference(mesh)
    a, b, c = ref.row_points(tris)
    shares = np.zeros((q.shape[0], tris.shape[0]), bool)
    per_point = []
    for v in (a, b, c):
        hit = np.zeros_like(shares)
        for k in (0, 3, 6):
            hit |= (q[:, None, k:k + 3] == v[None]).all(-1)
        per_point.append(int((hit & want.sat.live[:, None]).sum()))
        shares |= hit
    shares &= want.sat.live[:, None]
    print(mesh, "pairs sharing a point with a, b, c:", per_point)
    assert min(per_point) > 0 and not (shares & ~want.accepted).any()
    own = ref.rows_as_tris(tris)
    self_pairs = (q[:, None, :] == own[None]).all(-1)                                    # query i is row t's own a, b, c
    assert self_pairs.sum() >= min(tris.shape[0], 250) * 9 // 10 and want.accepted[self_pairs].all()   # (every 97th query became an empty slot)
    got = rt.tri_overlaps(nodes, tris, own)                                              # ... and through the library, every row
    assert all(t in rows for t, rows in enumerate(_lists_of(got)))


def test_a_tree_with_swapped_children_lists_in_walk_order():
    """Three nodes by hand: the root's LEFT child holds rows 0, 1, its RIGHT child rows 2, 3.  The walk takes the right child first: 2, 3, 0, 1.  With
    the children swapped in the root's links it is 0, 1, 2, 3.  Row x spans (x, 0, 0), (x + 0.5, 0, 0), (x, 0.5, 0.25); the queries lie in the plane
    y = 0.1, which cuts row x along z = 0.05 from x to x + 0.4."""
    t9 = np.array([[x, 0, 0, 0.5, 0, 0, 0, 0.5, 0.25] for x in (0.0, 1.0, 2.0, 3.0)], f32)
    tris = np.zeros((4, 12), f32)
    tris[:, 0:3], tris[:, 4:7], tris[:, 8:11] = t9[:, 0:3], t9[:, 3:6], t9[:, 6:9]

    def box(rows):
        v = np.concatenate([tris[rows, 0:3], tris[rows, 0:3] + tris[rows, 4:7], tris[rows, 0:3] + tris[rows, 8:11]])
        return v.min(0), v.max(0)

    nodes = np.zeros((3, 12), f32)
    for k, rows in enumerate(([0, 1, 2, 3], [0, 1], [2, 3])):
        nodes[k, 0:3], nodes[k, 4:7] = box(rows)
    nodes[0, 3], nodes[0, 7] = 1, 2
    nodes[1, 8], nodes[1, 9] = 0, 2
    nodes[2, 8], nodes[2, 9] = 2, 2
    q = np.array([[-1, 0.1, -1, 5, 0.1, -1, 2, 0.1, 5], [0.9, 0.1, -1, 2.6, 0.1, -1, 1.75, 0.1, 3], [2.6, 0, 0, 2.6, 0, 0, 2.6, 0, 0]], f32)
    got = rt.tri_overlaps(nodes, tris, q)
    want = ref.Answer(nodes, tris, q)
    assert [list(r) for r in _lists_of(got)] == [[2, 3, 0, 1], [2, 1], []] and [list(r) for r in want.lists] == [[2, 3, 0, 1], [2, 1], []]
    assert list(want.visits) == [3, 3, 3]
    assert np.array_equal(got.pairs(), [[0, 2], [0, 3], [0, 0], [0, 1], [1, 2], [1, 1]])
    nodes[0, 3], nodes[0, 7] = 2, 1
    got = rt.tri_overlaps(nodes, tris, q)
    assert [list(r) for r in _lists_of(got)] == [[0, 1, 2, 3], [1, 2], []]
    assert [list(r) for r in ref.Answer(nodes, tris, q).lists] == [[0, 1, 2, 3], [1, 2], []]
    # condition (a) is part of the definition: shrink the right child's box off its rows, and the walk no longer reaches rows 2 and 3
    nodes[2, 0] = 10.0
    got = rt.tri_overlaps(nodes, tris, q)
    assert [list(r) for r in _lists_of(got)] == [[0, 1], [1], []]
    assert [list(r) for r in ref.Answer(nodes, tris, q).lists] == [[0, 1], [1], []]


# ---------------------------------------------------------------- 3: the fixtures hold the cases where a wrong test shows

def test_the_fixtures_hold_the_telling_cases():
    alone = np.zeros(17, np.int64)
    for mesh in ref.MESHES:
        nodes, tris, q = ref.case(mesh)
        want = ref.reference(mesh)
        s = want.sat
        box_ok = ~s.sep[:3].any(0) & s.live[:, None]
        one = box_ok & (s.sep[3:].sum(0) == 1)
        here = np.array([(one & s.sep[3 + k]).sum() for k in range(17)])
        print(mesh, "pairs with overlapping boxes", int(box_ok.sum()), "accepted", int(want.accepted.sum()), "parted by one axis alone", dict(zip(ref.AXES, here)))
        alone += here
        dead = ~s.live
        assert (want.count == 0).sum() > 0 and dead.sum() >= q.shape[0] // 97
        assert (want.count[dead] == 0).all() and (want.visits[dead] == 0).all() and (want.visits[s.live] >= 1).all()
        assert np.isnan(q[dead]).any(0).sum() == 9 or dead.sum() < 9                            # the NaN rotates through the nine components
        assert ((q[:, 3:6] == q[:, 6:9]).all(1) & s.live).sum() > 0 and ((q[:, 0:3] == q[:, 3:6]).all(1) & (q[:, 3:6] == q[:, 6:9]).all(1)).sum() > 0
        assert np.isinf(q).any(1).sum() > 0 and (np.abs(q) == f32(3e38)).any(1).sum() > 0
        if tris.shape[0] > 8:
            assert (want.count > 8).sum() > 0 and ((want.count > 0) & (want.count <= 8)).sum() > 0
        # flush: the query's box ends exactly where a leaf box begins, or begins where it ends
        box = ref.aabb(q)
        leaves = [k for k in range(nodes.shape[0]) if nodes[k, 9] > 0]
        with np.errstate(all="ignore"):
            flush = ((box[:, None, 3:6] == nodes[None, leaves, 0:3]) | (box[:, None, 0:3] == nodes[None, leaves, 4:7])).any(-1).any(-1)
        assert (flush & s.live).sum() > 0, mesh
    assert (alone > 0).all(), dict(zip(ref.AXES, alone))
    s = ref.reference("bunny").sat                                                              # ... and all seventeen on the one generic mesh
    one = ~s.sep[:3].any(0) & s.live[:, None] & (s.sep[3:].sum(0) == 1)
    assert all((one & s.sep[3 + k]).any() for k in range(17))
    # coplanar pairs on the layer stack: all six points share y bit for bit
    nodes, tris, q = ref.case("layers")
    want = ref.reference("layers")
    s = want.sat
    a, b, c = ref.row_points(tris)
    assert (a[:, 1] == b[:, 1]).all() and (a[:, 1] == c[:, 1]).all()
    coplanar = ((q[:, None, 1] == a[None, :, 1]) & (q[:, None, 4] == a[None, :, 1]) & (q[:, None, 7] == a[None, :, 1])) & s.live[:, None]
    box_ok = ~s.sep[:3].any(0)
    in_plane_only = coplanar & box_ok & ~s.sep[3:ref.IN_PLANE.start].any(0) & s.sep[ref.IN_PLANE].any(0)
    print("layers: coplanar pairs", int(coplanar.sum()), "accepted", int((coplanar & want.accepted).sum()), "boxes overlapping and parted by in-plane axes only",
          int(in_plane_only.sum()))
    assert (coplanar & want.accepted).sum() > 0 and in_plane_only.sum() > 0
    assert not (coplanar & s.sep[3:ref.IN_PLANE.start].any(0)).any()                            # no axis along the common normal ever parts a coplanar pair


def test_against_the_float64_test():
    """Recorded, not bounded: the pairs on which the float32 definition and a float64 separating-axis test disagree."""
    for mesh in ref.MESHES:
        nodes, tris, q = ref.case(mesh)
        want = ref.reference(mesh)
        s64 = ref.sat64(tris, q)
        diff = s64 != want.sat.accept
        print(f"{mesh}: {int(diff.sum())} of {diff.size} pairs differ from float64 ({int((diff & want.sat.accept).sum())} accepted by float32 alone, "
              f"{int((diff & s64).sum())} by float64 alone)")
