"""The box query's definition on the host (rt_box_overlaps), no GPU: rt.box_overlaps against the numpy float32 restatement
(box_query_ref.py) bit for bit -- counts and lists, exact CSR slots and fixed capacities, strided boxes, counts alone and lists alone --, the entries
no list reaches left as they were, every refusal writing nothing, the two properties of library-built trees (the path mask removes nothing, every
list ascends), walk order on a hand-made tree with its children swapped, what the fixtures must hold for a wrong test to show, and the float64 test."""
import ctypes as C

import numpy as np
import pytest

import box_query_ref as ref
import opengl_raytracing_amd as rt

f32 = np.float32
SENTINEL = -77
CAPS = (0, 1, 3, 8)


def _raw(nodes, tris, boxes, stride, n, offsets, cap, prims, counts):
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    return rt.lib().rt_box_overlaps(p(nodes), nodes.shape[0], p(tris), tris.shape[0], p(boxes), stride, n, p(offsets), cap, p(prims), p(counts))


def _lists_of(got):
    return [got.prims[got.offsets[i]:got.offsets[i] + min(got.count[i], got.offsets[i + 1] - got.offsets[i])] for i in range(len(got))]


# ---------------------------------------------------------------- 1: against the numpy definition

@pytest.mark.parametrize("mesh", ref.MESHES)
def test_counts_and_lists_equal_the_numpy_definition(mesh):
    nodes, tris, boxes = ref.case(mesh)
    want = ref.reference(mesh)
    assert boxes.shape[0] >= 2049
    got = rt.box_overlaps(nodes, tris, boxes)
    bad = np.flatnonzero(got.count != want.count)
    assert bad.size == 0, (mesh, bad[:8], got.count[bad[:8]], want.count[bad[:8]], boxes[bad[:2]])
    assert np.array_equal(got.offsets, want.offsets()) and got.prims.dtype == np.int32
    assert np.array_equal(got.prims, want.filled(want.offsets())), mesh
    for cap in CAPS:
        got = rt.box_overlaps(nodes, tris, boxes, cap=cap)
        assert np.array_equal(got.count, want.count) and np.array_equal(got.offsets, np.arange(boxes.shape[0] + 1) * cap)
        assert np.array_equal(got.prims, want.filled(cap=cap, sentinel=-1)), (mesh, cap)
    hits = rt.box_overlaps(nodes, tris, boxes[:65], cap=3).hits()
    assert hits.shape == (195, 4) and np.array_equal(hits.view(np.int32)[:, 1], want.filled(cap=3, sentinel=-1)[:195])
    assert (hits[:, 0] == 0).all() and (hits[:, 2:4] == f32(1) / f32(3)).all()


@pytest.mark.parametrize("stride", [6, 7, 12])
def test_strided_boxes_counts_alone_lists_alone_and_sentinels(stride):
    nodes, tris, boxes = ref.case("bunny")
    want = ref.reference("bunny")
    N = boxes.shape[0]
    wide = np.full((N, stride), np.nan, f32)
    wide[:, :6] = boxes
    flat = np.ascontiguousarray(wide.reshape(-1)[:(N - 1) * stride + 6])          # exactly as long as a call may read
    view = np.lib.stride_tricks.as_strided(flat, (N, 6), (4 * stride, 4))
    got = rt.box_overlaps(nodes, tris, view)
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
    nodes, tris, boxes = ref.case("layers")
    boxes = np.array(boxes[:4])
    prims, counts = np.full(32, SENTINEL, np.int32), np.full(4, SENTINEL, np.int32)
    off = np.array([0, 8, 16, 24, 32], np.int32)
    ok = dict(nodes=nodes, tris=tris, boxes=boxes, stride=6, n=4, offsets=off, cap=0, prims=prims, counts=counts)
    call = lambda **kw: _raw(**dict(ok, **kw))
    assert call(n=-1) == rt.RT_ERR_INVALID
    assert call(stride=5) == rt.RT_ERR_INVALID
    assert call(boxes=None) == rt.RT_ERR_INVALID
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
    assert _raw(nodes, tris, None, 6, 0, None, 0, None, None) == rt.RT_OK                     # n == 0: a no-op
    assert call() == rt.RT_OK and (counts != SENTINEL).all()
    for bad_call in (lambda: rt.box_overlaps(nodes, tris, boxes[:, :5]), lambda: rt.box_overlaps(nodes, tris, boxes.astype(np.float64)),
                     lambda: rt.box_overlaps(nodes, tris, boxes, cap=-1), lambda: rt.box_overlaps(nodes, tris, list(boxes))):
        with pytest.raises(rt.RtError) as e:
            bad_call()
        assert e.value.code == rt.RT_ERR_INVALID
    empty = rt.box_overlaps(nodes, tris, boxes[:0])
    assert len(empty) == 0 and empty.prims.size == 0 and np.array_equal(empty.offsets, [0])


# ---------------------------------------------------------------- 2: the two properties of library-built trees, and walk order

@pytest.mark.parametrize("mesh", ref.MESHES)
def test_the_path_mask_removes_nothing_and_every_list_ascends(mesh):
    """Node boxes are the float min / max of exactly a, b, c of their rows, the box axes of the triangle test use the same values and comparisons do
    not round: a row the triangle test accepts lies under overlapping boxes all the way up.  And the right-first walk of rt_build_bvh's trees meets
    the rows in ascending order."""
    want = ref.reference(mesh)
    assert not (want.sat.accept & ~want.walk.path).any()
    assert np.array_equal(want.walk.order, np.arange(want.walk.order.size))
    assert all((np.diff(rows) > 0).all() for rows in want.lists)


def test_a_tree_with_swapped_children_lists_in_walk_order():
    """Three nodes by hand: the root's LEFT child holds rows 0, 1, its RIGHT child rows 2, 3.  The walk takes the right child first: 2, 3, 0, 1.  With
    the children swapped in the root's links it is 0, 1, 2, 3."""
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
    boxes = np.array([[-1, -1, -1, 5, 1, 1], [0.9, -1, -1, 2.2, 1, 1], [2.6, 0, 0, 2.6, 0, 0]], f32)
    got = rt.box_overlaps(nodes, tris, boxes)
    want = ref.Answer(nodes, tris, boxes)
    assert [list(r) for r in _lists_of(got)] == [[2, 3, 0, 1], [2, 1], []] and [list(r) for r in want.lists] == [[2, 3, 0, 1], [2, 1], []]
    assert list(want.visits) == [3, 3, 3]
    nodes[0, 3], nodes[0, 7] = 2, 1
    got = rt.box_overlaps(nodes, tris, boxes)
    assert [list(r) for r in _lists_of(got)] == [[0, 1, 2, 3], [1, 2], []]
    assert [list(r) for r in ref.Answer(nodes, tris, boxes).lists] == [[0, 1, 2, 3], [1, 2], []]
    # condition (a) is part of the definition: shrink the right child's box off its rows, and the walk no longer reaches rows 2 and 3
    nodes[2, 0] = 10.0
    got = rt.box_overlaps(nodes, tris, boxes)
    assert [list(r) for r in _lists_of(got)] == [[0, 1], [1], []]
    assert [list(r) for r in ref.Answer(nodes, tris, boxes).lists] == [[0, 1], [1], []]


# ---------------------------------------------------------------- 3: the fixtures hold the cases where a wrong test shows

def test_the_fixtures_hold_the_telling_cases():
    alone = np.zeros(10, np.int64)
    for mesh in ref.MESHES:
        nodes, tris, boxes = ref.case(mesh)
        want = ref.reference(mesh)
        s = want.sat
        box_ok = ~s.sep[:3].any(0) & s.live[:, None]
        one = box_ok & (s.sep[3:].sum(0) == 1)
        here = np.array([(one & s.sep[3 + k]).sum() for k in range(10)])
        print(mesh, "pairs with overlapping boxes", int(box_ok.sum()), "accepted", int(want.accepted.sum()), "parted by one axis alone", dict(zip(ref.AXES, here)))
        alone += here
        assert (want.count == 0).sum() > 0 and (~s.live).sum() >= boxes.shape[0] // 97
        assert (want.count[~s.live] == 0).all() and (want.visits[~s.live] == 0).all() and (want.visits[s.live] >= 1).all()
        if tris.shape[0] > 8:
            assert (want.count > 8).sum() > 0 and ((want.count > 0) & (want.count < 8)).sum() > 0
            assert (want.count == tris.shape[0]).sum() >= 2                                     # the root box and the infinite box list everything
        # touching: accepted with equality on a box axis
        with np.errstate(all="ignore"):
            a, b, c = tris[:, 0:3], (tris[:, 0:3] + tris[:, 4:7]).astype(f32), (tris[:, 0:3] + tris[:, 8:11]).astype(f32)
            tmin, tmax = np.fmin(np.fmin(a, b), c), np.fmax(np.fmax(a, b), c)
            touch = ((tmax[None] == boxes[:, None, 0:3]) | (tmin[None] == boxes[:, None, 3:6])).any(-1)
        assert (touch & want.accepted).sum() > 0, mesh
    assert (alone > 0).all(), dict(zip(ref.AXES, alone))
    s = ref.reference("bunny").sat                                                              # ... and all ten on the one generic mesh
    one = ~s.sep[:3].any(0) & s.live[:, None] & (s.sep[3:].sum(0) == 1)
    assert all((one & s.sep[3 + k]).any() for k in range(10))


@pytest.mark.parametrize("mesh", ref.MESHES)
def test_a_row_whose_first_vertex_lies_inside_the_closed_box_is_accepted(mesh):
    """Derived from 23.1, not from the code: on each of the ten axes the box's interval is the least and the greatest of its corners under the very
    steps the vertex a = v0 goes through (a rounded product, then fmaf), each step monotone in the coordinate and in the running value.  So with
    lo <= a <= hi the projection of a lies inside the interval exactly; the triangle's value on the normal IS that projection and its [tmin, tmax]
    on an edge axis holds it, so no axis separates -- even for the degenerate box lo == hi == a.  (Not so for b and c on the normal: dot(n, b) is not
    the value the triangle projects to.)"""
    nodes, tris, boxes = ref.case(mesh)
    want = ref.reference(mesh)
    with np.errstate(all="ignore"):
        a = tris[:, 0:3]
        inside = ((boxes[:, None, 0:3] <= a[None]) & (a[None] <= boxes[:, None, 3:6])).all(-1)
    degenerate = (boxes[:, 0:3] == boxes[:, 3:6]).all(1)
    assert (inside & degenerate[:, None]).sum() > 0 and not (inside & ~want.accepted).any()


def test_against_the_float64_test():
    """Recorded, not bounded: the pairs on which the float32 definition and a float64 separating-axis test disagree."""
    for mesh in ref.MESHES:
        nodes, tris, boxes = ref.case(mesh)
        want = ref.reference(mesh)
        s64 = ref.sat64(tris, boxes)
        diff = s64 != want.sat.accept
        print(f"{mesh}: {int(diff.sum())} of {diff.size} pairs differ from float64 ({int((diff & want.sat.accept).sum())} accepted by float32 alone, "
              f"{int((diff & s64).sum())} by float64 alone)")
