"""The hull query's definition on the host (rt_hull_overlaps), no GPU: rt.hull_overlaps against the numpy float32 restatement
(hull_query_ref.py) bit for bit -- counts and lists, exact CSR slots and fixed capacities, strided and [N,8,3] queries, counts alone and lists alone --,
the entries no list reaches left as they were, every refusal writing nothing, the properties of library-built trees (the path mask removes nothing
although the node test culls by six normals as well, every list ascends), the shared-point property, walk order on a hand-made tree, what the fixtures
must hold for a wrong test to show, the float64 tests, and the corner makers rt.box_corners and rt.rect_frusta against their numpy definitions.
Three of these -- the path mask and ascending lists, the telling cases, the generic set's numpy half -- assert properties of the definition and of the
fixtures as hull_query_ref.py states them, not of the library: they say that the other tests compare the library with something worth comparing with.
The bodies the three overlap queries share are overlap_cases.py's."""
import ctypes as C

import numpy as np
import pytest

import hull_query_ref as ref
import opengl_raytracing_amd as rt
import overlap_cases as oc
from overlap_cases import SENTINEL, _lists_of

f32 = np.float32


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


# ---------------------------------------------------------------- 1: against the numpy definition

@pytest.mark.parametrize("mesh", ref.MESHES)
def test_counts_and_lists_equal_the_numpy_definition(mesh):
    oc.counts_and_lists_equal_the_numpy_definition(oc.HULL, mesh)


@pytest.mark.parametrize("stride", [24, 25, 32])
def test_strided_queries_counts_alone_lists_alone_and_sentinels(stride):
    oc.strided_counts_alone_lists_alone_and_sentinels(oc.HULL, stride)


def test_every_refusal_writes_nothing():
    oc.every_refusal_writes_nothing(oc.HULL)


# ---------------------------------------------------------------- 2: the properties of library-built trees, the shared point, and walk order

@pytest.mark.parametrize("mesh", ref.MESHES)
def test_the_path_mask_removes_nothing_and_every_list_ascends(mesh):
    """node boxes are the float min / max of exactly a, b, c of their rows, and the box's interval on a face normal -- its corners
    through dot's own three steps, the least and the greatest kept at each -- contains dot(normal, p) of every point p inside the box, each step being
    monotone.  So a normal that parts a node from the hull's interval parts every row under it from the same interval, on the same axis of the row
    test: a row the row test accepts lies under entered nodes all the way up, whatever the node test culls."""
    oc.the_path_mask_removes_nothing_and_every_list_ascends(oc.HULL, mesh)


@pytest.mark.parametrize("mesh", ref.MESHES)
def test_a_pair_that_shares_a_point_is_accepted_and_a_hull_at_a_vertex_lists_its_rows(mesh):
    """Derived from 26.1, not from the code: if a corner equals one of the row's a, b, c in all three floats, then on every projected axis the same dot
    on the same operands yields the same float, which lies in both intervals, and on the box axes the comparisons are exact -- no axis separates.  The
    kept face normals' intervals hold the same float as well."""
    nodes, tris, q = ref.case(mesh)
    want = ref.reference(mesh)
    a, b, c = ref.row_points(tris)
    shares = np.zeros((q.shape[0], tris.shape[0]), bool)
    per_point = []
    for v in (a, b, c):
        hit = np.zeros_like(shares)
        for k in range(0, 24, 3):
            hit |= (q[:, None, k:k + 3] == v[None]).all(-1)
        per_point.append(int((hit & want.sat.live[:, None]).sum()))
        shares |= hit
    shares &= want.sat.live[:, None]
    print(mesh, "pairs sharing a point with a, b, c:", per_point)
    assert min(per_point) > 0 and not (shares & ~want.accepted).any()
    # a hull collapsed to a row's own vertex lists that row: every row, every one of its three points, through the library
    for v in (a, b, c):
        got = rt.hull_overlaps(nodes, tris, np.tile(v, (1, 8)))
        assert all(t in rows for t, rows in enumerate(_lists_of(got)))


def test_a_tree_with_swapped_children_lists_in_walk_order():
    """23.5's three nodes by hand: the root's LEFT child holds rows 0, 1, its RIGHT child rows 2, 3.  The walk takes the right child first: 2, 3, 0, 1.
    With the children swapped in the root's links it is 0, 1, 2, 3.  Row x spans (x, 0, 0), (x + 0.5, 0, 0), (x, 0.5, 0.25).  The hulls: a slab about
    the plane y = 0.1 over all four rows; a thin box turned 20 degrees about z that crosses rows 1 and 2; a point inside the right child's box."""
    oc.a_tree_with_swapped_children_lists_in_walk_order(oc.HULL)


# ---------------------------------------------------------------- 3: the fixtures hold the cases where a wrong test shows

def test_the_fixtures_hold_the_telling_cases():
    """Of the fixtures and the numpy definition alone: that they hold the cases on which a wrong library would differ from them."""
    alone = np.zeros(43, np.int64)
    fewer = 0
    for mesh in ref.MESHES:
        nodes, tris, q = ref.case(mesh)
        want = ref.reference(mesh)
        s = want.sat
        one = s.box_ok & (s.sep[3:].sum(0) == 1)
        here = np.array([(one & s.sep[3 + k]).sum() for k in range(43)])
        print(mesh, "pairs with overlapping boxes", int(s.box_ok.sum()), "accepted", int(want.accepted.sum()), "parted by one axis alone", dict(zip(ref.AXES, here)))
        alone += here
        dead = ~s.live
        assert (want.count == 0).sum() > 0 and dead.sum() >= q.shape[0] // 97
        assert (want.count[dead] == 0).all() and (want.visits[dead] == 0).all() and (want.visits[s.live] >= 1).all()
        assert np.isnan(q[dead]).any(0).sum() == 24 or dead.sum() < 24                          # the NaN rotates through the 24 floats
        c = ref.corners(q)
        point = (c == c[:, :1]).all((1, 2))
        segment = (c[:, :4] == c[:, :1]).all((1, 2)) & (c[:, 4:] == c[:, 4:5]).all((1, 2)) & ~point
        quad = (c[:, :4] == c[:, 4:]).all((1, 2)) & ~point
        assert (point & s.live).sum() > 0 and (segment & s.live).sum() > 0 and (quad & s.live).sum() > 0
        assert np.isinf(q).any(1).sum() > 0 and (np.abs(q) == f32(3e38)).any(1).sum() > 0
        assert ((want.count > 0) & (want.count <= 8)).sum() > 0
        if tris.shape[0] > 8:
            assert (want.count > 8).sum() > 0
        # flush: the hull's box ends exactly where a leaf box begins, or begins where it ends
        box = ref.aabb(q)
        leaves = [k for k in range(nodes.shape[0]) if nodes[k, 9] > 0]
        with np.errstate(all="ignore"):
            flush = ((box[:, None, 3:6] == nodes[None, leaves, 0:3]) | (box[:, None, 0:3] == nodes[None, leaves, 4:7])).any(-1).any(-1)
        assert (flush & s.live).sum() > 0, mesh
        # the node test: nodes the walk reached whose boxes overlap [lo, hi] and that a face normal rejected; visits against the box query's on [lo, hi]
        plain = ref.box_visits(nodes, q)
        assert (want.visits <= plain).all()
        print(mesh, "nodes rejected by a face normal alone:", int(want.walk.culled.sum()), "visits", int(want.visits.sum()), "the box query's on [lo, hi]", int(plain.sum()))
        assert want.walk.culled.sum() > 0
        fewer += int((want.visits < plain).sum())
    assert (alone > 0).all(), dict(zip(ref.AXES, alone))
    assert fewer > 0
    s = ref.reference("bunny").sat                                                              # ... and all 43 on the one generic mesh
    one = s.box_ok & (s.sep[3:].sum(0) == 1)
    assert all((one & s.sep[3 + k]).any() for k in range(43))
    want = ref.reference("bunny")
    assert (want.visits < ref.box_visits(*ref.case("bunny")[::2])).sum() > 0


def test_the_generic_set_equals_float64_clipping_on_every_pair():
    """Random hulls -- generic hexahedra, pyramids whose near face is the apex, sheared boxes -- against random triangles, nothing placed to touch: the
    float32 definition, the float64 43-axis test and a float64 clipping test that knows no axis agree on every one of the 6 000 pairs."""
    rows, hulls = ref.generic_pairs()
    assert rows.shape[0] == 6000
    box = ref.aabb(hulls)
    a, b, c = ref.row_points(rows)
    box_ok = ~((ref._max3(a, b, c) < box[:, 0:3]) | (box[:, 3:6] < ref._min3(a, b, c))).any(1)
    accept = box_ok & ~ref.pair_axes(rows, hulls).any(0)
    clip, sat64 = ref.pair_clip64(rows, hulls), ref.pair_sat64(rows, hulls)
    print("generic set: accepted", int(accept.sum()), "of", accept.size, "; differing from float64 clipping", int((accept != clip).sum()), ", from the float64 axes",
          int((accept != sat64).sum()))
    assert 600 < accept.sum() < 5400
    assert (accept != clip).sum() == 0 and (accept != sat64).sum() == 0
    # ... and through the library: each pair as a tree of one leaf
    for k in range(0, 6000, 40):
        nodes = np.zeros((1, 12), f32)
        nodes[0, 0:3], nodes[0, 4:7] = np.minimum(np.minimum(a[k], b[k]), c[k]), np.maximum(np.maximum(a[k], b[k]), c[k])
        nodes[0, 8], nodes[0, 9] = 0, 1
        assert rt.hull_overlaps(nodes, rows[k:k + 1], hulls[k:k + 1]).count[0] == int(accept[k]), k


def test_huge_turned_hulls_lose_no_overlap_float64_sees():
    """A hull some 1e19 across that is not axis-aligned has face normals and edge products that overflow float32: dot() then gives inf for some points
    and NaN for others.  Only finite projections separate, so such a hull errs towards overlap: on every fixture, every row the
    float64 axes accept for a hull of that size is accepted by the definition and listed by the library -- the node test loses none either."""
    seen = 0
    for mesh in ref.MESHES:
        nodes, tris, q = ref.case(mesh)
        want = ref.reference(mesh)
        box = ref.aabb(q)
        with np.errstate(all="ignore"):
            huge = np.isfinite(q).all(1) & ((box[:, 3:6] - box[:, 0:3]).max(1) > f32(ref.HUGE)) & (np.abs(q) < 1e30).all(1)
            turned = huge & ~(np.sort(np.abs(ref.normals(ref.corners(q))), -1)[:, :, 1] == 0).all(1)   # no face normal along a coordinate axis
        assert turned.sum() >= 40, (mesh, int(turned.sum()))
        qi = np.flatnonzero(turned)
        s64 = np.stack([ref.pair_sat64(tris, np.repeat(q[i:i + 1], tris.shape[0], 0)) for i in qi])
        lost = s64 & ~want.accepted[qi]
        overflowed = ~np.isfinite(ref.normals(ref.corners(q[qi]))).all((1, 2))
        print(f"{mesh}: {qi.size} huge turned hulls, {int(overflowed.sum())} with a normal that is not finite; float64 accepts {int(s64.sum())} pairs, "
              f"the definition {int(want.accepted[qi].sum())}, lost {int(lost.sum())}")
        assert overflowed.sum() >= 40 and s64.sum() > 0 and not lost.any()
        got = rt.hull_overlaps(nodes, tris, np.ascontiguousarray(q[qi]))
        assert all(set(np.flatnonzero(s64[k])) <= set(rows) for k, rows in enumerate(_lists_of(got)))
        seen += int(s64.sum())
    assert seen > 1000
    # two hulls by hand: half-extent 2^67 along u = (0.5, 0.75, 0), v = (-0.75, 0.5, 0), w = (0, 0, 1), every corner exact in float32.  Centred at -S u
    # the hull holds the row at (0.7, -0.8, -0.3) and not the one at (0.7, 0.5, -0.3) -- which float32 cannot tell apart at this size and keeps --;
    # centred at -0.875 S u it holds the row at (1, 1, -0.3) deep inside.  One leaf each: the root is a node like any other
    S = 2.0 ** 67
    R = np.array([[0.5, -0.75, 0.0], [0.75, 0.5, 0.0], [0.0, 0.0, 1.0]])
    for centre, at in ((-1.0, [(0.7, -0.8, -0.3), (0.7, 0.5, -0.3)]), (-0.875, [(1.0, 1.0, -0.3)])):
        hull = (R[:, 0] * S * centre + (ref.CUBE * S) @ R.T).reshape(1, 24).astype(f32)
        assert np.array_equal(hull.astype(np.float64), (R[:, 0] * S * centre + (ref.CUBE * S) @ R.T).reshape(1, 24))
        rows = np.zeros((len(at), 12), f32)
        rows[:, 0:3], rows[:, 4], rows[:, 9] = at, 0.1, 0.1
        a, b, c = ref.row_points(rows)
        nodes = np.zeros((1, 12), f32)
        nodes[0, 0:3], nodes[0, 4:7] = np.minimum(np.minimum(a, b), c).min(0), np.maximum(np.maximum(a, b), c).max(0)
        nodes[0, 8], nodes[0, 9] = 0, len(at)
        inside = ref.pair_sat64(rows, np.repeat(hull, len(at), 0)) & ref.pair_clip64(rows, np.repeat(hull, len(at), 0))
        assert inside[0]
        want = ref.Answer(nodes, rows, hull)
        got = rt.hull_overlaps(nodes, rows, hull)
        assert want.accepted[0, 0] and want.visits[0] == 1 and set(np.flatnonzero(inside)) <= set(_lists_of(got)[0]) and got.count[0] == want.count[0]


def test_against_the_float64_tests():
    """Recorded, not bounded: the pairs with overlapping boxes on which the float32 definition and the float64 tests disagree.  These
    sets place hulls to touch rows -- shared corners, collapsed hulls on faces, flush boxes."""
    for mesh in ref.MESHES:
        nodes, tris, q = ref.case(mesh)
        want = ref.reference(mesh)
        finite = np.isfinite(q).all(1) & (np.abs(q) < 1e30).all(1)
        qi, ti = np.nonzero(want.sat.box_ok & finite[:, None])
        s64 = ref.pair_sat64(tris[ti], q[qi])
        acc = want.sat.accept[qi, ti]
        c = ref.corners(q).astype(np.float64)                                                  # clipping needs a solid: at most the apex collapsed
        with np.errstate(all="ignore"):
            solid = sum((np.nan_to_num(np.cross(c[:, l] - c[:, i], c[:, k] - c[:, j])) != 0).any(1).astype(int) for (i, j, k, l) in ref.FACES) >= 5
        pick = np.flatnonzero(solid[qi])
        pick = pick[::max(pick.size // 1000, 1)]                                               # ... on a sample: a Python loop per pair
        clip = ref.pair_clip64(tris[ti[pick]], q[qi[pick]])
        print(f"{mesh}: {int((s64 != acc).sum())} of {qi.size} box-overlapping pairs differ from the float64 axes ({int((acc & ~s64).sum())} accepted by float32 alone, "
              f"{int((~acc & s64).sum())} by float64 alone); {int((clip != acc[pick]).sum())} of {pick.size} sampled pairs of solid hulls differ from float64 clipping "
              f"({int((acc[pick] & ~clip).sum())} accepted by float32 alone, {int((~acc[pick] & clip).sum())} by clipping alone)")


# ---------------------------------------------------------------- 4: the corner makers

def test_box_corners_equal_the_numpy_definition():
    rng = np.random.default_rng(5)
    n = 257
    boxes = np.sort(rng.normal(size=(n, 2, 3)), 1).reshape(n, 6).astype(f32)
    boxes[3, 1], boxes[9, 5], boxes[11, [0, 3]] = np.nan, np.nan, (2.0, 1.0)                    # empty slots: a NaN, lo > hi
    boxes[17, 3], boxes[19, 0] = np.inf, -np.inf
    boxes[23, 0:3] = boxes[23, 3:6]                                                            # a point
    Ms = np.stack([ref._matrix(rng, k % 3, rng.normal(size=3)) for k in range(n)]).astype(f32)
    for M in (None, Ms[1], Ms):
        got = rt.box_corners(boxes, M)
        assert got.dtype == f32 and _same_bits(got, ref.box_corners(boxes, M))
    assert np.isnan(rt.box_corners(boxes)[[3, 9, 11]]).all() and not np.isnan(rt.box_corners(boxes)[[0, 17, 19, 23]]).any()
    got = rt.box_corners(boxes)                                                                # the identity copies: infinities survive
    assert got[17, 3] == np.inf and np.array_equal(got[0].reshape(8, 3)[5], [boxes[0, 3], boxes[0, 1], boxes[0, 5]])
    wide = np.full((n, 9), np.nan, f32)
    wide[:, :6] = boxes
    assert _same_bits(rt.box_corners(wide[:, :6], Ms), ref.box_corners(boxes, Ms))              # strided rows
    L, p = rt.lib(), lambda a: C.c_void_p(a.ctypes.data)
    out = np.full((n, 24), SENTINEL, f32)
    for args in ((p(boxes), 5, n, None, 0, p(out)), (p(boxes), 6, -1, None, 0, p(out)), (p(boxes), 6, n, p(Ms), 12, p(out)), (None, 6, n, None, 0, p(out)),
                 (p(boxes), 6, n, None, 0, None)):
        assert L.rt_box_corners(*args) == rt.RT_ERR_INVALID
    assert (out == SENTINEL).all() and L.rt_box_corners(None, 6, 0, None, 0, None) == rt.RT_OK
    with pytest.raises(rt.RtError):
        rt.box_corners(boxes, Ms[:5])


def test_box_corners_under_the_identity_against_the_box_query():
    """Recorded, not bounded: an axis-aligned hull asks 46 axes where the box query asks 13, with other roundings on the nine edge axes."""
    for mesh in ref.MESHES:
        nodes, tris, q = ref.case(mesh)
        box = ref.aabb(q)[ref.live(q)]
        box = box[np.isfinite(box).all(1)]
        hull = rt.hull_overlaps(nodes, tris, rt.box_corners(box))
        plain = rt.box_overlaps(nodes, tris, box)
        a, b = set(map(tuple, hull.pairs())), set(map(tuple, rt.TriOverlaps(plain.count, plain.offsets, plain.prims).pairs()))
        print(f"{mesh}: {len(a)} pairs by the hull query, {len(b)} by the box query, {len(a - b)} by the hull query alone, {len(b - a)} by the box query alone")


@pytest.mark.parametrize("jitter", [None, (0.31, -0.22)])
def test_rect_frusta_equal_the_numpy_definition(jitter):
    rng = np.random.default_rng(8)
    nodes, tris = ref.mesh("bunny")
    lo, hi = nodes[0, 0:3], nodes[0, 4:7]
    W, H = 48, 36
    u = ref.view("bunny", W, H, jitter)
    n = 300
    x0, y0 = rng.uniform(-10, W + 5, n), rng.uniform(-10, H + 5, n)
    rects = np.stack([x0, y0, x0 + rng.uniform(0, 20, n), y0 + rng.uniform(0, 20, n)], 1).astype(f32)
    rects[:8] = [[0, 0, W, H], [3, 4, 4, 5], [-W, 0, 0, H], [5, 5, 5, 5], [np.nan, 0, 1, 1], [0, 0, 1, np.nan], [4, 0, 3, 1], [0, 9, 1, 8]]
    rects[8] = [-np.inf, 0, np.inf, 1]
    big = float((hi - lo).max())
    for t_near, t_far in ((0.0, None), (0.1 * big, None), (0.2 * big, 3.0 * big), (1.0 * big, 0.5 * big), (0.0, 0.0)):
        got = rt.rect_frusta(u, lo, hi, rects, t_near, t_far)
        assert got.dtype == f32 and _same_bits(got, ref.rect_frusta(u, lo, hi, rects, t_near, t_far)), (t_near, t_far)
        assert np.isnan(got[[4, 5, 6, 7]]).all() and not np.isnan(got[[0, 1, 2, 3]]).any()
    pyramid = rt.rect_frusta(u, lo, hi, rects[:1]).reshape(8, 3)
    assert (pyramid[:4] == np.array(list(u.camPos), f32)).all()                                 # tNear = 0: the near face is the eye
    far = float(ref.scene_far(u, lo, hi, 0.0))                                                   # the far face lies beyond every vertex of the mesh
    a, b, c = ref.row_points(tris)
    depth = (np.concatenate([a, b, c]).astype(np.float64) - np.array(list(u.camPos))) @ np.array(list(u.camFwd))
    box = np.array([[hi[k] if j >> k & 1 else lo[k] for k in range(3)] for j in range(8)], np.float64)
    reach = ((box - np.array(list(u.camPos))) @ np.array(list(u.camFwd))).max()                 # the root box's farthest corner, widened by 2^-10
    assert depth.max() <= reach < far < reach * (1 + 2.0 ** -9)
    wide = np.full((n, 7), np.nan, f32)
    wide[:, :4] = rects
    assert _same_bits(rt.rect_frusta(u, lo, hi, wide[:, :4], 0.5), ref.rect_frusta(u, lo, hi, rects, 0.5))      # strided rows
    L, p = rt.lib(), lambda a: C.c_void_p(a.ctypes.data)
    out = np.full((n, 24), SENTINEL, f32)
    bad_res, bad_res2 = ref.view("bunny", W, H), ref.view("bunny", W, H)
    bad_res.resolution[0], bad_res2.resolution[1] = 0.0, -4.0
    lo_, hi_ = np.ascontiguousarray(lo), np.ascontiguousarray(hi)
    ok = [C.byref(u), p(lo_), p(hi_), p(rects), 4, n, 0.0, -1.0, p(out)]
    for k, v in ((0, None), (0, C.byref(bad_res)), (0, C.byref(bad_res2)), (1, None), (2, None), (3, None), (4, 3), (5, -1), (6, -0.5), (6, float("nan")),
                 (7, float("nan")), (8, None)):
        args = list(ok)
        args[k] = v
        assert L.rt_rect_frusta(*args) == rt.RT_ERR_INVALID, (k, v)
    assert (out == SENTINEL).all()
    assert L.rt_rect_frusta(*ok) == rt.RT_OK and _same_bits(out, ref.rect_frusta(u, lo, hi, rects))
    assert rt.rect_frusta(u, lo, hi, rects[:0]).shape == (0, 24)
