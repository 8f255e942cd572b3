"""The triangle query's definition on the host (rt_tri_overlaps), no GPU: rt.tri_overlaps against the numpy float32 restatement
(tri_query_ref.py) bit for bit -- counts and lists, exact CSR slots and fixed capacities, strided and [N,3,3] queries, counts alone and lists alone --,
the entries no list reaches left as they were, every refusal writing nothing, the properties of library-built trees (the path mask removes nothing,
every list ascends), the shared-point property, walk order on a hand-made tree with its children swapped, what the fixtures must hold for a wrong
test to show, and the float64 test.  The bodies the three overlap queries share are overlap_cases.py's."""
import numpy as np
import pytest

import opengl_raytracing_amd as rt
import overlap_cases as oc
import tri_query_ref as ref
from overlap_cases import _lists_of

f32 = np.float32


# ---------------------------------------------------------------- 1: against the numpy definition

@pytest.mark.parametrize("mesh", ref.MESHES)
def test_counts_and_lists_equal_the_numpy_definition(mesh):
    oc.counts_and_lists_equal_the_numpy_definition(oc.TRI, mesh)


@pytest.mark.parametrize("stride", [9, 10, 12])
def test_strided_queries_counts_alone_lists_alone_and_sentinels(stride):
    oc.strided_counts_alone_lists_alone_and_sentinels(oc.TRI, stride)


def test_every_refusal_writes_nothing():
    oc.every_refusal_writes_nothing(oc.TRI)


# ---------------------------------------------------------------- 2: the properties of library-built trees, the shared point, and walk order

@pytest.mark.parametrize("mesh", ref.MESHES)
def test_the_path_mask_removes_nothing_and_every_list_ascends(mesh):
    """Node boxes are the float min / max of exactly a, b, c of their rows, the box axes of the triangle test compare the same values with the same
    [qlo, qhi] and comparisons do not round: a row the triangle test accepts lies under overlapping boxes all the way up.  And the right-first walk
    of rt_build_bvh's trees meets the rows in ascending order."""
    oc.the_path_mask_removes_nothing_and_every_list_ascends(oc.TRI, mesh)


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
    oc.a_tree_with_swapped_children_lists_in_walk_order(oc.TRI)


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
