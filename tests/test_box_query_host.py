"""The box query's definition on the host (rt_box_overlaps), no GPU: rt.box_overlaps against the numpy float32 restatement
(box_query_ref.py) bit for bit -- counts and lists, exact CSR slots and fixed capacities, strided boxes, counts alone and lists alone --, the entries
no list reaches left as they were, every refusal writing nothing, the two properties of library-built trees (the path mask removes nothing, every
list ascends), walk order on a hand-made tree with its children swapped, what the fixtures must hold for a wrong test to show, and the float64 test.
The bodies of the first five are overlap_cases.py's, shared with the triangle and hull queries."""
import numpy as np
import pytest

import box_query_ref as ref
import overlap_cases as oc

f32 = np.float32


# ---------------------------------------------------------------- 1: against the numpy definition

@pytest.mark.parametrize("mesh", ref.MESHES)
def test_counts_and_lists_equal_the_numpy_definition(mesh):
    oc.counts_and_lists_equal_the_numpy_definition(oc.BOX, mesh)


@pytest.mark.parametrize("stride", [6, 7, 12])
def test_strided_boxes_counts_alone_lists_alone_and_sentinels(stride):
    oc.strided_counts_alone_lists_alone_and_sentinels(oc.BOX, stride)


def test_every_refusal_writes_nothing():
    oc.every_refusal_writes_nothing(oc.BOX)


# ---------------------------------------------------------------- 2: the two properties of library-built trees, and walk order

@pytest.mark.parametrize("mesh", ref.MESHES)
def test_the_path_mask_removes_nothing_and_every_list_ascends(mesh):
    """Node boxes are the float min / max of exactly a, b, c of their rows, the box axes of the triangle test use the same values and comparisons do
    not round: a row the triangle test accepts lies under overlapping boxes all the way up.  And the right-first walk of rt_build_bvh's trees meets
    the rows in ascending order."""
    oc.the_path_mask_removes_nothing_and_every_list_ascends(oc.BOX, mesh)


def test_a_tree_with_swapped_children_lists_in_walk_order():
    """Three nodes by hand: the root's LEFT child holds rows 0, 1, its RIGHT child rows 2, 3.  The walk takes the right child first: 2, 3, 0, 1.  With
    the children swapped in the root's links it is 0, 1, 2, 3."""
    oc.a_tree_with_swapped_children_lists_in_walk_order(oc.BOX)


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
