"""Hull queries on the GPU (rt_query_hulls, rt_pick_rects): every answer against rt.hull_overlaps -- the host definition, itself pinned to
its numpy restatement in test_hull_query_host.py -- on the same arrays, bit for bit and with no query left out: query counts about the wave and block
sizes, the counts alone, the exact two-pass lists and fixed capacities, numpy and torch, query layouts, `visits` against the reference walk element
for element, the entries no list reaches left as they were, every node form (in fresh child processes), the dynamic mesh after a rebuild, a refit and
a rebuild of parts (with mesh_hit_parts over .hits() and the oriented box of a part), marquee picking against rt.rect_frusta, Renderer.pick and
Renderer.pick_multi, stream ordering with torch, isolation from the frame state, no allocation after the first query, and the refusals.  The bodies
are overlap_cases.py's, shared with the box and triangle queries; what the hull tests check beyond those -- the box kernel's visits, the parts' boxes,
the rect picks among the streams, frames and calls -- are HULL's hooks there.  The marquee test and the refusals of rt_pick_rects are here."""
import ctypes as C

import numpy as np
import pytest

import hull_query_ref as ref
import opengl_raytracing_amd as rt
import overlap_cases as oc
from overlap_cases import SENTINEL, _lists, _ptr, _same
from query_gpu import _clean_env, np_of, to  # noqa: F401  (_clean_env: autouse)

pytestmark = pytest.mark.gpu

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(np_of(a), f32).view(np.uint32)


# ---------------------------------------------------------------- 1: against the definition

@pytest.mark.parametrize("mesh", ref.MESHES)
def test_answers_equal_the_definition(mesh):
    oc.answers_equal_the_definition(oc.HULL, mesh)


def test_layouts_give_identical_bytes():
    oc.layouts_give_identical_bytes(oc.HULL)


def test_entries_no_list_reaches_are_left_as_they_were():
    """The C entries on arrays pre-filled with a sentinel, device and host path: the counts alone; lists alone in exact slots with a guard word behind;
    slots one short; fixed capacities; slots of negative length or with a negative start."""
    oc.entries_no_list_reaches_are_left_as_they_were(oc.HULL)


@pytest.mark.parametrize("option", ["RT_QNODES=2", "RT_FUSED=1", "RT_IMPLICIT=1"])
def test_every_node_form_gives_identical_bytes(option):
    """The query reads the two-child records and the triangle rows alone: what else the upload builds does not matter.  The options are read from
    the environment of the process, so each runs in a fresh child."""
    oc.every_node_form_gives_identical_bytes(oc.HULL, option)


# ---------------------------------------------------------------- 2: the dynamic mesh

def test_dynamic_mesh_rebuild_refit_and_parts():
    oc.dynamic_mesh_rebuild_refit_and_parts(oc.HULL)


# ---------------------------------------------------------------- 3: marquee picking

@pytest.mark.parametrize("jitter", [None, (0.31, -0.22)])
def test_pick_rects_against_rect_frusta_pick_and_pick_multi(jitter):
    nodes, tris = ref.mesh("bunny")
    assert tris.shape[0] == 320
    W, H = 48, 36
    u = oc.frame(nodes, tris, W, H, jitter)
    rects = np.array([[0, 0, W, H], [2 * W, 0, 3 * W, H], [10, 8, 30, 25], [20.25, 14.5, 27.75, 19], [23, 17, 24, 18], [0, 0, 12, 36], [30, 20, 47.5, 35.5],
                      [-5, -5, 20, 12], [24, 0, 24, 36], [np.nan, 0, 4, 4], [9, 9, 8, 10]], f32)
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H), indexing="xy"), -1).reshape(-1, 2).astype(np.int32)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        for t_near in (0.0, 0.25):
            want_corners = rt.rect_frusta(u, nodes[0, 0:3], nodes[0, 4:7], rects, t_near)
            want = rt.hull_overlaps(nodes, tris, want_corners)
            for arr, kind in ((rects, "numpy"), (to(rects), "torch")):
                got = ren.pick_rects(u, arr, t_near=t_near, visits=True)
                assert isinstance(got, rt.HullOverlaps) and np.array_equal(_bits(got.corners), _bits(want_corners)), (kind, t_near)
                _same(got, _lists(want), want.count, ("pick_rects", kind, t_near))
                assert np.array_equal(np_of(got.visits), ref.Walk(nodes, tris.shape[0], want_corners).visits)
                _same(ren.pick_rects(u, arr, t_near=t_near, cap=8), _lists(want), want.count, ("pick_rects", kind, t_near, 8), 8)
                _same(ren.hull_overlaps(got.corners), _lists(want), want.count, ("hull_overlaps on the corners", kind))
        wide = np.full((rects.shape[0], 6), np.nan, f32); wide[:, :4] = rects
        far = 2.0 * float((nodes[0, 4:7] - nodes[0, 0:3]).max())
        got = ren.pick_rects(u, to(wide)[:, :4], t_near=0.1, t_far=far)            # strided rows, a far depth of the caller's
        assert np.array_equal(_bits(got.corners), _bits(rt.rect_frusta(u, nodes[0, 0:3], nodes[0, 4:7], rects, 0.1, far)))
        # what the pixels show, and what lies behind them
        got = ren.pick_rects(u, rects)
        lists = _lists(got)
        first = ren.pick(u, xy).prim
        deep = ren.pick_multi(u, xy, max_hits=32)
        assert (first >= 0).sum() > 150 and (deep.count > 1).sum() > 100 and deep.count.max() <= 32
        cx, cy = xy[:, 0] + 0.5, xy[:, 1] + 0.5
        for i, r in enumerate(rects):
            inside = (r[0] < cx) & (cx < r[2]) & (r[1] < cy) & (cy < r[3])
            shown = set(first[inside & (first >= 0)]) | set(deep.prim[inside][deep.prim[inside] >= 0])
            assert shown <= set(lists[i]), (i, sorted(shown - set(lists[i])))
        assert set(first[first >= 0]) | set(deep.prim[deep.prim >= 0]) <= set(lists[0]) and len(lists[0]) > 100
        assert [len(lists[i]) for i in (1, 9, 10)] == [0, 0, 0] and 0 < len(lists[4]) < len(lists[3]) < len(lists[2]) < len(lists[0])


# ---------------------------------------------------------------- 4: stream ordering with torch

def test_queries_written_by_torch_just_before_the_call_are_the_ones_queried():
    oc.written_by_torch_just_before_the_call_are_the_ones_queried(oc.HULL)


def test_two_calls_on_two_torch_streams_without_a_host_wait():
    oc.two_calls_on_two_torch_streams_without_a_host_wait(oc.HULL)


# ---------------------------------------------------------------- 5: isolation from frames, no allocation

@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
def test_queries_do_not_touch_frame_state(pipeline):
    """Three BVH frames with hull queries and rect picks (host and device path) enqueued between them against the same three frames without: COLOR0 of
    every frame, the frame index, RtCounters (the megakernel's counting build), the traced-ray tallies and rt_debug_builds are identical."""
    oc.queries_do_not_touch_frame_state(oc.HULL, pipeline)


def test_no_allocation_after_the_first_query():
    oc.no_allocation_after_the_first_query(oc.HULL)


# ---------------------------------------------------------------- 6: refusals

def _rect_refusals_leave_the_outputs_unwritten():
    """rt_pick_rects and Renderer.pick_rects, as overlap_cases.every_refusal_leaves_the_outputs_unwritten does it for the query's own entries."""
    import torch
    L = rt.lib()
    nodes, tris, _ = ref.case("one_leaf")
    N, cap = 8, 4
    prims, counts, visits = np.full(N * cap, SENTINEL, np.int32), np.full(N, SENTINEL, np.int32), np.full(N, SENTINEL, np.int32)
    rects = np.tile(np.array([[3, 4, 20, 30]], f32), (N, 1))
    corners = np.full((N, 24), SENTINEL, f32)
    dp, dn, dv, dr, dc = to(prims), to(counts), to(visits), to(rects), to(corners)
    torch.cuda.synchronize()
    off = lambda a, k: C.c_void_p(_ptr(a).value + k)
    u = oc.frame(nodes, tris, 48, 36, None)

    with rt.Renderer() as ren:
        h = ren._h
        err = lambda: L.rt_last_error(h).decode()

        def rect_call(host, u_=0, r_=0, stride=4, n=N, t_near=0.0, t_far=-1.0, corners_=0, cap_=cap, prims_=0, counts_=0):
            A = (rects, corners, prims, counts, visits) if host else (dr, dc, dp, dn, dv)
            fn = L.rt_pick_rects_host if host else L.rt_pick_rects
            pick = lambda x, a: _ptr(a) if isinstance(x, int) and x == 0 else x
            return fn(h, C.byref(u) if isinstance(u_, int) else u_, pick(r_, A[0]), stride, n, t_near, t_far, pick(corners_, A[1]), None, cap_, pick(prims_, A[2]),
                      pick(counts_, A[3]), _ptr(A[4]))

        for host in (True, False):
            assert rect_call(host) == rt.RT_ERR_STATE and "no BVH uploaded" in err()
        ren.upload_bvh(nodes, tris)
        bad_res = oc.frame(nodes, tris, 48, 36, None)
        bad_res.resolution[0] = 0.0
        for host in (True, False):
            assert rect_call(host, u_=None) == rt.RT_ERR_INVALID and "null uniforms" in err()
            assert rect_call(host, u_=C.byref(bad_res)) == rt.RT_ERR_INVALID and "resolution" in err()
            assert rect_call(host, stride=3) == rt.RT_ERR_INVALID and "stride 3" in err()
            assert rect_call(host, t_near=-1.0) == rt.RT_ERR_INVALID and "tNear" in err()
            assert rect_call(host, t_near=float("nan")) == rt.RT_ERR_INVALID
            assert rect_call(host, t_far=float("nan")) == rt.RT_ERR_INVALID
            assert rect_call(host, r_=None) == rt.RT_ERR_INVALID and "null rect or corner array" in err()
            assert rect_call(host, corners_=None) == rt.RT_ERR_INVALID and "null rect or corner array" in err()
            assert rect_call(host, n=-1) == rt.RT_ERR_INVALID and "n = -1" in err()
            assert rect_call(host, prims_=None, counts_=None) == rt.RT_ERR_INVALID and "prims or counts" in err()
            assert rect_call(host, cap_=-1) == rt.RT_ERR_INVALID and "cap = -1" in err()
        # the device entry: alignment
        assert rect_call(False, r_=off(dr, 2)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert rect_call(False, corners_=off(dc, 1)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        ren.synchronize()
        assert (prims == SENTINEL).all() and (counts == SENTINEL).all() and (visits == SENTINEL).all() and (corners == SENTINEL).all()
        assert (dp.cpu().numpy() == SENTINEL).all() and (dn.cpu().numpy() == SENTINEL).all() and (dv.cpu().numpy() == SENTINEL).all()
        assert (dc.cpu().numpy() == SENTINEL).all()
        # Python: refused before any call into the library
        for bad in (lambda: ren.pick_rects(u, rects[:, :3]), lambda: ren.pick_rects(u, rects.astype(np.float64)), lambda: ren.pick_rects(u, torch.from_numpy(rects)),
                    lambda: ren.pick_rects(u, dr.t()), lambda: ren.pick_rects(u, rects, cap=-1), lambda: ren.pick_rects(u, rects, t_near=-1.0),
                    lambda: ren.pick_rects(None, rects), lambda: ren.pick_rects(None, dr)):
            with pytest.raises(rt.RtError) as e:
                bad()
            assert e.value.code == rt.RT_ERR_INVALID
        assert len(ren.pick_rects(u, rects[:0])) == 0 and len(ren.pick_rects(u, dr[:0], cap=4)) == 0


def test_every_refusal_leaves_the_outputs_unwritten():
    oc.every_refusal_leaves_the_outputs_unwritten(oc.HULL)
    _rect_refusals_leave_the_outputs_unwritten()
