"""rt_bvh_cost without a GPU: the quality metric of a tree, held to its numpy restatement (tests/bvh_cost_ref.py) in every integer and
in every double's bits.  It is the definition the device measurement (tests/test_gpu_mesh_quality.py) is held to.  The last test pins the claim the
refit-or-rebuild policy rests on: the metric tells the deformations a rebuild repairs from those it does not."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import bvh_build_ref as B
import bvh_cost_ref as K
import opengl_raytracing_amd as rt

CORPUS = B.corpus()


def _displaced_vertices(v, sigma=0.2, seed=5):
    return (v + np.random.default_rng(seed).normal(0, sigma, v.shape)).astype(np.float32)


def _trees(name):
    """(built nodes, the same tree refitted over vertices displaced by sigma = 0.2, the same tree refitted over the unmoved mesh)"""
    v, f = CORPUS[name]
    t9 = B.gather(v, f)
    nodes, t12, order = B.ref_build(t9)
    with np.errstate(all="ignore"):
        moved, _ = B.ref_refit(B.gather(_displaced_vertices(v), f), order, nodes, t12)
    same, _ = B.ref_refit(t9, order, nodes, t12)
    return nodes, moved, same


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_cost_equals_the_definition(name):
    nodes, moved, same = _trees(name)
    for what, n in (("built", nodes), ("refitted", moved)):
        want = K.ref_cost(n)
        got = rt.bvh_cost(n)
        K.assert_same(got, want, f"{name} {what}")
        assert got.nInner + got.nLeaves == n.shape[0]
        assert np.isfinite(got.cost) and np.isfinite(got.rootArea) and (got.degenerate == 1) == (got.rootArea == 0.0)
    # a refit of the unmoved mesh changes no box (but for the sign of a zero, which no extent sees): the record is unchanged
    K.assert_same(rt.bvh_cost(same), K.ref_cost(nodes), f"{name} refitted unmoved")


def test_anchors():
    """What the definition gives on meshes whose answer can be worked out by hand, and at both ends of the exponent range."""
    cost = {name: rt.bvh_cost(_trees(name)[0]) for name in ("count_1", "count_8", "floor_grid", "identical", "point", "denormal", "huge")}
    assert cost["count_1"].cost == 1.0 and cost["count_1"].nInner == 0            # one leaf = the root: 1 x A / A
    assert cost["count_8"].cost == 8.0 and cost["count_8"].inner == 0.0
    assert cost["identical"].inner == 127.0 and cost["identical"].leaf == 1000.0  # every box is the root's: the node and triangle counts
    assert cost["floor_grid"].leaf == 8.0 and abs(cost["floor_grid"].inner - 31.0 / 3.0) < 1e-9
    p = cost["point"]
    assert p.degenerate == 1 and p.rootArea == 0.0 and (p.innerQ, p.leafQ, p.inner, p.leaf, p.cost, p.rootExp) == (0, 0, 0.0, 0.0, 0.0, 0)
    assert cost["denormal"].rootExp == -265 and cost["huge"].rootExp == 203
    for name in ("denormal", "huge"):                                              # no overflow, no underflow to nothing
        assert np.isfinite(cost[name].cost) and cost[name].cost > 1.0 and cost[name].innerQ > 0 and not cost[name].degenerate


def test_order_of_the_nodes_does_not_matter():
    """A function of the set of nodes: any order of the rows behind the root gives the same bits (the device adds in whatever order its waves finish)."""
    nodes = _trees("lattice")[0]
    want = K.ref_cost(nodes)
    perm = np.concatenate([[0], 1 + np.random.default_rng(3).permutation(nodes.shape[0] - 1)])
    K.assert_same(rt.bvh_cost(nodes[perm]), want, "permuted")


def _raw(nodes, n=None):
    out = rt.RtBvhCost()
    a = np.ascontiguousarray(nodes, np.float32)
    return rt.lib().rt_bvh_cost(a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0] if n is None else n, C.byref(out)), out


def test_refusals():
    nodes = _trees("count_100" if "count_100" in CORPUS else "count_40")[0]
    assert _raw(nodes)[0] == rt.RT_OK
    L = rt.lib()
    out = rt.RtBvhCost()
    assert L.rt_bvh_cost(None, 3, C.byref(out)) == rt.RT_ERR_INVALID
    assert L.rt_bvh_cost(nodes.ctypes.data_as(C.POINTER(C.c_float)), nodes.shape[0], None) == rt.RT_ERR_INVALID
    assert _raw(nodes, 0)[0] == rt.RT_ERR_INVALID and _raw(nodes, -1)[0] == rt.RT_ERR_INVALID
    last = nodes.shape[0] - 1
    for row, col, value in ((last, 9, -1.0), (1, 9, -3.0),                              # a negative count
                            (last, 0, np.nan), (0, 5, np.inf), (2, 2, -np.inf), (1, 6, np.nan),   # a non-finite bound
                            (last, 4, nodes[last, 0] - 1.0), (0, 2, nodes[0, 6] + 1.0)):          # a max below its min
        bad = nodes.copy()
        bad[row, col] = value
        rc, rec = _raw(bad)
        assert rc == rt.RT_ERR_INVALID, (row, col, value)
        assert (rec.innerQ, rec.leafQ, rec.cost) == (0, 0, 0.0)
    with pytest.raises(rt.RtError) as e:
        rt.bvh_cost(np.zeros((0, 12), np.float32))
    assert e.value.code == rt.RT_ERR_INVALID


def test_exports_and_null_contexts():
    out = subprocess.run(["nm", "-D", "--defined-only", str(rt.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (rt_[a-z0-9_]+)", out))
    assert {"rt_bvh_cost", "rt_mesh_measure", "rt_mesh_quality", "rt_mesh_update"} <= exported
    L = rt.lib()
    q, action = rt.RtMeshQuality(), C.c_int(7)
    assert L.rt_mesh_measure(None) == rt.RT_ERR_INVALID
    assert L.rt_mesh_quality(None, rt.RT_MESH_QUALITY_LATEST, 0, C.byref(q)) == rt.RT_ERR_INVALID
    assert L.rt_mesh_update(None, rt.RT_MESH_UPDATE_SINGLE, None, 2.0, C.byref(action)) == rt.RT_ERR_INVALID and action.value == 7
    assert C.sizeof(rt.RtBvhCost) == 64 and C.sizeof(rt.RtMeshQuality) == 80
    assert rt.RtBvhCost.cost.offset == 40 and rt.RtBvhCost.rootExp.offset == 48 and rt.RtMeshQuality.update.offset == 64


def test_the_metric_separates_what_a_rebuild_repairs():
    """The numpy restatement alone, on the 32 x 32 grid of 2048 triangles (side 1): parts that drift apart inside one refitted tree inflate it, and a
    rebuild repairs that; random displacement of every vertex inflates a rebuilt tree as much as a refitted one, and a rebuild buys nothing."""
    v, f = K.grid(32)
    f, first = K.interleave_parts(f, 4)
    rest = K.gather_parts(v, f, first, K.translations(4, 0.0))
    nodes, t12, order = B.ref_build(rest)
    at_build = K.ref_cost(nodes)["cost"]

    def ratios(t9):
        refit, _ = B.ref_refit(t9, order, nodes, t12)
        rebuilt, _, _ = B.ref_build(t9)
        return K.ref_cost(refit)["cost"] / at_build, K.ref_cost(rebuilt)["cost"] / at_build

    table = {}
    for step in (0.5, 2.0):
        table[f"parts {step}"] = ratios(K.gather_parts(v, f, first, K.translations(4, step)))
    for sigma in (0.05, 0.2):
        moved = (v + np.random.default_rng(1).normal(0, sigma, v.shape)).astype(np.float32)
        table[f"noise {sigma}"] = ratios(K.gather_parts(moved, f, first, K.translations(4, 0.0)))
    for k, (a, b) in table.items():
        print(f"{k}: refitted {a:.2f}, rebuilt {b:.2f} x the cost at build")
    assert table["parts 0.5"][0] > 5 and table["parts 0.5"][1] < 1.5
    assert table["parts 2.0"][0] > 5 and table["parts 2.0"][1] < 1.5
    assert table["noise 0.05"][0] < table["noise 0.05"][1] and table["noise 0.05"][0] > 2
    assert table["noise 0.2"][0] < table["noise 0.2"][1] and table["noise 0.2"][0] > 2
