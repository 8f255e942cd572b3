"""The host packers of the BVH scene (csrc/rt_scene_pack.cpp) without a GPU.

  A. Nothing moved: rt.pack_scene reproduces, for every mesh and option set of tests/scene_pack_cases.py, the sha256 of the seven arrays and the
     RtSceneInfo that rt_upload_bvh left on the device BEFORE the packers moved out of it (tests/golden/scene_pack_parent.json, recorded on a GPU by
     tests/golden/make_scene_pack_golden.py).  A rejected quantisation is part of the record, not a reason to leave a case out.
  B. The arrays that commit could not show -- fused hubs and the five implicit arrays -- against the structure of the tree and against the arrays of A.
     The any-hit stack need against rt_bvh_layout's.
Every comparison is bit for bit."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scene_pack_cases as cases

GOLDEN = json.loads((Path(__file__).parent / "golden" / "scene_pack_parent.json").read_text())
NO_CHILD = 0x7FFFFFFF
u32 = np.uint32


def test_the_record_covers_every_case():
    assert set(GOLDEN) == {f"{m}/{o}" for m in cases.MESHES for o in cases.OPTION_SETS}


# ---------------------------------------------------------------- A
def _scene_info(info, packed):
    """RtSceneInfo as rt_get_scene_info derives it from the context's scalars."""
    quantised = packed["qnodes4"].size > 0
    return {"nNodes": info.nNodes, "nTris": info.nTris, "nInner": info.nInner, "treeDepth": info.treeDepth, "nWide4": info.nWide4, "nPairs": info.nPairs,
            "bytesNodes2": max(info.nInner, 1) * 64, "bytesNodes4": info.nWide4 * 64 + info.nLeafBoxes * 32 if quantised else info.nWide4 * 128,
            "bytesPairs": info.nPairs * 80, "bytesTris": info.nTris * 48, "nFused": info.nFused, "flags": info.flags, "implicitDepth": info.implicitDepth}


@pytest.mark.parametrize("oname", list(cases.OPTION_SETS))
@pytest.mark.parametrize("mname", cases.MESHES)
def test_pack_scene_equals_the_upload_before_the_move(mname, oname):
    want = GOLDEN[f"{mname}/{oname}"]
    nodes, tris = cases.mesh(mname)
    got = rt.pack_scene(nodes, tris, **cases.OPTION_SETS[oname][1])
    for name in rt.SCENE_ARRAYS:
        assert got[name].size == want["bytes"][name], (name, got[name].size, want["bytes"][name])
        assert hashlib.sha256(got[name].tobytes()).hexdigest() == want["sha256"][name], name
    assert _scene_info(got["info"], got) == want["info"]
    for name in rt.SCENE_ARRAYS_OPTIONAL:      # none of these option sets asks for them
        assert got[name].size == 0, name


def test_options_come_from_the_environment_when_none_are_given(monkeypatch):
    nodes, tris = cases.mesh("plain_40")
    for env, kw in cases.OPTION_SETS.values():
        for v in cases.PACK_VARS:
            monkeypatch.delenv(v, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        a, b = rt.pack_scene(nodes, tris), rt.pack_scene(nodes, tris, **kw)
        for name in list(rt.SCENE_ARRAYS) + list(rt.SCENE_ARRAYS_OPTIONAL):
            assert np.array_equal(a[name], b[name]), (env, name)
        assert {k: np.asarray(v).tolist() for k, v in vars(a["info"]).items()} == {k: np.asarray(v).tolist() for k, v in vars(b["info"]).items()}, env


# ---------------------------------------------------------------- B
class Tree:
    """nodes12 decoded as nodeFetch decodes it, every node's depth and path, and the pair-record reference of every leaf as nodes2w holds it."""

    def __init__(self, nodes, packed):
        self.bits = np.ascontiguousarray(nodes).view(u32)
        self.left, self.right, self.first, self.count = ((nodes[:, k] + np.float32(0.5)).astype(np.int64) for k in (3, 7, 8, 9))
        n = nodes.shape[0]
        self.depth, self.path = np.full(n, -1), np.zeros(n, np.int64)
        todo = [(0, 0, 0)]
        while todo:
            i, d, p = todo.pop()
            self.depth[i], self.path[i] = d, p
            if self.count[i] <= 0:
                todo += [(int(self.left[i]), d + 1, 2 * p), (int(self.right[i]), d + 1, 2 * p + 1)]
        assert (self.depth >= 0).all()
        inner = np.flatnonzero(self.count <= 0)
        w = packed["nodes2w"].view(np.int32).reshape(-1, 16)
        self.leaf_ref = {}
        for k, i in enumerate(inner):
            for child, word in ((self.left[i], 3), (self.right[i], 7)):
                if self.count[child] > 0:
                    self.leaf_ref[int(child)] = int(w[k, word])
        leaves = np.flatnonzero(self.count > 0)
        self.leaves = leaves
        self.uniform = len(set(self.depth[leaves])) == 1 and self.count[0] <= 0

    def is_leaf(self, i):
        return self.count[i] > 0

    def box(self, i):
        return self.bits[i, [0, 1, 2, 4, 5, 6]]


def _packed(mname, **kw):
    nodes, tris = cases.mesh(mname)
    p = rt.pack_scene(nodes, tris, **kw)
    return nodes, p, Tree(nodes, p)


@pytest.mark.parametrize("mname", cases.MESHES)
def test_fused_hubs_hold_the_tree(mname):
    nodes, p, t = _packed(mname, fused=True)
    if t.is_leaf(0):
        assert p["fused"].size == 0 and p["info"].nFused == 0 and not p["info"].flags & rt.RT_SCENE_NOT_FUSED
        return
    assert not p["info"].flags & rt.RT_SCENE_NOT_FUSED
    wF = p["fused"].view(u32).reshape(-1, 2, 2, 8)      # hub, half, child, [min.xyz ref | max.xyz -]
    assert p["info"].nFused == wF.shape[0]
    seen_leaves, seen_hubs, todo = [], [], [(0, 0)]
    while todo:
        node, hub = todo.pop()
        seen_hubs.append(hub)
        for h, X in enumerate((int(t.left[node]), int(t.right[node]))):
            kids = [X, -1] if t.is_leaf(X) else [int(t.left[X]), int(t.right[X])]
            refs = wF[hub, h, 0, [3, 7]].view(np.int32)
            for k, kid in enumerate(kids):
                got = wF[hub, h, k][[0, 1, 2, 4, 5, 6]]
                if kid < 0:
                    assert refs[k] == NO_CHILD and np.isnan(got.view(np.float32)).all()
                    continue
                assert np.array_equal(got, t.box(kid)), (hub, h, k)
                if t.is_leaf(kid):
                    assert refs[k] == t.leaf_ref[kid]
                    seen_leaves.append(kid)
                else:
                    assert 0 <= refs[k] < wF.shape[0]
                    todo.append((kid, int(refs[k])))
    assert sorted(seen_leaves) == t.leaves.tolist()                  # every leaf exactly once
    assert sorted(seen_hubs) == list(range(wF.shape[0]))             # every hub exactly once


@pytest.mark.parametrize("mname", ("plain_9", "plain_17", "plain_1000", "floor_grid"))
def test_a_box_that_is_not_the_union_of_its_children_is_not_fused(mname):
    nodes, tris = cases.mesh(mname)
    broken = nodes.copy()
    inner = np.flatnonzero((nodes[:, 9] + np.float32(0.5)).astype(np.int64) <= 0)[-1]
    broken[inner, 4] = np.nextafter(broken[inner, 4], np.float32(np.inf))        # max.x one ulp up: still contains its children, no longer their union
    p = rt.pack_scene(broken, tris, fused=True)
    assert p["fused"].size == 0 and p["info"].nFused == 0 and p["info"].flags & rt.RT_SCENE_NOT_FUSED
    q = rt.pack_scene(broken, tris, fused=False)
    assert not q["info"].flags & rt.RT_SCENE_NOT_FUSED
    for name in rt.SCENE_ARRAYS:
        assert np.array_equal(p[name], q[name]), name


IMPLICIT = ("impl_nodes2", "impl_pairs", "impl_nodes4", "impl_qnodes4", "impl_leafbox")


@pytest.mark.parametrize("qnodes", (0, 2))
@pytest.mark.parametrize("mname", cases.MESHES)
def test_implicit_records_hold_the_tree(mname, qnodes):
    nodes, p, t = _packed(mname, implicit=True, qnodes=qnodes)
    info = p["info"]
    if not t.uniform:
        for name in IMPLICIT:
            assert p[name].size == 0, name
        assert info.implicitDepth == 0 and not info.flags & rt.RT_SCENE_IMPLICIT
        return
    D = int(t.depth[t.leaves[0]])
    R = int(((t.count[t.leaves] + 1) // 2).max())
    assert info.implicitDepth == D and info.implicitRecords == R and info.flags & rt.RT_SCENE_IMPLICIT
    slot = lambda d, pth: d - bin(pth).count("1") + (pth << (D - d))
    quantised = p["qnodes4"].size > 0
    assert quantised == (qnodes == 2 and not info.flags & rt.RT_SCENE_QNODES_REJECTED)
    iN2 = p["impl_nodes2"].view(u32).reshape(-1, 12)
    iPairs = p["impl_pairs"].view(u32).reshape(-1, 20)
    iN4 = p["impl_nodes4"].view(u32).reshape(-1, 24)
    pairs = p["pairs"].view(u32).reshape(-1, 20)
    assert iN2.shape[0] == iN4.shape[0] == (1 << D) - 1 and iPairs.shape[0] == (1 << D) * R + 8
    if quantised:
        iQ4, iLB = p["impl_qnodes4"].view(u32).reshape(-1, 12), p["impl_leafbox"].view(u32).reshape(-1, 8)
        assert iQ4.shape[0] == (1 << D) - 1 and iLB.shape[0] == 1 << D
    else:
        assert p["impl_qnodes4"].size == 0 and p["impl_leafbox"].size == 0
    for i in range(nodes.shape[0]):
        d, pth = int(t.depth[i]), int(t.path[i])
        if not t.is_leaf(i):
            want = np.concatenate([t.box(int(t.left[i])), t.box(int(t.right[i]))])
            assert np.array_equal(iN2[slot(d, pth)], want), (i, d, pth)
            continue
        first, nrec = (-t.leaf_ref[i] - 1) >> 3, (int(t.count[i]) + 1) // 2
        want = pairs[first:first + nrec].copy()
        want[0, 19] = t.count[i]
        assert np.array_equal(iPairs[pth * R:pth * R + nrec], want), (i, pth)
        assert not iPairs[pth * R + nrec:(pth + 1) * R].any()
        if quantised:
            assert np.array_equal(iLB[pth], np.concatenate([t.box(i), [0, 0]]).astype(u32)), (i, pth)
    # the explicit four-wide tree walked from its root alongside the even-depth nodes: the same children in the same order
    w4 = p["nodes4"].view(u32).reshape(-1, 32)
    q4 = p["qnodes4"].view(u32).reshape(-1, 16)
    todo, seen = [(0, 0)], 0
    while todo:
        node, at = todo.pop()
        seen += 1
        d, pth = int(t.depth[node]), int(t.path[node])
        assert d % 2 == 0
        L, Rr = int(t.left[node]), int(t.right[node])
        kids = [L, Rr] if d + 1 == D else [int(t.left[L]), int(t.right[L]), int(t.left[Rr]), int(t.right[Rr])]
        refs = w4[at, 24:28].view(np.int32)
        for k in range(4):
            if k >= len(kids):
                assert refs[k] == NO_CHILD
                continue
            assert np.array_equal(w4[at, k:24:4], t.box(kids[k])), (at, k)
            if t.is_leaf(kids[k]):
                assert refs[k] == t.leaf_ref[kids[k]]
            else:
                todo.append((kids[k], int(refs[k])))
        assert np.array_equal(iN4[slot(d, pth)], w4[at, :24]), (at, d, pth)
        if quantised:
            assert np.array_equal(iQ4[slot(d, pth)], q4[at, :12]), (at, d, pth)
    assert seen == w4.shape[0]


def test_the_non_uniform_tree_has_no_implicit_records():
    _, p, t = _packed("plain_17", implicit=True, qnodes=2)
    assert sorted(t.depth[t.leaves]) == [1, 2, 2] and not t.uniform
    assert all(p[name].size == 0 for name in IMPLICIT)


@pytest.mark.parametrize("n", cases.PLAIN_COUNTS)
def test_stack_need_equals_the_layout_of_the_count(n):
    nodes, tris = cases.mesh(f"plain_{n}")
    info = rt.pack_scene(nodes, tris, qnodes=-1)["info"]
    L = rt.bvh_layout(n)
    assert info.anyStack == L.anyStack
    assert (info.nNodes, info.nInner, info.treeDepth, info.nWide4, info.nPairs) == (L.nNodes, L.nInner, L.treeDepth, L.nWide4, L.nPairs)


def test_a_tree_too_deep_is_refused_with_the_upload_s_message():
    nodes, tris = cases.chain(33)
    with pytest.raises(rt.RtError) as e:
        rt.pack_scene(nodes, tris, qnodes=-1)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED and "tree depth 34 exceeds the 32-entry traversal stack" in str(e.value)
