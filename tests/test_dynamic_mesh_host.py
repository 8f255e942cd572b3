"""The dynamic mesh without a GPU: rt_bvh_layout derives, from the triangle count alone, what the host builder and rt_upload_bvh
derive from the tree; the new entry points are exported with the declared signatures and refuse bad arguments without touching a device."""
import ctypes as C

import numpy as np
import pytest

import opengl_raytracing_amd as rt

SIZES = [1, 2, 8, 9, 16, 17, 100, 1000, 20480, 81920] + [int(x) for x in np.random.default_rng(7).integers(3, 60000, 5)]


def _tree_facts(nodes):
    """nNodes, nInner, depth (levels, the root being 1) and pair records (sum of ceil(count / 2) over the leaves) of a built tree."""
    left, right, cnt = nodes[:, 3].astype(int), nodes[:, 7].astype(int), nodes[:, 9].astype(int)
    depth = np.zeros(nodes.shape[0], int)
    depth[0] = 1
    for i in range(nodes.shape[0]):      # pre-order numbering: a parent comes before its children
        if cnt[i] == 0:
            depth[left[i]] = depth[right[i]] = depth[i] + 1
    return nodes.shape[0], int((cnt == 0).sum()), int(depth.max()), int(((cnt[cnt > 0] + 1) // 2).sum())


@pytest.mark.parametrize("n", SIZES)
def test_layout_equals_the_built_tree(n):
    t9 = np.random.default_rng(n).normal(0, 1, (n, 9)).astype(np.float32)
    nodes, tris = rt.build_bvh(t9)
    L = rt.bvh_layout(n)
    assert (L.nTris, L.nNodes, L.nInner, L.treeDepth, L.nPairs) == (n,) + _tree_facts(nodes)
    assert L.bytesNodes2 == max(L.nInner, 1) * 64 and L.bytesPairs == L.nPairs * 80 and L.bytesTris == n * 48
    # four-child records: an inner node at an even level absorbs its inner children
    left, right, cnt = nodes[:, 3].astype(int), nodes[:, 7].astype(int), nodes[:, 9].astype(int)
    n4, stack, todo = 0, {}, [0] if cnt[0] == 0 else []
    order = []
    while todo:
        i = todo.pop()
        order.append(i)
        n4 += 1
        for ch in (left[i], right[i]):
            for k in ([ch] if cnt[ch] > 0 else [left[ch], right[ch]]):
                if cnt[k] == 0:
                    todo.append(k)
    for i in reversed(order):            # S(node) = children - 1 + the deepest inner child's
        kids = [k for ch in (left[i], right[i]) for k in ([ch] if cnt[ch] > 0 else [left[ch], right[ch]])]
        stack[i] = len(kids) - 1 + max([stack[k] for k in kids if cnt[k] == 0], default=0)
    assert L.nWide4 == max(n4, 1)
    assert L.anyStack == (max(stack[0], 1) if n4 else 0)
    assert L.bytesNodes4 in (L.nWide4 * 128, L.nWide4 * 64 + int((cnt > 0).sum()) * 32)


def test_layout_refusals():
    out = rt.RtBvhLayout()
    L = rt.lib()
    assert L.rt_bvh_layout(0, C.byref(out)) == rt.RT_ERR_INVALID
    assert L.rt_bvh_layout(-5, C.byref(out)) == rt.RT_ERR_INVALID
    assert L.rt_bvh_layout(1 << 28, C.byref(out)) == rt.RT_ERR_UNSUPPORTED
    assert L.rt_bvh_layout((1 << 31) - 1, C.byref(out)) == rt.RT_ERR_UNSUPPORTED
    assert L.rt_bvh_layout(5, None) == rt.RT_ERR_INVALID
    with pytest.raises(rt.RtError) as e:
        rt.bvh_layout(0)
    assert e.value.code == rt.RT_ERR_INVALID
    big = rt.bvh_layout((1 << 28) - 1)            # the largest accepted count is laid out in O(log n)
    assert big.nTris == (1 << 28) - 1 and big.treeDepth <= 32 and big.nInner == big.nNodes // 2


def test_quantised_rule_follows_the_environment(monkeypatch):
    monkeypatch.setenv("RT_QNODES", "2")
    assert rt.bvh_layout(1000).quantised == 1 and rt.bvh_layout(8).quantised == 0      # a single leaf has no four-child tree
    monkeypatch.setenv("RT_QNODES", "0")
    assert rt.bvh_layout(1 << 20).quantised == 0
    monkeypatch.delenv("RT_QNODES")
    assert rt.bvh_layout(81920).quantised == 0 and rt.bvh_layout(1 << 20).quantised == 1   # beyond 4 MB of 112-byte nodes


def test_entry_points_exported_and_null_safe():
    L = rt.lib()
    names = ["rt_bvh_layout", "rt_mesh_upload", "rt_mesh_positions", "rt_mesh_set_positions", "rt_mesh_rebuild", "rt_get_mesh_info", "rt_debug_read_scene"]
    for n in names:
        assert n in rt.SIGNATURES and hasattr(L, n)
    v = np.zeros((3, 3), np.float32)
    idx = np.arange(3, dtype=np.uint32)
    U32 = C.POINTER(C.c_uint32)
    assert L.rt_mesh_upload(None, v.ctypes.data_as(C.POINTER(C.c_float)), 3, idx.ctypes.data_as(U32), 3) == rt.RT_ERR_INVALID
    assert L.rt_mesh_rebuild(None, None) == rt.RT_ERR_INVALID
    assert L.rt_mesh_set_positions(None, v.ctypes.data_as(C.POINTER(C.c_float))) == rt.RT_ERR_INVALID
    p, n = C.c_void_p(), C.c_size_t()
    assert L.rt_mesh_positions(None, C.byref(p), C.byref(n)) == rt.RT_ERR_INVALID
    assert L.rt_get_mesh_info(None, C.byref(rt.RtMeshInfo())) == rt.RT_ERR_INVALID
    assert L.rt_debug_read_scene(None, 0, None, 0, C.byref(n)) == rt.RT_ERR_INVALID
    assert C.sizeof(rt.RtBvhLayout) == 64 and C.sizeof(rt.RtMeshInfo) == 48
