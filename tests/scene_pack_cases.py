"""The meshes and option sets of the scene-pack checks (tests/test_scene_pack_host.py, tests/test_gpu_scene_pack.py and the recorder of
tests/golden/scene_pack_parent.json), in one place so that the recorder and the tests cannot drift apart.

Meshes: the corpus meshes whose numbers or ties are hard on a packer (flat boxes, one box a thousand times, a point, signed zeros, denormal and huge
coordinates, degenerate triangles), and plain random triangles at the counts where the tree changes shape: a single leaf (1, 8), the smallest inner
root (9), a non-uniform tree (17: a leaf at depth 1 and leaves at depth 2), uniform trees with odd leaf counts (40: eight leaves of five, so three pair
records per leaf and a non-zero leaf-box magic) and with mixed 7 / 8 leaves (1000, depth 7)."""
import functools

import numpy as np

import bvh_build_ref as ref
import opengl_raytracing_amd as rt

CORPUS = ("floor_grid", "identical", "point", "signed_zero", "denormal", "huge", "degenerate")
PLAIN_COUNTS = (1, 8, 9, 16, 17, 40, 100, 1000)
PLAIN = tuple(f"plain_{n}" for n in PLAIN_COUNTS)
MESHES = CORPUS + PLAIN

# name -> (environment of an upload, the same as rt.pack_scene options)
OPTION_SETS = {
    "default": ({}, {"qnodes": -1}),
    "qnodes0": ({"RT_QNODES": "0"}, {"qnodes": 0}),
    "qnodes2": ({"RT_QNODES": "2"}, {"qnodes": 2}),
    "qnodes2_sparse": ({"RT_QNODES": "2", "RT_QNODES_SPARSE_BOXES": "1"}, {"qnodes": 2, "sparse_leaf_boxes": True}),
    "anyhit_sah": ({"RT_ANYHIT_TREE": "sah"}, {"anyhit_sah": True}),
}
# ... and the option sets under which an upload builds the arrays the commit before the move could not show (tests/test_gpu_scene_pack.py)
OPTIONAL_SETS = {
    "fused": ({"RT_FUSED": "1"}, {"fused": True}),
    "implicit": ({"RT_IMPLICIT": "1"}, {"implicit": True}),
    "implicit_qnodes2": ({"RT_IMPLICIT": "1", "RT_QNODES": "2"}, {"implicit": True, "qnodes": 2}),
}
PACK_VARS = ("RT_QNODES", "RT_QNODES_SPARSE_BOXES", "RT_ANYHIT_TREE", "RT_FUSED", "RT_IMPLICIT", "RT_VERBOSE")
INFO_FIELDS = ("nNodes", "nTris", "nInner", "treeDepth", "nWide4", "nPairs", "bytesNodes2", "bytesNodes4", "bytesPairs", "bytesTris", "nFused", "flags",
               "implicitDepth")


@functools.lru_cache(maxsize=None)
def mesh(name):
    """-> (nodes12, tris12) of the host builder."""
    if name.startswith("plain_"):
        n = int(name[6:])
        t9 = np.random.default_rng(500 + n).normal(0, 1, (n, 9)).astype(np.float32)
    else:
        t9 = ref.gather(*_corpus()[name])
    nodes, tris = rt.build_bvh(t9)
    nodes.setflags(write=False); tris.setflags(write=False)
    return nodes, tris


@functools.lru_cache(maxsize=1)
def _corpus():
    return ref.corpus(None)


def chain(n_inner):
    """A chain-shaped tree: n_inner inner nodes, each with one leaf child (one triangle) and the next inner node; the last has two leaves.  Depth
    n_inner + 1; every box is the union of its children's."""
    n_tris = n_inner + 1
    t9 = np.random.default_rng(77).normal(0, 1, (n_tris, 9)).astype(np.float32)
    tris = np.zeros((n_tris, 12), np.float32)
    tris[:, 0:3], tris[:, 4:7], tris[:, 8:11] = t9[:, 0:3], t9[:, 3:6], t9[:, 6:9]
    v = np.stack([t9[:, 0:3], t9[:, 0:3] + t9[:, 3:6], t9[:, 0:3] + t9[:, 6:9]])
    lo, hi = v.min(0), v.max(0)
    nodes = np.zeros((2 * n_inner + 1, 12), np.float32)
    # node 2k: inner (children 2k + 1 = leaf of triangle k, 2k + 2 = the rest); the last node: the leaf of the last triangle
    for k in range(n_inner, -1, -1):
        if k == n_inner:
            nodes[2 * k, 0:3], nodes[2 * k, 4:7], nodes[2 * k, 8], nodes[2 * k, 9] = lo[k], hi[k], k, 1
            continue
        leaf, rest = 2 * k + 1, 2 * k + 2
        nodes[leaf, 0:3], nodes[leaf, 4:7], nodes[leaf, 8], nodes[leaf, 9] = lo[k], hi[k], k, 1
        nodes[2 * k, 0:3], nodes[2 * k, 4:7] = np.minimum(lo[k], nodes[rest, 0:3]), np.maximum(hi[k], nodes[rest, 4:7])
        nodes[2 * k, 3], nodes[2 * k, 7] = leaf, rest
    return nodes, tris
