"""The definition of the device BVH builders (rt_build_bvh_gpu, rt_mesh_rebuild, rt_mesh_refit), restated in plain numpy so that it can
be compared with them bit for bit -- ties included.  TEST INFRASTRUCTURE.  It imports numpy only and never calls the library, so what it says is
independent of every line of the product.

The tree (bvh.cpp:41-135 of the reference):
  * a range [b, e) of the triangle permutation is a leaf when e - b <= 8, else it splits at mid = (b + e) // 2;
  * nodes are numbered in pre-order (a node, its left subtree, its right subtree);
  * leaves are re-packed by a LIFO walk that pushes left then right, so the RIGHT subtree's leaves come first: the rows of the leaf [b, e) are
    [n - e, n - b), in the order the range holds them;
  * a node's box is the min / max over its range of the triangles' corners v0, v0 + e1, v0 + e2 (fp32), reduced in the order of the sortable key
    (u ^ 0xFFFFFFFF for negative floats, u | 0x80000000 otherwise), a total order in which -0 lies below +0;
  * the split axis comes from the fp32 extents: (ex > ey) ? ((ex > ez) ? 0 : 2) : ((ey > ez) ? 1 : 2);
  * THE TIE RULE: level by level, every inner range is sorted STABLY by the sortable key of the centroid ((v0 + v1) + v2) * f32(1/3) along its
    axis, starting from the order the level above left, and level 0 starts from input order.  Equal keys therefore keep the order they had.
"""
import numpy as np

f32 = np.float32
LEAF_MAX = 8
COORDS = [0, 1, 2, 4, 5, 6, 8, 9, 10]


# ---------------------------------------------------------------- keys

def sortable(x):
    """float32 -> uint32 whose unsigned order is the float order, with -0 below +0."""
    u = np.ascontiguousarray(x, f32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), u ^ np.uint32(0xFFFFFFFF), u | np.uint32(0x80000000)).astype(np.uint32)


def unsortable(s):
    s = np.ascontiguousarray(s, np.uint32)
    return np.where(s & np.uint32(0x80000000), s & np.uint32(0x7FFFFFFF), s ^ np.uint32(0xFFFFFFFF)).astype(np.uint32).view(f32)


def tri_keys(tris9):
    """Per triangle: (lo [n,3], hi [n,3], centroid [n,3]) as sortable keys."""
    t = np.ascontiguousarray(tris9, f32).reshape(-1, 9)
    with np.errstate(all="ignore"):
        v0 = t[:, 0:3]
        v1 = (v0 + t[:, 3:6]).astype(f32)
        v2 = (v0 + t[:, 6:9]).astype(f32)
        cen = (((v0 + v1).astype(f32) + v2).astype(f32) * f32(1.0 / 3.0)).astype(f32)
    k = np.stack([sortable(v0), sortable(v1), sortable(v2)])
    return k.min(0), k.max(0), sortable(cen)


# ---------------------------------------------------------------- the shape of the tree: the triangle count alone decides it

def tree_shape(n):
    """-> (begin, end, left, right, depth) per node in pre-order; left = right = -1 for a leaf."""
    begin, end, left, right, depth = [], [], [], [], []
    todo = [(0, n, -1, False, 0)]          # a stack: the left range is pushed last, so it is numbered first
    while todo:
        b, e, parent, is_right, d = todo.pop()
        me = len(begin)
        begin.append(b); end.append(e); left.append(-1); right.append(-1); depth.append(d)
        if parent >= 0:
            (right if is_right else left)[parent] = me
        if e - b > LEAF_MAX:
            mid = (b + e) // 2
            todo.append((mid, e, me, True, d + 1))
            todo.append((b, mid, me, False, d + 1))
    return tuple(np.array(a, np.int64) for a in (begin, end, left, right, depth))


def _range_reduce(op, keys, b, e):
    """op over keys[b[i]:e[i]] along axis 0 for disjoint ascending ranges."""
    idx = np.stack([b, e], 1).reshape(-1)
    if idx[-1] >= keys.shape[0]:
        idx = idx[:-1]
    return op.reduceat(keys, idx, axis=0)[::2]


# ---------------------------------------------------------------- build

def split_axis(ex, ey, ez):
    """The axis a range splits along, from the fp32 extents of its box: equal extents fall to the later axis."""
    return np.where(ex > ey, np.where(ex > ez, 0, 2), np.where(ey > ez, 1, 2))


def level_sort(key):
    """The permutation that sorts one level's keys (range rank << 32 | centroid key): stable, so equal keys keep the order they had."""
    return np.argsort(key, kind="stable")


def ref_build(tris9, stats=None):
    """-> (nodes12 [nNodes,12] float32, tris12 [n,12] float32, order [n] int32) as the device builders must produce them.
    stats (a dict) receives "tied_medians": the inner nodes whose two centroid keys on either side of the median are bit-equal."""
    t9 = np.ascontiguousarray(tris9, f32).reshape(-1, 9)
    n = t9.shape[0]
    assert n >= 1
    lo, hi, cen = tri_keys(t9)
    begin, end, left, right, depth = tree_shape(n)
    n_nodes = begin.size
    box = np.zeros((n_nodes, 6), np.uint32)
    perm = np.arange(n, dtype=np.int64)
    tied = 0
    for d in range(int(depth.max()) + 1):
        ids = np.flatnonzero(depth == d)            # pre-order ids ascend with the ranges' starts
        b, e = begin[ids], end[ids]
        box[ids, 0:3] = _range_reduce(np.minimum, lo[perm], b, e)
        box[ids, 3:6] = _range_reduce(np.maximum, hi[perm], b, e)
        inner = left[ids] >= 0
        if not inner.any():
            continue
        ids, b, e = ids[inner], b[inner], e[inner]
        with np.errstate(all="ignore"):
            ext = (unsortable(box[ids, 3:6]) - unsortable(box[ids, 0:3])).astype(f32)
        ex, ey, ez = ext[:, 0], ext[:, 1], ext[:, 2]
        axis = split_axis(ex, ey, ez)
        # the positions of this level's inner ranges, ascending, with the rank of their range
        size = e - b
        offs = np.cumsum(size) - size
        rank = np.repeat(np.arange(ids.size, dtype=np.int64), size)
        pos = np.repeat(b - offs, size) + np.arange(int(size.sum()), dtype=np.int64)
        tri = perm[pos]
        key = cen[tri, axis[rank]].astype(np.uint64) | (rank.astype(np.uint64) << np.uint64(32))
        by = level_sort(key)
        perm[pos] = tri[by]
        skey = key[by]
        mid_at = offs + (b + e) // 2 - b                           # index, within `pos`, of every range's median position
        tied += int((skey[mid_at] == skey[mid_at - 1]).sum())
    if stats is not None:
        stats["tied_medians"] = tied
    leaf = left < 0
    lb, le = begin[leaf], end[leaf]                                # the leaves in pre-order tile [0, n) in ascending order
    out_of_pos = np.repeat(n - le - lb, le - lb) + np.arange(n, dtype=np.int64)      # position b + k of the leaf [b, e) -> row (n - e) + k
    order = np.zeros(n, np.int32)
    order[out_of_pos] = perm
    nodes12 = np.zeros((n_nodes, 12), f32)
    nodes12[:, 0:3] = unsortable(box[:, 0:3])
    nodes12[:, 4:7] = unsortable(box[:, 3:6])
    nodes12[:, 3] = left
    nodes12[:, 7] = right
    nodes12[:, 8] = np.where(leaf, n - end, -1)
    nodes12[:, 9] = np.where(leaf, end - begin, 0)
    return nodes12, rows_of(t9, order), order


def rows_of(tris9, order):
    """tris12 rows (v0, 0, e1, 0, e2, 0) of the input triangles order[row]."""
    t9 = np.ascontiguousarray(tris9, f32).reshape(-1, 9)
    t12 = np.zeros((t9.shape[0], 12), f32)
    t12[:, COORDS] = t9[np.asarray(order, np.int64)]
    return t12


# ---------------------------------------------------------------- refit

def _levels(nodes12):
    """Lists of node ids per depth, from the links."""
    left, right = nodes12[:, 3].astype(np.int64), nodes12[:, 7].astype(np.int64)
    inner = nodes12[:, 9] == 0
    out, cur = [], np.array([0], np.int64)
    while cur.size:
        out.append(cur)
        cur = cur[inner[cur]]
        cur = np.concatenate([left[cur], right[cur]])
    return out


def ref_refit(tris9, order, nodes12, tris12):
    """The same tree over new triangles: rows from tris9[order]; every leaf's box from its rows, every inner node's from its children's, all reduced
    in sortable-key order.  Links, first and count stay.  -> (nodes12, tris12); the inputs are not modified."""
    nodes = np.array(nodes12, f32).reshape(-1, 12)
    t12 = rows_of(tris9, order)
    assert t12.shape == np.asarray(tris12).reshape(-1, 12).shape
    lo, hi, _ = tri_keys(t12[:, COORDS])
    first, count = nodes[:, 8].astype(np.int64), nodes[:, 9].astype(np.int64)
    leaf = np.flatnonzero(count > 0)
    leaf = leaf[np.argsort(first[leaf], kind="stable")]
    box = np.zeros((nodes.shape[0], 6), np.uint32)
    box[leaf, 0:3] = _range_reduce(np.minimum, lo, first[leaf], first[leaf] + count[leaf])
    box[leaf, 3:6] = _range_reduce(np.maximum, hi, first[leaf], first[leaf] + count[leaf])
    left, right = nodes[:, 3].astype(np.int64), nodes[:, 7].astype(np.int64)
    for ids in reversed(_levels(nodes)):
        ids = ids[count[ids] == 0]
        box[ids, 0:3] = np.minimum(box[left[ids], 0:3], box[right[ids], 0:3])
        box[ids, 3:6] = np.maximum(box[left[ids], 3:6], box[right[ids], 3:6])
    nodes[:, 0:3] = unsortable(box[:, 0:3])
    nodes[:, 4:7] = unsortable(box[:, 3:6])
    return nodes, t12


# ---------------------------------------------------------------- validity, from the arrays alone

def check_tree(nodes12, tris12, order, tris9):
    """A well-formed tree over exactly the input triangles: order a permutation, rows = tris9[order], the leaves' ranges cover every row once, every
    leaf's box is the bounds of its rows, every parent's the union of its children's (all in sortable-key order)."""
    nodes = np.asarray(nodes12, f32).reshape(-1, 12)
    t12 = np.asarray(tris12, f32).reshape(-1, 12)
    n = t12.shape[0]
    order = np.asarray(order)
    assert order.shape == (n,) and np.array_equal(np.sort(order), np.arange(n)), "order is not a permutation"
    assert np.array_equal(t12.view(np.uint32), rows_of(tris9, order).view(np.uint32)), "rows are not tris9[order]"
    first, count = nodes[:, 8].astype(np.int64), nodes[:, 9].astype(np.int64)
    leaf = np.flatnonzero(count > 0)
    assert (count[leaf] <= LEAF_MAX).all()
    covered = np.zeros(n + 1, np.int64)
    np.add.at(covered, first[leaf], 1)
    np.add.at(covered, first[leaf] + count[leaf], -1)
    assert (np.cumsum(covered)[:n] == 1).all(), "the leaves do not cover every row exactly once"
    levels = _levels(nodes)
    assert np.array_equal(np.sort(np.concatenate(levels)), np.arange(nodes.shape[0])), "the links do not reach every node exactly once"
    want, _ = ref_refit(tris9, order, nodes, t12)
    assert np.array_equal(want.view(np.uint32), nodes.view(np.uint32)), "a box is not the bounds of its range"


# ---------------------------------------------------------------- the corpus

def gather(positions, indices):
    """Identity-transform triangles (v0, e1, e2) of an indexed mesh, fp32: e1 = b - a, e2 = c - a."""
    p = np.ascontiguousarray(positions, f32).reshape(-1, 3)
    i = np.asarray(indices, np.int64).reshape(-1, 3)
    a, b, c = p[i[:, 0]], p[i[:, 1]], p[i[:, 2]]
    with np.errstate(all="ignore"):
        return np.concatenate([a, (b - a).astype(f32), (c - a).astype(f32)], 1).astype(f32)


def _soup(n, seed, nv=None):
    rng = np.random.default_rng(seed)
    nv = max(3, n // 2 + 3) if nv is None else nv
    return rng.normal(0, 1, (nv, 3)).astype(f32), rng.integers(0, nv, (n, 3)).astype(np.uint32).reshape(-1)


def _grid(g, fn):
    """g x g quads, two triangles each; fn(i, j) -> positions [.., 3] of the (g + 1)^2 vertices."""
    i, j = np.meshgrid(np.arange(g + 1), np.arange(g + 1), indexing="ij")
    v = fn(i.reshape(-1).astype(np.float64), j.reshape(-1).astype(np.float64)).astype(f32)
    q = (np.arange(g)[:, None] * (g + 1) + np.arange(g)[None, :]).reshape(-1)
    f = np.stack([q, q + 1, q + g + 2, q, q + g + 2, q + g + 1], 1).astype(np.uint32).reshape(-1)
    return v, f


def _cube(g, scale):
    """The surface of [-1, 1]^3 in g x g quads per face, scaled per axis: equal extents on the axes whose scales are equal."""
    vs, fs, base = [], [], 0
    for axis in range(3):
        for side in (-1.0, 1.0):
            def face(i, j, axis=axis, side=side):
                p = np.zeros((i.size, 3))
                p[:, axis] = side
                p[:, (axis + 1) % 3] = i * 2.0 / g - 1.0
                p[:, (axis + 2) % 3] = j * 2.0 / g - 1.0
                return p * np.asarray(scale, np.float64)
            v, f = _grid(g, face)
            vs.append(v); fs.append(f + np.uint32(base)); base += v.shape[0]
    return np.concatenate(vs), np.concatenate(fs)


TIE_HEAVY = ("lattice", "floor_grid", "dup8", "identical", "point", "bunny5", "bunny6", "million")
COUNTS = tuple(sorted(set(range(1, 41)) | {c for k in range(4, 13) for c in (2 ** k - 1, 2 ** k, 2 ** k + 1, 8 * 2 ** k - 1, 8 * 2 ** k + 1)}))


def corpus(meshgen=None):
    """name -> (positions [V,3] float32, indices [3n] uint32), every mesh built to hit one thing (see the comments).  Everything is generated from
    seeds.  meshgen: the package's mesh generators; with it the bunny stand-ins and the 1 M-triangle scene join the tie-heavy group."""
    c = {}
    rng = np.random.default_rng(2024)
    # ---- tie-heavy: centroid keys repeat, so medians tie on most levels
    c["lattice"] = (np.round(rng.normal(0, 4, (2500, 3))).astype(f32), rng.integers(0, 2500, (5000, 3)).astype(np.uint32).reshape(-1))
    c["floor_grid"] = _grid(48, lambda i, j: np.stack([i - 24.0, np.full(i.size, 0.5), j - 24.0], 1))        # flat boxes (extent 0 in y)
    v, f = _soup(600, 31)
    c["dup8"] = (v, np.tile(f.reshape(-1, 3), (8, 1)).reshape(-1))                                           # every triangle 8 times, copies apart
    c["identical"] = (np.array([[0.25, -1, 2], [1.5, 0.5, 2.25], [-0.75, 1, 3]], f32), np.tile(np.array([0, 1, 2], np.uint32), 1000))
    c["point"] = (np.tile(np.array([[0.75, -1.25, 2.5]], f32), (7, 1)), rng.integers(0, 7, (300, 3)).astype(np.uint32).reshape(-1))
    if meshgen is not None:
        c["bunny5"] = meshgen.bunny_standin(5)
        c["bunny6"] = meshgen.bunny_standin(6)
        c["million"] = meshgen.million_triangle_scene()
    # ---- axis ties: all three extents equal, and each pair of them
    c["cube_xyz"] = _cube(6, (1, 1, 1))
    c["cube_xy"] = _cube(6, (1, 1, 0.5))
    c["cube_xz"] = _cube(6, (1, 0.5, 1))
    c["cube_yz"] = _cube(6, (0.5, 1, 1))
    # ---- number edges
    sign = np.random.default_rng(7)
    v, f = _grid(24, lambda i, j: np.stack([i - 12.0, np.zeros(i.size), j - 12.0], 1))
    zero = v == 0
    v[zero & (sign.random(v.shape) < 0.5)] = f32(-0.0)                                                       # -0 / +0 mixed per vertex, on all axes
    c["signed_zero"] = (v, f)
    v, f = _soup(700, 41)
    c["denormal"] = ((v.astype(np.float64) * 1e-41).astype(f32), f)
    c["huge"] = ((np.where(sign.random(v.shape) < 0.5, -9e29, 9e29) * (1.0 + 0.02 * v.astype(np.float64))).astype(f32), f)
    tiny = (rng.normal(0, 1, (200, 3)) * 1e-30).astype(f32)
    far = (1e3 + rng.normal(0, 1, (200, 3))).astype(f32)
    c["mixed_scale"] = (np.concatenate([tiny, far]), np.concatenate([rng.integers(0, 200, (300, 3)), rng.integers(200, 400, (300, 3)),
                                                                    rng.integers(0, 400, (40, 3))]).astype(np.uint32).reshape(-1))
    v, f = _soup(400, 43)
    f = f.reshape(-1, 3).copy()
    f[0::5, 1] = f[0::5, 0]                        # two equal vertices: zero area
    f[1::5, 1] = f[1::5, 2] = f[1::5, 0]           # one vertex three times: a point
    v[:40] = v[40:80] * f32(2.0)                   # collinear triples with the origin ...
    f[2::50] = np.array([0, 40, 0], np.uint32)     # ... and a needle through two of them
    c["degenerate"] = (v, f.reshape(-1))
    # ---- counts: the leaf threshold and ragged last levels; half-integer coordinates, so these tie as well
    for n in COUNTS:
        v, f = _soup(n, 1000 + n)
        c[f"count_{n}"] = ((np.round(v * 2) / 2).astype(f32), f)
    return c
