"""The box query's definition restated in numpy float32, independent of the library's C++: the 13-axis separating-axis test with
every fmaf of 23.1 through analytic_ref.fma32, by brute force over all rows and vectorised over the boxes; the path mask (every node box from the
root to a row's leaf overlaps the query) computed separately; the walk order and `visits` from an explicit walk that takes the right child first.
Also a float64 separating-axis test on the float64 vertices v0, v0 + e1, v0 + e2, and the box sets the box tests share (meshes: nearest_ref.MESHES)."""
import functools

import numpy as np

import analytic_ref as ar
import nearest_ref
import overlap_ref as orf

f32 = np.float32
MESHES = nearest_ref.MESHES
mesh = nearest_ref.mesh
_idx = nearest_ref._idx
_min3, _max3, boxes_overlap, _leaves = orf.min3, orf.max3, orf.boxes_overlap, orf.leaves
# the ten axes that are not box axes, in the order of Sat.sep[3:]
AXES = ("normal", "e1 x X", "e1 x Y", "e1 x Z", "(e2-e1) x X", "(e2-e1) x Y", "(e2-e1) x Z", "e2 x X", "e2 x Y", "e2 x Z")


def live(boxes):
    """[N] bool: neither a NaN component nor lo > hi on any axis."""
    with np.errstate(all="ignore"):
        return (boxes[:, 0:3] <= boxes[:, 3:6]).all(1)


def _edge_axis(n1, n2, v1, v2, l1, h1, l2, h2):
    """One axis cross(unit_k, f) with the components n1, n2 [T] on the coordinates i, j; v1, v2: (a, b, c) coordinates i and j, each [T]; l1 .. h2 [N].
    -> [N,T] bool: the axis separates."""
    with np.errstate(all="ignore"):
        p = [ar.fma32(q2, n2, (q1 * n1).astype(f32)) for q1, q2 in zip(v1, v2)]
        tmin, tmax = _min3(*p)[None], _max3(*p)[None]
        l1p, h1p = (l1[:, None] * n1[None]).astype(f32), (h1[:, None] * n1[None]).astype(f32)
        m1, M1 = np.fmin(l1p, h1p), np.fmax(l1p, h1p)
        bmin = np.fmin(ar.fma32(l2[:, None], n2[None], m1), ar.fma32(h2[:, None], n2[None], m1))
        bmax = np.fmax(ar.fma32(l2[:, None], n2[None], M1), ar.fma32(h2[:, None], n2[None], M1))
        return (tmax < bmin) | (bmax < tmin)


class Sat:
    """The triangle test of 23.1 for boxes [N,6] against every row [T,12]: sep [13,N,T] bool -- whether the box axes x, y, z, the normal and the nine
    edge axes (AXES) separate -- and accept [N,T], no axis separating and the box live."""

    def __init__(self, tris12, boxes):
        tris12, boxes = np.asarray(tris12, f32), np.ascontiguousarray(boxes[:, :6], f32)
        lo, hi = boxes[:, 0:3], boxes[:, 3:6]
        v0, e1, e2 = tris12[:, 0:3], tris12[:, 4:7], tris12[:, 8:11]
        with np.errstate(all="ignore"):
            a, b, c = v0, (v0 + e1).astype(f32), (v0 + e2).astype(f32)
            tmin, tmax = _min3(a, b, c), _max3(a, b, c)
            sep = [(tmax[None, :, k] < lo[:, None, k]) | (hi[:, None, k] < tmin[None, :, k]) for k in range(3)]
            n = ar.cross(e1, e2)
            d = ar.dot(n, a)[None]
            L, H, nn = lo[:, None], hi[:, None], n[None]
            lx, hx = (nn[..., 0] * L[..., 0]).astype(f32), (nn[..., 0] * H[..., 0]).astype(f32)
            bmin, bmax = np.fmin(lx, hx), np.fmax(lx, hx)
            for k in (1, 2):                               # dot's own steps over the box's corners, the least and the greatest kept at each
                bmin = np.fmin(ar.fma32(nn[..., k], L[..., k], bmin), ar.fma32(nn[..., k], H[..., k], bmin))
                bmax = np.fmax(ar.fma32(nn[..., k], L[..., k], bmax), ar.fma32(nn[..., k], H[..., k], bmax))
            sep.append((d < bmin) | (bmax < d))
            for f in (e1, (e2 - e1).astype(f32), e2):
                for k in range(3):                         # cross(unit_k, f): n1 = -f[j] on coordinate i, n2 = f[i] on coordinate j; (i, j) = (k+1, k+2)
                    i, j = (k + 1) % 3, (k + 2) % 3
                    sep.append(_edge_axis(-f[:, j], f[:, i], (a[:, i], b[:, i], c[:, i]), (a[:, j], b[:, j], c[:, j]), lo[:, i], hi[:, i], lo[:, j], hi[:, j]))
        self.sep = np.stack(sep)
        self.live = live(boxes)
        self.accept = ~self.sep.any(0) & self.live[:, None]


def Walk(nodes12, n_tris, boxes):
    """overlap_ref.Walk for boxes [N,6]: a node is entered where its box overlaps the query box."""
    boxes = np.ascontiguousarray(boxes[:, :6], f32)
    alive = live(boxes)
    return orf.Walk(nodes12, n_tris, orf.box_enter(nodes12, boxes, alive), alive)


def Answer(nodes12, tris12, boxes):
    """overlap_ref.Answer of Sat and Walk for boxes against (nodes12, tris12)."""
    return orf.Answer(Sat(tris12, boxes), Walk(nodes12, tris12.shape[0], boxes))


def sat64(tris12, boxes):
    """[N,T] bool: the separating-axis test in float64 on the float64 vertices v0, v0 + e1, v0 + e2, axes from the float64 edges b - a, c - b, a - c,
    the box projected by the same min / max of products.  A NaN never separates; dead boxes accept nothing."""
    t, q = np.asarray(tris12, np.float64), np.asarray(boxes[:, :6], np.float64)
    lo, hi = q[:, None, 0:3], q[:, None, 3:6]
    a = t[None, :, 0:3]
    b, c = a + t[None, :, 4:7], a + t[None, :, 8:11]
    with np.errstate(all="ignore"):
        sep = ((np.maximum(np.maximum(a, b), c) < lo) | (hi < np.minimum(np.minimum(a, b), c))).any(-1)
        axes = [np.cross(b - a, c - a)]
        for f in (b - a, c - b, a - c):
            for k in range(3):
                axes.append(np.cross(np.eye(3)[k][None, None, :], f))
        for ax in axes:
            pa, pb, pc = ((ax * v).sum(-1) for v in (a, b, c))
            pl, ph = ax * lo, ax * hi
            bmin, bmax = np.fmin(pl, ph).sum(-1), np.fmax(pl, ph).sum(-1)
            sep |= (np.fmax(np.fmax(pa, pb), pc) < bmin) | (bmax < np.fmin(np.fmin(pa, pb), pc))
    return ~sep & live(np.asarray(boxes, f32))[:, None]


# ---------------------------------------------------------------- the box sets the tests share

def _directed(a, b, c, rng, per_axis):
    """Boxes placed to be parted from one row by one of the ten non-box axes alone.  Edge axis cross(unit_k, f): the box spans the row generously along
    k; in the plane of the other two coordinates it is a small rectangle just beyond the midpoint of the edge's projection.  Normal: a small cube just
    off the centroid along the normal."""
    out = []
    T = a.shape[0]
    A, B, Cc = a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)
    for _ in range(per_axis):
        t = int(rng.integers(0, T))
        P = (A[t], B[t], Cc[t])
        size = max(float(np.linalg.norm(P[1] - P[0])), float(np.linalg.norm(P[2] - P[0])), 1e-6)
        nrm = np.cross(P[1] - P[0], P[2] - P[0])
        if np.linalg.norm(nrm) > 0:
            nrm /= np.linalg.norm(nrm)
            h = 0.04 * size * rng.uniform(0.3, 1.0)
            ctr = (P[0] + P[1] + P[2]) / 3 + nrm * rng.choice((-1.0, 1.0)) * (h * np.abs(nrm).sum() + 0.3 * h)
            out.append(np.concatenate([ctr - h, ctr + h]))
        for (p, q, r) in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):           # the edge p -> q, the third vertex r
            for k in range(3):
                i, j = (k + 1) % 3, (k + 2) % 3
                e2d = np.array([P[q][i] - P[p][i], P[q][j] - P[p][j]])
                L = np.linalg.norm(e2d)
                if L == 0:
                    continue
                o = np.array([e2d[1], -e2d[0]]) / L                     # a unit normal of the projected edge, turned away from the third vertex
                mid = np.array([(P[p][i] + P[q][i]) * 0.5, (P[p][j] + P[q][j]) * 0.5])
                if o @ (np.array([P[r][i], P[r][j]]) - mid) > 0:
                    o = -o
                h = 0.04 * L * rng.uniform(0.3, 1.0)
                ctr = mid + o * (h * np.abs(o).sum() + 0.3 * h)
                lo, hi = np.zeros(3), np.zeros(3)
                lo[i], lo[j], hi[i], hi[j] = ctr[0] - h, ctr[1] - h, ctr[0] + h, ctr[1] + h
                lo[k] = min(P[0][k], P[1][k], P[2][k]) - size
                hi[k] = max(P[0][k], P[1][k], P[2][k]) + size
                out.append(np.concatenate([lo, hi]))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def case(name):
    """(nodes12, tris12, boxes [N,6]) with N >= 2 049, seeded: boxes centred on and near the surface with half-extents 2^-k of the root extent per axis;
    a face placed exactly at a vertex coordinate (touching); degenerate boxes lo == hi at a vertex and elsewhere; boxes flat on one axis cutting
    through the mesh; boxes flush with leaf-box faces; the root box and +-inf boxes; boxes far away; boxes placed for single axes (_directed); NaN and
    inverted boxes; every 97th box an empty slot."""
    nodes, tris = mesh(name)
    rng = np.random.default_rng(57 + len(name))
    v0, e1, e2 = tris[:, 0:3], tris[:, 4:7], tris[:, 8:11]
    a, b, c = v0, (v0 + e1).astype(f32), (v0 + e2).astype(f32)
    T = tris.shape[0]
    lo, hi = nodes[0, 0:3].astype(np.float64), nodes[0, 4:7].astype(np.float64)
    ext = np.maximum(hi - lo, 1e-3 * float((hi - lo).max()))
    mid = (lo + hi) * 0.5
    B = []

    def surface(m):
        k = rng.integers(0, T, m)
        w = rng.dirichlet((1, 1, 1), m)
        return a[k] * w[:, 0:1] + b[k] * w[:, 1:2] + c[k] * w[:, 2:3]

    def about(ctr, m):                                               # half-extents 2^-k of the root extent, k per axis
        half = ext * 2.0 ** -rng.integers(1, 11, (m, 3))
        return np.concatenate([ctr - half, ctr + half], 1)

    B.append(about(surface(500), 500))
    B.append(about(surface(250) + rng.normal(size=(250, 3)) * 0.05 * ext, 250))
    # touching: lo[k] (or hi[k]) is exactly the largest (least) coordinate of a row on axis k, the box lies beyond it and holds that vertex otherwise
    tmin, tmax = np.fmin(np.fmin(a, b), c), np.fmax(np.fmax(a, b), c)
    for _ in range(150):
        t, k, up = int(rng.integers(0, T)), int(rng.integers(0, 3)), bool(rng.integers(0, 2))
        V = np.stack([a[t], b[t], c[t]]).astype(np.float64)
        vtx = V[np.argmax(V[:, k]) if up else np.argmin(V[:, k])]
        half = ext * 2.0 ** -rng.integers(2, 8, 3)
        blo, bhi = vtx - half, vtx + half
        if up:
            blo[k] = tmax[t, k]
        else:
            bhi[k] = tmin[t, k]
        B.append(np.concatenate([blo, bhi])[None])
    k = rng.integers(0, T, 100)
    B.append(np.concatenate([a[k], a[k]], 1))                        # lo == hi at a vertex
    p = rng.uniform(lo, hi, (50, 3)).astype(f32)
    B.append(np.concatenate([p, p], 1))                              # ... and elsewhere
    flat = np.concatenate([np.tile(lo - 0.1 * ext, (150, 1)), np.tile(hi + 0.1 * ext, (150, 1))], 1)
    ax = rng.integers(0, 3, 150)
    at = np.where(rng.random(150) < 0.5, rng.uniform(lo, hi, (150, 3))[np.arange(150), ax], surface(150)[np.arange(150), ax]).astype(f32)
    flat[np.arange(150), ax] = at
    flat[np.arange(150), 3 + ax] = at
    B.append(flat)                                                   # flat on one axis, cutting through the mesh
    leaves = _leaves(nodes)
    k = leaves[rng.integers(0, leaves.size, 200)]
    llo, lhi = nodes[k, 0:3].astype(np.float64), nodes[k, 4:7].astype(np.float64)
    ctr = rng.uniform(llo, lhi)
    half = np.maximum(lhi - llo, 0.02 * ext) * rng.uniform(0.2, 1.5, (200, 3))
    flush = np.concatenate([ctr - half, ctr + half], 1).astype(f32)
    ax = rng.integers(0, 3, 200)
    below = rng.random(200) < 0.5                                    # the box ends exactly where the leaf box begins, or begins where it ends
    rows = np.arange(200)
    flush[rows, np.where(below, 3 + ax, ax)] = np.where(below, nodes[k, ax], nodes[k, 4 + ax])
    other = np.where(below, ax, 3 + ax)
    flush[rows, other] = np.where(below, flush[rows, 3 + ax] - half[rows, ax], flush[rows, ax] + half[rows, ax]).astype(f32)
    B.append(flush)
    inf = np.inf
    B.append(np.array([np.concatenate([nodes[0, 0:3], nodes[0, 4:7]]), [-inf, -inf, -inf, inf, inf, inf], [-inf, lo[1], lo[2], mid[0], hi[1], hi[2]],
                       [lo[0], mid[1], -inf, hi[0], inf, inf], [mid[0], -inf, -inf, inf, inf, mid[2]], [-inf, -inf, -inf, -inf, -inf, -inf],
                       [inf, inf, inf, inf, inf, inf], [-inf, -inf, -inf, lo[0] - 1, inf, inf], [-3e38, -3e38, -3e38, 3e38, 3e38, 3e38],
                       [-1e30, -1e30, -1e30, 1e30, 1e30, mid[2]]]))
    dirs = rng.normal(size=(100, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    B.append(about(mid + dirs * float(ext.max()) * 10.0 ** rng.uniform(0.5, 3.0, (100, 1)), 100))
    B.append(_directed(a, b, c, rng, 40))
    bad = about(np.tile(mid, (12, 1)), 12)
    for j in range(6):
        bad[j, j] = np.nan
    for j in range(3):
        bad[6 + j, [j, 3 + j]] = bad[6 + j, [3 + j, j]] + np.array([1e-3, 0]) * ext[j]      # lo > hi on one axis
        bad[9 + j, j] = inf                                                                 # lo = +inf
    B.append(bad)
    boxes = np.concatenate(B).astype(f32)
    if boxes.shape[0] < 2049:
        extra = 2049 - boxes.shape[0]
        boxes = np.concatenate([boxes, about(surface(extra), extra).astype(f32)])
    boxes = np.ascontiguousarray(boxes[rng.permutation(boxes.shape[0])])
    empty = np.arange(0, boxes.shape[0], 97)
    boxes[empty[0::2], 1] = np.nan                                   # every 97th box an empty slot: a NaN, or lo > hi
    boxes[empty[1::2], 5] = boxes[empty[1::2], 2] - f32(1.0)
    boxes.setflags(write=False)
    return nodes, tris, boxes


@functools.lru_cache(maxsize=None)
def reference(name):
    """The numpy definition's Answer on case(name).  Computed once; leave it unchanged."""
    nodes, tris, boxes = case(name)
    return Answer(nodes, tris, boxes)
