"""The triangle query's definition restated in numpy float32, independent of the library's C++: the 20-axis separating-axis test with
every fmaf of 24.1 through analytic_ref.fma32, by brute force over all (query, row) pairs and each axis's verdict kept apart; the path mask (every
node box from the root to a row's leaf overlaps the box of the query's points) computed separately; the walk order and `visits` from an explicit walk
that takes the right child first.  Also a float64 17-axis test on the float64 points, and the query sets the triangle tests share (meshes:
nearest_ref.MESHES)."""
import functools

import numpy as np

import analytic_ref as ar
import nearest_ref
import overlap_ref as orf

f32 = np.float32
MESHES = nearest_ref.MESHES
mesh = nearest_ref.mesh
_idx = nearest_ref._idx
_min3, _max3, _sub, row_points, rows_as_tris, boxes_overlap = orf.min3, orf.max3, orf.sub, orf.row_points, orf.rows_as_tris, orf.boxes_overlap
_leaves, _rotation = orf.leaves, orf.rotation
# the seventeen projected axes, in the order of Sat.sep[3:]
AXES = ("n", "m", "f1 x g1", "f1 x g2", "f1 x g3", "f2 x g1", "f2 x g2", "f2 x g3", "f3 x g1", "f3 x g2", "f3 x g3", "n x f1", "n x f2", "n x f3",
        "m x g1", "m x g2", "m x g3")
IN_PLANE = slice(3 + 11, 3 + 17)                           # Sat.sep rows of the six in-plane axes


def live(q9):
    """[N] bool: none of the nine components is a NaN."""
    return ~np.isnan(q9[:, :9]).any(1)


def aabb(q9):
    """[N,6] float32: qlo, qhi -- the fmin / fmax of the three points per component."""
    q = np.asarray(q9[:, :9], f32)
    return np.concatenate([_min3(q[:, 0:3], q[:, 3:6], q[:, 6:9]), _max3(q[:, 0:3], q[:, 3:6], q[:, 6:9])], 1)


def _axis_sep(ax, T, Q):
    """ax broadcastable to [N,T,3]; T = (a, b, c) and Q = (p0, p1, p2), each broadcastable likewise -> bool: the axis separates.  A NaN never does."""
    with np.errstate(all="ignore"):
        t = [ar.dot(ax, v) for v in T]
        q = [ar.dot(ax, v) for v in Q]
        return (_max3(*t) < _min3(*q)) | (_max3(*q) < _min3(*t))


class Sat:
    """The triangle test of 24.1 for queries [N,9] against every row [T,12]: sep [20,N,T] bool -- whether the box axes x, y, z and the seventeen
    projected axes (AXES) separate -- and accept [N,T], no axis separating and the query live."""

    def __init__(self, tris12, q9):
        tris12, q9 = np.asarray(tris12, f32), np.ascontiguousarray(q9[:, :9], f32)
        e1, e2 = tris12[:, 4:7], tris12[:, 8:11]
        a, b, c = row_points(tris12)
        p0, p1, p2 = q9[:, 0:3], q9[:, 3:6], q9[:, 6:9]
        box = aabb(q9)
        lo, hi = box[:, 0:3], box[:, 3:6]
        with np.errstate(all="ignore"):
            tmin, tmax = _min3(a, b, c), _max3(a, b, c)
            sep = [(tmax[None, :, k] < lo[:, None, k]) | (hi[:, None, k] < tmin[None, :, k]) for k in range(3)]
            f = (e1, _sub(e2, e1), e2)
            g = (_sub(p1, p0), _sub(p2, p1), _sub(p2, p0))
            n, m = ar.cross(e1, e2), ar.cross(g[0], g[2])
            T = (a[None], b[None], c[None])
            Q = (p0[:, None], p1[:, None], p2[:, None])
            sep.append(_axis_sep(n[None], T, Q))
            sep.append(_axis_sep(m[:, None], T, Q))
            for fi in f:
                for gj in g:
                    sep.append(_axis_sep(ar.cross(fi[None], gj[:, None]), T, Q))
            for fi in f:
                sep.append(_axis_sep(ar.cross(n, fi)[None], T, Q))
            for gj in g:
                sep.append(_axis_sep(ar.cross(m, gj)[:, None], T, Q))
        N, Tn = q9.shape[0], tris12.shape[0]
        self.sep = np.stack([np.broadcast_to(s, (N, Tn)) for s in sep])
        self.live = live(q9)
        self.accept = ~self.sep.any(0) & self.live[:, None]


def Walk(nodes12, n_tris, q9):
    """overlap_ref.Walk for query triangles [N,9]: a node is entered where its box overlaps [qlo, qhi]."""
    alive = live(q9)
    return orf.Walk(nodes12, n_tris, orf.box_enter(nodes12, aabb(q9), alive), alive)


def Answer(nodes12, tris12, q9):
    """overlap_ref.Answer of Sat and Walk for queries against (nodes12, tris12)."""
    return orf.Answer(Sat(tris12, q9), Walk(nodes12, tris12.shape[0], q9))


def sat64(tris12, q9):
    """[N,T] bool: the box axes and the seventeen projected axes in float64 on the float64 points a, a + e1, a + e2 and p0, p1, p2, edges and normals
    from float64 differences.  A NaN never separates; dead queries accept nothing."""
    t, q = np.asarray(tris12, np.float64), np.asarray(q9[:, :9], np.float64)
    a = t[None, :, 0:3]
    b, c = a + t[None, :, 4:7], a + t[None, :, 8:11]
    p0, p1, p2 = q[:, None, 0:3], q[:, None, 3:6], q[:, None, 6:9]
    with np.errstate(all="ignore"):
        lo, hi = np.fmin(np.fmin(p0, p1), p2), np.fmax(np.fmax(p0, p1), p2)
        sep = ((np.fmax(np.fmax(a, b), c) < lo) | (hi < np.fmin(np.fmin(a, b), c))).any(-1)
        f = (b - a, c - b, c - a)
        g = (p1 - p0, p2 - p1, p2 - p0)
        n, m = np.cross(f[0], f[2]), np.cross(g[0], g[2])
        axes = [n, m] + [np.cross(fi, gj) for fi in f for gj in g] + [np.cross(n, fi) for fi in f] + [np.cross(m, gj) for gj in g]
        for ax in axes:
            tp = [(ax * v).sum(-1) for v in (a, b, c)]
            qp = [(ax * v).sum(-1) for v in (p0, p1, p2)]
            sep = sep | (_max3(*tp) < _min3(*qp)) | (_max3(*qp) < _min3(*tp))
    return ~sep & live(np.asarray(q9, f32))[:, None]


# ---------------------------------------------------------------- the query sets the tests share

def _frame(P):
    """An orthonormal frame (u, v, w) of the triangle P [3,3] in float64: u along P1 - P0, w the normal.  None for a zero-area triangle."""
    u = P[1] - P[0]
    w = np.cross(u, P[2] - P[0])
    if np.linalg.norm(u) == 0 or np.linalg.norm(w) == 0:
        return None
    u, w = u / np.linalg.norm(u), w / np.linalg.norm(w)
    return u, np.cross(w, u), w


def _candidates(P, rng, per_family):
    """Query triangles [M,3,3] (float64) placed about the triangle P so that few axes can part them from it: a small tilted triangle just off P's
    interior (n), P just off the interior of a large tilted triangle (m), an edge held skew just off an edge of P (f_i x g_j), a vertex pointing at an
    edge of P from just outside, nearly in P's plane but crossing it (n x f_i), and an edge facing a vertex of P likewise (m x g_j)."""
    fr = _frame(P)
    if fr is None:
        return np.zeros((0, 3, 3))
    u, v, w = fr
    ctr = P.mean(0)
    size = max(np.linalg.norm(P[1] - P[0]), np.linalg.norm(P[2] - P[0]), np.linalg.norm(P[2] - P[1]))
    out = []
    for _ in range(per_family):
        gap = size * 10.0 ** rng.uniform(-3, -1)
        s = rng.choice((-1.0, 1.0))
        # n: a small triangle over the interior, tilted, its lowest point `gap` off the plane
        wts = rng.dirichlet((2, 2, 2))
        at = wts @ P
        r = 0.1 * size * rng.uniform(0.2, 1.0)
        tri = at + r * (rng.normal(size=(3, 1)) * u + rng.normal(size=(3, 1)) * v) + s * w * (gap + r * rng.uniform(0, 1, (3, 1)))
        out.append(tri)
        # m: P over the interior of a large triangle in a plane tilted against P's, `gap` beyond P's nearest point
        R = _rotation(rng)
        tilt = w + 0.3 * (R @ w)
        tilt /= np.linalg.norm(tilt)
        tu = np.cross(tilt, u)
        tu /= np.linalg.norm(tu)
        tv = np.cross(tilt, tu)
        low = min((P - ctr) @ tilt * s) * s
        base = ctr + tilt * (low - s * gap)
        ang = rng.uniform(0, 2 * np.pi) + np.array([0, 2.1, 4.2])
        out.append(base + 4 * size * (np.cos(ang)[:, None] * tu + np.sin(ang)[:, None] * tv))
        # f_i x g_j: an edge held skew across edge i of P from outside, the third point farther out
        for i, (p, q, o) in enumerate(((0, 1, 2), (1, 2, 0), (0, 2, 1))):
            d = P[q] - P[p]
            mid = P[p] + d * rng.uniform(0.25, 0.75)
            outw = np.cross(d, w)
            outw /= np.linalg.norm(outw)
            if outw @ (P[o] - mid) > 0:
                outw = -outw
            away = outw * rng.uniform(0.3, 1.0) + w * rng.choice((-1.0, 1.0)) * rng.uniform(0.3, 1.0)
            away /= np.linalg.norm(away)
            along = np.cross(away, d)
            along /= np.linalg.norm(along)
            along = along + 0.3 * rng.normal() * away + 0.2 * rng.normal() * d / np.linalg.norm(d)
            h = 0.5 * size * rng.uniform(0.2, 1.0)
            e0, e1_ = mid + away * gap - along * h, mid + away * gap + along * h
            far = mid + away * (gap + h * rng.uniform(0.5, 2.0)) + rng.normal(size=3) * 0.2 * h
            order = rng.permutation(3)
            out.append(np.stack([e0, e1_, far])[order])
            # n x f_i: a vertex pointing at edge i from `gap` outside, the triangle crossing P's plane
            tip = mid + outw * gap
            spread = h * rng.uniform(0.3, 1.0)
            b1 = tip + outw * h + (d / np.linalg.norm(d)) * spread * 0.4 + w * spread * rng.uniform(0.05, 0.5)
            b2 = tip + outw * h - (d / np.linalg.norm(d)) * spread * 0.4 - w * spread * rng.uniform(0.05, 0.5)
            out.append(np.stack([tip + w * 1e-3 * gap * rng.normal(), b1, b2])[rng.permutation(3)])
            # m x g_j: an edge facing vertex o of P from `gap` beyond it, the triangle crossing P's plane
            vtx = P[o]
            back = vtx - (P[p] + P[q]) * 0.5
            back /= np.linalg.norm(back)
            side = np.cross(w, back)
            L = 2 * size * rng.uniform(0.5, 1.5)
            lift = w * L * rng.uniform(0.02, 0.2)
            q0, q1 = vtx + back * gap - side * L + lift, vtx + back * gap + side * L - lift
            q2 = vtx + back * (gap + L * rng.uniform(0.3, 1.0)) + w * L * rng.uniform(-0.1, 0.1)
            out.append(np.stack([q0, q1, q2])[rng.permutation(3)])
            # the same two in P's plane as float64 has it.  Only an in-plane axis parts such a pair by more than rounding; on n, m and the nine
            # f_i x g_j, all along the common normal, both triangles project to three nearly equal numbers and part by the chance of rounding, so a good
            # share of these pairs is parted by n x f_i (the tip at the edge) or by m x g_j (the edge at the vertex) alone
            unit = d / np.linalg.norm(d)
            skew = rng.choice((0.4, 2.5))                                # (the far edge not parallel to edge i: its normal would be n x f_i again)
            out.append(np.stack([tip, tip + outw * h * skew + unit * spread * 0.4, tip + outw * h - unit * spread * 0.4])[rng.permutation(3)])
            e0, e1_, e2_ = vtx + back * gap - side * L, vtx + back * gap + side * L, vtx + back * (gap + L * rng.uniform(0.3, 1.0))
            for order in ((0, 1, 2), (2, 0, 1), (0, 2, 1)):               # the facing edge as g1 = p1 - p0, g2 = p2 - p1, g3 = p2 - p0
                out.append(np.stack([e0, e1_, e2_])[list(order)])
    return np.array(out)


def _directed(tris12, rng, rows, per_family, keep):
    """Queries that ONE projected axis alone parts from one row, their boxes overlapping: candidates about `rows` random rows (_candidates), judged by
    the definition above on the (candidate, row) pair alone, at most `keep` kept per axis."""
    T = tris12.shape[0]
    kept = [[] for _ in AXES]
    for t in rng.integers(0, T, rows):
        P = np.stack(row_points(tris12[t:t + 1]), 1)[0].astype(np.float64)
        cand = _candidates(P, rng, per_family).reshape(-1, 9).astype(f32)
        if cand.shape[0] == 0:
            continue
        s = Sat(tris12[t:t + 1], cand).sep[:, :, 0]
        alone = ~s[:3].any(0) & (s[3:].sum(0) == 1)
        for k in range(len(AXES)):
            for j in np.flatnonzero(alone & s[3 + k]):
                if len(kept[k]) < keep:
                    kept[k].append(cand[j])
    return np.array([q for axis in kept for q in axis], f32).reshape(-1, 9)


def _coplanar(tris12, rng, m):
    """Exactly coplanar queries for rows that lie in an axis-aligned plane (all three points share one coordinate bit for bit: the faces of `layers`):
    the query takes that coordinate as it stands and dyadic numbers (multiples of 1/8) in the other two.  Per row, in the frame of its own points:
    overlapping; sharing only an edge; sharing only a vertex; disjoint in the plane with overlapping boxes (inside the row's box beyond its longest
    edge, and an edge of the query facing a vertex of the row)."""
    a, b, c = row_points(tris12)
    out = []
    flat = [(t, k) for t in range(tris12.shape[0]) for k in range(3) if a[t, k] == b[t, k] == c[t, k]]
    if not flat:
        return np.zeros((0, 9), f32)
    for _ in range(m):
        t, k = flat[int(rng.integers(0, len(flat)))]
        A, B, Cc = a[t].astype(np.float64), b[t].astype(np.float64), c[t].astype(np.float64)
        r8 = lambda p: np.where(np.arange(3) == k, A[k], np.round(p * 8) / 8)           # dyadic in the plane, the plane's coordinate as it stands
        ctr = (A + B + Cc) / 3
        s = rng.uniform(0.05, 0.4)
        out.append([r8(ctr + (A - ctr) * s), r8(ctr + (B - ctr) * s), r8(ctr + (Cc - ctr) * s)])          # overlapping: a shrunken copy inside
        out.append([r8(A + (B - A) * 0.25 + (Cc - A) * 0.25), r8(A + (B - A) * 3), r8(A + (Cc - A) * 3)])  # overlapping: pokes through
        for (p, q, o) in ((A, B, Cc), (B, Cc, A), (Cc, A, B)):
            out.append([p, q, r8(p + q - o)])                                             # sharing only the edge p q: the third point mirrored out
            out.append([p, r8(p - (q - p) * s), r8(p - (o - p) * s)])                     # sharing only the vertex p: mirrored through it
            far = p + q - o                                                               # the parallelogram's fourth corner, beyond the edge p q
            out.append([r8(far), r8(far + (p - far) * 0.3), r8(far + (q - far) * 0.3)])   # disjoint beyond the edge p q; for the longest edge inside the row's box
            mid, d = (p + q) / 2, (q - p)
            outw = mid - o
            out.append([r8(p - d + outw * 0.0625), r8(q + d + outw * 0.0625), r8(mid + outw * 2)])   # ... an edge parallel to p q just beyond it
            e = o + (o - mid) * 0.0625                                                    # an edge of the query facing the vertex o, just beyond it
            out.append([r8(e - d * 2), r8(e + d * 2), r8(e + (o - mid) * 2)])
    return np.array(out, np.float64).reshape(-1, 9).astype(f32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(nodes12, tris12, qtris [N,9]) with N >= 2 049, seeded: the mesh's own rows (a, b, c by the definition's adds); those rows translated by 2^-k of
    the root extent, and rotated; random triangles on and near the surface with edges 2^-k of the root extent; exactly coplanar queries on
    axis-aligned faces (_coplanar); queries sharing exactly one point with a row; segment and point queries piercing and lying on faces; queries whose
    box is flush with a leaf box; +-inf, 3e38 and far-away queries; queries one axis alone parts from a row (_directed); every 97th query an empty
    slot, the NaN rotating through the nine components."""
    nodes, tris = mesh(name)
    rng = np.random.default_rng(91 + len(name))
    a, b, c = row_points(tris)
    T = tris.shape[0]
    own = rows_as_tris(tris)
    lo, hi = nodes[0, 0:3].astype(np.float64), nodes[0, 4:7].astype(np.float64)
    ext = np.maximum(hi - lo, 1e-3 * float((hi - lo).max()))
    mid = (lo + hi) * 0.5
    Qs = []

    def pick(m):
        return rng.integers(0, T, m)

    def surface(m):
        k = pick(m)
        w = rng.dirichlet((1, 1, 1), m)
        return a[k] * w[:, 0:1] + b[k] * w[:, 1:2] + c[k] * w[:, 2:3], k

    Qs.append(own[np.arange(min(T, 300))] if T <= 300 else own[rng.choice(T, 300, replace=False)])
    k = pick(250)
    Qs.append(own[k].astype(np.float64) + np.tile(rng.normal(size=(250, 3)) * ext * 2.0 ** -rng.integers(1, 16, (250, 1)), (1, 3)))       # translated
    k = pick(150)
    P = own[k].astype(np.float64).reshape(-1, 3, 3)
    ctr = P.mean(1, keepdims=True)
    Qs.append(np.stack([(P[i] - ctr[i]) @ _rotation(rng).T + ctr[i] for i in range(150)]).reshape(-1, 9))                                  # rotated
    at, _ = surface(500)
    off = rng.normal(size=(500, 3)) * ext * np.where(rng.random((500, 1)) < 0.5, 0.0, 0.03)
    edge = ext * 2.0 ** -rng.integers(1, 11, (500, 1))
    Qs.append(np.concatenate([at + off + rng.normal(size=(500, 3)) * edge * 0.5 for _ in range(3)], 1))                                    # on and near the surface
    Qs.append(_coplanar(tris, rng, 12))
    k = pick(150)                                                                                                                          # exactly one shared point
    shared = np.stack([a, b, c], 1)[k, rng.integers(0, 3, 150)]
    others = [shared + rng.normal(size=(150, 3)) * ext * 2.0 ** -rng.integers(2, 9, (150, 1)) for _ in range(2)]
    one = np.stack([shared.astype(np.float64)] + others, 1)
    Qs.append(np.stack([one[i][rng.permutation(3)] for i in range(150)]).reshape(-1, 9))
    # segments (p1 == p2) and points (p0 == p1 == p2): piercing a face at an interior point, lying in it, and off it
    at, k = surface(120)
    nrm = np.cross((b[k] - a[k]).astype(np.float64), (c[k] - a[k]).astype(np.float64))
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    h = ext.max() * 2.0 ** -rng.integers(2, 10, (120, 1))
    Qs.append(np.concatenate([at + nrm * h, at - nrm * h, at - nrm * h], 1))                                                               # piercing
    at2, k2 = surface(60)
    Qs.append(np.concatenate([a[k2], at2, at2], 1))                                                                                        # lying in the face, from a vertex
    k3 = pick(40)
    Qs.append(np.concatenate([a[k3], b[k3], b[k3]], 1))                                                                                    # ... along an edge
    k3 = pick(60)
    Qs.append(np.tile(np.stack([a, b, c], 1)[k3, rng.integers(0, 3, 60)], (1, 3)))                                                         # a point at a vertex
    at3, _ = surface(60)
    Qs.append(np.tile(at3.astype(f32), (1, 3)))                                                                                            # a point on a face, as rounded
    Qs.append(np.tile(rng.uniform(lo, hi, (40, 3)), (1, 3)))                                                                               # a point elsewhere
    # [qlo, qhi] flush with a leaf box: the query's largest (least) coordinate on one axis is exactly the leaf box's least (largest)
    leaves = _leaves(nodes)
    kl = leaves[rng.integers(0, leaves.size, 200)]
    llo, lhi = nodes[kl, 0:3].astype(np.float64), nodes[kl, 4:7].astype(np.float64)
    half = np.maximum(lhi - llo, 0.02 * ext)
    flush = np.stack([rng.uniform(llo - 0.3 * half, lhi + 0.3 * half) for _ in range(3)], 1).astype(f32)                                   # [200,3,3]
    ax = rng.integers(0, 3, 200)
    below = rng.random(200) < 0.5
    rows = np.arange(200)
    face = np.where(below, nodes[kl, ax], nodes[kl, 4 + ax]).astype(f32)
    for j in range(3):                                                                                                                     # all three points on the far side of the face ...
        d = np.abs(flush[rows, j, ax] - face) + f32(1e-3) * half[rows, ax].astype(f32)
        flush[rows, j, ax] = np.where(below, face - d, face + d)
    flush[rows, rng.integers(0, 3, 200), ax] = face                                                                                        # ... and one of them on it
    Qs.append(flush.reshape(-1, 9))
    inf = np.inf
    big = np.array([[-inf, -inf, -inf, inf, inf, inf, 0, 0, 0], [-inf, 0, 0, inf, 0, 0, 0, inf, 0], [inf, inf, inf, inf, inf, inf, inf, inf, inf],
                    [-inf, -inf, -inf, -inf, -inf, -inf, -inf, -inf, -inf], [lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], inf, mid[1], mid[2]],
                    [-3e38, -3e38, -3e38, 3e38, 3e38, 3e38, 3e38, -3e38, 3e38], [-3e38, mid[1], mid[2], 3e38, mid[1], mid[2], mid[0], 3e38, mid[2]],
                    [3e38, 3e38, 3e38, 3e38, 3e38, 3e38, 3e38, 3e38, 3e38], [-1e30, -1e30, -1e30, 1e30, 1e30, mid[2], mid[0], mid[1], 1e30],
                    [lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], lo[0], hi[1], lo[2]], [-1e20, lo[1], mid[2], 1e20, mid[1], mid[2], mid[0], hi[1], 1e20]])
    Qs.append(big)
    dirs = rng.normal(size=(100, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    far = mid + dirs * float(ext.max()) * 10.0 ** rng.uniform(0.5, 3.0, (100, 1))
    Qs.append(np.concatenate([far + rng.normal(size=(100, 3)) * ext * 0.1 for _ in range(3)], 1))                                          # far away
    Qs.append(_directed(tris, rng, rows=40, per_family=6, keep=4))
    q = np.concatenate([np.asarray(x, np.float64).reshape(-1, 9) for x in Qs]).astype(f32)
    if q.shape[0] < 2049:
        extra = 2049 - q.shape[0]
        at, _ = surface(extra)
        edge = ext * 2.0 ** -rng.integers(1, 9, (extra, 1))
        q = np.concatenate([q, np.concatenate([at + rng.normal(size=(extra, 3)) * edge * 0.5 for _ in range(3)], 1).astype(f32)])
    q = np.ascontiguousarray(q[rng.permutation(q.shape[0])])
    empty = np.arange(0, q.shape[0], 97)
    q[empty, np.arange(empty.size) % 9] = np.nan                      # every 97th query an empty slot, the NaN rotating through the nine components
    q.setflags(write=False)
    return nodes, tris, q


@functools.lru_cache(maxsize=None)
def reference(name):
    """The numpy definition's Answer on case(name).  Computed once; leave it unchanged."""
    nodes, tris, q = case(name)
    return Answer(nodes, tris, q)


@functools.lru_cache(maxsize=None)
def walk(name):
    """The reference Walk alone on case(name): order, path and visits without the triangle test.  Computed once; leave it unchanged."""
    nodes, tris, q = case(name)
    return Walk(nodes, tris.shape[0], q)
