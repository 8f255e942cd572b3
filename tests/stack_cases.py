"""Trees and rays that drive every tree walk to the bound of its LDS stack, and plain-Python models of the two walks that say how far
they get.  Shared by tests/test_stack_cases_host.py (the conditions, on the CPU) and tests/test_gpu_walk_stacks.py (the device).

Rungs: rung k of a fixture is the triangle (x_k, 0, 0), (x_k, 1, 0), (x_k, 0, 1) in the plane x = x_k, so every leaf box and every node box has the
unit square as its y-z cross-section.  A ray that stays inside that square over the whole x range enters EVERY box of the tree; it hits rung k where
y + z < 1 at x_k.  The rays run along x with a slope of 1/128 per coordinate (packets: a little more, from a shared origin) and cross the hypotenuse
y + z = 1 halfway between two rungs, so which rungs a ray hits -- all at or below its rung j, or all at or above -- is known by construction, and so
is its closest hit.

  ladder(n_inner, leaf_left)   a chain in the node layout of scene_pack_cases.chain: inner node 2k has the leaf of rung k (node 2k + 1) and the rest
                               of the chain (node 2k + 2); depth n_inner + 1; x_k = k.  The leaf is the left or the right child at every level.
  slab(D)                      5 << D rungs at x_k = k / 16 through rt.build_bvh: a perfect tree, every leaf (five rungs) at depth D.
"""
import functools
import math

import numpy as np

import opengl_raytracing_amd as rt

f32 = np.float32
LADDER_DEPTHS = (4, 5, 16, 17, 24, 25, 32)
SLAB_DEPTHS = (3, 6, 7)
NO_CHILD = 0x7fffffff
SLOPE = 1.0 / 128.0          # per coordinate: y = z = 1/2 + SLOPE (x - x_cross)
PAD = 1.0                    # the single rays start this far before the first / beyond the last rung
EDGE_MARGIN = {"ladder": 1.0 / 256.0, "slab": 1.0 / 4096.0}
# The distance from the hypotenuse at the rungs next to the crossing is 2 SLOPE (spacing / 2) / sqrt 2: 0.0055 on a ladder (spacing 1), and a sixteenth
# of that on a slab (spacing 1/16), whose 40 units of length do not allow a steeper ray inside the unit square: the slab's margin is the ladder's 1/256
# scaled by the spacing.  The y = 0 and z = 0 edges and the box faces are at least 1/8 away on every fixture.


class Fixture:
    """nodes12, tris12 (read-only), kind ("ladder" / "slab"), x [n + 1] float64 the rungs' planes, row [n + 1] the row of tris12 of rung k,
    rung [T] the rung of a row, depth (the binary tree's, root = 1)."""

    def __init__(self, name, kind, nodes, tris, depth):
        nodes.setflags(write=False); tris.setflags(write=False)
        self.name, self.kind, self.nodes, self.tris, self.depth = name, kind, nodes, tris, depth
        xs = tris[:, 0].astype(np.float64)
        self.row = np.argsort(xs, kind="stable")
        self.x = xs[self.row]
        assert (np.diff(self.x) > 0).all()
        self.rung = np.empty_like(self.row)
        self.rung[self.row] = np.arange(self.row.size)
        self.n = self.row.size - 1               # the last rung
        self.spacing = float(self.x[1] - self.x[0])

    def __repr__(self):
        return self.name


def _rung_rows(x):
    t = np.zeros((x.size, 12), f32)
    t[:, 0] = x
    t[:, 5] = 1.0      # e1 = (0, 1, 0)
    t[:, 10] = 1.0     # e2 = (0, 0, 1)
    return t


@functools.lru_cache(maxsize=None)
def ladder(n_inner, leaf_left):
    n_tris = n_inner + 1
    tris = _rung_rows(np.arange(n_tris, dtype=f32))
    nodes = np.zeros((2 * n_inner + 1, 12), f32)

    def leaf(at, k):
        nodes[at, 0:3], nodes[at, 4:7], nodes[at, 8], nodes[at, 9] = (k, 0, 0), (k, 1, 1), k, 1

    leaf(2 * n_inner, n_inner)
    for k in range(n_inner):
        leaf(2 * k + 1, k)
        nodes[2 * k, 0:3], nodes[2 * k, 4:7] = (k, 0, 0), (n_inner, 1, 1)        # exactly the union of the children's
        nodes[2 * k, 3], nodes[2 * k, 7] = (2 * k + 1, 2 * k + 2) if leaf_left else (2 * k + 2, 2 * k + 1)
    return Fixture(f"ladder{n_inner + 1}{'L' if leaf_left else 'R'}", "ladder", nodes, tris, n_inner + 1)


@functools.lru_cache(maxsize=None)
def slab(D):
    x = np.arange(5 << D, dtype=np.float64) / 16.0
    t9 = np.zeros((x.size, 9), f32)
    t9[:, 0] = x          # (v0, e1, e2), as gather_triangles writes them
    t9[:, 4] = 1.0
    t9[:, 8] = 1.0
    nodes, tris = rt.build_bvh(t9)
    assert np.array_equal(tris[:, 4:7], np.tile(f32([0, 1, 0]), (x.size, 1))) and np.array_equal(tris[:, 8:11], np.tile(f32([0, 0, 1]), (x.size, 1)))
    return Fixture(f"slab{D}", "slab", nodes.copy(), tris.copy(), D + 1)


def ladders(depths=LADDER_DEPTHS):
    return [ladder(d - 1, left) for d in depths for left in (True, False)]


def fixtures():
    return ladders() + [slab(D) for D in SLAB_DEPTHS]


def by_name(name):
    if name.startswith("slab"):
        return slab(int(name[4:]))
    return ladder(int(name[6:-1]) - 1, name[-1] == "L")


# ---------------------------------------------------------------- rays

class Rays:
    """org, dirs [N,3] float32 and tmax [N] float32 (the any-hit limit); per ray, by construction: first (the rung of the closest hit, -1: a miss),
    t_first (float64, along the float32 ray), hits [N] (how many rungs the unbounded ray hits), lo / hi (it hits exactly the rungs lo .. hi),
    occluded (a rung it hits lies within tmax: the first one and no other)."""


def _make(fx, origin, cross_x, above, n_rays=None):
    """Rays from `origin` [N,3] through (cross_x, 1/2, 1/2); above [N] bool: the ray hits the rungs with x > cross_x (else x < cross_x)."""
    r = Rays()
    o64 = np.asarray(origin, np.float64)
    c64 = np.stack([cross_x, np.full_like(cross_x, 0.5), np.full_like(cross_x, 0.5)], 1)
    d64 = c64 - o64
    d64 /= np.linalg.norm(d64, axis=1, keepdims=True)
    r.org, r.dirs = o64.astype(f32), d64.astype(f32)
    o, d = r.org.astype(np.float64), r.dirs.astype(np.float64)
    r.lo = np.where(above, np.searchsorted(fx.x, cross_x), 0)
    r.hi = np.where(above, fx.n, np.searchsorted(fx.x, cross_x) - 1)
    r.hits = np.maximum(r.hi - r.lo + 1, 0)
    forward = d[:, 0] > 0
    r.first = np.where(r.hits > 0, np.where(forward, r.lo, r.hi), -1)
    r.t_first = np.where(r.hits > 0, (fx.x[np.clip(r.first, 0, fx.n)] - o[:, 0]) / d[:, 0], np.inf)
    # any-hit limit: half a spacing beyond the first rung the ray hits; a ray that hits nothing runs past the whole fixture
    end = np.where(r.hits > 0, fx.x[np.clip(r.first, 0, fx.n)] + np.where(forward, 0.5, -0.5) * fx.spacing, np.where(forward, fx.x[-1] + PAD, fx.x[0] - PAD))
    r.tmax = ((end - o[:, 0]) / d[:, 0]).astype(f32)
    r.occluded = r.hits > 0
    return r


def _rung_of_ray(fx, i):
    """The interleaved rungs j in -1 .. n: a multiplier coprime to n + 2, so that every run of n + 2 consecutive rays holds all of them."""
    m = next(m for m in (7, 11, 13) if math.gcd(m, fx.n + 2) == 1)
    return (m * i) % (fx.n + 2) - 1


FAMILIES = ("-x below", "+x below", "-x above", "+x above")      # travel direction; the ray hits the rungs below (<= j) or above (>= n - j) its crossing


@functools.lru_cache(maxsize=None)
def rays(fx, n_rays=None):
    """The four families, a quarter of the rays each (1024 on a ladder, 2048 on a slab).  Ray i of a family has the rung j = _rung_of_ray(i): j = -1
    hits nothing, j = n everything; the last ray of each family is j = n whatever the interleaving says."""
    n_rays = n_rays or (1024 if fx.kind == "ladder" else 2048)
    q = n_rays // 4
    j = _rung_of_ray(fx, np.arange(q))
    j[-1] = fx.n
    j[-2] = -1
    org, cross, above = [], [], []
    for fam in range(4):
        backward, mirror = fam % 2 == 0, fam >= 2
        # below: the crossing lies half a spacing above rung j; above (the mirror image): half a spacing below rung n - j
        cx = (fx.x[0] + (j + 0.5) * fx.spacing) if not mirror else (fx.x[-1] - (j + 0.5) * fx.spacing)
        xo = np.full(q, fx.x[-1] + PAD if backward else fx.x[0] - PAD)
        s = -SLOPE if mirror else SLOPE
        yz = 0.5 + s * (xo - cx)
        org.append(np.stack([xo, yz, yz], 1)); cross.append(cx); above.append(np.full(q, mirror))
    r = _make(fx, np.concatenate(org), np.concatenate(cross), np.concatenate(above))
    r.family = np.repeat(np.arange(4), q)
    r.j = np.tile(j, 4)
    return r


@functools.lru_cache(maxsize=None)
def packet_rays(fx, n_packets=256):
    """Packets of four rays from one origin, far beyond an end of the fixture (so that the four slopes differ little), crossing at four different
    rungs: j, j + s, j + 2 s, j + 3 s (mod n + 2), s about a quarter of the rungs.  The same four families, a quarter of the packets each."""
    q = n_packets // 4
    span = fx.x[-1] - fx.x[0]
    step = max((fx.n + 2) // 4, 1)
    j0 = _rung_of_ray(fx, np.arange(q))
    j0[-1] = fx.n
    j = (j0[:, None] + 1 + step * np.arange(4)[None, :]) % (fx.n + 2) - 1           # [q,4]
    org, cross, above = [], [], []
    far = 8.0 * (span + 2.0 * PAD)
    for fam in range(4):
        backward, mirror = fam % 2 == 0, fam >= 2
        cx = (fx.x[0] + (j + 0.5) * fx.spacing) if not mirror else (fx.x[-1] - (j + 0.5) * fx.spacing)
        xo = fx.x[-1] + far if backward else fx.x[0] - far
        # y + z - 1 at the origin: the steepest ray of the family (the crossing farthest from the origin ... nearest: the largest slope) has 2 SLOPE
        c = 2.0 * SLOPE * (far - PAD) * (1.0 if backward else -1.0) * (-1.0 if mirror else 1.0)
        o = np.array([xo, 0.5 + c / 2.0, 0.5 + c / 2.0])
        org.append(np.broadcast_to(o, (q, 4, 3)).reshape(-1, 3)); cross.append(cx.reshape(-1)); above.append(np.full(4 * q, mirror))
    r = _make(fx, np.concatenate(org), np.concatenate(cross), np.concatenate(above))
    assert np.array_equal(r.org.reshape(-1, 4, 3)[:, 0], r.org.reshape(-1, 4, 3)[:, 3])
    return r


# ---------------------------------------------------------------- float64 conditions

def slab64(o, d, lo, hi):
    """(t_enter, t_exit) [N,M] float64 of rays [N] against boxes [M]; flat boxes (lo == hi on x) are planes the ray crosses."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (lo[None] - o[:, None]) / d[:, None]
        t1 = (hi[None] - o[:, None]) / d[:, None]
    return np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)


def box_margin(r, lo, hi):
    """[N,M] float64: how far inside the boxes' y-z cross-section each ray stays over the boxes' x range, as a fraction of the y / z extent."""
    o, d = r.org.astype(np.float64), r.dirs.astype(np.float64)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    out = np.full((o.shape[0], lo.shape[0]), np.inf)
    for xb in (lo[:, 0], hi[:, 0]):
        t = (xb[None] - o[:, 0:1]) / d[:, 0:1]
        for a in (1, 2):
            p = o[:, a:a + 1] + t * d[:, a:a + 1]
            ext = (hi[:, a] - lo[:, a])[None]
            out = np.minimum(out, np.minimum(p - lo[None, :, a], hi[None, :, a] - p) / ext)
    return out


def edge_margin(fx, r):
    """([N,n+1] float64, [N,n+1] bool): the distance of each ray's point in each rung's plane from the rung's nearest edge, and whether it lies inside."""
    o, d = r.org.astype(np.float64), r.dirs.astype(np.float64)
    t = (fx.x[None] - o[:, 0:1]) / d[:, 0:1]
    y, z = o[:, 1:2] + t * d[:, 1:2], o[:, 2:3] + t * d[:, 2:3]
    return np.minimum(np.minimum(np.abs(y), np.abs(z)), np.abs(y + z - 1.0) / math.sqrt(2.0)), (y > 0) & (z > 0) & (y + z < 1.0)


# ---------------------------------------------------------------- models of the walks (float32 slab arithmetic, as the kernels compute it)

def _slab32(o, inv, lo, hi):
    """rt_device_shade.hpp slab(): (hit, tmin) in float32."""
    with np.errstate(all="ignore"):
        t0 = ((lo - o) * inv).astype(f32)
        t1 = ((hi - o) * inv).astype(f32)
        tmin = max(max(min(t0[0], t1[0]), min(t0[1], t1[1])), max(min(t0[2], t1[2]), f32(0)))
        tmax = min(min(max(t0[0], t1[0]), max(t0[1], t1[1])), max(t0[2], t1[2]))
    return bool(tmax >= tmin), f32(tmin)


def _tri_t32(o, d, v0):
    """tri_hit() on a rung (e1 = +y, e2 = +z), float32 -> (u, v, t) or None for a parallel ray."""
    det = f32(-d[0])                                                    # dot(e1, cross(rd, e2))
    if abs(det) < f32(1e-8):
        return None
    inv = f32(1) / det
    tv = (o - v0).astype(f32)
    u = f32(f32(f32(tv[0] * d[1]) - f32(tv[1] * d[0])) * inv)           # dot(tvec, pvec) inv, pvec = (rd.y, -rd.x, 0)
    v = f32(f32(f32(d[2] * tv[0]) - f32(d[0] * tv[2])) * inv)           # dot(rd, qvec) inv, qvec = (-tvec.z, 0, tvec.x)
    return u, v, f32(tv[0] * inv)


def _tri_hit32(o, d, v0, eps, t_max):
    uvt = _tri_t32(o, d, v0)
    if uvt is None:
        return None
    u, v, t = uvt
    if u < 0 or u > 1 or v < 0 or f32(u + v) > 1 or t < eps or t > t_max:
        return None
    return t


def closest_model(fx, o, d, eps=1e-4, inf=1e30):
    """bvh_closest / k_trace's closest-hit walk of the binary tree for one ray: near child first, far child deferred with its entry distance, the
    `tmin > best` cull at the pop, ties overwrite -> (row of the hit or -1, t float32, peak sp)."""
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    nodes, tris = fx.nodes, fx.tris
    with np.errstate(divide="ignore"):
        inv = (f32(1) / d).astype(f32)
    best, tri, eps = f32(inf), -1, f32(eps)
    hit, tmin = _slab32(o, inv, nodes[0, 0:3], nodes[0, 4:7])
    if not hit or tmin > best:
        return -1, best, 0
    stack, peak, ref = [], 0, 0
    while True:
        nd = nodes[ref]
        if nd[9] > 0:
            first, count = int(nd[8]), int(nd[9])
            for k in range(first, first + count):
                t = _tri_hit32(o, d, tris[k, 0:3], eps, best)
                if t is not None:
                    best, tri = t, k
        else:
            L, R = int(nd[3]), int(nd[7])
            hl, tl = _slab32(o, inv, nodes[L, 0:3], nodes[L, 4:7])
            hr, tr = _slab32(o, inv, nodes[R, 0:3], nodes[R, 4:7])
            hl, hr = hl and tl <= best, hr and tr <= best
            if hl and hr:
                left_first = tl < tr
                stack.append((R, tr) if left_first else (L, tl))
                peak = max(peak, len(stack))
                ref = L if left_first else R
                continue
            if hl or hr:
                ref = L if hl else R
                continue
        found = False
        while stack and not found:
            ref, t = stack.pop()
            found = not t > best            # the cull at the pop
        if not found:
            return tri, best, peak


def wide4(packed):
    """pack_scene's four-wide records -> (lo [M,4,3], hi [M,4,3], ref [M,4]): child k of node m, absent children NO_CHILD with NaN boxes."""
    w = packed["nodes4"].view(f32).reshape(-1, 32)
    lo = np.stack([w[:, 0:4], w[:, 4:8], w[:, 8:12]], -1)
    hi = np.stack([w[:, 12:16], w[:, 16:20], w[:, 20:24]], -1)
    return lo, hi, w[:, 24:28].copy().view(np.int32)


def implicit4(fx):
    """The implicit four-wide topology of a perfect tree (csrc/rt_scene_pack.cpp pack_implicit): an even-depth node (d, p) has the children (d + 2, 4p + j),
    or its two leaves where d + 1 == D -> (lo, hi, ref) in wide4's form, nodes numbered in the order met, leaves as -(ordinal + 1)."""
    nodes = fx.nodes
    lo, hi, ref, todo = [], [], [], [0]
    index = {0: 0}
    leaf_ordinal = {}
    while todo:
        at = todo.pop(0)
        kids = []
        for ch in (int(nodes[at, 3]), int(nodes[at, 7])):
            kids += [ch] if nodes[ch, 9] > 0 else [int(nodes[ch, 3]), int(nodes[ch, 7])]
        l4, h4, r4 = np.full((4, 3), np.nan, f32), np.full((4, 3), np.nan, f32), np.full(4, NO_CHILD, np.int32)
        for k, ch in enumerate(kids):
            l4[k], h4[k] = nodes[ch, 0:3], nodes[ch, 4:7]
            if nodes[ch, 9] > 0:
                r4[k] = -(leaf_ordinal.setdefault(ch, len(leaf_ordinal)) + 1)
            else:
                index[ch] = len(index)
                r4[k] = index[ch]
                todo.append(ch)
        lo.append(l4); hi.append(h4); ref.append(r4)
    return np.stack(lo), np.stack(hi), np.stack(ref)


def any_stack_need(ref):
    """csrc/rt_scene_pack.hpp any_stack_need over ref [M,4]: S(node) = children - 1 + the largest S of its inner children; at least 1."""
    need = {}

    def S(m):
        if m not in need:
            kids = [int(r) for r in ref[m] if r != NO_CHILD]
            need[m] = max(len(kids) - 1, 0) + max([S(r) for r in kids if r >= 0], default=0)
        return need[m]

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    return max(S(0), 1)


def any_model(w4, o, d, t_max, register=False, near=False):
    """The depth-first walk of the four-wide tree w4 = (lo, hi, ref) for one any-hit ray that no triangle stops (the rays that matter for the stack: a
    hit ends a walk early) -> (peak sp, leaves met).  Every child whose box the ray enters within t_max is taken in record order; the walk goes on
    with one and pushes the others.
    register=False: the plain walk any_stack_need is the bound of -- it goes on with the first inner child (else the first leaf).
    register=True: k_trace's and k_trace_packets' walk, which keep the first leaf met in a register instead of on the stack (`leaf`, tested once the
    lane holds no inner node), prefer an inner child to go on with, and at a pop move a leaf to the empty register and look on for an inner node.
    near=True (RT_NEAR_FIRST): the nearest inner child that was hit is taken first."""
    lo, hi, ref = w4
    o, d, t_max = np.asarray(o, f32), np.asarray(d, f32), f32(t_max)
    with np.errstate(divide="ignore"):
        inv = (f32(1) / d).astype(f32)
    stack, peak, met = [], 0, 0
    cur, leaf = 0, None
    while True:
        while cur is not None and cur >= 0:                   # inner nodes
            taken = []
            for k in range(4):
                if ref[cur, k] == NO_CHILD:
                    continue
                h, t = _slab32(o, inv, lo[cur, k], hi[cur, k])
                if h and t <= t_max:
                    taken.append((int(ref[cur, k]), t))
            if near:
                inner = [(t, i) for i, (r, t) in enumerate(taken) if r >= 0]
                if inner:
                    i = min(inner, key=lambda e: e[0])[1]        # the first of the nearest
                    taken[0], taken[i] = taken[i], taken[0]
            nxt = None
            for r, _ in taken:
                if register and r < 0 and leaf is None:
                    leaf = r
                elif nxt is None:
                    nxt = r
                else:
                    if r >= 0 and nxt < 0:
                        nxt, r = r, nxt
                    stack.append(r)
                    peak = max(peak, len(stack))
            cur = nxt
            if cur is None:
                break
        # leaves: the register's, then one waiting in `cur`
        if leaf is not None:
            met += 1
            leaf = None
        if cur is not None and cur < 0:
            if register:
                leaf, cur = cur, None
            else:
                met += 1
                cur = None
        while cur is None and stack:
            r = stack.pop()
            if register and r < 0 and leaf is None:
                leaf = r
                continue
            cur = r
        if cur is None and leaf is None:
            return peak, met


# ---------------------------------------------------------------- the oracle's answers, computed once per fixture

def uniforms(fx, w=64, h=64):
    return rt.frame_uniforms(rt.default_render_params(), rt.default_camera(), w, h, 0, True, fx.nodes.shape[0], fx.tris.shape[0])


@functools.lru_cache(maxsize=None)
def oracle_answers(fx):
    """(prim [N] int, t [N] float32, occluded [N] bool) of rays(fx) by the oracle's traceBVH / traceBVHShadow; read-only."""
    import oracle as orc
    u, r = uniforms(fx), rays(fx)
    n = r.org.shape[0]
    prim, t, occ = np.zeros(n, np.int64), np.zeros(n, f32), np.zeros(n, bool)
    for i in range(n):
        prim[i], t[i] = orc.trace_bvh_prim(u, fx.nodes, fx.tris, r.org[i], r.dirs[i])
        occ[i] = orc.trace_bvh_shadow(u, fx.nodes, fx.tris, r.org[i], r.dirs[i], r.tmax[i])
    for a in (prim, t, occ):
        a.setflags(write=False)
    return prim, t, occ


@functools.lru_cache(maxsize=None)
def oracle_packet_answers(fx):
    """occluded [N] bool of packet_rays(fx) by the oracle's traceBVHShadow; read-only."""
    import oracle as orc
    u, r = uniforms(fx), packet_rays(fx)
    occ = np.array([orc.trace_bvh_shadow(u, fx.nodes, fx.tris, r.org[i], r.dirs[i], r.tmax[i]) for i in range(r.org.shape[0])], bool)
    occ.setflags(write=False)
    return occ


def implicit_need(D):
    """any_stack_need of the implicit four-wide topology of a perfect tree of leaf depth D: three pushes per full even level, one where d + 1 == D."""
    return max(sum(3 if d + 2 <= D else 1 for d in range(0, D, 2)), 1)
