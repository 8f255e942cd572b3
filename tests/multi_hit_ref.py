"""The multi-hit query's definition in plain Python over the oracle's two primitives, independent of the library: the set walk of
traceBVHShadow's loop with its `return true` removed (oracle.aabb_hit / oracle.tri_hit, one call at a time), the (key(t), prim) order, u, v through
the float32 restatement of triHit's operations (analytic_ref.fma32), and a brute-force variant over all triangles.  Also the meshes and rays the
multi-hit tests share."""
import ctypes as C
import functools

import numpy as np

import analytic_ref as ar
import opengl_raytracing_amd as rt
import oracle as orc
import scenes

f32 = np.float32


def key(t):
    """The monotone map of float32 bits: ascending keys are ascending t; NaNs are ordered too (positive ones last)."""
    b = np.ascontiguousarray(t, f32).view(np.uint32).astype(np.uint64)
    return np.where(b >> 31, b ^ 0xFFFFFFFF, b ^ 0x80000000).astype(np.uint32)


def _uniforms(eps):
    u = rt.RtUniforms()
    u.eps = float(eps)
    return u


@functools.lru_cache(maxsize=None)
def _prims():
    """oracle.aabb_hit / oracle.tri_hit bound once: the same two exports, called on addresses inside float32 arrays (a third of a million calls)."""
    L = orc.lib()
    orc.aabb_hit(np.zeros(3, f32), np.ones(3, f32), np.zeros(3, f32), np.ones(3, f32))      # (sets the exports' argument types)
    orc.tri_hit(_uniforms(0), np.zeros(3, f32), np.ones(3, f32), np.zeros(12, f32), 1.0)
    fp = C.POINTER(C.c_float)
    at = lambda a, row=0: C.cast(a.ctypes.data + row * a.strides[0], fp)
    return L.orc_aabb_hit, L.orc_tri_hit, at


def walk(nodes12, tris12, ro, rd, T, eps):
    """One ray: [(t, prim, slab entry of the triangle's leaf)] for every triangle the walk accepts at the limit T, in no particular order."""
    aabb, tri, at = _prims()
    u = _uniforms(eps)
    out, stack = [], [0]
    if nodes12.shape[0] == 0 or tris12.shape[0] == 0:
        return out
    nodes12, tris12 = np.ascontiguousarray(nodes12, f32), np.ascontiguousarray(tris12, f32)
    lo, hi = np.ascontiguousarray(nodes12[:, 0:3]), np.ascontiguousarray(nodes12[:, 4:7])
    ro, rd = np.ascontiguousarray(ro, f32), np.ascontiguousarray(rd, f32)
    box, h = np.zeros(4, f32), np.zeros(5, f32)
    while stack:
        ni = stack.pop()
        aabb(at(ro), at(rd), at(lo, ni), at(hi, ni), at(box))
        if not (box[0] and box[1] <= T):
            continue
        N = nodes12[ni]
        count = int(N[9] + f32(0.5))
        if count > 0:
            first = int(N[8] + f32(0.5))
            for prim in range(first, first + count):
                tri(C.byref(u), at(ro), at(rd), at(tris12, prim), float(T), at(h))
                if h[0]:
                    out.append((f32(h[1]), prim, f32(box[1])))
        else:
            stack.append(int(N[3] + f32(0.5)))
            stack.append(int(N[7] + f32(0.5)))
    return out


def brute(tris12, origins, dirs, T, eps):
    """Per ray: [(t, prim)] of every triangle triHit accepts at the limit T, boxes ignored."""
    _, tri, at = _prims()
    u = C.byref(_uniforms(eps))
    tris12 = np.ascontiguousarray(tris12, f32)
    rows = [at(tris12, prim) for prim in range(tris12.shape[0])]
    origins, dirs = np.ascontiguousarray(origins[:, :3], f32), np.ascontiguousarray(dirs[:, :3], f32)
    h = np.zeros(5, f32)
    ph, T = at(h), float(T)
    res = []
    for i in range(origins.shape[0]):
        po, pd, out = at(origins, i), at(dirs, i), []
        for prim, row in enumerate(rows):
            tri(u, po, pd, row, T, ph)
            if h[0]:
                out.append((f32(h[1]), prim))
        res.append(out)
    return res


def ordered(found):
    """The total order of the definition: (key(t), prim) ascending."""
    if not found:
        return []
    k = key(np.array([f[0] for f in found], f32))
    return [found[i] for i in sorted(range(len(found)), key=lambda i: (int(k[i]), found[i][1]))]


def all_hits(nodes12, tris12, origins, dirs, tmax=None, eps=1e-4, inf=1e30):
    """Per ray the ordered list of everything the walk accepts; an empty slot (tmax[i] < 0) has none."""
    res = []
    for i in range(origins.shape[0]):
        T = f32(inf) if tmax is None else f32(tmax[i])
        if tmax is not None and T < 0:
            res.append([])
            continue
        res.append(ordered(walk(nodes12, tris12, origins[i, :3], dirs[i, :3], T, eps)))
    return res


def tri_uv(ro, rd, tri12):
    """u, v of triHit on the given rows, in its operation order."""
    v0, e1, e2 = tri12[:, 0:3], tri12[:, 4:7], tri12[:, 8:11]
    with np.errstate(all="ignore"):
        pvec = ar.cross(rd, e2)
        inv = (f32(1.0) / ar.dot(e1, pvec)).astype(f32)
        tvec = (ro - v0).astype(f32)
        u = (ar.dot(tvec, pvec) * inv).astype(f32)
        v = (ar.dot(rd, ar.cross(tvec, e1)) * inv).astype(f32)
    return u, v


def answer(lists, tris12, origins, dirs, K, inf=1e30):
    """(hits [N,K,4] float32, counts [N] int32) from all_hits' lists: the K first of each, the miss record behind them."""
    n = len(lists)
    hits = np.zeros((n, K, 4), f32)
    hits[:, :, 0] = f32(inf)
    hits.view(np.int32)[:, :, 1] = -1
    counts = np.array([len(l) for l in lists], np.int32)
    where = [(i, j) for i, l in enumerate(lists) for j in range(min(K, len(l)))]
    if where:
        ii = np.array([w[0] for w in where]); jj = np.array([w[1] for w in where])
        prim = np.array([lists[i][j][1] for i, j in where], np.int32)
        hits[ii, jj, 0] = np.array([lists[i][j][0] for i, j in where], f32)
        hits.view(np.int32)[ii, jj, 1] = prim
        u, v = tri_uv(np.ascontiguousarray(origins[ii, :3]), np.ascontiguousarray(dirs[ii, :3]), tris12[prim])
        hits[ii, jj, 2], hits[ii, jj, 3] = u, v
    return hits, counts


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------- the meshes and rays the tests share

@functools.lru_cache(maxsize=None)
def layer_stack():
    """(nodes12, tris12): six layers at y = float32(0.25 k + 0.1), each three coincident copies of a 60 x 60 quad -- 36 triangles, 15 nodes.  Every ray
    down through it has equal-t triples, and triangles flush with their leaf's box."""
    tris9 = []
    for k in range(6):
        y = f32(0.25 * k + 0.1)
        for _ in range(3):
            tris9.append([-30, y, -30, 60, 0, 0, 60, 0, 60])
            tris9.append([-30, y, -30, 60, 0, 60, 0, 0, 60])
    nodes, tris = rt.build_bvh(np.array(tris9, f32))
    assert nodes.shape[0] == 15 and tris.shape[0] == 36
    return nodes, tris


@functools.lru_cache(maxsize=None)
def layer_rays(n=3000, seed=4):
    """Rays of the floor-tie kind over the layer stack: origins on the 1/8 grid with y in [2, 8), half straight down, half along exact small-integer
    slopes."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.integers(-40, 40, n) / f32(8), rng.integers(16, 64, n) / f32(8), rng.integers(-40, 40, n) / f32(8)], 1).astype(f32)
    d = np.zeros((n, 3), f32)
    d[:, 1] = -1.0
    k = n // 2
    d[k:, 0] = rng.integers(-2, 3, n - k)
    d[k:, 2] = rng.integers(-2, 3, n - k)
    d[k:] = ar.normalize(d[k:])
    return o, d


@functools.lru_cache(maxsize=None)
def bunny_rays(subdiv=2, n=150):
    """(nodes12, tris12, origins, dirs, tmax) of scenes.adversarial_rays on the bunny stand-in, every 97th slot empty."""
    nodes, tris = scenes.bunny_bvh(subdiv)
    o, d, tm = scenes.adversarial_rays(nodes, tris, n=n)
    tm = tm.copy()
    tm[::97] = f32(-1.0)
    return nodes, tris, o, d, tm


@functools.lru_cache(maxsize=None)
def one_leaf_rays(n=40):
    nodes, tris = scenes.one_leaf_mesh()
    assert nodes.shape[0] == 1
    o, d, tm = scenes.adversarial_rays(nodes, tris, n=n, seed=5)
    tm = tm.copy()
    tm[::97] = f32(-1.0)
    return nodes, tris, o, d, tm
