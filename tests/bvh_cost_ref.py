"""The definition of the BVH quality metric (rt_bvh_cost, rt_mesh_quality), restated in plain numpy so that the library can be compared
with it in every integer and in every double's bits.  TEST INFRASTRUCTURE.  It imports numpy (and math) only and never calls the library.

Per node of the reference's 12-float nodes (min at 0-2, max at 4-6, count at 9, count > 0 = a leaf):
  * d = max - min per axis in fp32, widened to double; half-area a = (dx*dy + dy*dz) + dz*dx in double (the products are exact);
  * A = node 0's half-area; A == 0: degenerate, every sum zero; otherwise A = m * 2^e with m in [0.5, 1) (frexp);
  * q = floor(a * 2^(32 - e)) as an integer (<= 2^32, as every box lies inside the root's and rounding is monotone);
  * innerQ = sum of q over inner nodes, leafQ = sum of q * count over leaves -- Python integers, so the order cannot matter;
  * inner = (innerQ * 2^(e - 32)) / A, leaf likewise, cost = inner + leaf: the surface-area heuristic with both unit costs 1.
"""
import math

import numpy as np

f32 = np.float32
FIELDS = ("innerQ", "leafQ", "rootArea", "inner", "leaf", "cost", "rootExp", "degenerate", "nInner", "nLeaves")


def half_areas(nodes12):
    n = np.ascontiguousarray(nodes12, f32).reshape(-1, 12)
    with np.errstate(all="ignore"):
        d = (n[:, 4:7] - n[:, 0:3]).astype(f32).astype(np.float64)
        return (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2]) + d[:, 2] * d[:, 0]


def ref_cost(nodes12):
    """-> dict with FIELDS' keys: Python ints and floats."""
    n = np.ascontiguousarray(nodes12, f32).reshape(-1, 12)
    assert n.shape[0] >= 1
    count = n[:, 9].astype(np.int64)
    leaf = count > 0
    a = half_areas(n)
    A = float(a[0])
    out = dict(innerQ=0, leafQ=0, rootArea=A, inner=0.0, leaf=0.0, cost=0.0, rootExp=0, degenerate=0, nInner=int((~leaf).sum()), nLeaves=int(leaf.sum()))
    if A == 0.0:
        out["degenerate"] = 1
        return out
    _, e = math.frexp(A)
    q = [int(math.floor(math.ldexp(float(x), 32 - e))) for x in a]
    assert all(0 <= x <= 1 << 32 for x in q), "a box larger than the root's"
    out["rootExp"] = e
    out["innerQ"] = sum(x for x, lf in zip(q, leaf) if not lf)
    out["leafQ"] = sum(x * int(c) for x, c, lf in zip(q, count, leaf) if lf)
    assert out["innerQ"] < 1 << 64 and out["leafQ"] < 1 << 64
    out["inner"] = math.ldexp(float(out["innerQ"]), e - 32) / A        # float(int) rounds to nearest even, as the C conversion does
    out["leaf"] = math.ldexp(float(out["leafQ"]), e - 32) / A
    out["cost"] = out["inner"] + out["leaf"]
    return out


def bits(x):
    return np.float64(x).view(np.uint64)


def assert_same(got, want, what=""):
    """got: anything with FIELDS as attributes (the ctypes record); want: ref_cost's dict.  Integers equal, doubles equal in their bits."""
    for k in FIELDS:
        g, w = getattr(got, k), want[k]
        if isinstance(w, float):
            assert bits(g) == bits(w), f"{what}: {k} = {g!r} ({int(bits(g)):#x}), the definition says {w!r} ({int(bits(w)):#x})"
        else:
            assert int(g) == w, f"{what}: {k} = {g}, the definition says {w}"


# ---------------------------------------------------------------- the deformations of the 2048-triangle grid the feature's claim rests on

def grid(g=32):
    """g x g quads of side 1 / g in the plane y = 0 (the unit square about the origin), two triangles each -> (positions [(g+1)^2, 3], indices [6 g^2])."""
    i, j = np.meshgrid(np.arange(g + 1), np.arange(g + 1), indexing="ij")
    v = np.stack([(i.reshape(-1) - g / 2.0) / g, np.zeros((g + 1) ** 2), (j.reshape(-1) - g / 2.0) / g], 1).astype(f32)
    q = (np.arange(g)[:, None] * (g + 1) + np.arange(g)[None, :]).reshape(-1)
    f = np.stack([q, q + 1, q + g + 2, q, q + g + 2, q + g + 1], 1).astype(np.uint32).reshape(-1)
    return v, f


def interleave_parts(indices, n_parts=4):
    """Reorders the index triples so that part p holds the triangles i with i % n_parts == p -> (indices, part_first).  Parts are contiguous runs of
    triples, so the interleaving is in space: every part covers the whole grid."""
    t = np.asarray(indices, np.uint32).reshape(-1, 3)
    runs = [t[p::n_parts] for p in range(n_parts)]
    first = np.concatenate([[0], np.cumsum([r.shape[0] for r in runs])]).astype(np.int32)
    return np.concatenate(runs).reshape(-1), first


def translations(n_parts, step):
    """[n_parts, 16] column-major: part p translated by step * p in x."""
    m = np.tile(np.eye(4, dtype=f32).reshape(-1), (n_parts, 1))
    m[:, 12] = (step * np.arange(n_parts)).astype(f32)
    return m


def gather_parts(positions, indices, part_first, models):
    """rt_gather_triangles_parts in numpy, for translations and the identity only (one rounding per coordinate, whatever the order of the sums):
    [n, 9] = v0, e1, e2 of every triangle under its part's matrix."""
    p = np.ascontiguousarray(positions, f32).reshape(-1, 3)
    t = np.asarray(indices, np.int64).reshape(-1, 3)
    m = np.asarray(models, f32).reshape(-1, 16)
    lin = m[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]
    assert np.array_equal(lin, np.tile(np.eye(3, dtype=f32).reshape(-1), (m.shape[0], 1))), "translations only"
    part = np.repeat(np.arange(m.shape[0]), np.diff(part_first))
    off = m[part, 12:15]
    a, b, c = ((p[t[:, k]] + off).astype(f32) for k in range(3))
    return np.concatenate([a, (b - a).astype(f32), (c - a).astype(f32)], 1).astype(f32)
