"""The proximity query's definition restated in numpy float32 on top of nearest_ref.py: e(t) for every row as nearest_ref.Table
computes it, the accepted set e(t) <= L, its order under (e, prim), and the K records and the count by brute force, vectorised over the points.  Also
the limits the proximity tests share: per mesh one fixed fraction of the root box's diagonal (every 97th slot empty), and the unlimited case."""
import functools

import numpy as np

import nearest_ref as ref

f32 = np.float32
INF = ref.INF
bits = ref.bits
MESHES = ref.MESHES
KS = (0, 1, 2, 3, 4, 8, 32)

# max_dist as a fraction of the root box's diagonal.  Chosen on the CPU so that every mesh has points with more than 8 rows within the limit (where it
# has more than 8 rows), points with 1 .. K - 1 rows (where its rows allow such a count) and points with none: test_nearest_multi_host.py asserts them.
FRACTION = {"one_triangle": 0.25, "one_leaf": 0.25, "bunny": 0.0625, "layers": 0.0078125, "two_clusters": 0.015625}


@functools.lru_cache(maxsize=None)
def limit(name):
    """max_dist [N] of case(name): the mesh's fraction of the root box's diagonal, rounded once to float32; every 97th slot empty (< 0)."""
    nodes, tris, pts, _ = ref.case(name)
    diag = np.linalg.norm(nodes[0, 4:7].astype(np.float64) - nodes[0, 0:3].astype(np.float64))
    md = np.full(pts.shape[0], f32(FRACTION[name] * diag), f32)
    md[::97] = f32(-1.0)
    md.setflags(write=False)
    return md


class Sorted:
    """The accepted set of every point in order: `order` [N,T], the rows under (e, prim) ascending with the rows that are not accepted last; `count`
    [N] = |S|."""

    def __init__(self, table, max_dist=None):
        t = table
        n = t.p.shape[0]
        with np.errstate(all="ignore"):
            L = np.full(n, INF, f32) if max_dist is None else (max_dist * max_dist).astype(f32)
            live = np.isfinite(t.p).all(1)
            if max_dist is not None:
                live &= ~(max_dist < 0)
            self.acc = (t.e <= L[:, None]) & live[:, None]
        self.count = self.acc.sum(1).astype(np.int32)
        # a stable sort by e keeps equal e in row order: (e, prim); what is not accepted sorts behind everything (an accepted e may be +inf: the flag decides)
        key = np.where(self.acc, t.e, INF)
        by_e = np.argsort(key, axis=1, kind="stable")
        flag = np.take_along_axis(~self.acc, by_e, 1)
        self.order = np.take_along_axis(by_e, np.argsort(flag, axis=1, kind="stable"), 1)
        self.table = t


def answer(tris12, srt, K):
    """(hits [N,K,4], closest [N,K,3], count [N]) of the definition from a Sorted."""
    t = srt.table
    n, T = t.e.shape
    k = min(K, T)
    hits = np.zeros((n, K, 4), f32)
    hits[:, :, 0] = INF
    hits.view(np.int32)[:, :, 1] = -1
    closest = np.zeros((n, K, 3), f32)
    if k:
        prim = srt.order[:, :k]
        have = np.arange(k)[None, :] < srt.count[:, None]
        rows = np.arange(n)[:, None]
        u, v = t.u[rows, prim], t.v[rows, prim]
        hits[:, :k, 0] = np.where(have, t.e[rows, prim], INF)
        hits.view(np.int32)[:, :k, 1] = np.where(have, prim, -1)
        hits[:, :k, 2] = np.where(have, u, 0)
        hits[:, :k, 3] = np.where(have, v, 0)
        c = ref.point_at(tris12[prim, 0:3], tris12[prim, 4:7], tris12[prim, 8:11], u, v)
        closest[:, :k] = np.where(have[:, :, None], c, f32(0))
    return hits, closest, srt.count


@functools.lru_cache(maxsize=None)
def ordered(name, limited):
    """The Sorted of case(name) at limit(name) or without a limit.  Computed once; leave it unchanged."""
    return Sorted(ref.reference(name, False)[2], limit(name) if limited else None)


@functools.lru_cache(maxsize=None)
def reference(name, limited, K):
    """(hits, closest, count) of the numpy definition on case(name).  Computed once; leave it unchanged."""
    return answer(ref.case(name)[1], ordered(name, limited), K)
