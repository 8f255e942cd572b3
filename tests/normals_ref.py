"""float32 numpy restatement of the smooth vertex normals of the dynamic mesh (include/rt_mi355.h): rt_vertex_normals, rt_hit_normals
and the packed vertex -> triangle adjacency rt_debug_normal_pack hands out.  Every operation rounds to float32; fma only where cross and dot write it.

    cross(a, b), dot(a, b)                                   rt_device_math.hpp's expressions
    face_vectors(tris12, order)                              cross(e1, e2) of every row, filed by input triangle
    vertex_normals(tris12, order, indices, n_verts)          the area-weighted sums in incidence order, normalised, or three +0
    hit_normals(tris12, order, indices, normals, rec)        the blend of the corner normals at the hit's barycentrics, or the face normal
    pack(indices, n_verts)                                   -> {"slice_first", "entries", "info"}: slices of 64 vertices, -1 as padding

rec is the [N,4] float32 record array of RtHit (t, prim as int32 bits, u, v); a prim outside [0, nTris) gives zeros."""
import numpy as np

from analytic_ref import fma32

f32 = np.float32
SLICE = 64


def cross(a, b):
    with np.errstate(all="ignore"):
        return np.stack([fma32(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1]).astype(f32)), fma32(a[:, 2], b[:, 0], -(a[:, 0] * b[:, 2]).astype(f32)),
                         fma32(a[:, 0], b[:, 1], -(a[:, 1] * b[:, 0]).astype(f32))], axis=1).astype(f32)


def dot(a, b):
    with np.errstate(all="ignore"):
        return fma32(a[:, 2], b[:, 2], fma32(a[:, 1], b[:, 1], (a[:, 0] * b[:, 0]).astype(f32))).astype(f32)


def unit(v):
    """(ok, v * (1 / sqrt(dot(v, v)))): ok where dot(v, v) > 0 and finite."""
    with np.errstate(all="ignore"):
        d = dot(v, v)
        ok = (d > 0) & (d < np.inf)
        inv = (f32(1.0) / np.sqrt(d).astype(f32)).astype(f32)
        return ok, (v * inv[:, None]).astype(f32)


def face_vectors(tris12, order):
    T = np.asarray(tris12, f32).reshape(-1, 12)
    out = np.zeros((T.shape[0], 3), f32)
    out[np.asarray(order, np.int64)] = cross(T[:, 4:7], T[:, 8:11])
    return out


def vertex_normals(tris12, order, indices, n_verts):
    face = face_vectors(tris12, order)
    ix = np.asarray(indices, np.int64).reshape(-1)
    S = np.zeros((n_verts, 3), f32)
    seen = np.zeros(n_verts, bool)
    with np.errstate(all="ignore"):
        for e, v in enumerate(ix):                          # k ascending, then c: input order
            S[v] = (S[v] + face[e // 3]).astype(f32) if seen[v] else face[e // 3]
            seen[v] = True
    ok, n = unit(S)
    return np.where(ok[:, None], n, f32(0.0)).astype(f32)


def prims(rec):
    return np.ascontiguousarray(rec, f32)[:, 1].copy().view(np.int32)


def face_normals(tris12):
    """tri_normal: normalize(cross(e1, e2)) of every row, whatever that is for a degenerate one."""
    T = np.asarray(tris12, f32).reshape(-1, 12)
    f = cross(T[:, 4:7], T[:, 8:11])
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / np.sqrt(dot(f, f)).astype(f32)).astype(f32)
        return (f * inv[:, None]).astype(f32)


def hit_normals(tris12, order, indices, normals, rec):
    T = np.asarray(tris12, f32).reshape(-1, 12)
    N = np.asarray(normals, f32)[:, :3]
    rec = np.ascontiguousarray(rec, f32)
    prim = prims(rec)
    ok = (prim >= 0) & (prim < T.shape[0])
    p = np.where(ok, prim, 0)
    ix = np.asarray(indices, np.int64).reshape(-1, 3)[np.asarray(order, np.int64)[p]]
    n0, n1, n2 = N[ix[:, 0]], N[ix[:, 1]], N[ix[:, 2]]
    a, b = rec[:, 2:3], rec[:, 3:4]
    same = ((n0.view(np.uint32) == n1.view(np.uint32)) & (n0.view(np.uint32) == n2.view(np.uint32))).all(axis=1)
    zero0 = (n0 == 0).all(axis=1)
    with np.errstate(all="ignore"):
        w = ((f32(1.0) - a).astype(f32) - b).astype(f32)
        m = (((n0 * w).astype(f32) + (n1 * a).astype(f32)).astype(f32) + (n2 * b).astype(f32)).astype(f32)
    m_ok, m_unit = unit(m)
    out = face_normals(T)[p]
    out = np.where((~same & m_ok)[:, None], m_unit, out)
    out = np.where((same & ~zero0)[:, None], n0, out).astype(f32)
    out[~ok] = 0
    return out


def pack(indices, n_verts):
    ix = np.asarray(indices, np.int64).reshape(-1)
    count = np.bincount(ix, minlength=n_verts)
    n_slices = (n_verts + SLICE - 1) // SLICE
    width = np.array([count[s * SLICE:(s + 1) * SLICE].max() for s in range(n_slices)], np.int64)
    first = np.zeros(n_slices + 1, np.int64)
    np.cumsum(width * SLICE, out=first[1:])
    entries = np.full(int(first[-1]), -1, np.int32)
    nxt = np.zeros(n_verts, np.int64)
    for e, v in enumerate(ix):
        entries[first[v // SLICE] + nxt[v] * SLICE + v % SLICE] = e // 3
        nxt[v] += 1
    n_tris = ix.size // 3
    info = {"nVerts": n_verts, "nTris": n_tris, "nSlices": n_slices, "maxPerVertex": int(width.max()), "incidences": int(ix.size),
            "paddedEntries": int(first[-1]), "bytes": int(first[-1]) * 4 + (n_slices + 1) * 4 + n_tris * 16 + n_verts * 16 + n_tris * 48}
    return {"slice_first": first.astype(np.uint32), "entries": entries, "info": info}
