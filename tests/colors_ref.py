"""The per-vertex colours of the dynamic mesh restated in numpy float32: every product and every sum rounded on its own, no fmaf --
the float model of csrc/rt_mesh_colors.hpp -- for rt_hit_colors, rt_color_rows and the device arrays to be compared with bit for bit."""
import numpy as np

f32 = np.float32
GREY = f32(0.85)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def records(prim, u, v):
    """RtHit records [N,4] float32: t = 1, prim as its int32 bits, u, v."""
    rec = np.zeros((len(prim), 4), f32)
    rec[:, 0], rec[:, 2], rec[:, 3] = 1.0, u, v
    rec[:, 1] = np.asarray(prim, np.int32).view(f32)
    return rec


def prims(rec):
    return np.ascontiguousarray(rec[:, 1]).view(np.int32)


def color_rows(order, indices, colors) -> np.ndarray:
    """[T,12]: row i holds (r, g, b, 0) of the three corners of input triangle order[i]."""
    order = np.asarray(order, np.int64)
    ix = np.asarray(indices, np.int64).reshape(-1, 3)
    c = np.asarray(colors, f32)[:, :3]
    out = np.zeros((order.size, 3, 4), f32)
    out[:, :, :3] = c[ix[order]]
    return out.reshape(-1, 12)


def hit_colors(order, indices, colors, rec) -> np.ndarray:
    """[N,3]: zeros for a prim outside the triangles; c0 where a barycentric is not finite; else per channel c0's value where the channel's three
    corner values are bit-equal (so three bit-equal corners give c0) and (c0 * ((1 - a) - b) + c1 * a) + c2 * b elsewhere, every operation rounded
    to float32."""
    order = np.asarray(order, np.int64)
    ix = np.asarray(indices, np.int64).reshape(-1, 3)
    c = np.asarray(colors, f32)[:, :3]
    rec = np.asarray(rec, f32)
    p = prims(rec).astype(np.int64)
    on = (p >= 0) & (p < order.size)
    corner = c[ix[order[np.where(on, p, 0)]]]                                     # [N,3 corners,3 channels]
    c0, c1, c2 = corner[:, 0], corner[:, 1], corner[:, 2]
    a, b = rec[:, 2:3], rec[:, 3:4]
    with np.errstate(all="ignore"):
        w = ((f32(1.0) - a).astype(f32) - b).astype(f32)
        m = (((c0 * w).astype(f32) + (c1 * a).astype(f32)).astype(f32) + (c2 * b).astype(f32)).astype(f32)
    same = (bits(c0) == bits(c1)) & (bits(c0) == bits(c2))                        # per channel
    keep = same | ~np.isfinite(a) | ~np.isfinite(b)
    out = np.where(keep, c0, m).astype(f32)
    out[~on] = 0
    return out


def vertex_colors_from_parts(indices, part_first, rgb, n_verts) -> np.ndarray:
    ix = np.asarray(indices, np.int64).reshape(-1, 3)
    out = np.full((n_verts, 3), GREY, f32)
    for p in range(len(part_first) - 1):
        for k in range(part_first[p], part_first[p + 1]):
            out[ix[k]] = np.asarray(rgb, f32)[p]
    return out


def brute_force_hits(tris12, origins, d):
    """Closest hits of parallel rays (origins [R,3], one direction d) on rows [T,12], in float64 -> (hit mask [R], prim, a, b, points), the last
    four over the rays that hit."""
    T = np.asarray(tris12, np.float64)
    v0, e1, e2 = T[:, 0:3], T[:, 4:7], T[:, 8:11]
    pvec = np.cross(d, e2)
    det = (e1 * pvec).sum(axis=1)
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        tvec = origins[:, None, :] - v0[None, :, :]
        a = (tvec * pvec[None]).sum(axis=2) * inv
        qvec = np.cross(tvec, e1[None])
        b = (qvec * d).sum(axis=2) * inv
        t = (qvec * e2[None]).sum(axis=2) * inv
    ok = (a >= 0) & (b >= 0) & (a + b <= 1) & (t > 0) & np.isfinite(t)
    t = np.where(ok, t, np.inf)
    prim = t.argmin(axis=1)
    r = np.arange(origins.shape[0])
    hit = np.isfinite(t[r, prim])
    return hit, prim[hit], a[r, prim][hit], b[r, prim][hit], origins[hit] + d * t[r, prim][hit, None]
