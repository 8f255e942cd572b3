"""float32 numpy restatement of rt_hit_motion (include/rt_mi355.h): where a hit point of the dynamic mesh was in the previous pose and
the motion that follows from it.  Every operation rounds to float32; fma only where ndcFromWorld writes it.

    prev_points(tris12, prev12, rec, points)      the delta form, or the point's own bits where the row did not change
    ndc_from_world(p, VP)                         ndcFromWorld (rt_taa.glsl:175-179, csrc/rt_device_shade.hpp)
    hit_motion(u, tris12, prev12, rec, points)    -> (prev_points, motion)

rec is the [N,4] float32 record array of RtHit (t, prim as int32 bits, u, v); a prim outside [0, nTris) gives zeros in both outputs."""
import numpy as np

from analytic_ref import fma32

f32 = np.float32
GEOMETRY = [0, 1, 2, 4, 5, 6, 8, 9, 10]   # the nine geometry floats of a 12-float row


def prims(rec):
    return np.ascontiguousarray(rec, f32)[:, 1].copy().view(np.int32)


def prev_points(tris12, prev12, rec, points):
    T, P = np.asarray(tris12, f32).reshape(-1, 12), np.asarray(prev12, f32).reshape(-1, 12)
    rec, x = np.ascontiguousarray(rec, f32), np.asarray(points, f32).reshape(-1, 3)
    prim = prims(rec)
    ok = (prim >= 0) & (prim < T.shape[0])
    p = np.where(ok, prim, 0)
    t, q = T[p], P[p]
    a, b = rec[:, 2:3], rec[:, 3:4]
    same = (t[:, GEOMETRY].view(np.uint32) == q[:, GEOMETRY].view(np.uint32)).all(axis=1)
    with np.errstate(all="ignore"):
        d0 = (q[:, 0:3] - t[:, 0:3]).astype(f32)
        d1 = ((q[:, 4:7] - t[:, 4:7]).astype(f32) * a).astype(f32)
        d2 = ((q[:, 8:11] - t[:, 8:11]).astype(f32) * b).astype(f32)
        d = ((d0 + d1).astype(f32) + d2).astype(f32)
        moved = (x + d).astype(f32)
    out = np.where(same[:, None], x, moved).astype(f32)
    out[~ok] = 0
    return out


def ndc_from_world(p, VP):
    VP = np.asarray(VP, f32).reshape(16)
    p = np.asarray(p, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        def clip(k):
            return (fma32(VP[8 + k], p[:, 2], fma32(VP[4 + k], p[:, 1], (VP[k] * p[:, 0]).astype(f32))) + VP[12 + k]).astype(f32)
        cx, cy, cw = clip(0), clip(1), clip(3)
        w = np.where(cw > f32(1e-6), cw, f32(1e-6)).astype(f32)   # fmaxf: a NaN cw gives 1e-6
        return np.stack([(cx / w).astype(f32), (cy / w).astype(f32)], axis=1)


def hit_motion(u, tris12, prev12, rec, points):
    x = np.asarray(points, f32).reshape(-1, 3)
    prev = prev_points(tris12, prev12, rec, x)
    with np.errstate(all="ignore"):
        mo = (ndc_from_world(x, list(u.currViewProj)) - ndc_from_world(prev, list(u.prevViewProj))).astype(f32)
    prim = prims(rec)
    mo[~((prim >= 0) & (prim < np.asarray(tris12).reshape(-1, 12).shape[0]))] = 0
    return prev, mo
