"""float32 numpy restatement of the analytic scene query and the primary ray, in the float model of DESIGN.md 2: every operation
rounds to float32, fma only where rt_device_math.hpp writes it (dot, cross, normalize), no contraction anywhere else.

    intersect_plane / intersect_sphere   rt_scene_analytic.glsl:71-81 / :96-111 (csrc/rt_device_analytic.hpp)
    trace_analytic                       traceAnalyticCore with its glass / marker flags
    primary_dir                          primaryDirJ (rt.frag:58-68, csrc/rt_device_shade.hpp)
    trace_hybrid                         traceScene's rule: the mesh (the oracle's traceBVH) wins only at a strictly smaller t

All functions take [N,3] float32 arrays and answer every ray at once: Answer(t, obj, normal, point), t = uINF and obj = -1 on a miss (normal
and point are then zero)."""
from collections import namedtuple

import numpy as np

f32 = np.float32
Answer = namedtuple("Answer", "t obj normal point")

# floor (plane y = 0), then the spheres of traceAnalyticCore in list order: (centre, radius, object id)
FLOOR = 0
SPHERES = ((np.array([-1.2, 1.0, -3.5], f32), f32(1.0), 1),   # albedo
           (np.array([0.7, 1.0, -5.0], f32), f32(1.0), 2),    # glass
           (np.array([1.2, 0.7, -2.5], f32), f32(0.7), 3))    # mirror
MARKER_RADIUS, MARKER = f32(0.15), 4
MESH = 5


def fma32(a, b, c):
    """fmaf on float32 arrays, exactly: a*b is exact in float64, the sum is rounded once to float64 and corrected where that rounding
    lands on a float32 rounding midpoint (the only place where rounding twice differs from rounding once)."""
    a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                     # s + err == p + c exactly (TwoSum)
        r = s.astype(np.float32)
        other = np.nextafter(r, np.where(s > r.astype(np.float64), np.float32(np.inf), np.float32(-np.inf)))
        mid = (r.astype(np.float64) + other.astype(np.float64)) * 0.5
        at_mid = (s == mid) & (err != 0) & np.isfinite(s)
        s = np.where(at_mid, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def dot(a, b):
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], (a[..., 0] * b[..., 0]).astype(f32)))


def cross(a, b):
    return np.stack([fma32(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1]).astype(f32)),
                     fma32(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2]).astype(f32)),
                     fma32(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]).astype(f32))], axis=-1)


def normalize(a):
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / np.sqrt(dot(a, a))).astype(f32)
        return (a * inv[..., None]).astype(f32)


def _f(a):
    return np.asarray(a, f32)


def _point(ro, rd, t):
    with np.errstate(all="ignore"):
        return (ro + (rd * t[:, None]).astype(f32)).astype(f32)


def intersect_plane(eps, ro, rd):
    """intersectPlane(n = (0, 1, 0), d = 0) -> (hit, t, p, n)."""
    n = np.broadcast_to(np.array([0.0, 1.0, 0.0], f32), ro.shape)
    with np.errstate(all="ignore"):
        denom = dot(n, rd)
        t = ((-((dot(n, ro) + f32(0.0)).astype(f32))) / denom).astype(f32)
    hit = ~(np.abs(denom) < f32(1e-6)) & ~(t < f32(eps))
    return hit, t, _point(ro, rd, t), np.array(n)


def intersect_sphere(eps, ro, rd, c, r):
    """intersectSphere -> (hit, t, p, n); the far root when the near one lies below eps (a ray starting inside)."""
    eps = f32(eps)
    with np.errstate(all="ignore"):
        oc = (ro - c).astype(f32)
        b = dot(oc, rd)
        c2 = (dot(oc, oc) - f32(r * r)).astype(f32)
        disc = ((b * b).astype(f32) - c2).astype(f32)
        s = np.sqrt(np.maximum(disc, f32(0.0))).astype(f32)
        t = (-b - s).astype(f32)
        t = np.where(t < eps, (-b + s).astype(f32), t)
        hit = ~(disc < f32(0.0)) & ~(t < eps)
        p = _point(ro, rd, t)
        n = normalize((p - c).astype(f32))
    return hit, t, p, n


def trace_analytic(u, ro, rd, include_glass=True, include_marker=True):
    """traceAnalyticCore(ro, rd, includeGlass, includeMarker): the objects in list order, a later one wins only at a strictly smaller t."""
    ro, rd = _f(ro), _f(rd)
    n = ro.shape[0]
    t = np.full(n, f32(u.inf), f32)
    obj = np.full(n, -1, np.int32)
    nrm, pt = np.zeros((n, 3), f32), np.zeros((n, 3), f32)

    def take(hit, tt, p, nn, oid):
        win = hit & (tt < t)
        t[win], obj[win], pt[win], nrm[win] = tt[win], oid, p[win], nn[win]

    take(*intersect_plane(u.eps, ro, rd), FLOOR)
    for (c, r, oid) in SPHERES:
        if oid == 2 and not include_glass:
            continue
        take(*intersect_sphere(u.eps, ro, rd, c, r), oid)
    if include_marker and u.pointLightEnabled == 1:
        take(*intersect_sphere(u.eps, ro, rd, _f(list(u.pointLightPos)), MARKER_RADIUS), MARKER)
    return Answer(t, obj, nrm, pt)


def bounded(u, a, tmax):
    """The answer as a query with per-ray tMax reports it: a hit exactly when t <= tMax (tMax < 0: an empty slot)."""
    if tmax is None:
        return a
    tmax = _f(tmax)
    keep = (a.obj >= 0) & ~(tmax < 0) & (a.t <= tmax)
    return Answer(np.where(keep, a.t, f32(u.inf)).astype(f32), np.where(keep, a.obj, -1).astype(np.int32),
                  np.where(keep[:, None], a.normal, f32(0)).astype(f32), np.where(keep[:, None], a.point, f32(0)).astype(f32))


def primary_dir(u, x, y):
    """primaryDirJ(u, x + 0.5, y + 0.5, u.jitter) for integer pixel coordinates x, y (arrays)."""
    jx = f32(u.jitter[0]) if u.enableJitter == 1 else f32(0.0)
    jy = f32(u.jitter[1]) if u.enableJitter == 1 else f32(0.0)
    fcx = (np.asarray(x).astype(f32) + f32(0.5)).astype(f32)
    fcy = (np.asarray(y).astype(f32) + f32(0.5)).astype(f32)
    uvx = ((fcx + jx).astype(f32) / f32(u.resolution[0])).astype(f32)
    uvy = ((fcy + jy).astype(f32) / f32(u.resolution[1])).astype(f32)
    nx = ((uvx * f32(2.0)).astype(f32) - f32(1.0)).astype(f32)
    ny = ((uvy * f32(2.0)).astype(f32) - f32(1.0)).astype(f32)
    right, up, fwd = _f(list(u.camRight)), _f(list(u.camUp)), _f(list(u.camFwd))
    sx = (f32(u.tanHalfFov) * f32(u.aspect)).astype(f32)
    a = ((nx[:, None] * right).astype(f32) * sx).astype(f32)
    b = ((ny[:, None] * up).astype(f32) * f32(u.tanHalfFov)).astype(f32)
    return normalize(((fwd + a).astype(f32) + b).astype(f32))


def pixel_rays(u, xy):
    xy = np.asarray(xy, np.int32).reshape(-1, 2)
    rd = primary_dir(u, xy[:, 0], xy[:, 1])
    ro = np.broadcast_to(_f(list(u.camPos)), rd.shape).copy()
    return ro, rd


def mesh_answers(u, nodes12, tris12, ro, rd):
    """The oracle's traceBVH on every ray -> Answer (obj MESH on a hit)."""
    import oracle as orc
    n = ro.shape[0]
    t = np.full(n, f32(u.inf), f32)
    obj = np.full(n, -1, np.int32)
    nrm, pt = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    for i in range(n):
        hit, tt, p, nn, _ = orc.trace_bvh(u, nodes12, tris12, ro[i], rd[i])
        if hit:
            t[i], obj[i], nrm[i] = tt, MESH, nn
            pt[i] = _point(ro[i:i + 1], rd[i:i + 1], np.array([tt], f32))[0]
    return Answer(t, obj, nrm, pt)


def combine(a, m):
    """traceScene's rule: the mesh answer m replaces the analytic answer a only at a strictly smaller t (a miss has t = uINF)."""
    win = (m.obj >= 0) & (m.t < a.t)
    return Answer(np.where(win, m.t, a.t).astype(f32), np.where(win, m.obj, a.obj).astype(np.int32),
                  np.where(win[:, None], m.normal, a.normal).astype(f32), np.where(win[:, None], m.point, a.point).astype(f32))


def trace_hybrid(u, nodes12, tris12, ro, rd, include_glass=True, include_marker=True):
    ro, rd = _f(ro), _f(rd)
    return combine(trace_analytic(u, ro, rd, include_glass, include_marker), mesh_answers(u, nodes12, tris12, ro, rd))


def gbuffer(a):
    """The frame's GPOS / GNRM at a pixel whose primary answer is a: (f16(point), 1) / (f16(normalize(normal)), 0) on a hit, zero on a miss,
    as uint16 half bits [N,4]."""
    hit = a.obj >= 0
    n = a.t.shape[0]
    pos, nrm = np.zeros((n, 4), f32), np.zeros((n, 4), f32)
    pos[hit, :3], pos[hit, 3] = a.point[hit], 1.0
    nrm[hit, :3] = normalize(a.normal[hit]) if hit.any() else nrm[hit, :3]
    return pos.astype(np.float16).view(np.uint16), nrm.astype(np.float16).view(np.uint16)
