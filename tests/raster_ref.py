"""numpy reference of the raster preview (rt_render_raster), rule for rule as DESIGN.md 11 states them.

Everything is float32 / int64 numpy in the same operation order as csrc/rt_raster.hip, so the device frame must equal this one
bit for bit (RGBA8, primitive id, depth24).  `window=(x0, y0, x1, y1)` restricts the work to a pixel rectangle (row 0 = bottom), so
1080p frames can be checked in pieces.
"""
from __future__ import annotations

import numpy as np

F = np.float32
GUARD2 = F(2097152.0)          # 2 x the guard band of 2^20 pixels
SNAP_LIMIT = F(536870912.0)    # |snapped coordinate| < 2^29 (1/256 pixel)
D24_MAX = 0xFFFFFF
BACKGROUND = 0xFFFFFFFF
CLEAR = (0.1, 0.0, 0.2)
MAX_POLY = 8                   # a triangle clipped by five planes has at most 3 + 5 vertices in exact arithmetic


def mat4_mul(a, b):
    """rt_mat4_mul: column-major, out[c*4+r] = ((a[r]*b[4c] + a[4+r]*b[4c+1]) + a[8+r]*b[4c+2]) + a[12+r]*b[4c+3], float32."""
    a, b = np.asarray(a, F).reshape(16), np.asarray(b, F).reshape(16)
    out = np.zeros(16, F)
    for c in range(4):
        for r in range(4):
            out[c * 4 + r] = ((a[r] * b[c * 4] + a[4 + r] * b[c * 4 + 1]) + a[8 + r] * b[c * 4 + 2]) + a[12 + r] * b[c * 4 + 3]
    return out


def unorm8(x):
    c = np.clip(F(x), F(0), F(1))
    if c != c:
        c = F(0)
    return int(np.rint(c * F(255)))


def pack_rgba(color):
    return unorm8(color[0]) | (unorm8(color[1]) << 8) | (unorm8(color[2]) << 16) | (255 << 24)


def _plane(v, p, gx, gy):
    x, y, z, w = v
    return (z + w, gx * w - x, gx * w + x, gy * w - y, gy * w + y)[p]


def _lerp(a, b, t):   # from the inside vertex a towards the outside vertex b
    return tuple(F(a[i] + t * (b[i] - a[i])) for i in range(4))


def clip_polygon(v, gx, gy):
    """Sutherland-Hodgman against near (z >= -w), x <= gx w, x >= -gx w, y <= gy w, y >= -gy w, in that order; [] when a plane's
    output would pass MAX_POLY vertices."""
    for p in range(5):
        if not v:
            break
        out = []
        n = len(v)
        for k in range(n):
            a, b = v[k], v[(k + 1) % n]
            da, db = _plane(a, p, gx, gy), _plane(b, p, gx, gy)
            ia, ib = da >= 0, db >= 0
            if ia:
                out.append(a)
            if ia != ib:
                out.append(_lerp(a, b, F(da / (da - db))) if ia else _lerp(b, a, F(db / (db - da))))
        if len(out) > MAX_POLY:   # rounding added sign changes: the triangle is dropped (the device's record holds 8 vertices)
            return []
        v = out
    return v


def setup(positions, indices, mvp, W, H, prim_base=0):
    """One draw: -> (set-up triangles {"prim", "n", "x", "y", "z"} (vertex arrays [T, 8], the first n used), stats dict).
    A triangle is drawable when it has a fan piece of nonzero area (it is 'set up'); the others are 'dropped'."""
    pos = np.asarray(positions, F).reshape(-1, 3)
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    m = np.asarray(mvp, F).reshape(16)
    gx, gy = F(1) + GUARD2 / F(W), F(1) + GUARD2 / F(H)
    p = pos[idx]                                        # [T,3,3]
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):   # non-finite positions are legal input (the triangle is dropped)
        cx = ((m[0] * px + m[4] * py) + m[8] * pz) + m[12]
        cy = ((m[1] * px + m[5] * py) + m[9] * pz) + m[13]
        cz = ((m[2] * px + m[6] * py) + m[10] * pz) + m[14]
        cw = ((m[3] * px + m[7] * py) + m[11] * pz) + m[15]
        finite = np.isfinite(cx).all(1) & np.isfinite(cy).all(1) & np.isfinite(cz).all(1) & np.isfinite(cw).all(1)
        inside = (cz + cw >= 0) & (gx * cw - cx >= 0) & (gx * cw + cx >= 0) & (gy * cw - cy >= 0) & (gy * cw + cy >= 0)
    need_clip = finite & ~inside.all(1)
    T = idx.shape[0]
    n = np.zeros(T, np.int64)
    xs, ys, zs = np.zeros((T, 8), np.int64), np.zeros((T, 8), np.int64), np.zeros((T, 8), F)
    # triangles inside every plane: projected all at once (the same float32 operations as _project)
    fast = finite & ~need_clip
    with np.errstate(all="ignore"):
        xw = ((cx / cw) * F(0.5) + F(0.5)) * F(W)
        yw = ((cy / cw) * F(0.5) + F(0.5)) * F(H)
        zw = (cz / cw) * F(0.5) + F(0.5)
        sx, sy = np.rint(xw * F(256)), np.rint(yw * F(256))
        ok = (np.isfinite(sx) & np.isfinite(sy) & np.isfinite(zw) & (np.abs(sx) < SNAP_LIMIT) & (np.abs(sy) < SNAP_LIMIT)).all(1) & fast
    xs[ok, :3] = sx[ok].astype(np.int64); ys[ok, :3] = sy[ok].astype(np.int64); zs[ok, :3] = zw[ok]
    area = (xs[:, 1] - xs[:, 0]) * (ys[:, 2] - ys[:, 0]) - (ys[:, 1] - ys[:, 0]) * (xs[:, 2] - xs[:, 0])
    n[ok & (area != 0)] = 3
    for t in np.nonzero(need_clip)[0]:
        v = clip_polygon([(cx[t, k], cy[t, k], cz[t, k], cw[t, k]) for k in range(3)], gx, gy)
        poly = _project(v, W, H) if len(v) >= 3 else None
        if poly is None or not _drawable(poly[0], poly[1]):
            continue
        k = len(poly[0])
        xs[t, :k], ys[t, :k], zs[t, :k], n[t] = poly[0], poly[1], poly[2], k
    keep = n > 0
    polys = {"prim": np.arange(T, dtype=np.int64)[keep] + prim_base, "n": n[keep], "x": xs[keep], "y": ys[keep], "z": zs[keep]}
    stats = {"in": int(T), "dropped": int(T - keep.sum()), "clipped": int(need_clip.sum()), "set_up": int(keep.sum())}
    return polys, stats


def _project(v, W, H):
    xs, ys, zs = [], [], []
    with np.errstate(all="ignore"):
        for x, y, z, w in v:
            xw = ((x / w) * F(0.5) + F(0.5)) * F(W)
            yw = ((y / w) * F(0.5) + F(0.5)) * F(H)
            zw = (z / w) * F(0.5) + F(0.5)
            sx, sy = np.rint(xw * F(256)), np.rint(yw * F(256))
            if not (np.isfinite(sx) and np.isfinite(sy) and np.isfinite(zw) and abs(sx) < SNAP_LIMIT and abs(sy) < SNAP_LIMIT):
                return None
            xs.append(int(sx)); ys.append(int(sy)); zs.append(F(zw))
    return np.array(xs, np.int64), np.array(ys, np.int64), np.array(zs, F)


def _drawable(xs, ys):
    return any(int((xs[k] - xs[0]) * (ys[k + 1] - ys[0]) - (ys[k] - ys[0]) * (xs[k + 1] - xs[0])) != 0 for k in range(1, len(xs) - 1))


def _top_left(dx, dy):
    return dy < 0 or (dy == 0 and dx < 0)


def raster_piece(keys, win, prim, a, b, c):
    """One fan piece (vertices (x, y, z) in 1/256 pixel, z_w float32) into the uint64 key buffer of window win = (x0, y0, x1, y1)."""
    (ax, ay, az), (bx, by, bz), (cx, cy, cz) = a, b, c
    area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    if area == 0:
        return
    if area < 0:
        bx, by, bz, cx, cy, cz = cx, cy, cz, bx, by, bz
        area = -area
    x0, y0, x1, y1 = win
    # pixels whose centre 256 p + 128 lies in the piece's box, within the window
    i0 = max(x0, (min(ax, bx, cx) - 128 + 255) >> 8); i1 = min(x1 - 1, (max(ax, bx, cx) - 128) >> 8)
    j0 = max(y0, (min(ay, by, cy) - 128 + 255) >> 8); j1 = min(y1 - 1, (max(ay, by, cy) - 128) >> 8)
    if i0 > i1 or j0 > j1:
        return
    px = (np.arange(i0, i1 + 1, dtype=np.int64) * 256 + 128)[None, :]
    py = (np.arange(j0, j1 + 1, dtype=np.int64) * 256 + 128)[:, None]
    d0x, d0y, d1x, d1y, d2x, d2y = cx - bx, cy - by, ax - cx, ay - cy, bx - ax, by - ay
    e0 = d0x * (py - by) - d0y * (px - bx)
    e1 = d1x * (py - cy) - d1y * (px - cx)
    e2 = d2x * (py - ay) - d2y * (px - ax)
    cov = (e0 >= (0 if _top_left(d0x, d0y) else 1)) & (e1 >= (0 if _top_left(d1x, d1y) else 1)) & (e2 >= (0 if _top_left(d2x, d2y) else 1))
    if not cov.any():
        return
    z = ((e0.astype(F) * F(az) + e1.astype(F) * F(bz)) + e2.astype(F) * F(cz)) / np.int64(area).astype(F)   # int64 -> float32 in one rounding
    d24 = np.rint(np.maximum(z, F(0)) * F(16777215.0)).astype(np.uint64)
    ok = cov & (z <= F(1)) & (d24 < D24_MAX)
    key = (d24 << np.uint64(32)) | np.uint64(prim)
    sub = keys[j0 - y0:j1 - y0 + 1, i0 - x0:i1 - x0 + 1]
    np.minimum(sub, np.where(ok, key, np.uint64(0xFFFFFFFFFFFFFFFF)), out=sub)


def raster_polys(polys, W, H, window=None):
    """Key buffer (uint64, [h, w]) of the set-up triangles `polys` (a list of setup() results) over the window."""
    win = (0, 0, W, H) if window is None else tuple(int(v) for v in window)
    keys = np.full((win[3] - win[1], win[2] - win[0]), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    lo_x, lo_y, hi_x, hi_y = win[0] * 256 + 128, win[1] * 256 + 128, (win[2] - 1) * 256 + 128, (win[3] - 1) * 256 + 128
    for P in polys:
        used = np.arange(8)[None, :] < P["n"][:, None]
        big, small = np.int64(1) << 40, -(np.int64(1) << 40)
        hit = (np.where(used, P["x"], small).max(1) >= lo_x) & (np.where(used, P["x"], big).min(1) <= hi_x) & \
              (np.where(used, P["y"], small).max(1) >= lo_y) & (np.where(used, P["y"], big).min(1) <= hi_y)
        for t in np.nonzero(hit)[0]:
            k = int(P["n"][t])
            v = [(int(P["x"][t, q]), int(P["y"][t, q]), P["z"][t, q]) for q in range(k)]
            for q in range(1, k - 1):
                raster_piece(keys, win, int(P["prim"][t]), v[0], v[q], v[q + 1])
    return keys


def render(meshes, draws, view, proj, W, H, window=None, return_stats=False):
    """meshes: {slot: (positions [N,3], indices)}; draws: sequence of (slot, model16, color3) or RtRasterDraw-like objects.
    -> (rgba8 [h,w,4] uint8, prim_id [h,w] uint32, depth24 [h,w] uint32) over the window (default: the whole frame)."""
    vp = mat4_mul(proj, view)
    polys, colors, base = [], {}, 0
    stats = {"in": 0, "dropped": 0, "clipped": 0, "set_up": 0}
    for d in draws:
        slot, model, color = (d.mesh, list(d.model), list(d.color)) if hasattr(d, "mesh") else d
        pos, idx = meshes[slot]
        n = np.asarray(idx).size // 3
        mvp = mat4_mul(vp, model)
        if n:
            got, st = setup(pos, idx, mvp, W, H, base)
            polys.append(got)
        else:
            st = {"in": 0, "dropped": 0, "clipped": 0, "set_up": 0}
        for k in stats:
            stats[k] += st[k]
        colors[(base, base + n)] = pack_rgba(color)
        base += n
    keys = raster_polys(polys, W, H, window)
    prim = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    depth = (keys >> np.uint64(32)).astype(np.uint32)
    bg = keys == np.uint64(0xFFFFFFFFFFFFFFFF)
    prim[bg], depth[bg] = BACKGROUND, D24_MAX
    rgba32 = np.full(keys.shape, pack_rgba(CLEAR), np.uint32)
    for (lo, hi), c in colors.items():
        rgba32[~bg & (prim >= lo) & (prim < hi)] = c
    rgba = rgba32.view(np.uint8).reshape(keys.shape + (4,))
    return (rgba, prim, depth, stats) if return_stats else (rgba, prim, depth)
