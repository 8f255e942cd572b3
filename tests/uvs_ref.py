"""The UVs and the albedo texture of the dynamic mesh restated in numpy float32: every product and every sum rounded on its own, no
fmaf -- the float model of csrc/rt_mesh_uvs.hpp -- for rt_uv_rows, rt_hit_uvs, rt_sample_texture and the device arrays to be compared with bit for
bit.  The decode table is an argument: the tests take it from the library and check it separately."""
import numpy as np

from colors_ref import bits, prims

f32 = np.float32
NEAREST, CLAMP, SRGB = 1, 2, 4


def uv_rows(order, indices, uvs) -> np.ndarray:
    """[T,8]: row i holds (u0, v0, u1, v1), (u2, v2, 0, 0) of input triangle order[i]."""
    order = np.asarray(order, np.int64)
    ix = np.asarray(indices, np.int64).reshape(-1, 3)
    uv = np.asarray(uvs, f32)
    out = np.zeros((order.size, 8), f32)
    out[:, :6] = uv[ix[order]].reshape(-1, 6)
    return out


def hit_uvs(order, indices, uvs, rec) -> np.ndarray:
    """[N,2]: colors_ref.hit_colors' rule on two components."""
    order = np.asarray(order, np.int64)
    ix = np.asarray(indices, np.int64).reshape(-1, 3)
    uv = np.asarray(uvs, f32)
    rec = np.asarray(rec, f32)
    p = prims(rec).astype(np.int64)
    on = (p >= 0) & (p < order.size)
    corner = uv[ix[order[np.where(on, p, 0)]]]                                    # [N,3 corners,2]
    c0, c1, c2 = corner[:, 0], corner[:, 1], corner[:, 2]
    a, b = rec[:, 2:3], rec[:, 3:4]
    with np.errstate(all="ignore"):
        w = ((f32(1.0) - a).astype(f32) - b).astype(f32)
        m = (((c0 * w).astype(f32) + (c1 * a).astype(f32)).astype(f32) + (c2 * b).astype(f32)).astype(f32)
    same = (bits(c0) == bits(c1)) & (bits(c0) == bits(c2))
    keep = same | ~np.isfinite(a) | ~np.isfinite(b)
    out = np.where(keep, c0, m).astype(f32)
    out[~on] = 0
    return out


def srgb_table_f64() -> np.ndarray:
    """The sRGB decode of the 256 codes in double: the yardstick rt_srgb_table is held to."""
    x = np.arange(256, dtype=np.float64) / 255.0
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def _wrap(i, n, clamp):
    i = i.astype(np.int64)
    return np.clip(i, 0, n - 1) if clamp else ((i % n) + n) % n


def _axis(u, n, nearest, clamp):
    """-> (i0, i1, f) of one coordinate array on an edge of n texels."""
    u = np.asarray(u, f32).copy()
    u[~np.isfinite(u)] = 0
    with np.errstate(all="ignore"):
        if clamp:
            s = np.minimum(np.maximum(u, f32(0)), f32(1)).astype(f32)
        else:
            s = (u - np.floor(u).astype(f32)).astype(f32)
        sn = (s * f32(n)).astype(f32)
        if nearest:
            i = _wrap(np.floor(sn), n, clamp)
            return i, i, np.zeros_like(s)
        x = (sn - f32(0.5)).astype(f32)
        fl = np.floor(x).astype(f32)
        f = (x - fl).astype(f32)
    return _wrap(fl, n, clamp), _wrap(fl + 1, n, clamp), f


def sample_texture(texels, flags, uvs, table) -> np.ndarray:
    """[N,3]: texels uint8 [H,W,4] with row 0 at v = 0, table the 256 decoded values."""
    t = np.asarray(texels, np.uint8)
    H, W = t.shape[:2]
    uv = np.asarray(uvs, f32).reshape(-1, 2)
    table = np.asarray(table, f32)
    nearest, clamp = bool(flags & NEAREST), bool(flags & CLAMP)
    i0, i1, a = _axis(uv[:, 0], W, nearest, clamp)
    j0, j1, b = _axis(uv[:, 1], H, nearest, clamp)
    if nearest:
        return table[t[j0, i0, :3]]
    t00, t10, t01, t11 = table[t[j0, i0, :3]], table[t[j0, i1, :3]], table[t[j1, i0, :3]], table[t[j1, i1, :3]]
    one = f32(1)
    a, b = a[:, None], b[:, None]
    w00 = ((one - a).astype(f32) * (one - b).astype(f32)).astype(f32)
    w10 = (a * (one - b).astype(f32)).astype(f32)
    w01 = ((one - a).astype(f32) * b).astype(f32)
    w11 = (a * b).astype(f32)
    m = ((((t00 * w00).astype(f32) + (t10 * w10).astype(f32)).astype(f32) + (t01 * w01).astype(f32)).astype(f32) + (t11 * w11).astype(f32)).astype(f32)
    flat = (bits(t00) == bits(t10)) & (bits(t00) == bits(t01)) & (bits(t00) == bits(t11))
    return np.where(flat, t00, m).astype(f32)
