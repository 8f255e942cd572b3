"""Shared cases of the beam-cull tests (test_beam_cull_host.py, test_gpu_beam_cull.py; DESIGN.md 4.2 "Beam cull"): the views, their uniform blocks, and the
float32 restatements of slab() (rt_device_shade.hpp:128) and of the interval walk the host tests hold rt_beam.hpp against."""
import functools

import numpy as np

import opengl_raytracing_amd as rt
import scenes
import test_gpu_queue_diet as qd

f32 = np.float32
K = 8      # sub-frames of a stock case's launch set
HAND_K = 4  # ... of a case whose view is written into the uniform block by hand (HAND)

# name -> (mesh, W, H, camera position or None = the stock close-up, yaw)
CASES = {
    "bunny2_64x48": ("bunny2", 64, 48, None, -90.0),
    "bunny2_160x96": ("bunny2", 160, 96, None, -90.0),
    "bunny3_64x48": ("bunny3", 64, 48, None, -90.0),
    "bunny3_160x96": ("bunny3", 160, 96, None, -90.0),          # the non-vacuity case: dead tiles, and kept tiles that hold a missing pixel
    "two_mesh_160x96": ("two_mesh", 160, 96, None, -90.0),
    "one_leaf_64x48": ("one_leaf", 64, 48, (0.25, 0.9, 3.0), -90.0),
    "inside_root_box_64x48": ("bunny3", 64, 48, (-2.01, 1.51, 0.01), -90.0),
    "misses_root_box_64x48": ("bunny3", 64, 48, None, 90.0),     # the close-up camera turned round and up (no axis changes sign in a tile): no ray meets the root box
}

# The comb scenes: N slabs in depth behind the central ray of tile (2, 1) of a 160x96 frame, the first `straddle` of them on the ray (comb_tris).  Tile (2, 1)'s
# walk stands on one inner node per straddling slab at level log2 N and finds every leaf box missing one level later: a verdict behind a level of that many lanes.
# name -> (slabs, straddle: None = all, s = the first s, "alternate" = one slab of every pair, the front and the back one in turns: a level of 64 nodes each of
# which keeps one inner child, left and right children alike -- a compaction out of the upper 32 lanes, which a level of the other scenes never needs;
# hit: None, or the one straddling slab that has a cluster on the ray.  A dead verdict does not show a node the compaction lost -- the leaves below it miss
# anyway; in a hit scene the tile is alive through that one node alone, wherever the walk's order put it among the 64 lanes)
COMBS = {"comb32": (32, None, None), "comb64s33": (64, 33, None), "comb64s40": (64, 40, None), "comb64": (64, None, None), "comb128s64": (128, 64, None),
         "comb128s65": (128, 65, None), "comb128": (128, None, None), "comb128alt": (128, "alternate", None)}
COMB_HITS = (0, 35, 64, 67, 92, 99, 124, 127)
COMBS.update({f"comb128alt_h{h}": (128, "alternate", h) for h in COMB_HITS})
COMBS.update({f"comb64_h{h}": (64, None, h) for h in (21, 63)})
COMB_TILE = (2, 1)
COMB_TAN = float(np.tan(np.radians(0.75)))     # the narrow field of view keeps a tile's interval tight enough for the slabs to be apart in depth
# The sliver scenes: a strip in the plane x = camPos.x, thinner than a pixel, that only the rays with dir.x == 0 exactly meet -- 1 / 0 in rdInv.x.  With a jitter of
# -0.5 those are pixel column 32 of a 64-wide frame, the first column of tile column 2: tile 2 lives by the unusable-component rule alone.  name -> (triangles
# along y per side, jitter x)
SLIVERS = {"sliver2_zero": (1, -0.5), "sliver16_zero": (8, -0.5), "sliver2_ctrl": (1, -0.25), "sliver16_ctrl": (8, -0.25)}
SLIVER_POS = (0.3, 0.7, 2.0)
SLIVER_TILE = 2

# views written into the uniform block by hand, the axis-aligned basis (right +x, up +y, forward -z): case -> (camPos, tanHalfFov or None = the stock one,
# jitter x or None = the stock jitters; frame f's jitter y is then 0.1 f - 0.2)
HAND = {}
for _n in COMBS:
    CASES[f"{_n}_160x96"] = (_n, 160, 96, None, None)
    HAND[f"{_n}_160x96"] = ((0.0, 0.0, 0.0), COMB_TAN, None)
for _n, (_, _jx) in SLIVERS.items():
    CASES[f"{_n}_64x48"] = (_n, 64, 48, None, None)
    HAND[f"{_n}_64x48"] = (SLIVER_POS, None, _jx)
COMB_CASES = [f"{n}_160x96" for n in COMBS]
SLIVER_CASES = [f"{n}_64x48" for n in SLIVERS]


def stock_tan_half_fov():
    p = rt.default_render_params()
    return float(rt.frame_uniforms(p, scenes.camera("closeup", aspect=64 / 48), 64, 48, 0, True, 1, 1).tanHalfFov)


def comb_moved(j, straddle):
    return False if straddle is None else (j % 2 != (j // 2) % 2) if straddle == "alternate" else j >= straddle


def comb_tris(slabs, straddle=None, hit=None):
    """[slabs * 16, 9] rows of (v0, e1, e2).  d: the central ray of tile COMB_TILE (pixel corner (40, 24), no jitter).  Slab j sits at d * (10 + 4 j) / -d.z: two
    clusters of eight tiny triangles at (+-1.5, (q - 3.5) * 0.02, 0) from there.  The depth spacing exceeds a slab's width, the leaf limit is eight: the median
    split separates the slabs first, then a slab's two clusters.  The slabs outside `straddle` (COMBS) are moved sideways by 6: their inner node no longer straddles the beam.  Slab `hit` has its second cluster on the ray."""
    w, h = 160.0, 96.0
    cx, cy = COMB_TILE[0] * 16 + 8, COMB_TILE[1] * 16 + 8
    d = np.array([(cx / w * 2 - 1) * COMB_TAN * (w / h), (cy / h * 2 - 1) * COMB_TAN, -1.0])
    rows = []
    for j in range(slabs):
        c = d * (10.0 + 4.0 * j) / -d[2]
        if comb_moved(j, straddle):
            c = c + np.array([6.0, 0.0, 0.0])
        for side in (-1.5, 0.0 if j == hit else 1.5):
            for q in range(8):
                v0 = c + np.array([side, (q - 3.5) * 0.02, 0.0])
                rows.append(np.concatenate([v0, [0.01, 0.0, 0.0], [0.0, 0.01, 0.0]]))
    return np.array(rows, f32)


def sliver_tris(n):
    """[2 n, 9] rows of (v0, e1, e2): the strip x in [0.299, 0.301], z from -1.0 to -1.01 (three units in front of SLIVER_POS), y over the part of the frame's
    height that shows in tile row 0 only, cut into n quads along y."""
    t = stock_tan_half_fov()
    ys = np.linspace(SLIVER_POS[1] - 3 * t * 0.95, SLIVER_POS[1] - 3 * t * 0.45, n + 1)
    rows = []
    for y0, y1 in zip(ys[:-1], ys[1:]):
        a, b, c, d = (0.299, y0, -1.0), (0.301, y0, -1.01), (0.301, y1, -1.01), (0.299, y1, -1.0)
        for p, q, r in ((a, b, c), (a, c, d)):
            p, q, r = (np.array(v) for v in (p, q, r))
            rows.append(np.concatenate([p, q - p, r - p]))
    return np.array(rows, f32)


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "two_mesh":
        return qd._mesh("two_mesh")
    if name == "one_leaf":
        return scenes.one_leaf_mesh()
    if name in COMBS:
        return rt.build_bvh(comb_tris(*COMBS[name]))
    if name in SLIVERS:
        return rt.build_bvh(sliver_tris(SLIVERS[name][0]))
    return scenes.bunny_bvh(int(name[-1]))


@functools.lru_cache(maxsize=None)
def packed(name):
    return rt.pack_scene(*mesh(name))


def camera(case):
    _, w, h, pos, yaw = CASES[case]
    cam = scenes.camera("closeup", aspect=w / h)
    if pos is not None:
        cam.pos[0], cam.pos[1], cam.pos[2] = pos
    cam.yaw = yaw
    if yaw > 0:
        cam.pitch = 40.0
    return cam


def frames_of(case):
    return HAND_K if case in HAND else K


def uniforms(case, frames=None, params=(("sppPerFrame", 2),)):
    m, w, h, _, _ = CASES[case]
    frames = frames_of(case) if frames is None else frames
    nodes, tris = mesh(m)
    p = rt.default_render_params()
    for k, v in params:
        setattr(p, k, v)
    if case not in HAND:
        cam = camera(case)
        return [rt.frame_uniforms(p, cam, w, h, f, True, nodes.shape[0], tris.shape[0]) for f in range(frames)]
    # primaryDirJ reads camPos, the basis, tanHalfFov, aspect, resolution and the jitter, on host and device alike: the view is those fields
    pos, tan, jitter_x = HAND[case]
    us = [rt.frame_uniforms(p, scenes.camera("closeup", aspect=w / h), w, h, f, True, nodes.shape[0], tris.shape[0]) for f in range(frames)]
    for f, u in enumerate(us):
        for a in range(3):
            u.camPos[a], u.camRight[a], u.camUp[a], u.camFwd[a] = pos[a], (1.0, 0.0, 0.0)[a], (0.0, 1.0, 0.0)[a], (0.0, 0.0, -1.0)[a]
        if tan is not None:
            u.tanHalfFov = tan
        u.enableJitter = 1
        if jitter_x is not None:
            u.jitter[0], u.jitter[1] = jitter_x, 0.1 * f - 0.2
    return us


def jitters(us):
    return np.array([[u.jitter[0], u.jitter[1]] for u in us], f32)


@functools.lru_cache(maxsize=None)
def host_cull(case, rank=0, world=1, frames=None):
    """(dead, stats, rd_inv [K, H, W, 3]) of the case by the host definition."""
    m = CASES[case][0]
    us = uniforms(case, frames)
    return rt.beam_cull(us[0], *mesh(m), jitters=jitters(us), rank=rank, world=world, rays=True, packed=packed(m))


def tile_of_pixels(w, h):
    """[H, W] -> index of the pixel's 16x16 tile (one rank: local tile == tile)."""
    tx = (w + 15) // 16
    y, x = np.mgrid[0:h, 0:w]
    return (y // 16) * tx + x // 16


def slab(ro, rd_inv, lo, hi):
    """slab() in float32 numpy, operation for operation -> (tmax >= tmin, tmin, tmax); arrays broadcast over the last axis of 3."""
    ro, rd_inv, lo, hi = (np.asarray(a, f32) for a in (ro, rd_inv, lo, hi))
    with np.errstate(all="ignore"):
        t0 = ((lo - ro).astype(f32) * rd_inv).astype(f32)
        t1 = ((hi - ro).astype(f32) * rd_inv).astype(f32)
        n, f = np.fmin(t0, t1), np.fmax(t0, t1)
        tmin = np.fmax(np.fmax(n[..., 0], n[..., 1]), np.fmax(n[..., 2], f32(0.0)))
        tmax = np.fmin(np.fmin(f[..., 0], f[..., 1]), f[..., 2])
        return tmax >= tmin, tmin, tmax


# ---- the interval walk restated: nothing below calls rt.beam_walk, rt.beam_cull or rt.beam_slab, or reads rt_beam.hpp's constants

FRONTIER = 64      # inner nodes a level holds at most: the lanes of a wave
DEAD, ALIVE, OVERFLOW = 0, 1, 2


def usable(v):
    """finite, normal, not zero"""
    v = np.asarray(v, f32)
    return np.isfinite(v) & (np.abs(v) >= np.finfo(f32).tiny)


def interval_ok(L, H):
    L, H = np.asarray(L, f32), np.asarray(H, f32)
    with np.errstate(invalid="ignore"):
        return bool((usable(L) & usable(H) & (L <= H) & ((L > 0) == (H > 0))).all())


def slab_fails(ro, lo, hi, L, H):
    """slab_bounds in float32 numpy, operation for operation, over boxes [..., 3] against one interval: tmaxHi < tminLo, and every bound finite -> bool [...]"""
    ro, lo, hi, L, H = (np.asarray(a, f32) for a in (ro, lo, hi, L, H))
    with np.errstate(all="ignore"):
        c0, c1 = (lo - ro).astype(f32), (hi - ro).astype(f32)
        finite = (np.isfinite(c0) & np.isfinite(c1)).all(-1)
        a0, b0, a1, b1 = (c0 * L).astype(f32), (c0 * H).astype(f32), (c1 * L).astype(f32), (c1 * H).astype(f32)
        t0lo, t0hi, t1lo, t1hi = np.fmin(a0, b0), np.fmax(a0, b0), np.fmin(a1, b1), np.fmax(a1, b1)
        nlo, fhi = np.fmin(t0lo, t1lo), np.fmax(t0hi, t1hi)
        tmin_lo = np.fmax(np.fmax(nlo[..., 0], nlo[..., 1]), np.fmax(nlo[..., 2], f32(0.0)))
        tmax_hi = np.fmin(np.fmin(fhi[..., 0], fhi[..., 1]), fhi[..., 2])
        return finite & (tmax_hi < tmin_lo)


def walk(p, ro, L, H):
    """A tile's verdict by the frontier walk over the two-child records of the pack_scene result p -> (verdict, levels, widths).  The root box first; then level
    by level: alive at the first level one of whose surviving children is a leaf, overflow when more than FRONTIER inner children survive a level, dead when none
    does.  levels: levels of records read.  widths: the inner nodes each level read stood on, and last the survivors of the level that overflowed."""
    info = p["info"]
    if not interval_ok(L, H):
        return ALIVE, 0, []
    if slab_fails(ro, f32(info.rootMin), f32(info.rootMax), L, H):
        return DEAD, 0, []
    n_inner, root = int(info.nInner), int(info.rootRefW)
    if root < 0 or root >= n_inner:
        return ALIVE, 0, []
    rec = np.ascontiguousarray(p["nodes2w"]).view(f32).reshape(-1, 16)
    cur, levels, widths = np.array([root]), 0, []
    while cur.size:
        levels += 1
        widths.append(int(cur.size))
        r = rec[cur]
        lo, hi = np.stack([r[:, 0:3], r[:, 8:11]], 1), np.stack([r[:, 4:7], r[:, 12:15]], 1)      # [n, 2, 3]: left, right
        refs = np.ascontiguousarray(r[:, [3, 7]]).view(np.int32)
        kept = refs[~slab_fails(ro, lo, hi, L, H)]
        if ((kept < 0) | (kept >= n_inner)).any():
            return ALIVE, levels, widths
        if kept.size > FRONTIER:
            return OVERFLOW, levels, widths + [int(kept.size)]
        cur = kept
    return DEAD, levels, widths


def tile_intervals(rd, w, h):
    """rd_inv [K, H, W, 3] -> per 16x16 tile (L, H, every component of every ray usable)"""
    out = []
    for ty in range((h + 15) // 16):
        for tx in range((w + 15) // 16):
            r = rd[:, ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].reshape(-1, 3)
            with np.errstate(invalid="ignore"):
                out.append((r.min(0), r.max(0), bool(usable(r).all())))
    return out


@functools.lru_cache(maxsize=None)
def independent_cull(case):
    """[(verdict, levels, widths)] per tile of the case's frame, one rank, by walk() over the rays rt.beam_cull(rays=True) returns."""
    m, w, h, _, _ = CASES[case]
    _, _, rd = host_cull(case)
    ro = np.array(list(uniforms(case)[0].camPos), f32)
    return [walk(packed(m), ro, L, H) if ok else (ALIVE, 0, []) for L, H, ok in tile_intervals(rd, w, h)]
