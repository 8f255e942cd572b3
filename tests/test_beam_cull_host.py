"""The beam cull on the host (csrc/rt_beam.hpp, csrc/rt_beam.cpp; DESIGN.md 4.2 "Beam cull"), without a GPU.

A tile is dead when every primary ray of it, in every sub-frame of the launch set, surely misses the mesh: the interval [L, H] of the rays' reciprocal directions is
pushed through slab() at its two ends, and a walk over the two-child records finds no leaf whose box a ray of the interval could pass.

* enclosure: for random boxes, origins and intervals -- flat boxes and origins exactly on a box plane among them -- slab() restated in float32 numpy stays inside
  the bounds for r at both ends, at their neighbours inside the interval and at random points between, and beam_slab_fails implies that slab() is false for every
  such r;
* keep-cases: intervals that touch 0, span signs or hold inf, NaN or denormals, and bounds that are not finite, are kept whatever the box.  A flat box and an
  origin on a box plane are inside the argument (c = 0 gives t = +-0 at both ends, c0 == c1 gives t0 == t1; rt_beam.hpp): their keep-cases are the boxes a ray of
  the interval passes -- slab() holds there with tmax == tmin or at t = 0 -- and those must be kept;
* the walk, per view: no ray of any sub-frame of a dead tile reaches a leaf in a brute-force per-ray walk of the same records, and the oracle's primary hits show
  every such pixel as a miss; the non-vacuity conditions on the 160x96 close-up; a beam that covers the whole mesh is kept by frontier overflow.
"""
import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scenes
import beam_cull_cases as bc

f32 = np.float32


def _intervals(rng, n):
    """n x 3 intervals of one sign per axis, magnitudes over six decades, some degenerate (L == H)."""
    mag = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (n, 3, 2))).astype(f32)
    lo, hi = mag.min(2), mag.max(2)
    hi = np.where(rng.random((n, 3)) < 0.1, lo, hi)
    neg = rng.random((n, 3)) < 0.5
    return np.where(neg, -hi, lo).astype(f32), np.where(neg, -lo, hi).astype(f32)


def _samples(rng, L, H, m):
    """[m + 4, n, 3]: both ends, their neighbours inside the interval, m random points between."""
    inner_l, inner_h = np.minimum(np.nextafter(L, H), H), np.maximum(np.nextafter(H, L), L)
    mid = [(L + (H - L) * rng.random(L.shape).astype(f32)).astype(f32) for _ in range(m)]
    return np.clip(np.stack([L, H, inner_l, inner_h] + mid), L, H).astype(f32)


def test_bounds_enclose_slab():
    rng = np.random.default_rng(28)
    n = 20000
    L, H = _intervals(rng, n)
    ro = rng.uniform(-3, 3, (n, 3)).astype(f32)
    a, b = rng.uniform(-4, 4, (n, 3)).astype(f32), rng.uniform(-4, 4, (n, 3)).astype(f32)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    flat = rng.random((n, 3)) < 0.05
    hi = np.where(flat, lo, hi)                                              # flat boxes
    on = rng.random((n, 3)) < 0.05
    ro = np.where(on, np.where(rng.random((n, 3)) < 0.5, lo, hi), ro)       # the origin exactly on a box plane
    small = rng.random(n) < 0.3                                              # boxes a beam can miss: small ones
    hi = np.where(small[:, None], (lo + (hi - lo) * f32(0.02)).astype(f32), hi)
    fails, bounds = rt.beam_slab(ro, lo, hi, L, H)
    assert not np.isnan(bounds).any()
    assert 0.05 < fails.mean() < 0.95, fails.mean()                          # both answers occur
    assert (fails[(flat.any(1)) | (on.any(1))] != 0).any()                   # ... among the flat and on-plane cases too
    for r in _samples(rng, L, H, 6):
        ok, tmin, tmax = bc.slab(ro, r, lo, hi)
        assert (bounds[:, 0] <= tmin).all() and (tmin <= bounds[:, 1]).all()
        assert (bounds[:, 2] <= tmax).all() and (tmax <= bounds[:, 3]).all()
        assert not (ok & (fails != 0)).any()
    # per axis the r of a ray is free: mixed picks of the sample sets
    S = _samples(rng, L, H, 6)
    for _ in range(6):
        pick = rng.integers(0, S.shape[0], (n, 3))
        r = np.take_along_axis(S, pick[None], 0)[0]
        ok, tmin, tmax = bc.slab(ro, r, lo, hi)
        assert (bounds[:, 0] <= tmin).all() and (tmin <= bounds[:, 1]).all() and (bounds[:, 2] <= tmax).all() and (tmax <= bounds[:, 3]).all()
        assert not (ok & (fails != 0)).any()


def test_keep_cases():
    ro = np.array([0, 0, 0], f32)
    lo, hi = np.array([10, 10, 10], f32), np.array([11, 11, 11], f32)      # a box far off every beam below: only the keep rules can keep it
    good_l, good_h = np.array([-2, -2, -2], f32), np.array([-1, -1, -1], f32)
    assert rt.beam_slab(ro, lo, hi, good_l, good_h)[0][0] == 1               # (the control: this beam does fail the box)
    nan, inf, den = f32("nan"), f32("inf"), f32(1e-41)
    bad = [(0.0, 1.0), (-1.0, 0.0), (-0.0, -0.0), (0.0, 0.0), (-1.0, 1.0), (-1.0, den), (1.0, inf), (-inf, -1.0), (inf, inf), (nan, 1.0), (1.0, nan), (nan, nan),
           (den, 1.0), (-1.0, -den), (den, den), (2.0, 1.0)]
    for axis in range(3):
        for l, h in bad:
            L, H = good_l.copy(), good_h.copy()
            L[axis], H[axis] = l, h
            fails, bounds = rt.beam_slab(ro, lo, hi, L, H)
            assert fails[0] == 0 and np.isnan(bounds).all(), (axis, l, h)
            verdict, _ = rt.beam_walk(ro, L, H, packed=bc.packed("bunny3"))
            assert verdict[0] == 1, (axis, l, h)
    for axis in range(3):                                                    # bounds that are not finite
        for which, v in ((0, nan), (1, nan), (0, -inf), (1, inf)):
            b = [lo.copy(), hi.copy()]
            b[which][axis] = v
            assert rt.beam_slab(ro, b[0], b[1], good_l, good_h)[0][0] == 0, (axis, which, v)
        o = ro.copy(); o[axis] = nan
        assert rt.beam_slab(o, lo, hi, good_l, good_h)[0][0] == 0
    # flat boxes and origins on a box plane that a ray of the beam passes: slab() holds there with equality, the beam keeps them
    rng = np.random.default_rng(5)
    n = 4000
    L, H = _intervals(rng, n)
    r = (L + (H - L) * rng.random((n, 3)).astype(f32)).astype(f32)
    r = np.clip(r, L, H)
    o = rng.uniform(-2, 2, (n, 3)).astype(f32)
    with np.errstate(all="ignore"):
        p = (o + (f32(1.0) / r) * rng.uniform(0.5, 2.0, (n, 1)).astype(f32)).astype(f32)     # a point on the ray of reciprocal direction r
    blo, bhi = (p - f32(0.25)).astype(f32), (p + f32(0.25)).astype(f32)
    ax = rng.integers(0, 3, n)
    rows = np.arange(n)
    flat_lo, flat_hi = blo.copy(), bhi.copy()
    flat_lo[rows, ax] = p[rows, ax]; flat_hi[rows, ax] = p[rows, ax]          # flat through the point
    hit = bc.slab(o, r, flat_lo, flat_hi)[0]
    assert hit.sum() > n // 2
    assert (rt.beam_slab(o, flat_lo, flat_hi, L, H)[0][hit] == 0).all()
    on_lo, on_hi = np.minimum(blo, o), np.maximum(bhi, o)                    # the box grown to the origin ...
    on_lo[rows, ax] = np.where(r[rows, ax] > 0, o[rows, ax], on_lo[rows, ax])  # ... whose plane facing the ray goes through the origin
    on_hi[rows, ax] = np.where(r[rows, ax] < 0, o[rows, ax], on_hi[rows, ax])
    assert ((on_lo == o) | (on_hi == o)).any(1).all()
    hit = bc.slab(o, r, on_lo, on_hi)[0]
    assert hit.all()
    assert (rt.beam_slab(o, on_lo, on_hi, L, H)[0] == 0).all()


def test_no_bvh_keeps_everything():
    us = bc.uniforms("misses_root_box_64x48")
    nodes, tris = bc.mesh("bunny3")
    dead, stats = rt.beam_cull(us[0], nodes, tris, jitters=bc.jitters(us), packed=bc.packed("bunny3"))
    assert dead.all() and stats.deadTiles == dead.size
    us[0].nodeCount = 0                                                      # hasBVH == 0
    dead, stats = rt.beam_cull(us[0], nodes, tris, jitters=bc.jitters(us), packed=bc.packed("bunny3"))
    assert not dead.any() and stats.deadTiles == 0 and stats.tiles == dead.size


def _reaches_a_leaf(records, n_inner, root_ref, root_lo, root_hi, ro, rd_inv):
    """Brute force, per ray: does the ray pass the box of any leaf child on a walk that enters every node whose box it passes?  (No closest-hit cull: a superset
    of the nodes the launch visits.)  -> bool [n]"""
    n = rd_inv.shape[0]
    out = np.zeros(n, bool)
    idx = np.nonzero(bc.slab(ro, rd_inv, root_lo, root_hi)[0])[0]
    if root_ref < 0:
        out[idx] = True
        return out
    stack = [(root_ref, idx)]
    rec = records.reshape(-1, 16)
    refs = rec[:, [3, 7]].view(np.int32)
    while stack:
        node, idx = stack.pop()
        if idx.size == 0:
            continue
        for c in range(2):
            lo, hi = rec[node, 8 * c:8 * c + 3], rec[node, 8 * c + 4:8 * c + 7]
            sub = idx[bc.slab(ro, rd_inv[idx], lo, hi)[0]]
            ref = int(refs[node, c])
            if ref < 0:
                out[sub] = True
            else:
                assert ref < n_inner
                stack.append((ref, sub))
    return out


@pytest.mark.parametrize("case", list(bc.CASES))
def test_dead_tiles_hold_no_ray_that_reaches_a_leaf(orc, case):
    m, w, h, _, _ = bc.CASES[case]
    dead, stats, rd = bc.host_cull(case)
    us = bc.uniforms(case)
    p = bc.packed(m)
    rec = np.ascontiguousarray(p["nodes2w"]).view(f32)
    ro = np.array(list(us[0].camPos), f32)
    tile = bc.tile_of_pixels(w, h)
    in_dead = dead[tile] != 0                                                # [H, W]
    assert stats.tiles == dead.size and stats.deadTiles == int(dead.sum())
    nodes, tris = bc.mesh(m)
    for k, u in enumerate(us):
        rays = rd[k][in_dead]
        reach = _reaches_a_leaf(rec, p["info"].nInner, p["info"].rootRefW, f32(p["info"].rootMin), f32(p["info"].rootMax), ro, rays)
        assert not reach.any(), f"{case}: {int(reach.sum())} rays of dead tiles reach a leaf in sub-frame {k}"
        hits, _ = orc.primary_hits(u, nodes, tris)
        prim = hits[:, 1].copy().view(np.int32).reshape(h, w)
        assert (prim[in_dead] < 0).all(), f"{case}: the oracle hits a pixel of a dead tile in sub-frame {k}"
    if case == "misses_root_box_64x48":
        assert dead.all() and stats.levels == 0                              # culled at the root box
    if case in ("one_leaf_64x48", "inside_root_box_64x48"):
        assert not dead.all()                                                # somebody sees the mesh


def test_non_vacuity_of_the_closeup(orc):
    """160x96 close-up: at least a tenth of the tiles dead, at least a tenth alive with a missing pixel inside (the stock close-up satisfies both)."""
    case = "bunny3_160x96"
    m, w, h, _, _ = bc.CASES[case]
    dead, stats, _ = bc.host_cull(case)
    u = bc.uniforms(case)[0]
    hits, _ = orc.primary_hits(u, *bc.mesh(m))
    miss = hits[:, 1].copy().view(np.int32).reshape(h, w) < 0
    tile = bc.tile_of_pixels(w, h)
    tile_has_miss = np.bincount(tile[miss], minlength=dead.size) > 0
    assert dead.sum() * 10 >= dead.size, (int(dead.sum()), dead.size)
    assert ((dead == 0) & tile_has_miss).sum() * 10 >= dead.size


def test_a_beam_over_the_whole_mesh_overflows_the_frontier():
    p = rt.pack_scene(*scenes.bunny_bvh(4))
    lo, hi = f32(p["info"].rootMin), f32(p["info"].rootMax)
    ro = ((lo + hi) * f32(0.5) + np.array([5, 4, 6], f32)).astype(f32)
    corners = np.array([[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)], f32)
    d = corners - ro
    r = (f32(1.0) / (d / np.linalg.norm(d, axis=1, keepdims=True))).astype(f32)
    L, H = r.min(0), r.max(0)
    assert (H < 0).all()                                                     # one sign per axis: the interval is inside the argument
    verdict, levels = rt.beam_walk(ro, L, H, packed=p)
    assert verdict[0] == 2 and 6 <= levels[0] <= 8                           # 128 inner nodes at depth 7, every box inside the beam
    one = r[:1]                                                              # the same tree, one ray: never an overflow
    assert rt.beam_walk(ro, one, one, packed=p)[0][0] in (0, 1)


def test_rank_of_two_sees_its_own_tiles():
    case = "bunny3_160x96"
    full, _, _ = bc.host_cull(case)
    for rank in (0, 1):
        part, stats, _ = bc.host_cull(case, rank, 2)
        info, xy = rt.frame_geom(160, 96, rank, 2, slots=True)
        assert part.size == info.nLocalTiles == stats.tiles
        for lt in range(part.size):
            x, y = xy[lt * 256, 0], xy[lt * 256, 1]
            assert part[lt] == full[(y // 16) * 10 + x // 16]


def test_entries_refuse_bad_arguments():
    L = rt.lib()
    for name in ("rt_debug_beam_cull", "rt_debug_beam_slab", "rt_debug_beam_walk", "rt_debug_beam_cull_stats", "rt_debug_beam_cull_flags"):
        assert name in rt.SIGNATURES and hasattr(L, name), name
    u = bc.uniforms("bunny3_64x48")[0]
    dead = np.zeros(12, np.uint8)
    z3 = np.zeros(3, f32)
    fp = lambda a: a.ctypes.data_as(rt._FP)
    d8 = dead.ctypes.data_as(rt._U8P)
    assert L.rt_debug_beam_cull(None, None, 1, 0, 1, None, 0, -1, fp(z3), fp(z3), d8, 12, None, None) == rt.RT_ERR_INVALID
    assert L.rt_debug_beam_cull(u, None, 2, 0, 1, None, 0, -1, fp(z3), fp(z3), d8, 12, None, None) == rt.RT_ERR_INVALID       # a batch without jitters
    assert L.rt_debug_beam_cull(u, None, 1, 0, 1, None, 0, -1, fp(z3), fp(z3), d8, 11, None, None) == rt.RT_ERR_INVALID       # not the frame's tile count
    assert L.rt_debug_beam_cull(u, None, 1, 2, 2, None, 0, -1, fp(z3), fp(z3), d8, 12, None, None) == rt.RT_ERR_INVALID
    assert L.rt_debug_beam_cull(u, None, 1, 0, 1, None, 5, 0, fp(z3), fp(z3), d8, 12, None, None) == rt.RT_ERR_INVALID        # records missing
    assert L.rt_debug_beam_slab(1, None, None, None, None, None, None, None) == rt.RT_ERR_INVALID
    assert L.rt_debug_beam_walk(1, None, None, None, None, 0, -1, fp(z3), fp(z3), None, None) == rt.RT_ERR_INVALID
