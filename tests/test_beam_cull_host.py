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
  every such pixel as a miss; the non-vacuity conditions on the 160x96 close-up; a beam that covers the whole mesh is kept by frontier overflow;
* the walk against a restatement that shares no line with rt_beam.hpp (beam_cull_cases.walk): per tile of every view the same verdict and the same count of
  levels, over all tiles the sums rt.beam_cull reports; the comb scenes reach the widths they were built for -- dead behind a level of 32, of 33 .. 63 and of 64
  nodes, a level of 64 behind a level of 64, overflow at exactly 65 survivors and at 128 -- and their hit variants are alive through one node of the widest level;
* a ray with a zero direction component (the sliver scenes): the tile that holds it is kept by that rule alone and holds the only hits of the frame.
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


def _widest(entry):
    return max(entry[2]) if entry[2] else 0


@pytest.mark.parametrize("case", list(bc.CASES))
def test_the_header_walk_equals_an_independent_walk(case):
    """bc.walk restates the root-box test, the breadth-first frontier, the overflow rule and the count of levels in numpy, and shares no line with rt_beam.hpp:
    per tile rt.beam_walk gives its verdict and its levels, and rt.beam_cull's flags and sums are those of the tiles."""
    m, w, h, _, _ = bc.CASES[case]
    dead, stats, rd = bc.host_cull(case)
    ro = np.array(list(bc.uniforms(case)[0].camPos), f32)
    mine = bc.independent_cull(case)
    assert len(mine) == dead.size
    for t, ((L, H, ok), (verdict, levels, _)) in enumerate(zip(bc.tile_intervals(rd, w, h), mine)):
        if not ok or ((L > 0) != (H > 0)).any():                            # an unusable component, or an axis of both signs: kept, nothing walked
            assert (verdict, levels) == (bc.ALIVE, 0), (case, t)
        v, lv = rt.beam_walk(ro, L, H, packed=bc.packed(m))
        assert (int(v[0]), int(lv[0])) == (verdict, levels), (case, t)
        assert dead[t] == (verdict == bc.DEAD), (case, t)
    verdicts = [e[0] for e in mine]
    assert (stats.tiles, stats.deadTiles, stats.overflowTiles, stats.levels) == (len(mine), verdicts.count(bc.DEAD), verdicts.count(bc.OVERFLOW), sum(e[1] for e in mine))


def test_the_comb_scenes_reach_the_wide_levels():
    """The widths the comb scenes exist for, by the independent walk -- conditions, not measurements: a dead verdict behind a level of 32 inner nodes, of 33 .. 63
    and of exactly 64; a level of 64 that follows a level of more than 32 (a compaction out of the upper half of the lanes); overflow at exactly 65 survivors and
    at 128 or more.  At this builder: tile (2, 1) of comb32 32, comb64s33 33, comb64s40 40, comb64 64, comb128s64 64, comb128alt 64 behind 64, all dead;
    comb128s65 65 and comb128 128, both kept by overflow.  The hit scenes (comb128alt_h*, comb64_h*): the same widths, and the tile alive through one node of
    the widest level -- the verdict that shows a node lost on the way."""
    dead_widths, overflow_widths, full_steps = set(), set(), []
    for case in bc.COMB_CASES:
        mine = bc.independent_cull(case)
        t = bc.COMB_TILE[1] * 10 + bc.COMB_TILE[0]
        for verdict, levels, widths in mine:
            if verdict == bc.DEAD and levels:
                dead_widths.add(max(widths))
                full_steps += [case for a, b in zip(widths, widths[1:]) if a > 32 and b == 64]
            if verdict == bc.OVERFLOW:
                assert max(widths[:-1]) <= 64 < widths[-1]
                overflow_widths.add(widths[-1])
        # the scene's own tile carries the scene's width
        slabs, straddle, hit = bc.COMBS[bc.CASES[case][0]]
        want = slabs if straddle is None else slabs // 2 if straddle == "alternate" else straddle
        assert _widest(mine[t]) == want and mine[t][0] == (bc.ALIVE if hit is not None else bc.DEAD if want <= 64 else bc.OVERFLOW), (case, mine[t])
        if hit is not None:
            # alive through one node of the 64: the same scene without the hit is dead, and the leaf shows at the level that stands on the 64 slabs
            assert not bc.comb_moved(hit, straddle) and mine[t][2][-1] == 64 and mine[t][1] == len(mine[t][2])
            assert bc.independent_cull(f"comb{slabs}{'alt' if straddle else ''}_160x96")[t][0] == bc.DEAD
            if straddle == "alternate":
                assert mine[t][2][-2:] == [64, 64]                           # ... behind a compaction of 64 nodes into 64
        verdicts = [e[0] for e in mine]
        assert verdicts.count(bc.ALIVE) > 0 and sum(1 for e in mine if e[0] == bc.DEAD and e[1] == 0) > 0      # tiles that see a leaf, tiles dead at the root box
    assert 32 in dead_widths, f"no dead tile behind a level of 32: {sorted(dead_widths)}"
    assert any(33 <= x <= 63 for x in dead_widths), f"no dead tile behind a level of 33 .. 63: {sorted(dead_widths)}"
    assert 64 in dead_widths, f"no dead tile behind a level of 64: {sorted(dead_widths)}"
    assert full_steps, "no dead tile with a level of 64 behind a level of more than 32"
    assert 65 in overflow_widths, f"no overflow at exactly 65 survivors: {sorted(overflow_widths)}"
    assert any(x >= 128 for x in overflow_widths), f"no overflow at 128 or more survivors: {sorted(overflow_widths)}"


@pytest.mark.parametrize("tris", [2, 16])
def test_a_zero_direction_component_keeps_the_tile(orc, tris):
    """The sliver scenes: with a jitter of -0.5 pixel column 32 has dir.x == 0 and rdInv.x == inf, and only those rays meet the strip.  Tile 2 is alive by the
    unusable-component rule alone -- the interval of its other rays fails the root box -- and holds the strip's hits; with a jitter of -0.25 nothing is infinite,
    no ray of the tile passes the box and the tile is dead."""
    zero, ctrl = f"sliver{tris}_zero_64x48", f"sliver{tris}_ctrl_64x48"
    m, w, h, _, _ = bc.CASES[zero]
    p = bc.packed(m)
    assert (p["info"].rootRefW < 0) == (tris == 2) and bc.mesh(m)[1].shape[0] == tris         # the root a leaf / a walk below the root
    lo, hi = f32(p["info"].rootMin), f32(p["info"].rootMax)
    ro = np.array(bc.SLIVER_POS, f32)
    tile = bc.tile_of_pixels(w, h) == bc.SLIVER_TILE
    # jitter -0.5
    dead, _, rd = bc.host_cull(zero)
    inf_cols = np.unique(np.nonzero(np.isinf(rd[..., 0]))[2])
    assert inf_cols.tolist() == [32] and np.isinf(rd[:, :, 32, 0]).all() and bc.usable(rd[..., 1:]).all()
    assert dead[bc.SLIVER_TILE] == 0 and bc.independent_cull(zero)[bc.SLIVER_TILE] == (bc.ALIVE, 0, [])
    rays = rd[:, tile]                                                       # [K, 256, 3]
    good = rays[bc.usable(rays).all(-1)]
    assert good.shape[0] == bc.HAND_K * 240
    L, H = good.min(0), good.max(0)
    assert bc.interval_ok(L, H) and bc.slab_fails(ro, lo, hi, L, H) and rt.beam_slab(ro, lo, hi, L, H)[0][0] == 1
    assert rt.beam_walk(ro, L, H, packed=p)[0][0] == bc.DEAD
    passing = bc.slab(ro, rays.reshape(-1, 3), lo, hi)[0].reshape(bc.HAND_K, 16, 16)
    assert passing.sum() == 48 and passing[:, :, 1:].sum() == 0 and (passing[:, :, 0].sum(1) == 12).all()     # 12 pixels x 4 frames, all in column 32
    hits = 0
    for u in bc.uniforms(zero):
        prim = orc.primary_hits(u, *bc.mesh(m))[0][:, 1].copy().view(np.int32).reshape(h, w)
        assert (prim[~tile] < 0).all() and (prim[:, 33:] < 0).all()
        hits += int((prim[:, 32] >= 0).sum())
    assert hits > 0
    # jitter -0.25
    dead, _, rd = bc.host_cull(ctrl)
    assert bc.usable(rd).all()
    assert dead[bc.SLIVER_TILE] == 1 and bc.independent_cull(ctrl)[bc.SLIVER_TILE] == (bc.DEAD, 0, [])
    assert not bc.slab(ro, rd[:, tile].reshape(-1, 3), lo, hi)[0].any()
    for u in bc.uniforms(ctrl):
        prim = orc.primary_hits(u, *bc.mesh(m))[0][:, 1].copy().view(np.int32).reshape(h, w)
        assert (prim[tile] < 0).all()


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
