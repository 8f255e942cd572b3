"""The beam cull on the GPU (k_beam_cull, RT_BEAM_CULL; DESIGN.md 4.2 "Beam cull").

In front of a launch set's primary stage one wave per local spatial tile decides whether every primary ray of the tile, in every frame of the set, surely misses
the mesh; the primary stage finishes the pixels of such a tile at once -- the call k_post_primary would have made -- and they are no candidates.

* the device's flags and counts equal the host definition's (rt.beam_cull, test_beam_cull_host.py) for every view of beam_cull_cases.py, and for one rank of two;
* rt_render_frames with RT_BEAM_CULL=1 against 0: all four targets bit for bit for K = 1, 2, 3, 8, 16 frames on frames of 160x96, 64x48, 48x48 and 12x40 pixels
  and on rank 1 of 2, in both candidate orders and with a queue budget of 1 MB; the candidates and primary rays drop by the pixels of dead tiles that pass
  the root box, every other count but gatherLoadsShadow stays; K = 8 also against the oracle;
* the comb and the sliver scenes of beam_cull_cases.py among those views: k_beam_cull's own lane-parallel walk behind levels of 32, 33, 40 and 64 lanes (dead),
  through a compaction of 64 nodes into 64 out of both ballots (alive by one node of them, eight positions of it), at 65 and 128 survivors (kept by overflow),
  and its `bad` ballot for a ray with a zero direction component; frames of four of them cull on against off and two against the oracle;
* the cull stands down under RT_FUSED=1 and RT_IMPLICIT=1 (no tiles counted, no flags, the same targets); a lane's flag buffer regrows with the frame;
* a batch right behind rt_mesh_rebuild and behind a refit of moved positions: the flags follow the new tree, the targets equal the path without the cull.
"""
import functools
import types

import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scenes
import test_gpu_queue_diet as qd
import beam_cull_cases as bc

f32 = np.float32
VARS = qd.VARS + ("RT_BATCH_INTERLEAVE", "RT_LIGHT_MASKS", "RT_BEAM_CULL", "RT_FUSED", "RT_IMPLICIT")
KS = (1, 2, 3, 8, 16)
MOVES = ("candidatePixels", "primary", "gatherLoadsPrimary", "mergedLoadsPrimary", "gatherLoadsShadow")      # counts the cull changes (and the one no run fixes)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)


def _renderer(mesh, w, h, rank=0, world=1):
    r = rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT, rank=rank, world_size=world)
    r.upload_bvh(*bc.mesh(mesh)); r.upload_env(scenes.tiny_env(8)); r.resize(w, h)
    r.traced_rays(reset=True)
    return r


# ---------------------------------------------------------------- 1. flags

@pytest.mark.gpu
@pytest.mark.parametrize("case,rank,world", [(c, 0, 1) for c in bc.CASES] + [("bunny3_160x96", 1, 2), ("two_mesh_160x96", 0, 2)])
def test_device_flags_equal_the_host_definition(monkeypatch, case, rank, world):
    monkeypatch.setenv("RT_BEAM_CULL", "1")
    m, w, h, _, _ = bc.CASES[case]
    want, wstats, _ = bc.host_cull(case, rank, world)
    with _renderer(m, w, h, rank, world) as r:
        r.beam_cull_stats(reset=True)
        r.render_frames(bc.uniforms(case))
        got = r.beam_cull_flags(want.size)
        st = r.beam_cull_stats()
    assert np.array_equal(got, want), f"{case} rank {rank}/{world}: {int((got != want).sum())} of {want.size} flags differ"
    assert (st.tiles, st.deadTiles, st.overflowTiles, st.levels) == (wstats.tiles, wstats.deadTiles, wstats.overflowTiles, wstats.levels)


@pytest.mark.gpu
def test_single_frames_are_culled_only_on_request(monkeypatch):
    """auto: launch sets of two or more frames; 1: single frames too; 0: never."""
    case = "bunny3_160x96"
    m, w, h, _, _ = bc.CASES[case]
    us = bc.uniforms(case, 2)
    for mode, single, pair in ((None, False, True), ("auto", False, True), ("1", True, True), ("0", False, False)):
        if mode is None:
            monkeypatch.delenv("RT_BEAM_CULL", raising=False)
        else:
            monkeypatch.setenv("RT_BEAM_CULL", mode)
        with _renderer(m, w, h) as r:
            r.beam_cull_stats(reset=True)
            r.render_frame(us[0])
            assert (r.beam_cull_stats(reset=True).tiles > 0) == single, mode
            if not single:                                                   # no flags of a set that was not culled
                with pytest.raises(rt.RtError):
                    r.beam_cull_flags(60)
            r.reset_accum()
            r.render_frames(us)
            assert (r.beam_cull_stats().tiles > 0) == pair, mode


# ---------------------------------------------------------------- 2. frames, cull on against off

SHAPES = {"160x96": ("bunny3", 160, 96, 0, 1), "64x48": ("bunny3", 64, 48, 0, 1), "48x48": ("bunny3", 48, 48, 0, 1), "12x40": ("bunny3", 12, 40, 0, 1),
          "rank1of2": ("bunny3", 160, 96, 1, 2)}


def _uniforms(mesh, w, h, frames):
    nodes, tris = bc.mesh(mesh)
    p = rt.default_render_params()
    p.sppPerFrame = 2
    cam = scenes.camera("closeup", aspect=w / h)
    return [rt.frame_uniforms(p, cam, w, h, f, True, nodes.shape[0], tris.shape[0]) for f in range(frames)]


def _render_set(monkeypatch, mesh, w, h, rank, world, us, env):
    with monkeypatch.context() as mp:
        for k, v in env:
            mp.setenv(k, v)
        with _renderer(mesh, w, h, rank, world) as r:
            r.render_frames(us)
            return [t.copy() for t in r.read_all()], r.traced_rays().to_dict()


def _render(monkeypatch, shape, K, env):
    mesh, w, h, rank, world = SHAPES[shape]
    return _render_set(monkeypatch, mesh, w, h, rank, world, _uniforms(mesh, w, h, K), env)


@functools.lru_cache(maxsize=None)
def _off(shape, K, budget):
    mp = pytest.MonkeyPatch()
    try:
        return _render(mp, shape, K, (("RT_BEAM_CULL", "0"),) + ((("RT_QUEUE_BUDGET_MB", "1"),) if budget else ()))
    finally:
        mp.undo()


def _culled_of(mesh, w, h, us):
    """Pixels of dead tiles, over the frames of us, whose ray passes the root box: what k_primary would have listed."""
    dead, _, rd = rt.beam_cull(us[0], *bc.mesh(mesh), jitters=bc.jitters(us), rays=True, packed=bc.packed(mesh))
    info = bc.packed(mesh)["info"]
    in_dead = dead[bc.tile_of_pixels(w, h)] != 0
    ro = np.array(list(us[0].camPos), f32)
    n = 0
    for k in range(len(us)):
        ok, tmin, _ = bc.slab(ro, rd[k][in_dead], f32(info.rootMin), f32(info.rootMax))
        n += int((ok & ~(tmin > f32(us[0].inf))).sum())
    return n, int(dead.sum())


def _culled_candidates(shape, K):
    mesh, w, h, _, _ = SHAPES[shape]
    return _culled_of(mesh, w, h, _uniforms(mesh, w, h, K))


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_cull_on_equals_cull_off(monkeypatch, shape, K):
    for interleave, budget in (("1", False), ("0", False), ("1", True)):
        want, a = _off(shape, K, budget)
        env = (("RT_BEAM_CULL", "1"), ("RT_BATCH_INTERLEAVE", interleave)) + ((("RT_QUEUE_BUDGET_MB", "1"),) if budget else ())
        got, b = _render(monkeypatch, shape, K, env)
        for g, x, n in zip(got, want, ("color", "motion", "gpos", "gnrm")):
            assert np.array_equal(g, x), f"{shape} K={K} interleave={interleave} budget={budget}: {n} differs in {int((g != x).sum())} values"
        assert b["primary"] == b["candidatePixels"] >= b["hitPixels"] == a["hitPixels"] > 0
        assert {k: v for k, v in a.items() if k not in MOVES} == {k: v for k, v in b.items() if k not in MOVES}
        if SHAPES[shape][4] == 1:
            culled, dead_tiles = _culled_candidates(shape, K)
            assert a["candidatePixels"] - b["candidatePixels"] == culled == a["primary"] - b["primary"], (shape, K, dead_tiles)
            if shape == "160x96":
                assert culled > 0


@functools.lru_cache(maxsize=None)
def _oracle8(orc):
    mesh, w, h, _, _ = SHAPES["64x48"]
    prev = None
    for u in _uniforms(mesh, w, h, 8):
        want, _ = orc.render(u, *bc.mesh(mesh), scenes.tiny_env(8), prev, nthreads=16)
        prev = want[0]
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("interleave", ["1", "0"])
def test_culled_batch_of_eight_equals_the_oracle(orc, monkeypatch, interleave):
    got, _ = _render(monkeypatch, "64x48", 8, (("RT_BEAM_CULL", "1"), ("RT_BATCH_INTERLEAVE", interleave)))
    qd._equal(got, _oracle8(orc), orc, f"culled batch of 8, interleave={interleave}")


# ---------------------------------------------------------------- 2b. frames of the comb and the sliver scenes (beam_cull_cases.py)

# comb64: dead tiles behind a level of 64 lanes; comb128s65: a tile kept at 65 survivors beside dead ones; the slivers: a tile kept by the `bad` ballot alone
FRAME_CASES = ("comb64_160x96", "comb128s65_160x96", "sliver2_zero_64x48", "sliver16_zero_64x48")


def _render_case(monkeypatch, case, env):
    m, w, h, _, _ = bc.CASES[case]
    return _render_set(monkeypatch, m, w, h, 0, 1, bc.uniforms(case), env)


@pytest.mark.gpu
@pytest.mark.parametrize("case", FRAME_CASES)
def test_cull_on_equals_cull_off_on_the_hard_scenes(monkeypatch, case):
    m, w, h, _, _ = bc.CASES[case]
    want, a = _render_case(monkeypatch, case, (("RT_BEAM_CULL", "0"),))
    culled, dead_tiles = _culled_of(m, w, h, bc.uniforms(case))
    assert dead_tiles > 0
    for interleave in ("1", "0"):
        got, b = _render_case(monkeypatch, case, (("RT_BEAM_CULL", "1"), ("RT_BATCH_INTERLEAVE", interleave)))
        for g, x, n in zip(got, want, ("color", "motion", "gpos", "gnrm")):
            assert np.array_equal(g, x), f"{case} interleave={interleave}: {n} differs in {int((g != x).sum())} values"
        assert b["primary"] == b["candidatePixels"] >= b["hitPixels"] == a["hitPixels"] > 0
        assert {k: v for k, v in a.items() if k not in MOVES} == {k: v for k, v in b.items() if k not in MOVES}
        assert a["candidatePixels"] - b["candidatePixels"] == culled == a["primary"] - b["primary"], (case, dead_tiles)
        if case.startswith("sliver"):                                        # the picture a missing `bad` rule would lose: the strip in column 32 of tile 2
            assert (got[2][0:16, 32] & 0x7fff).any() and not (got[2][:, 33:48] & 0x7fff).any()


@functools.lru_cache(maxsize=None)
def _oracle_of(orc, case):
    m = bc.CASES[case][0]
    prev = None
    for u in bc.uniforms(case):
        want, _ = orc.render(u, *bc.mesh(m), scenes.tiny_env(8), prev, nthreads=16)
        prev = want[0]
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["comb64_160x96", "sliver2_zero_64x48"])
def test_culled_hard_scenes_equal_the_oracle(orc, monkeypatch, case):
    got, _ = _render_case(monkeypatch, case, (("RT_BEAM_CULL", "1"),))
    qd._equal(got, _oracle_of(orc, case), orc, f"culled {case}")


# ---------------------------------------------------------------- 2c. standing down, and the flag buffer's regrow

@pytest.mark.gpu
@pytest.mark.parametrize("form", ["RT_FUSED", "RT_IMPLICIT"])
def test_the_cull_stands_down_for_the_other_record_forms(monkeypatch, form):
    """rt_wave_beam_flags: a primary launch that walks the fused or the implicit records is not culled, RT_BEAM_CULL=1 or not."""
    case = "bunny3_160x96"
    m, w, h, _, _ = bc.CASES[case]
    us = bc.uniforms(case, 4)
    monkeypatch.setenv(form, "1")
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("RT_BEAM_CULL", mode)
        with _renderer(m, w, h) as r:
            info = r.scene_info()                                           # the mesh takes the form: otherwise the cull is rightly on
            if form == "RT_FUSED":
                assert info.nFused > 0 and not info.flags & rt.RT_SCENE_NOT_FUSED
            else:
                assert info.flags & rt.RT_SCENE_IMPLICIT
            r.beam_cull_stats(reset=True)
            r.debug_builds(reset=True)
            r.render_frames(us)
            assert {"RT_FUSED": "FUSE", "RT_IMPLICIT": "IMPL"}[form] in r.debug_builds()["closest"]
            assert r.beam_cull_stats().tiles == 0
            with pytest.raises(rt.RtError):
                r.beam_cull_flags(60)
            out[mode] = [t.copy() for t in r.read_all()]
    for g, x, n in zip(out["1"], out["0"], ("color", "motion", "gpos", "gnrm")):
        assert np.array_equal(g, x), f"{form}: {n} differs"
    monkeypatch.delenv(form)                                                 # (the control: the same batch without the form is culled)
    monkeypatch.setenv("RT_BEAM_CULL", "1")
    with _renderer(m, w, h) as r:
        r.beam_cull_stats(reset=True)
        r.render_frames(us)
        assert r.beam_cull_stats().tiles == 60 and r.beam_cull_flags(60).any()


@pytest.mark.gpu
def test_the_flag_buffer_regrows_with_the_frame(monkeypatch):
    """One context through 64x48 -> 160x96 -> 64x48 -> 160x96: a lane's flag buffer grows behind the lane's stream when the frame has more tiles than any before
    (rt_wave_beam_flags), and is reused, part of it, when it has fewer.  Four launch sets at the first size give every lane a buffer of 12 flags, four at the last
    make every lane grow it to 60; no synchronisation between the sets of a size but what the regrow does itself."""
    mesh, K = "bunny3", 4
    nodes, tris = bc.mesh(mesh)
    p = rt.default_render_params()
    p.sppPerFrame = 2
    steps = ((64, 48, 4), (160, 96, 1), (64, 48, 1), (160, 96, 4))           # (W, H, launch sets)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("RT_BEAM_CULL", mode)
        with _renderer(mesh, 64, 48) as r:
            assert r.memory_info().lanes == 4
            res, prev_tiles = [], None
            for w, h, sets in steps:
                r.resize(w, h)
                cam = scenes.camera("closeup", aspect=w / h)
                cam.pos[0] += 0.5                                            # dead and live tiles at both sizes
                for _ in range(sets):
                    us = [rt.frame_uniforms(p, cam, w, h, r.frame_index + k, True, nodes.shape[0], tris.shape[0]) for k in range(K)]
                    r.render_frames(us)
                tiles = (w // 16) * (h // 16)
                if mode == "1":
                    flags = r.beam_cull_flags(tiles)                         # of the set rendered last
                    want, _ = rt.beam_cull(us[0], nodes, tris, jitters=bc.jitters(us), packed=bc.packed(mesh))
                    assert np.array_equal(flags, want), (w, h)
                    assert 0 < flags.sum() < flags.size
                    if prev_tiles is not None:
                        with pytest.raises(rt.RtError):
                            r.beam_cull_flags(prev_tiles)
                res.append([t.copy() for t in r.read_all()])
                prev_tiles = tiles
            out[mode] = res
    for (w, h, _), on, off in zip(steps, out["1"], out["0"]):
        for g, x, n in zip(on, off, ("color", "motion", "gpos", "gnrm")):
            assert np.array_equal(g, x), f"{w}x{h}: {n} differs"


# ---------------------------------------------------------------- 3. the dynamic mesh

def _device_tree(r):
    """The two-child records the device holds now, as rt.beam_cull takes them: the root box is the union of node 0's child boxes."""
    rec = r.debug_read_scene("nodes2w")
    n_inner = r.scene_info().nInner
    f = np.ascontiguousarray(rec).view(f32)[:n_inner * 16].reshape(-1, 16)
    lo, hi = np.minimum(f[0, 0:3], f[0, 8:11]), np.maximum(f[0, 4:7], f[0, 12:15])
    return {"nodes2w": np.ascontiguousarray(f).view(np.uint8).reshape(-1), "info": types.SimpleNamespace(nInner=n_inner, rootRefW=0, rootMin=lo, rootMax=hi)}


@pytest.mark.gpu
def test_flags_follow_a_rebuild_and_a_refit(monkeypatch):
    w, h, K = 160, 96, 4
    v, f = rt.meshgen.bunny_standin(3)
    model = rt.default_bvh_transform()
    cam = scenes.camera("closeup", aspect=w / h)
    p = rt.default_render_params()
    p.sppPerFrame = 2
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("RT_BEAM_CULL", mode)
        with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r:
            r.upload_env(scenes.tiny_env(8)); r.resize(w, h)
            r.mesh_upload(v, f)
            steps = []
            for step, pos in (("rebuild", v), ("refit", (v * f32(0.8) + np.array([0.0, 0.05, 0.0], f32)).astype(f32))):
                r.mesh_set_positions(pos)
                (r.mesh_rebuild if step == "rebuild" else r.mesh_refit)(model)
                us = [rt.frame_uniforms(p, cam, w, h, r.frame_index + k, True, r.n_nodes, r.n_tris) for k in range(K)]
                r.render_frames(us)                                          # right behind the update, no synchronisation in between
                targets = [t.copy() for t in r.read_all()]
                flags = None
                if mode == "1":
                    flags = r.beam_cull_flags(60)
                    want, _ = rt.beam_cull(us[0], None, None, jitters=bc.jitters(us), packed=_device_tree(r))
                    assert np.array_equal(flags, want), step
                    assert 0 < flags.sum() < flags.size
                steps.append((targets, flags))
            out[mode] = steps
    for (on, flags_on), (off, _), step in zip(out["1"], out["0"], ("rebuild", "refit")):
        for g, x, n in zip(on, off, ("color", "motion", "gpos", "gnrm")):
            assert np.array_equal(g, x), f"{step}: {n} differs"
    assert not np.array_equal(out["1"][0][1], out["1"][1][1])               # the smaller mesh leaves more tiles dead
