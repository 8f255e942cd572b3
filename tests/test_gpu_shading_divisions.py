"""The shading stages without their divisions, on the device: the texel decode, the halton pair from the frame descriptor, the slot -> pixel
arithmetic from reciprocals and the (sample, hit) mapping of the generators change no bit of any frame.

* the production helpers through rt_debug_eval: the texel decode for all 256 codes against numpy's float32 division; halton evaluated in place on the
  device against the table the host writes into the frame descriptor, for uFrameIndex 0 .. 4096 and both bases;
* whole frames against the oracle, all four targets, at the smallest shapes where the slot arithmetic can go wrong -- 160x96 (tilesX 10, 60 tiles) and
  200x120 (tilesX 13, partial tiles on both edges), frame by frame and as a batch of three (frames 0 .. 2), on one rank and on rank 1 of 3 (the row shift
  is live), with 4 spp and 1 spp, and once with a ray-queue budget of 1 MB so that the number of live hits differs from chunk to chunk.  The close-up
  view has lit and unlit waves, bounce hits and primary misses;
* rt_debug_disk_skip's ten sums on the close-up case equal what the commit before the change counted (tests/golden/shading_divisions_parent.json): the
  (sample, hit) mapping of the generators and with it the wave-granular skip are what they were."""
import functools
import json
from pathlib import Path

import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scenes
from opengl_raytracing_amd import tiles

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "shading_divisions_parent.json"
FRAMES = 3
VARS = ("RT_BOUNCE_PROBE", "RT_BIN_GI", "RT_QUEUE_BUDGET_MB", "RT_Q2_CAP", "RT_LANES", "RT_ARENAS", "RT_DENSE_TAKE", "RT_PACKET_AO", "RT_CHUNKS_FROM_SLOTS")
DISK_FIELDS = ("directPairs", "directUnlit", "directSkipped", "directWaves", "directWavesSkipped", "giPairs", "giUnlit", "giSkipped", "giWaves", "giWavesSkipped")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)


def test_device_texel_decode_equals_the_division():
    codes = np.arange(256, dtype=np.float32)
    with rt.Renderer() as r:
        got = r.debug_eval(10, codes)
    want = codes / np.float32(255)
    assert np.array_equal(got, want.view(np.uint32)), np.flatnonzero(got != want.view(np.uint32))
    assert np.array_equal(got, rt.texel_unorm8().view(np.uint32))       # and the host's build of the helper


def test_halton_table_equals_the_device_loop():
    idx = np.arange(1, 4098, dtype=np.float32)                          # halton(uFrameIndex + 1, base), uFrameIndex 0 .. 4096
    table = rt.halton_pairs(0, 4097).view(np.uint32)
    with rt.Renderer() as r:
        for col, base in enumerate((2, 3)):
            got = r.debug_eval(11, idx, np.full_like(idx, base))
            assert np.array_equal(got, table[:, col]), (base, np.flatnonzero(got != table[:, col])[:8])


def test_generator_thread_mapping_equals_the_division():
    """sample_and_hit (rt_frame.hpp): thread index -> (tid // live, tid % live) for every tid < live * spp, from a reciprocal estimate and a correction.
    Every thread for the small chunks; for the large ones every boundary k live - 1, k live, k live + 1 (where an estimate that is off by one shows) and a
    random sample.  live * spp stays below 2^31, as rt_wave_render guarantees; spp 4097 takes the dividing path."""
    rng = np.random.default_rng(5)
    tid, live, spp = [], [], []
    for lv in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 8191, 65_537, 1_000_003, 3_700_000, 16_777_217, 33_554_431, 400_000_000):
        for sp in (1, 2, 4, 5, 16, 64, 4096, 4097):
            n = lv * sp
            if n >= 2**31:
                continue
            if n <= 300_000:
                t = np.arange(n, dtype=np.int64)
            else:
                k = np.arange(0, sp + 1, dtype=np.int64) * lv
                t = np.concatenate([k - 1, k, k + 1, rng.integers(0, n, 2000)])
                t = np.unique(t[(t >= 0) & (t < n)])
            tid.append(t); live.append(np.full(t.size, lv, np.int64)); spp.append(np.full(t.size, sp, np.int64))
    tid, live, spp = (np.concatenate(x).astype(np.uint32) for x in (tid, live, spp))
    assert tid.size > 1_000_000
    with rt.Renderer() as r:
        s = r.debug_eval(12, tid.view(np.float32), live.view(np.float32), spp.view(np.float32))
        j = r.debug_eval(13, tid.view(np.float32), live.view(np.float32), spp.view(np.float32))
    bad = np.flatnonzero((s != tid // live) | (j != tid % live))
    assert bad.size == 0, (tid[bad[:8]], live[bad[:8]], spp[bad[:8]], s[bad[:8]], j[bad[:8]])


# ---------------------------------------------------------------- frames

@functools.lru_cache(maxsize=None)
def _scene():
    return scenes.bunny_bvh(3) + (scenes.tiny_env(8),)


def _uniforms(w, h, spp):
    nodes, tris, _ = _scene()
    p = rt.default_render_params()
    p.sppPerFrame = spp
    cam = scenes.camera("closeup", aspect=w / h)
    return [rt.frame_uniforms(p, cam, w, h, f, True, nodes.shape[0], tris.shape[0]) for f in range(FRAMES)]


@functools.lru_cache(maxsize=None)
def _oracle(orc, w, h, spp):
    """The oracle's frames 0 .. 2, rendered once per (shape, spp) and shared by the cases; never modified."""
    nodes, tris, faces = _scene()
    wants, prev = [], None
    for u in _uniforms(w, h, spp):
        want, _ = orc.render(u, nodes, tris, faces, prev, nthreads=16)
        wants.append(want)
        prev = want[0]
    return wants


def _equal(r, want, mine, what):
    for g, w, name in zip(r.read_all(), want, ("color", "motion", "gpos", "gnrm")):
        assert g.shape == w.shape, (what, name)
        assert np.array_equal(g[mine], w[mine]), f"{what}/{name}: {np.count_nonzero(np.any(g[mine] != w[mine], axis=-1))} of this rank's pixels differ"
        assert not g[~mine].any(), f"{what}/{name}: a pixel of another rank was written"


def _render(orc, w, h, spp, world, rank, what):
    nodes, tris, faces = _scene()
    us, wants = _uniforms(w, h, spp), _oracle(orc, w, h, spp)
    mine = tiles.owner_mask(w, h, rank, world).astype(bool)
    assert mine.any() and (world == 1 or not mine.all())
    hits = []
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT, rank=rank, world_size=world) as one, \
         rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT, rank=rank, world_size=world) as many:
        for r in (one, many):
            r.upload_bvh(nodes, tris); r.upload_env(faces); r.resize(w, h)
        for f, u in enumerate(us):                                       # batch 1: frames 0 .. 2 one by one
            one.render_frame(u)
            _equal(one, wants[f], mine, f"{what} frame {f}")
        many.render_frames(us)                                           # batch 3: the targets hold the last frame
        _equal(many, wants[-1], mine, f"{what} batch of {FRAMES}")
        hits = [one.traced_rays().hitPixels, many.traced_rays().hitPixels]
    assert hits[0] == hits[1] > 0
    # the view has what the issue asks for: pixels that hit and pixels that miss on this rank
    assert 0 < hits[0] < FRAMES * int(mine.sum()), (hits, int(mine.sum()))
    return hits[0]


@pytest.mark.parametrize("spp", [4, 1])
@pytest.mark.parametrize("world,rank", [(1, 0), (3, 1)])
@pytest.mark.parametrize("w,h", [(160, 96), (200, 120)])
def test_frames_equal_the_oracle(orc, w, h, world, rank, spp):
    g = tiles.geometry(w, h, world)
    assert (g["tilesX"], g["nTiles"]) == {(160, 96): (10, 60), (200, 120): (13, 104)}[(w, h)]
    _render(orc, w, h, spp, world, rank, f"{w}x{h} rank {rank}/{world} {spp} spp")


def test_frames_equal_the_oracle_when_chunks_differ_in_size(orc, monkeypatch):
    """A ray-queue budget of 1 MB cuts a frame's hits into chunks; the last is shorter, so the divisor of the (sample, hit) mapping changes between launches."""
    monkeypatch.setenv("RT_QUEUE_BUDGET_MB", "1")
    w, h, spp = 160, 96, 4
    hits = _render(orc, w, h, spp, 1, 0, "160x96 budget 1 MB")
    per_frame = hits // FRAMES
    plan = rt.wave_plan(w * h, spp, rt.default_render_params().aoSamples, hits=per_frame)
    print(f"{per_frame} hits per frame, chunks of {plan.chBudget}: {plan.nChunks} per frame, the last of {per_frame - (plan.nChunks - 1) * plan.ch}")
    assert plan.options["budgetBytes"] == 1 << 20 and plan.nChunks >= 2 and per_frame % plan.ch != 0


ORDER_FREE = ("directPairs", "directUnlit", "directWaves", "giPairs", "giUnlit")


@pytest.mark.parametrize("batch", [1, 3])
def test_disk_skip_sums_are_the_parents(batch):
    """rt_debug_disk_skip on the close-up case against the record taken on the commit before (tests/golden/shading_divisions_parent.json).

    Five of the ten sums are properties of the (hit, sample) pairs and of the grid -- pairs, unlit pairs and waves of k_gen_direct, pairs and unlit pairs of
    the bounce-hit generator -- and must equal the parent's exactly.  The other five -- pairs and waves that SKIPPED the disk loop in either generator, and the
    bounce-hit generator's waves -- count whole waves, and which hits share a wave follows the order of the hit list, which k_primary and k_post_primary
    build with one atomicAdd per workgroup: it differs from run to run of the same library.  The parent commit's own record shows it: frame by frame and as a batch of
    three it counted the same pairs and unlit pairs (86 756 / 73 660) and 62 884 against 62 656 skipped pairs, 47 against 46 bounce-generator waves; this tree,
    in the run that found this out, 62 952 skipped pairs in 985 instead of 984 waves with every order-free sum equal (profiles/r18_shading_divisions.txt 3).
    For those five the test asserts what holds for every order: a skipped wave holds 1 .. 64 pairs, all of them unlit; a wave that did not skip
    holds at least one lit pair, so at most 63 of the unlit pairs that were not skipped sit in each such wave.  That the mapping of threads to (sample, hit)
    itself is the parent's is test_generator_thread_mapping_equals_the_division's exact statement."""
    gold = json.loads(GOLDEN.read_text())
    w, h = gold["case"]["size"]
    assert (w, h, gold["case"]["spp"], gold["case"]["frames"]) == (160, 96, 4, FRAMES)
    nodes, tris, faces = _scene()
    us = _uniforms(w, h, 4)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r:
        r.upload_bvh(nodes, tris); r.upload_env(faces); r.resize(w, h)
        r.disk_skip(reset=True)                                          # switches the counting on
        if batch == 1:
            for u in us:
                r.render_frame(u)
        else:
            r.render_frames(us)
        d = r.disk_skip()
    got = {k: int(getattr(d, k)) for k in DISK_FIELDS}
    want = gold["sums"][f"batch{batch}"]
    print(got, want)
    assert {k: got[k] for k in ORDER_FREE} == {k: want[k] for k in ORDER_FREE}
    for g in ("direct", "gi"):
        pairs, unlit, skipped, waves, wskip = (got[g + k] for k in ("Pairs", "Unlit", "Skipped", "Waves", "WavesSkipped"))
        assert wskip <= skipped <= 64 * wskip and skipped <= unlit <= pairs and wskip <= waves
        assert unlit - skipped <= 63 * (waves - wskip)
        assert (pairs + 63) // 64 <= waves <= pairs
    assert 0 < got["directSkipped"] < got["directPairs"] and got["giPairs"] > 0   # lit and unlit waves, bounce hits
