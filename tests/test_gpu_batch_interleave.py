"""The candidate order of a batch of frames (DESIGN.md 4.2 "Frame batching", RT_BATCH_INTERLEAVE).

A launch set of K frames holds K nearly identical copies of every pixel's work.  k_primary_interleaved appends the batch's candidates pixel-major -- the frames of a pixel
side by side -- so that every later list and queue puts them into adjacent lanes; RT_BATCH_INTERLEAVE=0 keeps the frame-major order of the slots.  The order
changes which lane traces which ray and nothing else: no ray, record, slot or result.

* the order itself, on the host (rt_debug_batch_tiles / rt_debug_batch_order: the arithmetic k_primary_interleaved runs) against an enumeration;
* on the GPU, rt_render_frames against K calls of rt_render_frame, all four targets bit for bit, for K = 1, 2, 3, 5, 8, 16, both orders; K = 8 also against the
  oracle; frames with an odd tile count, narrower than a tile, one rank of two; several chunks per set, chunks cut by slots, GI off; the ray counters of the
  two orders.
"""
import functools

import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scenes
import test_gpu_queue_diet as qd

VARS = qd.VARS + ("RT_BATCH_INTERLEAVE", "RT_LIGHT_MASKS", "RT_CHUNK", "RT_REVERSE")
KS = (1, 2, 3, 5, 8, 16)
APPEND = 8          # kAppendBatch: iterations of a workgroup of the primary stage
SPP2 = (("sppPerFrame", 2),)
NO_GI = SPP2 + (("enableGI", 0),)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)


# ---------------------------------------------------------------- 1. the order, without a GPU

def _brute_order(ballots):
    """Positions of a workgroup's items: wave by wave, lane by lane, a lane's items by iteration."""
    n, waves = ballots.shape
    out = np.full((n, waves, 64), 0xFFFFFFFF, np.uint32)
    pos = 0
    for w in range(waves):
        for lane in range(64):
            for k in range(n):
                if (int(ballots[k, w]) >> lane) & 1:
                    out[k, w, lane] = pos
                    pos += 1
    return out, pos


def test_order_equals_enumeration_for_random_ballots():
    rng = np.random.default_rng(27)
    cases = [np.zeros((APPEND, 4), np.uint64), np.full((APPEND, 4), 0xFFFFFFFFFFFFFFFF, np.uint64),
             np.full((APPEND, 4), 1 << 63, np.uint64), np.full((APPEND, 4), 1, np.uint64)]
    for density in (0.05, 0.45, 0.5, 0.95):
        for n, waves in ((APPEND, 4), (APPEND, 4), (1, 1), (3, 2), (32, 4)):
            bits = rng.random((n, waves, 64)) < density
            cases.append((bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64))
    for b in cases:
        want, total = _brute_order(b)
        got = rt.batch_order(b)
        assert np.array_equal(got, want)
        live = got[got != 0xFFFFFFFF]
        assert np.array_equal(np.sort(live), np.arange(total, dtype=np.uint32))      # a permutation of [0, total)


@pytest.mark.parametrize("K", KS)
def test_batch_order_is_pixel_major(K):
    """A made-up batch of K frames of nl tiles with random candidates, through the arithmetic of k_primary_interleaved: every candidate gets one position of [0, total);
    inside a wave the list runs pixel by pixel (lane, then spatial tile) with a pixel's frames ascending; where K divides the workgroup's iterations the
    candidate frames of a pixel stand on consecutive positions."""
    rng = np.random.default_rng(100 + K)
    for nl in (1, 3, 7, 8, 30):
        tiles = rt.batch_tiles(K, nl)
        v = np.arange(K * nl)
        assert np.array_equal(tiles, (v % K) * nl + v // K)                          # frames of a spatial tile follow each other ...
        assert np.array_equal(np.sort(tiles), v)                                     # ... and every local tile of the batch is handled once
        cand = rng.random((K * nl, 256)) < 0.45                                      # [local tile lt', thread]
        position = np.full((K * nl, 256), -1, np.int64)
        base = 0
        for g in range((K * nl + APPEND - 1) // APPEND):                             # workgroups, in the order their atomics happen to come
            vs = [g * APPEND + i for i in range(APPEND)]
            lts = [int(tiles[x]) if x < K * nl else -1 for x in vs]
            pred = np.stack([cand[lt] if lt >= 0 else np.zeros(256, bool) for lt in lts]).reshape(APPEND, 4, 64)
            ballots = (pred.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)
            order = rt.batch_order(ballots)
            for i, lt in enumerate(lts):
                if lt >= 0:
                    o = order[i].reshape(256)
                    assert np.array_equal(o != 0xFFFFFFFF, cand[lt])
                    position[lt][cand[lt]] = base + o[cand[lt]].astype(np.int64)
            # inside each wave of this workgroup: ascending positions <=> ascending (lane, spatial tile, frame)
            for w in range(4):
                items = sorted((int(order[i, w, lane]), lane, lts[i] % nl, lts[i] // nl) for i in range(APPEND) if lts[i] >= 0 for lane in range(64)
                               if order[i, w, lane] != 0xFFFFFFFF)
                keys = [it[1:] for it in items]
                assert keys == sorted(keys)
                assert [it[0] for it in items] == list(range(items[0][0], items[0][0] + len(items))) if items else True
            base += int(pred.sum())
        total = int(cand.sum())
        assert np.array_equal(np.sort(position[cand]), np.arange(total))             # a permutation of [0, total)
        if APPEND % K == 0:      # a pixel's candidate frames: consecutive positions, frames ascending
            p = position.reshape(K, nl, 256)
            c = cand.reshape(K, nl, 256)
            for lt in range(nl):
                for t in range(0, 256, 37):
                    ps = p[:, lt, t][c[:, lt, t]]
                    assert np.array_equal(ps, np.arange(ps[0], ps[0] + len(ps))) if len(ps) else True


# ---------------------------------------------------------------- 2. frames

def _mesh(scene):
    return qd._mesh(qd.SCENES[scene])


def _uniforms(scene, w, h, params, frames):
    nodes, tris = _mesh(scene)
    p = rt.default_render_params()
    for k, v in params:
        setattr(p, k, v)
    cam = scenes.camera("closeup", aspect=w / h)
    return [rt.frame_uniforms(p, cam, w, h, f, True, nodes.shape[0], tris.shape[0]) for f in range(frames)]


def _renderer(scene, w, h, rank, world):
    r = rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT, rank=rank, world_size=world)      # world 2: a tile-parallel context without a communicator
    nodes, tris = _mesh(scene)
    r.upload_bvh(nodes, tris); r.upload_env(scenes.tiny_env(8)); r.resize(w, h)
    r.traced_rays(reset=True)
    return r


@functools.lru_cache(maxsize=None)
def _frame_by_frame(scene, w, h, params, rank=0, world=1):
    """{K: the four targets after K calls of rt_render_frame} for every K of KS, rendered once (a single frame runs k_primary, the plain order)."""
    out = {}
    with _renderer(scene, w, h, rank, world) as r:
        for f, u in enumerate(_uniforms(scene, w, h, params, max(KS))):
            r.render_frame(u)
            if f + 1 in KS:
                out[f + 1] = [t.copy() for t in r.read_all()]
    return out


def _batched(monkeypatch, scene, w, h, params, K, interleave, env=(), rank=0, world=1):
    """One rt_render_frames of K frames against the K single frames; returns the ray counters."""
    want = _frame_by_frame(scene, w, h, params, rank, world)[K]      # (before the case's environment is set)
    for k, v in dict(env, RT_BATCH_INTERLEAVE=interleave).items():
        monkeypatch.setenv(k, v)
    with _renderer(scene, w, h, rank, world) as r:
        r.render_frames(_uniforms(scene, w, h, params, K))
        got = r.read_all()
        tr = r.traced_rays().to_dict()
    for g, x, n in zip(got, want, ("color", "motion", "gpos", "gnrm")):
        assert np.array_equal(g, x), f"{scene} {w}x{h} K={K} interleave={interleave} {dict(env)} rank {rank}/{world}: {n} differs in {int((g != x).sum())} values"
    assert tr["frames"] == K and tr["primary"] > 0
    return got, tr


@pytest.mark.gpu
@pytest.mark.parametrize("interleave", ["1", "0"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("scene,w,h", [("two_mesh", 160, 96), ("closeup", 64, 48)])
def test_batch_equals_frame_by_frame(monkeypatch, scene, w, h, K, interleave):
    _batched(monkeypatch, scene, w, h, SPP2, K, interleave)


@functools.lru_cache(maxsize=None)
def _oracle8(orc):
    nodes, tris = _mesh("two_mesh")
    prev = None
    for u in _uniforms("two_mesh", 64, 48, SPP2, 8):
        want, _ = orc.render(u, nodes, tris, scenes.tiny_env(8), prev, nthreads=16)
        prev = want[0]
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("interleave", ["1", "0"])
def test_batch_of_eight_equals_the_oracle(orc, monkeypatch, interleave):
    got, _ = _batched(monkeypatch, "two_mesh", 64, 48, SPP2, 8, interleave)
    qd._equal(got, _oracle8(orc), orc, f"batch of 8, interleave={interleave}")


# odd_tiles: 3 x 3 tiles.  narrow: one column of three tiles, 12 of a tile's 16 pixel columns.  rank 1 of 2: nLocalTiles differs from nTiles (30 of 60; 4 of 9)
SHAPES = {"odd_tiles": (48, 48, 0, 1), "narrow": (12, 40, 0, 1), "rank1of2": (160, 96, 1, 2), "rank1of2_odd": (48, 48, 1, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("interleave", ["1", "0"])
@pytest.mark.parametrize("K", [3, 8, 16])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_frame_shapes(monkeypatch, shape, K, interleave):
    w, h, rank, world = SHAPES[shape]
    _batched(monkeypatch, "two_mesh", w, h, SPP2, K, interleave, rank=rank, world=world)


CHUNKING = {"chunked": (SPP2, {"RT_QUEUE_BUDGET_MB": "1"}), "from_slots": (SPP2, {"RT_QUEUE_BUDGET_MB": "1", "RT_CHUNKS_FROM_SLOTS": "1"}),
            "no_gi": (NO_GI, {}), "no_gi_chunked": (NO_GI, {"RT_QUEUE_BUDGET_MB": "1"}), "plain": (SPP2, {})}


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 8])
@pytest.mark.parametrize("case", list(CHUNKING))
def test_chunking_and_counters(monkeypatch, case, K):
    """Both orders render the single frames' targets and trace the same rays with the same loads (gatherLoadsShadow apart: the any-hit walks stop at their
    first occluder, and where a walk meets it depends on its wave's schedule, test_gpu_ray_query.py)."""
    params, env = CHUNKING[case]
    _, a = _batched(monkeypatch, "two_mesh", 160, 96, params, K, "1", env)
    _, b = _batched(monkeypatch, "two_mesh", 160, 96, params, K, "0", env)
    print(f"{case} K={K}: interleaved {a}\n{case} K={K}: frame-major {b}")
    ga, gb = a.pop("gatherLoadsShadow"), b.pop("gatherLoadsShadow")
    assert ga > 0 and gb > 0
    assert a == b
