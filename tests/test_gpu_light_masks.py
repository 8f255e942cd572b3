"""Light-slot liveness masks of the wavefront frames' shadow queues.

The ray generators mark the light slots that hold a ray in bit masks beside the queues -- a dead slot is not written at all -- and the any-hit launch deals its
refills from those bits.  What can go wrong: a set bit that is never taken or taken twice, a clear bit that is taken (its tMax word and record are whatever the
arena held), bits that survive into another chunk, launch set or view, and the bit arithmetic where a run does not start on a word, ends inside one or crosses
a slot.  RT_LIGHT_MASKS=0 is the path before the masks; both must render the oracle's frames.

Every frame case is three chained frames of 160 x 96 (tests/test_gpu_queue_diet.py's harness: frame by frame on one renderer, as one batch of three on another)
against the oracle, bit for bit on all four targets, with queue 1 masked (RT_LIGHT_MASKS=1, the default), both queues masked (2) and none (0).
"""
import functools
import math

import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scenes
import test_gpu_queue_diet as qd

W, H = qd.W, qd.H
FRAMES = 3
VARS = qd.VARS + ("RT_LIGHT_MASKS", "RT_CHUNK", "RT_REVERSE")
LIGHT = np.array([0.0, 5.0, -3.0], np.float32)      # centre of the disk light (rt_lighting.glsl:29)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)


# ---------------------------------------------------------------- scenes and views

@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "away_quad":
        # a flat 8 x 8 grid of quads whose plane faces away from the disk light, seen from the far side: every hit is unlit (dot(N, light - hp) = -|light - centre|
        # all over the plane, far below the light's radius), no bounce ray and no AO ray can meet the plane again
        c = np.array([0.0, 1.0, 0.0], np.float32)
        n = (c - LIGHT) / np.linalg.norm(c - LIGHT)
        t = np.cross(n, [0.0, 1.0, 0.0]); t /= np.linalg.norm(t)
        b = np.cross(n, t)
        tris = []
        for i in range(8):
            for j in range(8):
                p = lambda a, e: c + t * (a / 4.0 - 1.0) + b * (e / 4.0 - 1.0)
                tris.append(np.concatenate([p(i, j), p(i + 1, j) - p(i, j), p(i + 1, j + 1) - p(i, j)]))      # rt_build_bvh's input: v0, e1, e2
                tris.append(np.concatenate([p(i, j), p(i + 1, j + 1) - p(i, j), p(i, j + 1) - p(i, j)]))
        return rt.build_bvh(np.asarray(tris, np.float32))
    return qd._mesh(qd.SCENES.get(name, name))


def _centre(tris):
    v0, e1, e2 = tris[:, 0:3], tris[:, 4:7], tris[:, 8:11]
    pts = np.concatenate([v0, v0 + e1, v0 + e2])
    return (pts.min(axis=0) + pts.max(axis=0)) / 2


def _look_at(eye, target):
    cam = scenes.camera("closeup", aspect=W / H)
    f = (target - eye) / np.linalg.norm(target - eye)
    cam.pos[0], cam.pos[1], cam.pos[2] = (float(x) for x in eye)
    cam.pitch = math.degrees(math.asin(float(f[1])))
    cam.yaw = math.degrees(math.atan2(float(f[2]), float(f[0])))
    return cam


def _camera(view, mesh):
    if view == "closeup":
        return qd._camera()
    c = _centre(_mesh(mesh)[1])
    to_light = (LIGHT - c) / np.linalg.norm(LIGHT - c)
    if view == "light_side":        # from the light towards the mesh: nearly every visible surface faces the light
        return _look_at(c + to_light * np.float32(2.2), c)
    assert view == "far_side"       # from behind the mesh towards the light
    return _look_at(c - to_light * np.float32(2.5), c)


# a case: (mesh, view, render parameters as (field, value) pairs, environment)
SPP2 = (("sppPerFrame", 2),)
DARK = SPP2 + (("sunEnabled", 0), ("pointLightEnabled", 0))
CASES = {
    "closeup": ("closeup", "closeup", SPP2, {}),                              # mostly unlit
    "light_side": ("closeup", "light_side", SPP2, {}),                        # nearly every disk slot live
    "two_mesh": ("two_mesh", "closeup", SPP2, {}),                            # bounce hits: queue 2 in use
    "spp_1": ("two_mesh", "closeup", (("sppPerFrame", 1),), {}),
    "spp_4": ("two_mesh", "closeup", (("sppPerFrame", 4),), {}),
    "no_ao": ("two_mesh", "closeup", SPP2 + (("enableAO", 0),), {}),           # no dense slots in front of the light slots
    "no_gi": ("two_mesh", "closeup", SPP2 + (("enableGI", 0),), {}),           # the single-queue source
    "lanes_1": ("two_mesh", "closeup", SPP2, {"RT_LANES": "1"}),
    "chunked": ("two_mesh", "closeup", SPP2, {"RT_QUEUE_BUDGET_MB": "1"}),     # several chunks, c0 != 0, a last chunk whose hit count is no multiple of 64
    "chunk_8": ("two_mesh", "closeup", SPP2, {"RT_CHUNK": "8"}),               # runs shorter than a word
    "chunk_8_chunked": ("two_mesh", "closeup", SPP2, {"RT_CHUNK": "8", "RT_QUEUE_BUDGET_MB": "1"}),   # ... that cross slot boundaries off a word boundary
    "reverse_0": ("two_mesh", "closeup", SPP2, {"RT_REVERSE": "0"}),
    "bin_gi": ("two_mesh", "closeup", SPP2, {"RT_BIN_GI": "1"}),
    "packet_ao": ("two_mesh", "closeup", SPP2, {"RT_PACKET_AO": "1"}),         # the any-hit launch starts behind the AO slots
    "dense_take_0": ("two_mesh", "closeup", SPP2, {"RT_DENSE_TAKE": "0"}),     # the dense slots are probed window by window, up to their end and not beyond
    "all_unlit": ("away_quad", "far_side", DARK, {}),                          # every mask word zero; the launch still answers the AO rays
}


def _uniforms(mesh, view, params):
    nodes, tris = _mesh(mesh)
    p = rt.default_render_params()
    for k, v in params:
        setattr(p, k, v)
    return [rt.frame_uniforms(p, _camera(view, mesh), W, H, f, True, nodes.shape[0], tris.shape[0]) for f in range(FRAMES)]


@functools.lru_cache(maxsize=None)
def _oracle(orc, mesh, view, params):
    if view == "closeup" and mesh in qd.SCENES:
        return qd._oracle(orc, mesh, params)          # computed once for the files that share the harness
    nodes, tris = _mesh(mesh)
    wants, prev = [], None
    for u in _uniforms(mesh, view, params):
        want, _ = orc.render(u, nodes, tris, scenes.tiny_env(8), prev, nthreads=16)
        wants.append(want)
        prev = want[0]
    return wants


def _hit(target):          # gpos.w = 1 (fp16) on a hit
    return target[2][:, :, 3] == 0x3C00


def _prepare(r, mesh):
    nodes, tris = _mesh(mesh)
    r.upload_bvh(nodes, tris); r.upload_env(scenes.tiny_env(8)); r.resize(W, H)
    r.light_masks(reset=True)         # switches the counting on
    r.traced_rays(reset=True)


def _run(orc, monkeypatch, case, masks):
    """The case frame by frame and as one batch, against the oracle.  Returns per renderer (light_masks, traced_rays)."""
    mesh, view, params, env = CASES[case]
    for k, v in dict(env, RT_LIGHT_MASKS=masks).items():
        monkeypatch.setenv(k, v)
    us, wants = _uniforms(mesh, view, params), _oracle(orc, mesh, view, params)
    what = f"{case} masks={masks}"
    out = []
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r, rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as rb:
        _prepare(r, mesh); _prepare(rb, mesh)
        for f, u in enumerate(us):
            r.render_frame(u)
            qd._equal(r.read_all(), wants[f], orc, f"{what} frame {f}")
        rb.render_frames(us)
        qd._equal(rb.read_all(), wants[-1], orc, f"{what} batch")
        for x in (r, rb):
            out.append((x.light_masks(), x.traced_rays()))
    return out


def _account(case, masks, out):
    """Set bits of both queues + live AO slots = the any-hit rays the launches started: every set bit taken exactly once, no clear bit taken."""
    params = dict(CASES[case][2])
    p = rt.default_render_params()
    ao = 0 if params.get("enableAO", p.enableAO) == 0 or params.get("aoRadius", p.aoRadius) <= 0 else params.get("aoSamples", p.aoSamples)
    for lm, tr in out:
        anyhit = tr.shadow + tr.bounceShadow + tr.ao      # (tr.ao: AO rays traced as packets, RT_PACKET_AO)
        print(f"{case} masks={masks}: hits {tr.hitPixels}, any-hit rays {anyhit}, AO {tr.hitPixels * ao}; bits {lm.bits1} + {lm.bits2}, words scanned {lm.wordsScanned}, "
              f"passes {lm.refillPasses}, mask words {lm.maskWords1} + {lm.maskWords2}")
        assert tr.frames == FRAMES and tr.hitPixels > 0
        if masks == "2":          # both queues masked: every any-hit ray is a set bit or a live AO slot
            assert lm.bits1 + lm.bits2 + tr.hitPixels * ao == anyhit, (case, lm.bits1, lm.bits2, tr.hitPixels * ao, anyhit)
            assert lm.maskWords1 > 0 and lm.maskWords2 > 0
            assert (lm.refillPasses > 0 and lm.wordsScanned >= lm.refillPasses) or lm.bits1 + lm.bits2 == 0
        elif masks == "1":        # queue 1 masked (the default): the rest of the any-hit rays are queue 2's, whose count the run with both queues masked gives
            assert lm.bits2 == 0 and lm.maskWords1 > 0 and lm.maskWords2 == 0
            assert lm.bits1 + tr.hitPixels * ao <= anyhit
            assert (lm.refillPasses > 0 and lm.wordsScanned >= lm.refillPasses) or lm.bits1 == 0
        else:
            assert (lm.bits1, lm.bits2, lm.wordsScanned, lm.refillPasses, lm.maskWords1, lm.maskWords2) == (0, 0, 0, 0, 0, 0)
    (a, ta), (b, tb) = out
    assert (a.bits1, a.bits2) == (b.bits1, b.bits2) and ta.shadow + ta.bounceShadow + ta.ao == tb.shadow + tb.bounceShadow + tb.ao      # frame by frame and batched: the same rays


# ---------------------------------------------------------------- 1. frames against the oracle, masks on and off; 3. accounting

_TRACED = {}


@pytest.mark.gpu
@pytest.mark.parametrize("masks", ["1", "2", "0"])
@pytest.mark.parametrize("case", list(CASES))
def test_frames_equal_the_oracle(orc, monkeypatch, case, masks):
    out = _run(orc, monkeypatch, case, masks)
    _account(case, masks, out)
    lm, tr = out[0]
    if masks != "0":
        if case == "all_unlit":
            assert lm.bits1 == 0 and lm.bits2 == 0 and tr.shadow > 0      # nothing but AO rays, and they were traced
        if case == "light_side":
            assert lm.bits1 > 4 * tr.hitPixels                             # of the ten light slots of a hit (four per sample, sun, point) more than four live
        if masks == "2" and case in ("two_mesh", "bin_gi", "chunked"):
            assert lm.bits2 > 1000                                         # queue 2 in use
    # the launches start the same rays whatever is masked, and the generators set the same bits for queue 1
    mine = _TRACED[(case, masks)] = (tr.shadow + tr.bounceShadow + tr.ao, lm.bits1)
    for other in ("0", "1", "2"):
        if other != masks and (case, other) in _TRACED:
            assert _TRACED[(case, other)][0] == mine[0], (case, other, _TRACED[(case, other)], mine)
            if "0" not in (other, masks):
                assert _TRACED[(case, other)][1] == mine[1], (case, other, _TRACED[(case, other)], mine)


# ---------------------------------------------------------------- 2. stale bits

@pytest.mark.gpu
def test_bits_of_another_view_do_not_survive(orc, monkeypatch):
    """One renderer with one launch set in flight (RT_LANES=1: each lane's mask words see both views): the bunny from the light's side -- most light slots live --,
    then the close-up view, where most are dead, frame by frame and as a batch.  The second view equals the same frames on a fresh renderer and the oracle."""
    monkeypatch.setenv("RT_LANES", "1")
    mesh = "closeup"
    first, second = _uniforms(mesh, "light_side", SPP2), _uniforms(mesh, "closeup", SPP2)
    wants = _oracle(orc, mesh, "closeup", SPP2)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as fresh:
        _prepare(fresh, mesh)
        fresh.render_frames(second)
        want_fresh, few = fresh.read_all(), fresh.light_masks().bits1
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r:
        _prepare(r, mesh)
        for u in first:
            r.render_frame(u)
        r.render_frames(first)
        many = r.light_masks(reset=True).bits1
        print(f"bits set: light side {many} (frames + batch), close-up {few} (batch)")
        assert many > 4 * few > 0                      # precondition: the first view leaves many more bits behind than the second sets
        r.reset_accum()
        for f, u in enumerate(second):
            r.render_frame(u)
            qd._equal(r.read_all(), wants[f], orc, f"close-up after the light side, frame {f}")
        r.reset_accum()
        r.render_frames(second)
        got = r.read_all()
        qd._equal(got, wants[-1], orc, "close-up batch after the light side")
        for g, w in zip(got, want_fresh):
            assert np.array_equal(g, w)
        assert r.light_masks().bits1 == few * 2        # the frames and the batch set the close-up's bits, no more
