"""The ray-queue diet of the wavefront frames.

* bounce hits shaded from the probe's hit list: behind a bounce probe k_gen_gi_listed visits the (hit, sample) pairs the probe listed instead of every pair.
  rt_debug_gi_list says which generator ran and how many pairs it visited; on the list path that is the number of rays the probe handed to the re-trace.
* dense slots (AO slots of shadow queue 1, the bounce queue): one float4 {dir, limit} per ray, one origin per hit and group.

Every frame case renders three frames of 160 x 96 at 2 spp (unless the case is about the spp) frame by frame and as one batch, against the oracle chained
from frame to frame, bit for bit on all four targets.
"""
import functools

import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scenes

W, H = 160, 96
VARS = ("RT_BOUNCE_PROBE", "RT_BIN_GI", "RT_QUEUE_BUDGET_MB", "RT_Q2_CAP", "RT_LANES", "RT_ARENAS", "RT_DENSE_TAKE", "RT_PACKET_AO", "RT_CHUNKS_FROM_SLOTS",
        "RT_QNODES", "RT_ANYHIT_TREE")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "two_mesh":   # two copies facing each other: bounce rays hit the other copy
        v, f = rt.meshgen.bunny_standin(4)
        a = rt.gather_triangles(v, f)
        b = a.copy()
        b[:, 0] += np.float32(0.7); b[:, 2] += np.float32(0.5)
        return rt.build_bvh(np.concatenate([a, b]).astype(np.float32))
    return scenes.bunny_bvh(3)


SCENES = {"closeup": "bunny", "two_mesh": "two_mesh"}
# render parameters away from the defaults, as (field, value) pairs so that a case can be a cache key
DEFAULT = (("sppPerFrame", 2),)


def _camera(moved=False):
    cam = scenes.camera("closeup", aspect=W / H)
    if moved:
        cam.yaw += 12.0
    return cam


def _uniforms(scene, params=DEFAULT, frames=3, moved=False):
    nodes, tris = _mesh(SCENES[scene])
    p = rt.default_render_params()
    for k, v in params:
        setattr(p, k, v)
    return [rt.frame_uniforms(p, _camera(moved), W, H, f, True, nodes.shape[0], tris.shape[0]) for f in range(frames)]


@functools.lru_cache(maxsize=None)
def _oracle(orc, scene, params=DEFAULT):
    nodes, tris = _mesh(SCENES[scene])
    wants, prev = [], None
    for u in _uniforms(scene, params):
        want, _ = orc.render(u, nodes, tris, scenes.tiny_env(8), prev, nthreads=16)
        wants.append(want)
        prev = want[0]
    return wants


def _equal(got, want, orc, what):
    for g, w, n in zip(got, want, ("color", "motion", "gpos", "gnrm")):
        st = orc.compare(g, w)
        assert st["bit_diff"] == 0, f"{what}/{n}: not bit-identical: {st}"


def _prepare(r, scene):
    nodes, tris = _mesh(SCENES[scene])
    r.upload_bvh(nodes, tris); r.upload_env(scenes.tiny_env(8)); r.resize(W, H)
    r.gi_list(reset=True)             # switches the counting on
    r.bounce_probe(reset=True)
    r.traced_rays(reset=True)


def _run(orc, monkeypatch, scene, env, params=DEFAULT, stale=False):
    """Frame by frame and batched against the oracle.  Returns per renderer (gi_list, bounce_probe, hit pixels)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    us, wants = _uniforms(scene, params), _oracle(orc, scene, params)
    what = f"{scene} {dict(params)} {env}"
    out = []
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r, rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as rb:
        for x in (r, rb):
            if stale:
                # the per-lane arrays hold the giPos of other launch sets: another mesh, then this mesh from elsewhere 
                _prepare(x, "closeup")
                x.render_frames(_uniforms("closeup", params))
                _prepare(x, scene)
                x.render_frames(_uniforms(scene, params, moved=True))
                x.reset_accum()       # the library counts the frames itself: back to frame 0, arenas and their contents stay
                x.gi_list(reset=True); x.bounce_probe(reset=True); x.traced_rays(reset=True)
            else:
                _prepare(x, scene)
        for f, u in enumerate(us):
            r.render_frame(u)
            _equal(r.read_all(), wants[f], orc, f"{what} frame {f}")
        rb.render_frames(us)
        _equal(rb.read_all(), wants[-1], orc, f"{what} batch")
        for x in (r, rb):
            out.append((x.gi_list(), x.bounce_probe(), x.traced_rays().hitPixels))
    spp = dict(params).get("sppPerFrame", 1)
    for gl, bp, hits in out:
        print(f"{what}: hits {hits} x spp {spp}; generator visited {gl.visited} shaded {gl.shaded} launches listed {gl.listedLaunches} per pair {gl.pairLaunches}; "
              f"probe walked {bp.probed} re-traced {bp.retraced}")
    (gl, _, hits), (glb, _, hitsb) = out
    assert hits == hitsb and gl.shaded == glb.shaded, what      # the same pairs bounced frame by frame and batched
    return out, spp


def _assert_listed(out, spp, what=""):
    for gl, bp, hits in out:
        assert gl.listedLaunches > 0 and gl.pairLaunches == 0, (what, gl.listedLaunches, gl.pairLaunches)
        assert bp.probeLaunches == gl.listedLaunches and bp.closestLaunches == 0, what
        assert gl.visited == bp.retraced, (what, gl.visited, bp.retraced)     # exactly the rays the probe handed on
        assert gl.shaded <= gl.visited, what
        assert 4 * gl.visited < hits * spp, (what, gl.visited, hits * spp)    # far below every (hit, sample) pair


def _assert_per_pair(out, spp, what=""):
    for gl, bp, hits in out:
        assert gl.pairLaunches > 0 and gl.listedLaunches == 0, (what, gl.listedLaunches, gl.pairLaunches)
        assert gl.visited == hits * spp, (what, gl.visited, hits * spp)
        assert gl.shaded <= gl.visited, what


# ---------------------------------------------------------------- which generator ran

@pytest.mark.gpu
@pytest.mark.parametrize("probe", ["1", "0"])
@pytest.mark.parametrize("scene", list(SCENES))
def test_list_path_and_pair_path_equal_the_oracle(orc, monkeypatch, scene, probe):
    out, spp = _run(orc, monkeypatch, scene, {"RT_BOUNCE_PROBE": probe})
    if probe == "1":
        _assert_listed(out, spp, scene)
    else:
        _assert_per_pair(out, spp, scene)
        assert all(bp.probeLaunches == 0 for _, bp, _ in out)
    shaded = out[0][0].shaded
    if scene == "closeup":
        assert shaded * 1000 < out[0][2] * spp, shaded      # the (almost) empty list
    else:
        assert shaded > 1000, shaded                         # thousands of bounce hits


@pytest.mark.gpu
def test_both_paths_shade_the_same_pairs(orc, monkeypatch):
    a, _ = _run(orc, monkeypatch, "two_mesh", {"RT_BOUNCE_PROBE": "1"})
    b, _ = _run(orc, monkeypatch, "two_mesh", {"RT_BOUNCE_PROBE": "0"})
    assert a[0][0].shaded == b[0][0].shaded > 0


@pytest.mark.gpu
def test_overflow_on_the_list_path_with_stale_positions(orc, monkeypatch):
    """RT_Q2_CAP=64: shadow queue 2 holds 64 entries, k_gen_gi_overflow shades the rest from the list.  The renderers rendered other launch sets before,
    so giPos of the pairs outside the list holds their values."""
    out, spp = _run(orc, monkeypatch, "two_mesh", {"RT_BOUNCE_PROBE": "1", "RT_Q2_CAP": "64"}, stale=True)
    _assert_listed(out, spp, "overflow")
    assert out[0][0].shaded > 64 * 3


@pytest.mark.gpu
def test_overflow_on_the_pair_path(orc, monkeypatch):
    out, spp = _run(orc, monkeypatch, "two_mesh", {"RT_BOUNCE_PROBE": "0", "RT_Q2_CAP": "64"}, stale=True)
    _assert_per_pair(out, spp, "overflow")


# ---------------------------------------------------------------- queue options, list path forced on

OPTIONS = {
    "chunked": {"RT_QUEUE_BUDGET_MB": "1"},
    "chunked_overflow": {"RT_QUEUE_BUDGET_MB": "1", "RT_Q2_CAP": "64"},
    "lanes_1": {"RT_LANES": "1"},
    "lanes_4": {"RT_LANES": "4"},
    "dense_take_0": {"RT_DENSE_TAKE": "0"},
    "packet_ao": {"RT_PACKET_AO": "1"},
    "bin_gi": {"RT_BIN_GI": "1"},
    "qnodes_2": {"RT_QNODES": "2"},
}


@pytest.mark.gpu
@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("scene", list(SCENES))
def test_queue_options_on_the_list_path(orc, monkeypatch, scene, option):
    env = dict(OPTIONS[option], RT_BOUNCE_PROBE="1")
    out, spp = _run(orc, monkeypatch, scene, env)
    if option == "bin_gi":          # the permuted bounce queue falls back to the per-pair generator, behind the probe all the same
        _assert_per_pair(out, spp, option)
        assert all(bp.probeLaunches > 0 for _, bp, _ in out)
    else:
        _assert_listed(out, spp, option)
    if option.startswith("chunked"):
        assert out[1][0].listedLaunches > 1, "one chunk for the batch: the budget did not split it"


# ---------------------------------------------------------------- parameter corners of the dense slots

CORNERS = {
    "ao_radius_0": (("sppPerFrame", 2), ("aoRadius", 0.0)),
    "no_ao": (("sppPerFrame", 2), ("enableAO", 0)),
    "no_gi": (("sppPerFrame", 2), ("enableGI", 0)),
    "ao_samples_1": (("sppPerFrame", 2), ("aoSamples", 1)),
    "ao_samples_3": (("sppPerFrame", 2), ("aoSamples", 3)),
    "ao_samples_6": (("sppPerFrame", 2), ("aoSamples", 6)),
    "spp_1": (("sppPerFrame", 1),),
    "spp_3": (("sppPerFrame", 3),),
}


@pytest.mark.gpu
@pytest.mark.parametrize("corner", list(CORNERS))
def test_parameter_corners(orc, monkeypatch, corner):
    params = CORNERS[corner]
    out, spp = _run(orc, monkeypatch, "two_mesh", {"RT_BOUNCE_PROBE": "1"}, params)
    if corner == "no_gi":
        assert all(gl.listedLaunches == 0 and gl.pairLaunches == 0 and gl.visited == 0 for gl, _, _ in out)
    else:
        _assert_listed(out, spp, corner)
    if corner.startswith("spp_"):
        hits = out[1][2]
        print(f"{corner}: hits x spp = {hits * spp}")


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"RT_PACKET_AO": "1"}, {"RT_DENSE_TAKE": "0"}], ids=["packet_ao", "dense_take_0"])
def test_ao_sample_counts_under_the_other_ao_readers(orc, monkeypatch, env):
    """AO sample counts that are no multiple of the packet's four rays, through k_trace_packets and through the probing refill."""
    for corner in ("ao_samples_3", "ao_samples_6"):
        _run(orc, monkeypatch, "two_mesh", dict(env, RT_BOUNCE_PROBE="1"), CORNERS[corner])


# ---------------------------------------------------------------- sample 0 declines, another sample casts

def _hash2(vx, vy):
    vx = vx * np.uint32(1664525) + np.uint32(1013904223)
    vy = vy * np.uint32(1664525) + np.uint32(1013904223)
    vx = vx ^ (vy >> np.uint32(16))
    vy = vy ^ (vx << np.uint32(5))
    vx = vx * np.uint32(1664525) + np.uint32(1013904223)
    vy = vy * np.uint32(1664525) + np.uint32(1013904223)
    return vx ^ vy


def _rand(px, py, frame):
    """rand() of rt_common.glsl on float32 arrays: hash of the truncated coordinates and the frame, over 2^32."""
    f2u = lambda p: np.clip(p, np.float32(0.0), np.float32(4294967040.0)).astype(np.uint32)
    fr = np.uint32(frame & 0xffffffff)
    with np.errstate(over="ignore"):
        bits = _hash2(f2u(px) ^ fr, f2u(py) ^ (fr * np.uint32(1663)))
    return (bits.astype(np.float32) / np.float32(4294967296.0)).astype(np.float32)


def bounce_casts(hit_mask, frame, spp):
    """[spp, H, W] bool: does sample s of the pixel cast a bounce ray (oneBounceGIBVH: cosTheta > 0.1)?  cosTheta = dot(N, wi) of the cosine-weighted
    direction wi = normalize(x T + z B + y N) is y = sqrt(1 - u2) up to rounding, whatever N is.  Second value: pairs within 1e-4 of the threshold."""
    py, px = np.mgrid[0:H, 0:W]
    fcx, fcy = (px + 0.5).astype(np.float32), (py + 0.5).astype(np.float32)
    cast = np.zeros((spp, H, W), bool)
    near = 0
    for s in range(spp):
        seed = np.uint32((frame * spp + s) & 0xffffffff)
        with np.errstate(over="ignore"):
            o41 = np.float32(np.int32(seed * np.uint32(41)))
        u2 = _rand(fcy + o41, fcx + o41, frame)
        y = np.sqrt(np.maximum(np.float32(0.0), np.float32(1.0) - u2))
        cast[s] = (y > np.float32(0.1)) & hit_mask
        near += int((np.abs(y - np.float32(0.1)) < 1e-4)[hit_mask].sum())
    return cast, near


@pytest.mark.gpu
def test_hits_whose_sample_0_declines_while_another_casts(orc, monkeypatch):
    """What the once-per-hit bounce origin must survive: sample 0 of a hit has cosTheta <= 0.1 and casts no ray, another sample of the hit casts one.  The
    pairs are found on the CPU from the frame's random numbers; that the CPU's casting pairs are the GPU's is checked against the rays the probe walked."""
    monkeypatch.setenv("RT_BOUNCE_PROBE", "1")
    us, wants = _uniforms("closeup"), _oracle(orc, "closeup")
    silent0 = 0
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r:
        _prepare(r, "closeup")
        for f, u in enumerate(us):
            r.render_frame(u)
            got = r.read_all()
            _equal(got, wants[f], orc, f"closeup frame {f}")
            hit = got[2][:, :, 3] == 0x3C00          # gpos.w = 1 on a hit
            cast, near = bounce_casts(hit, f, 2)
            walked = r.bounce_probe(reset=True).probed
            n = int((~cast[0] & cast[1:].any(axis=0) & hit).sum())
            print(f"frame {f}: hits {int(hit.sum())}, casting pairs CPU {int(cast.sum())} GPU {walked} (within 1e-4 of the threshold: {near}), "
                  f"hits with sample 0 silent and another casting: {n}")
            assert hit.sum() == r.traced_rays(reset=True).hitPixels
            assert abs(int(cast.sum()) - walked) <= near, (int(cast.sum()), walked, near)
            silent0 += n
    assert silent0 > 0
