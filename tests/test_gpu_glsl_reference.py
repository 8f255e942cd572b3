"""The HIP path (through the C ABI) against the REFERENCE's own GLSL outputs (tests/golden/glsl_*.npz, produced by
tests/golden/make_glsl_golden.py: the reference shaders executed by SwiftShader).  Same inputs, same history (handed over
with rt_write_target), same tolerances as the oracle's check in tests/test_glsl_reference.py -- the product is compared
with the reference directly, not only through the oracle."""
from pathlib import Path

import numpy as np
import pytest

import opengl_raytracing_amd as rt
from test_glsl_reference import (FRAME_FIXTURES, WINDOW_FIXTURES, check_present_window, check_targets, check_taa_regimes, check_trace_kat,
                                 check_window, embed_outer, load_window_fixture, present_window_inputs, window_history)

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def ren():
    r = rt.Renderer()
    yield r
    r.close()


@pytest.mark.parametrize("name", FRAME_FIXTURES)
def test_hip_matches_reference_glsl_frames(ren, name):
    d = np.load(GOLDEN / f"{name}.npz")
    u0 = rt.RtUniforms.from_buffer_copy(d["uniforms"][0].tobytes())
    ren.resize(int(u0.resolution[0]), int(u0.resolution[1]))
    ren.upload_env(d["env"] if "env" in d else None)
    if "nodes12" in d:
        ren.upload_bvh(d["nodes12"], d["tris12"])
    ren.reset_accum()
    for f in range(d["uniforms"].shape[0]):
        u = rt.RtUniforms.from_buffer_copy(d["uniforms"][f].tobytes())
        if f > 0:
            ren.write_target(rt.RT_TARGET_COLOR, d[f"color{f - 1}"])      # the shader's own history, as in the fixture
        ren.render_frame(u)
        check_targets(name, f, ren.read_all(), d)


@pytest.mark.parametrize("name", [n for n in FRAME_FIXTURES if "_bvh_" in n])
def test_hip_megakernel_matches_reference_glsl_bvh_frames(name):
    """The default renderer takes the wavefront pipeline for BVH frames (test above); the same fixtures through the megakernel."""
    d = np.load(GOLDEN / f"{name}.npz")
    u0 = rt.RtUniforms.from_buffer_copy(d["uniforms"][0].tobytes())
    with rt.Renderer(pipeline=rt.RT_PIPELINE_MEGAKERNEL) as r:
        r.resize(int(u0.resolution[0]), int(u0.resolution[1]))
        r.upload_env(d["env"] if "env" in d else None)
        r.upload_bvh(d["nodes12"], d["tris12"])
        for f in range(d["uniforms"].shape[0]):
            if f > 0:
                r.write_target(rt.RT_TARGET_COLOR, d[f"color{f - 1}"])
            r.render_frame(rt.RtUniforms.from_buffer_copy(d["uniforms"][f].tobytes()))
            check_targets(name, f, r.read_all(), d)


@pytest.mark.parametrize("pipeline", [rt.RT_PIPELINE_WAVEFRONT, rt.RT_PIPELINE_MEGAKERNEL])
def test_hip_matches_reference_glsl_taa_weight_regimes(pipeline):
    """Frames 0, 1, 7, 8, 9, 31, 32, 33 of a 34-frame accumulation as the reference GLSL rendered them; the library takes uFrameIndex
    from its own frame counter, so the frames in between are rendered too (their output is irrelevant: every checked frame gets
    the reference's own history through rt_write_target)."""
    d = np.load(GOLDEN / "glsl_bvh_taa_regimes_48x36.npz")
    u0 = rt.RtUniforms.from_buffer_copy(d["uniforms0"].tobytes())
    with rt.Renderer(pipeline=pipeline) as r:
        r.resize(int(u0.resolution[0]), int(u0.resolution[1]))
        r.upload_env(d["env"])
        r.upload_bvh(d["nodes12"], d["tris12"])

        def render(u, prev):
            while r.frame_index < u.frameIndex:           # advance the frame counter to the fixture's frame
                r.render_frame(u)
            assert r.frame_index == u.frameIndex
            if prev is not None:
                r.write_target(rt.RT_TARGET_COLOR, prev)
            r.render_frame(u)
            return r.read_all()

        check_taa_regimes(d, render)


# the 1 M-triangle scene on the wavefront pipeline with defaults
WINDOW_CASES = [(n, p) for n in WINDOW_FIXTURES if "_bench_" in n for p in (rt.RT_PIPELINE_WAVEFRONT, rt.RT_PIPELINE_MEGAKERNEL)] + \
               [(n, rt.RT_PIPELINE_WAVEFRONT) for n in WINDOW_FIXTURES if "_million_" in n]


@pytest.mark.parametrize("name,pipeline", WINDOW_CASES)
def test_hip_matches_reference_glsl_baseline_windows(name, pipeline):
    """Whole frames at the BASELINE configurations' own size, spp and depth against the reference GLSL's window (section K of
    make_glsl_golden.py).  uFrameIndex comes from the library's counter: frames before a fixture's first frame are rendered (their output
    is irrelevant), then each checked frame gets the fixture's history over window + margin, zeros elsewhere, through rt_write_target."""
    d, nodes, tris, faces = load_window_fixture(name)
    u0 = rt.RtUniforms.from_buffer_copy(d["uniforms"][0].tobytes())
    W, H = int(u0.resolution[0]), int(u0.resolution[1])
    with rt.Renderer(pipeline=pipeline) as r:
        r.resize(W, H)
        r.upload_env(faces)
        if nodes is not None:
            r.upload_bvh(nodes, tris)
        r.debug_builds(reset=True)
        for i, f in enumerate(int(v) for v in d["frames"]):
            u = rt.RtUniforms.from_buffer_copy(d["uniforms"][i].tobytes())
            while r.frame_index < f:
                r.render_frame(u)
            assert r.frame_index == f
            hist = window_history(d, f)
            if hist is not None:
                r.write_target(rt.RT_TARGET_COLOR, embed_outer(d, hist, (H, W)))
            r.render_frame(u)
            check_window(name, f, r.read_all(), d)
        if "_million_" in name:
            # the default any-hit walk of this scene is the quantised 64-byte node form, which no smaller fixture reaches
            assert "QN2" in r.debug_builds()["any"]
            assert not (r.scene_info().flags & rt.RT_SCENE_QNODES_REJECTED)


@pytest.mark.parametrize("tag", ["svgf", "plain", "motion"])
def test_hip_matches_reference_glsl_present_1080p_window(ren, tag):
    d, targets = present_window_inputs()
    pp = rt.RtPresentParams.from_buffer_copy(d[f"pp_{tag}"].tobytes())
    ren.resize(1920, 1080)
    for which, a in zip((rt.RT_TARGET_COLOR, rt.RT_TARGET_MOTION, rt.RT_TARGET_GPOS, rt.RT_TARGET_GNRM), targets):
        ren.write_target(which, a)
    check_present_window(tag, ren.present_with(pp), d)


@pytest.mark.parametrize("tag", ["crate", "bunny"])
def test_hip_matches_reference_glsl_traversal_loops(ren, tag):
    """rt_debug_trace (the device traversal) against traceBVH / traceBVHShadow as the reference GLSL executed them."""
    d = np.load(GOLDEN / "glsl_bvh_trace_kat.npz")
    nodes, tris, rays = d[f"{tag}_nodes12"], d[f"{tag}_tris12"], d[f"{tag}_rays"]
    ren.upload_bvh(nodes, tris)
    eps, inf = float(d["eps"]), float(d["inf"])
    c = ren.debug_trace(0, rays[:, 0:3], rays[:, 4:7], eps=eps, inf=inf)
    a = ren.debug_trace(1, rays[:, 0:3], rays[:, 4:7], rays[:, 3], eps=eps, inf=inf)
    compared, hits, tie_rays = check_trace_kat(tag, d, lambda i: (c[i, 0] < np.float32(inf), c[i, 0], c[i, 1:4], c[i, 4:7]), lambda i: a[i, 0] != 0.0)
    assert compared >= 1000 and hits >= 900
    if tag == "crate":
        assert tie_rays >= 300


@pytest.mark.parametrize("tag", ["svgf", "plain", "motion", "svgf_moving"])
def test_hip_matches_reference_glsl_present(ren, tag):
    d = np.load(GOLDEN / "glsl_present_48x36.npz")
    pp = rt.RtPresentParams.from_buffer_copy(d[f"pp_{tag}"].tobytes())
    ren.resize(48, 36)
    for which, k in ((rt.RT_TARGET_COLOR, "color"), (rt.RT_TARGET_MOTION, "motion"), (rt.RT_TARGET_GPOS, "gpos"), (rt.RT_TARGET_GNRM, "gnrm")):
        ren.write_target(which, d[f"{k}_{tag}"])
    got = ren.present_with(pp)
    want = d[f"rgba_{tag}"]
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert diff.max() <= 1 and np.mean(got == want) >= 0.995, (tag, diff.max(), np.mean(got == want))


def test_write_target_round_trip(ren):
    rng = np.random.default_rng(1)
    ren.resize(70, 37)                                    # ragged: partial tiles on both axes
    for which, ch in ((rt.RT_TARGET_COLOR, 4), (rt.RT_TARGET_MOTION, 2), (rt.RT_TARGET_GPOS, 4), (rt.RT_TARGET_GNRM, 4)):
        img = rng.integers(0, 0x7C00, size=(37, 70, ch), dtype=np.uint16)
        ren.write_target(which, img)
        assert np.array_equal(ren.read_target(which), img)
