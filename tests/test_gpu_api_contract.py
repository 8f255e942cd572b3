"""The C API outside the dynamic mesh after csrc/rt_api.hip was split by concern.  Contract: every call of tests/api_cases.py, in every
state it belongs to, returns the code and leaves the rt_last_error text that tests/golden/api_parent.json recorded on the commit before the split,
and touches no output; the three query families give the same bytes through their host and their device entry point, for query sizes that grow and
then reuse the one staging buffer; rt_read_target, rt_present and rt_present_gathered, which share that buffer through one helper, give the same
bytes in either order; the four lane-summed getters return the parent's numbers on one fixed render.  Every comparison is exact."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import api_cases as cases
import opengl_raytracing_amd as rt
import scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "api_parent.json").read_text())
W, H = cases.W, cases.H


def _same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ---------------------------------------------------------------- 1: refusals pinned to the parent commit
def test_the_table_is_the_recorded_one():
    assert set(GOLDEN["refusals"]) == set(cases.STATES)
    for state in cases.STATES:
        assert set(GOLDEN["refusals"][state]) == {name for name, (_, states) in cases.CALLS.items() if state in states}, state


@pytest.mark.parametrize("state", cases.STATES)
def test_refusals_are_the_parents(state):
    got, want = cases.run(state), GOLDEN["refusals"][state]
    assert set(got) == set(want)
    for name, g in got.items():
        assert name in cases.QUIET or g["rc"] != rt.RT_OK, (state, name, "was not refused")
        assert g["untouched"] and g.get("out7_untouched", True), (state, name, "an output was written")
        assert g == want[name], (state, name, g, want[name])


# ---------------------------------------------------------------- 2: the queries through both entry points, sharing one staging buffer
def test_queries_agree_across_their_two_paths():
    nodes, tris = scenes.bunny_bvh(3)
    rng = np.random.default_rng(19)
    cam = scenes.camera("closeup", aspect=W / H)
    u = rt.frame_uniforms(rt.default_render_params(), cam, W, H, 0, True, nodes.shape[0], tris.shape[0])
    lo, hi = nodes[0, 0:3], nodes[0, 4:7]
    centre, ext = ((lo + hi) / 2).astype(f32), float((hi - lo).max())
    org = (centre + rng.normal(0, 1, (5000, 3)) * ext).astype(f32)
    dirs = centre + rng.uniform(-0.6, 0.6, (5000, 3)) * ext - org    # towards the mesh and past it: hits and misses
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(f32)
    tmax = rng.uniform(0.2, 3.0, 5000).astype(f32) * f32(ext)
    xy = np.stack([rng.integers(0, W, 5000), rng.integers(0, H, 5000)], axis=1).astype(np.int32)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with rt.Renderer() as r:
        r.upload_bvh(nodes, tris)
        for m in (1, 64, 65, 5000, 3):                              # the staging buffer grows, then is reused oversize
            o, d, tm, px = org[:m], dirs[:m], tmax[:m], xy[:m]
            pairs = {
                "rays": (r.trace_rays(o, d, normals=True), r.trace_rays(t(o), t(d), normals=True)),
                "rays/any": (r.trace_rays(o, d, tm, any_hit=True), r.trace_rays(t(o), t(d), t(tm), any_hit=True)),
                "scene": (r.trace_scene_rays(u, o, d, normals=True, points=True), r.trace_scene_rays(u, t(o), t(d), normals=True, points=True)),
                "scene/any": (r.trace_scene_rays(u, o, d, tm, any_hit=True), r.trace_scene_rays(u, t(o), t(d), t(tm), any_hit=True)),
                "pick": (r.pick(u, px), r.pick(u, t(px))),
            }
            torch.cuda.synchronize()
            for name, (host, device) in pairs.items():
                if name.endswith("/any"):
                    assert _same(host, device.cpu().numpy()), (m, name)
                    continue
                for field in ("record", "normal", "object", "point"):
                    if hasattr(host, field):
                        assert _same(getattr(host, field), getattr(device, field).cpu().numpy()), (m, name, field)
            if m == 5000:                                           # the comparison is of answers, not of all-miss records
                for name in ("rays", "scene", "pick"):
                    assert pairs[name][0].hit.any(), name
                assert not pairs["rays"][0].hit.all() and pairs["rays/any"][0].any() and not pairs["rays/any"][0].all()


# ---------------------------------------------------------------- 3: the three read-backs through the one staging buffer
def test_read_backs_share_the_staging_buffer_in_either_order():
    nodes, tris = scenes.bunny_bvh(3)
    p = rt.default_render_params()
    p.sppPerFrame = 1
    cam = scenes.camera("closeup", aspect=W / H)
    pp = rt.make_present_params(p, False, W, H)
    with rt.Renderer() as r:
        r.upload_bvh(nodes, tris)
        r.resize(W, H)
        r.render_frame(rt.frame_uniforms(p, cam, W, H, 0, True, nodes.shape[0], tris.shape[0]))
        local = [r.local_target(which)[0] for which in range(4)]     # world 1: the local targets are the one gathered block
        calls = [lambda: r.read_target(rt.RT_TARGET_COLOR, rt.RT_FORMAT_F32), lambda: r.present_with(pp), lambda: r.present_gathered(pp, *local)]
        first = [c() for c in calls]
        again = [c() for c in reversed(calls)][::-1]
        for i, (a, b) in enumerate(zip(first, again)):
            assert _same(a, b), i
        assert first[0].any() and first[1].any()                    # a frame, not zeros
        assert _same(first[1], first[2])                            # one rank's gathered block is its own targets
        assert _same(r.read_target(rt.RT_TARGET_COLOR), r.read_target(rt.RT_TARGET_COLOR))   # the smaller format in the buffer the larger one grew


# ---------------------------------------------------------------- 4: the lane-summed getters on one fixed render
def test_lane_sums_are_the_parents():
    got = cases.lane_sums()
    assert set(got) == {"rt_get_traced_rays", "rt_debug_bounce_probe", "rt_debug_disk_skip", "rt_debug_gi_list"}
    assert got == GOLDEN["lane_sums"], (got, GOLDEN["lane_sums"])
