"""rt.trace_build -- the build choice in plain C++ (csrc/rt_trace_build.cpp) -- predicts the k_trace builds a context launches: fed with what
the UPLOADED scene offers (the record forms on the device, the tree's depth, the any-hit stack size) under the environment the context was created in, it
names the builds Renderer.debug_builds reports after one closest-hit and one any-hit rt_debug_trace launch.  rt_debug_trace gives its launches no sums to
add to, so under RT_TRACE_STATS it launches the production builds (only a frame's launches count): stats is False throughout.
"""
import numpy as np
import pytest

import opengl_raytracing_amd as rt
import test_gpu_options as gpu_options
import trace_build_cases

pytestmark = pytest.mark.gpu

ENVS = {"none": {}, "qnodes2": {"RT_QNODES": "2"}, "implicit": {"RT_IMPLICIT": "1"}, "coop_fused": {"RT_COOP": "1", "RT_FUSED": "1"},
        "trace_stats": {"RT_TRACE_STATS": "1"}}


def _rays(nodes, n=64, seed=3):
    """n rays from outside the root box towards points inside it; tMax beyond the box."""
    rng = np.random.default_rng(seed)
    lo, hi = nodes[0, 0:3].astype(np.float64), nodes[0, 4:7].astype(np.float64)
    ext = float((hi - lo).max())
    target = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    org = target - d * 2.0 * ext
    return org.astype(np.float32), d.astype(np.float32), np.full(n, 4.0 * ext, np.float32)


@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("mesh", ["one_leaf", "bunny"])
def test_trace_build_predicts_debug_builds(monkeypatch, mesh, env):
    for v in gpu_options.OPTION_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, v)
    nodes, tris = gpu_options._mesh(mesh)
    org, dirs, tmax = _rays(nodes)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r:
        r.upload_bvh(nodes, tris)
        forms = tuple(f for f, a in trace_build_cases.FORM_ARRAYS.items() if r.debug_read_scene(a).size)
        depth = int(r.scene_info().treeDepth)
        packed_depth, any_stack, packed_forms = trace_build_cases.scene_offers(nodes, tris)     # (the any-hit stack size is the host packers' alone to report)
        assert (packed_depth, packed_forms) == (depth, forms)
        r.debug_builds(reset=True)
        r.debug_trace(2, org, dirs)
        r.debug_trace(3, org, dirs, tmax)
        got = r.debug_builds()
    want = {kind: frozenset({"k_trace"}) | rt.trace_build(kind == "any", depth=depth, stats=False, any_stack=any_stack, forms=forms).bits for kind in ("closest", "any")}
    assert got == want, (mesh, env, forms, depth, any_stack)
    if mesh == "bunny":      # the environment was not ignored
        assert want["closest"] - {"k_trace"} == {"coop_fused": {"COOP"}, "implicit": {"IMPL"}}.get(env, set())
        assert want["any"] - {"k_trace"} == {"qnodes2": {"QN2"}, "implicit": {"IMPL"}}.get(env, set())
