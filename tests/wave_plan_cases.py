"""The four smallest launch sets a renderer can produce among the shape cases of test_wave_plan_host.py, shared by tests/golden/make_wave_plan_golden.py
(which records what a commit allocated for them) and tests/test_gpu_wave_plan.py (which holds the planner to the device and to that record).

A case is (name, W, H, spp, AO rays per hit or 0 for AO off, environment).  The environment is set before the Renderer exists: the lane reads its
options when it is created."""
import opengl_raytracing_amd as rt
import scenes

GPU_CASES = (
    ("64x64_spp1_no_ao", 64, 64, 1, 0, {}),
    ("64x64_spp2_ao3", 64, 64, 2, 3, {}),
    ("160x96_spp2_1mb", 160, 96, 2, 3, {"RT_QUEUE_BUDGET_MB": "1"}),
    ("160x96_spp2_1mb_bin_gi", 160, 96, 2, 3, {"RT_QUEUE_BUDGET_MB": "1", "RT_BIN_GI": "1"}),
)
# every variable the lane's options read (rtl::wave_options_from_env), so that a test can start from a clean environment
OPTION_VARS = ("RT_QUEUE_BUDGET_MB", "RT_BIN_GI", "RT_PACKET_AO", "RT_BOUNCE_PROBE", "RT_CHUNKS_FROM_SLOTS", "RT_CU_SPLIT", "RT_SHADE_PRIORITY",
               "RT_DEBUG_SKIP_TRAVERSAL", "RT_Q2_PREDICT", "RT_Q2_CAP", "RT_GRID_PCT", "RT_GRID_PCT_PRIMARY", "RT_CHUNK_PRIMARY", "RT_TRACE_STATS",
               "RT_TRACE_TIMING")


def options_of(env):
    """The environment of a case as keywords of rt.wave_plan."""
    names = {"RT_QUEUE_BUDGET_MB": "budget_mb", "RT_BIN_GI": "binGi"}
    return {names[k]: int(v) for k, v in env.items()}


def render_one_frame(case, setenv):
    """One frame of `case` on a fresh one-lane renderer.  setenv(name, value) sets a variable (monkeypatch.setenv or os.environ.__setitem__).
    -> dict of the rt_get_memory_info fields the planner answers for, the frame's hit pixels and its bounce-launch counts."""
    name, W, H, spp, ao, env = case
    setenv("RT_LANES", "1")
    for k, v in env.items():
        setenv(k, v)
    nodes, tris = scenes.bunny_bvh(3)
    p = rt.default_render_params()
    p.sppPerFrame = spp
    p.enableAO = 1 if ao else 0
    if ao:
        p.aoSamples = ao
    cam = scenes.camera("closeup", aspect=W / H)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r:
        r.upload_bvh(nodes, tris)
        r.upload_env(scenes.tiny_env(8))
        r.resize(W, H)
        r.traced_rays(reset=True)
        r.bounce_probe(reset=True)
        r.render_frame(rt.frame_uniforms(p, cam, W, H, 0, True, nodes.shape[0], tris.shape[0]))
        r.read_target(0)
        m, t, b = r.memory_info(), r.traced_rays(), r.bounce_probe()
        return {"queueArenaBytes": int(m.queueArenaBytes), "queueArenas": int(m.queueArenas), "frameArrayBytes": int(m.frameArrayBytes),
                "hitPixels": int(t.hitPixels), "bounceLaunches": int(b.probeLaunches + b.closestLaunches)}
