"""The named cases of tests/golden/trace_build_parent.json -- shared by its generator (tests/golden/make_trace_build_golden.py, which runs the parent's
launch_trace) and tests/test_trace_build_host.py: every environment of RAY_CASES, FRAME_CASES and test_instrumented_builds in tests/test_gpu_options.py on
the mesh that case uses, and no environment at all on a scene without and with quantised nodes.  What a scene offers a launch comes from the host packers
(rt.pack_scene) under the case's environment: no GPU."""
import os

import opengl_raytracing_amd as rt
import test_gpu_options as gpu_options

# the environments of test_instrumented_builds (its parametrize list), and the builds it expects of a frame's launches: (closest, any)
INSTRUMENTED = {"stats1": ({"RT_TRACE_STATS": "1"}, {"STATS"}, {"STATS"}), "stats2": ({"RT_TRACE_STATS": "2"}, {"STATS"}, {"STATS"}),
                "timing": ({"RT_TRACE_TIMING": "1"}, {"TIMING"}, {"TIMING"})}
FORM_ARRAYS = {"q4": "qnodes4", "wF": "fused", "iN2": "impl_nodes2", "iN4": "impl_nodes4", "iQ4": "impl_qnodes4"}   # TRACE_FORMS -> rt.pack_scene's names


def with_env(env, fn):
    """fn() under exactly the option variables of env (every other one of test_gpu_options.OPTION_VARS deleted); the environment is restored."""
    saved = {v: os.environ.get(v) for v in gpu_options.OPTION_VARS}
    try:
        for v in gpu_options.OPTION_VARS:
            os.environ.pop(v, None)
        os.environ.update(env)
        return fn()
    finally:
        for v, old in saved.items():
            os.environ.pop(v, None)
            if old is not None:
                os.environ[v] = old


def scene_offers(nodes, tris, **options):
    """(depth, anyStack, forms) of the scene an upload of this tree installs under the current environment (or pack_scene's options)."""
    p = rt.pack_scene(nodes, tris, **options)
    return int(p["info"].treeDepth), int(p["info"].anyStack), tuple(f for f, a in FORM_ARRAYS.items() if p[a].size)


def cases():
    """[(name, env, any, stats, depth, anyStack, forms, expected extra bits or None)] -- stats: a frame's launch under RT_TRACE_STATS / RT_TRACE_TIMING."""
    out = []

    def add(name, env, mesh, stats, want_closest, want_any, **options):
        nodes, tris = gpu_options._mesh(mesh)
        depth, any_stack, forms = with_env(env, lambda: scene_offers(nodes, tris, **options))
        out.append((f"{name}/closest", env, False, stats, depth, any_stack, forms, want_closest))
        out.append((f"{name}/any", env, True, stats, depth, any_stack, forms, want_any))

    for cid, (mesh, env, wc, wa) in gpu_options.RAY_CASES.items():
        add(f"ray/{cid}", env, mesh, False, wc, wa)
    for cid, (env, mesh, _, _, want) in gpu_options.FRAME_CASES.items():
        add(f"frame/{cid}", env, mesh, False, set(want["closest"]) - {"k_trace"}, set(want["any"]) - {"k_trace"})
    for cid, (env, wc, wa) in INSTRUMENTED.items():
        add(f"instrumented/{cid}", env, "bunny", True, wc, wa)
    add("default/exact", {}, "bunny", False, set(), set())
    add("default/quantised", {}, "bunny", False, set(), {"QN2"}, qnodes=1)   # (a tree beyond the L2 gets them by size; here the packer is told to)
    return out
