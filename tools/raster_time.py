"""Times rt_render_raster (device ms from rt_get_raster_stats, and wall ms per frame over back-to-back calls).

    python tools/raster_time.py [--frames N] [--out profiles/raster_time.json]

Cases: renderRaster's scene at 1920x1080 (2-triangle ground quad, bunny stand-in of 81 920 triangles, UV sphere, point-light marker)
with the default and the close-up camera (and the default camera once more with bin arrays for half of its pairs, so that half of
the triangles take the path past the capacity), and the 1 M-triangle scene of BASELINE configs[4] drawn as one mesh with the identity model.

    python tools/raster_time.py --dynamic [--reps N] [--out profiles/raster_dynamic.json]

The raster preview of a mesh that is animated every step, 1920x1080, default and close-up camera, the bench mesh (81 920 triangles)
and the 1 M scene, positions displaced every step, routes alternated in one process, medians (min .. max) of the wall clock per step:
  route A  rt_raster_mesh of the host positions -> rt_render_raster -> rt_synchronize                   (the only route without a binding)
  route B  rt_mesh_set_positions -> rt_render_raster on a slot bound to the dynamic mesh -> rt_synchronize, bound with RT_RASTER_BIND_SINGLE and with
           RT_RASTER_BIND_PARTS at 1, 64 and 4096 parts (a distinct matrix per part, rewritten every step)
and RtRasterStats.deviceMs of each bound draw beside the same geometry drawn from a static slot uploaded once.  --route-a-only times route A alone
(the code a tree without the binding has too).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import opengl_raytracing_amd as rt  # noqa: E402
from opengl_raytracing_amd import meshgen  # noqa: E402
import scenes  # noqa: E402


def case(ren, name, draws, cam, frames, W, H):
    view, proj = rt.camera_view(cam), rt.camera_proj(cam)
    for _ in range(3):
        ren.render_raster(draws, view, proj)          # warm-up: sizes the bin arrays
    dev = []
    for _ in range(frames):
        ren.render_raster_async(draws, view, proj)
        dev.append(ren.raster_stats().deviceMs)
    ren.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        ren.render_raster_async(draws, view, proj)
    ren.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / frames
    st = ren.raster_stats()
    r = {"case": name, "size": [W, H], "frames": frames, "device_ms_median": float(np.median(dev)), "device_ms_min": float(np.min(dev)),
         "wall_ms_per_frame": wall, "triangles_in": st.trianglesIn, "set_up": st.trianglesSetUp, "dropped": st.trianglesDropped,
         "clipped": st.trianglesClipped, "bin_entries": st.binEntries, "bin_capacity": st.binCapacity, "raster_bytes": st.rasterBytes}
    print(json.dumps(r), flush=True)
    return r


def _mmm(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x))}


def _fmt(m):
    return f"{m['median']:.3f} ({m['min']:.3f} .. {m['max']:.3f})"


def _part_matrices(k, step):
    """k distinct matrices that change with the step: small translations, so every part stays where the camera looks"""
    m = np.tile(np.eye(4, dtype=np.float32).reshape(-1), (k, 1))
    p = np.arange(k)
    m[:, 12] = 1e-3 * ((p + step) % 17)
    m[:, 13] = 1e-3 * ((p + 2 * step) % 13)
    return m


def dynamic_case(ren, name, pos, idx, model, cam, reps, W, H, route_a_only=False):
    view, proj = rt.camera_view(cam), rt.camera_proj(cam)
    n = idx.size // 3
    rng = np.random.default_rng(1)
    steps = [(pos + rng.normal(0, 1e-3, pos.shape)).astype(np.float32) for _ in range(4)]     # positions displaced every step
    color = (0.8, 0.7, 0.6)
    A_SLOT, B_SLOT, S_SLOT = 0, 1, 2
    draw_a, draw_b, draw_s = [rt.raster_draw(A_SLOT, model, color)], [rt.raster_draw(B_SLOT, model, color)], [rt.raster_draw(S_SLOT, model, color)]

    def route_a(i):
        t0 = time.perf_counter()
        ren.raster_mesh(A_SLOT, steps[i % 4], idx)
        ren.render_raster_async(draw_a, view, proj)
        ren.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = []
    if route_a_only:
        for i in range(3):
            route_a(i)
        a_ms = [route_a(i) for i in range(reps)]
        r = {"case": name, "triangles": n, "route_a_wall_ms": _mmm(a_ms)}
        print(json.dumps(r), flush=True)
        return [r]
    ren.raster_mesh(S_SLOT, pos, idx)                                 # the same geometry from a static slot, uploaded once
    for variant in ("single", 1, 64, 4096):
        k = 1 if variant == "single" else variant
        ren.mesh_upload_parts(pos, idx, np.linspace(0, n, k + 1).astype(np.int32))
        ren.raster_mesh_dynamic(B_SLOT, parts=variant != "single")

        mats = [_part_matrices(k, i) for i in range(4)]               # a distinct matrix per part, rewritten every step

        def route_b(i):
            t0 = time.perf_counter()
            ren.mesh_set_positions(steps[i % 4])
            if variant != "single":
                ren.mesh_set_part_matrices(mats[i % 4])
            ren.render_raster_async(draw_b, view, proj)
            ren.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for i in range(3):                                            # warm-up: sizes the bin arrays and the MVP table
            route_a(i); route_b(i)
        a_ms, b_ms = [], []
        for i in range(reps):                                         # alternated
            a_ms.append(route_a(i)); b_ms.append(route_b(i))
        # device time on identical geometry: the base positions in the mesh, the static slot beside it, alternated
        ren.mesh_set_positions(pos)
        if variant != "single":
            ren.mesh_set_part_matrices(np.tile(np.eye(4, dtype=np.float32).reshape(-1), (k, 1)))
        dev_b, dev_s = [], []
        for i in range(reps):
            ren.render_raster_async(draw_s, view, proj); dev_s.append(ren.raster_stats().deviceMs)
            ren.render_raster_async(draw_b, view, proj); dev_b.append(ren.raster_stats().deviceMs)
        a, b, ds, db = _mmm(a_ms), _mmm(b_ms), _mmm(dev_s), _mmm(dev_b)
        r = {"case": name, "triangles": n, "variant": f"{variant}" if variant == "single" else f"parts={variant}", "reps": reps,
             "route_a_wall_ms": a, "route_b_wall_ms": b, "static_device_ms": ds, "bound_device_ms": db,
             "condition1": bool(b["median"] < a["median"] and b["max"] < a["min"])}
        if variant == "single":
            r["condition2"] = bool(ds["min"] <= db["median"] <= ds["max"])
        print(json.dumps(r), flush=True)
        print(f"# {name}, {r['variant']}: A {_fmt(a)} ms, B {_fmt(b)} ms; device static {_fmt(ds)} ms, bound {_fmt(db)} ms; "
              f"condition 1 {'holds' if r['condition1'] else 'FAILS'}" + (f", condition 2 {'holds' if r['condition2'] else 'FAILS'}" if "condition2" in r else ""),
              flush=True)
        out.append(r)
    ren.raster_mesh(B_SLOT, None)
    ren.mesh_upload(pos, None)
    return out


def dynamic(a):
    W, H = 1920, 1080
    out = []
    b = meshgen.bunny_standin(6)
    bunny = np.ascontiguousarray(b[0], np.float32), np.ascontiguousarray(b[1], np.uint32).reshape(-1)
    bunny_model = list(rt.raster_scene_draws(rt.default_render_params(), 0, 1, 2)[1].model)
    m = meshgen.million_triangle_scene()[:2]
    million = np.ascontiguousarray(m[0], np.float32), np.ascontiguousarray(m[1], np.uint32).reshape(-1)
    with rt.Renderer() as ren:
        ren.resize(W, H)
        for cam in ("default", "closeup"):
            for name, (pos, idx), model in (("bench mesh", bunny, bunny_model), ("1M scene", million, None)):
                out += dynamic_case(ren, f"{name}, {cam} camera", pos, idx, model, scenes.camera(cam, aspect=W / H), a.reps, W, H, a.route_a_only)
    if not a.route_a_only:
        c1 = [r["condition1"] for r in out]
        c2 = [r["condition2"] for r in out if "condition2" in r]
        print(f"# condition 1 (route B below route A: medians, and B's whole range below A's minimum): holds in {sum(c1)} of {len(c1)} rows")
        print(f"# condition 2 (RT_RASTER_BIND_SINGLE device median inside the static draw's min .. max): holds in {sum(c2)} of {len(c2)} rows")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dynamic", action="store_true", help="the animated-mesh measurement of DESIGN.md 11.4")
    ap.add_argument("--route-a-only", action="store_true", help="with --dynamic: time route A alone")
    ap.add_argument("--reps", type=int, default=12)
    a = ap.parse_args()
    if a.dynamic:
        return dynamic(a)
    W, H = 1920, 1080
    out = []
    with rt.Renderer() as ren:
        ren.resize(W, H)
        b = meshgen.bunny_standin(6)
        s = meshgen.uv_sphere(32, 16)
        g = np.array([[-20, 0, -20], [20, 0, -20], [20, 0, 20], [-20, 0, 20]], np.float32), np.array([0, 2, 1, 0, 3, 2], np.uint32)
        ren.raster_mesh(0, *g)
        ren.raster_mesh(1, b[0], b[1])
        ren.raster_mesh(2, s[0], s[1])
        draws = rt.raster_scene_draws(rt.default_render_params(), 0, 1, 2)
        for cam in ("default", "closeup"):
            out.append(case(ren, f"renderRaster scene, {cam} camera", draws, scenes.camera(cam, aspect=W / H), a.frames, W, H))
        # the path past the bin capacity (a first call whose pairs outgrow the initial size): bins for half of the default camera's pairs
        half = out[0]["bin_entries"] // 2
        ren.debug_raster_bin_capacity(half)
        out.append(case(ren, f"renderRaster scene, default camera, bins for {half} of {out[0]['bin_entries']} pairs (fallback walk)", draws,
                        scenes.camera("default", aspect=W / H), max(a.frames // 5, 3), W, H))
        ren.debug_raster_bin_capacity(0)
        pos, idx = meshgen.million_triangle_scene()[:2]
        ren.raster_mesh(3, pos, idx)
        out.append(case(ren, "1M-triangle scene, identity model", [rt.raster_draw(3, None, (0.8, 0.7, 0.6))], scenes.camera("default", aspect=W / H),
                        a.frames, W, H))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
