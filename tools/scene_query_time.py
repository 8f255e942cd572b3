"""Times rt_trace_scene_rays / rt_pick_pixels (Renderer.trace_scene_rays and Renderer.pick on torch device tensors).

    python tools/scene_query_time.py [--calls N] [--out profiles/scene_query_time.json]

Cases at 1920x1080:
  * a full-frame pick (every pixel) in each scene mode: analytic (default camera), BVH and hybrid (the bench mesh -- bunny stand-in,
    81 920 triangles -- with the close-up camera), and the 1 M-triangle scene in hybrid mode (default camera);
  * 2 073 600 analytic closest-hit rays (the default camera's primary rays) with normals and objects;
  * hybrid closest hit on the close-up primary rays, next to the analytic leg alone and rt_trace_rays on the same rays;
  * hybrid any hit, one cosine-hemisphere AO-style ray per primary hit, tMax = aoRadius;
  * the trace_primary stage of rt_render_frame for the same camera (BVH mode), and a one-pixel pick (device time and host wall time).
Device times: torch.cuda events on the caller's stream around each call, after warm-up (the call makes that stream wait for the query).
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import opengl_raytracing_amd as rt  # noqa: E402
import scenes  # noqa: E402
from query_time import ao_rays, frame_stages, primary_rays, timed  # noqa: E402

W, H = 1920, 1080


def uniforms(mode, cam, nodes=None, tris=None):
    cam.aspect = W / H
    nt = (nodes.shape[0], tris.shape[0]) if nodes is not None else ()
    return rt.frame_uniforms(rt.default_render_params(), cam, W, H, 1, mode, *nt, env_loaded=False)


def all_pixels(torch, dev):
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.int32), torch.arange(W, device=dev, dtype=torch.int32), indexing="ij")
    return torch.stack([xs.reshape(-1), ys.reshape(-1)], 1).contiguous()


def record(out, r, **kw):
    r.update(kw)
    if "rays" in r:
        r["mrays_per_s"] = r["rays"] / (r["ms_median"] * 1e3)
    print(json.dumps(r), flush=True)
    out.append(r)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    out = []
    nodes, tris = scenes.bunny_bvh()
    v, f = rt.meshgen.million_triangle_scene()
    nodes_m, tris_m = rt.build_bvh(rt.gather_triangles(v, f, np.eye(4, dtype=np.float32).reshape(-1)))
    xy = all_pixels(torch, dev)
    n = xy.shape[0]
    with rt.Renderer() as ren:
        # analytic scene: full-frame pick, and 2 073 600 closest-hit rays with normals and objects
        ua = uniforms(0, scenes.camera("default"))
        record(out, timed(torch, lambda: ren.pick(ua, xy, normals=True, points=True), a.calls), case="analytic: full-frame pick 1920x1080", rays=n)
        o, d = primary_rays(torch, ua, W, H, dev)
        record(out, timed(torch, lambda: ren.trace_scene_rays(ua, o, d, normals=True), a.calls),
               case="analytic: 2 073 600 closest-hit rays (default camera's primary rays), objects + normals", rays=n)
        # bench mesh, close-up camera: BVH and hybrid picks; hybrid closest hit against its legs; hybrid any hit
        ren.upload_bvh(nodes, tris)
        ub = uniforms(1, scenes.camera("closeup"), nodes, tris)
        uh = uniforms(rt.RT_SCENE_HYBRID, scenes.camera("closeup"), nodes, tris)
        pb = record(out, timed(torch, lambda: ren.pick(ub, xy, normals=True, points=True), a.calls), case="BVH: full-frame pick 1920x1080, bench mesh, close-up",
                    rays=n)
        record(out, timed(torch, lambda: ren.pick(uh, xy, normals=True, points=True), a.calls), case="hybrid: full-frame pick 1920x1080, bench mesh, close-up",
               rays=n)
        o, d = primary_rays(torch, ub, W, H, dev)
        hy = record(out, timed(torch, lambda: ren.trace_scene_rays(uh, o, d, normals=True), a.calls),
                    case="hybrid: closest hit, close-up primary rays, objects + normals", rays=n)
        uan = uniforms(0, scenes.camera("closeup"))
        an = record(out, timed(torch, lambda: ren.trace_scene_rays(uan, o, d, normals=True), a.calls),
                    case="analytic leg alone: the same rays in analytic mode", rays=n)
        tr = record(out, timed(torch, lambda: ren.trace_rays(o, d, eps=ub.eps, inf=ub.inf, normals=True), a.calls),
                    case="rt_trace_rays: the same rays, normals", rays=n)
        hy["target_ms"] = an["ms_median"] + 1.1 * tr["ms_median"]
        hits = ren.trace_scene_rays(uh, o, d, normals=True)
        p = rt.default_render_params()
        ao_o, ao_d = ao_rays(torch, o, d, SimpleNamespace(prim=hits.object, normal=hits.normal, t=hits.t), float(p.aoBias))
        tm = torch.full((ao_o.shape[0],), float(p.aoRadius), device=dev)
        occ = ren.trace_scene_rays(uh, ao_o, ao_d, tm, any_hit=True)
        record(out, timed(torch, lambda: ren.trace_scene_rays(uh, ao_o, ao_d, tm, any_hit=True), a.calls),
               case=f"hybrid: any hit, one cosine-hemisphere ray per primary hit, tMax = aoRadius {p.aoRadius}", rays=int(ao_o.shape[0]),
               occluded=int(occ.sum()))
        # one pixel: latency
        one = xy[n // 2 + W // 2:n // 2 + W // 2 + 1].contiguous()
        r = timed(torch, lambda: ren.pick(uh, one), max(a.calls, 50))
        wall = []
        for _ in range(50):
            t0 = time.perf_counter()
            ren.pick(uh, one)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        record(out, r, case="hybrid: one-pixel pick (latency)", rays=1, wall_ms_call_and_sync_median=float(np.median(wall)))
        # the 1 M-triangle scene, hybrid mode
        ren.upload_bvh(nodes_m, tris_m)
        um = uniforms(rt.RT_SCENE_HYBRID, scenes.camera("default"), nodes_m, tris_m)
        record(out, timed(torch, lambda: ren.pick(um, xy, normals=True, points=True), a.calls),
               case="hybrid: full-frame pick 1920x1080, 1M-triangle scene, default camera", rays=n)
    cam = scenes.camera("closeup")
    cam.aspect = W / H
    fs = frame_stages(nodes, tris, cam, W, H, a.frames)
    record(out, {"case": "rt_render_frame stage times, bench mesh, close-up camera, BVH mode (ms per frame)", **fs,
                 "bvh_pick_over_trace_primary": pb["ms_median"] / fs["trace_primary"] if fs.get("trace_primary") else None})
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
