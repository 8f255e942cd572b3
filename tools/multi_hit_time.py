"""Times rt_trace_rays_multi (Renderer.trace_rays_multi on torch device tensors) against rt_trace_rays on the same rays, in one visit.

    python tools/multi_hit_time.py [--calls N] [--out profiles/multi_hit_time.json]

Rays: the bench mesh's (bunny stand-in, 81 920 triangles) 1920x1080 close-up primary rays.  Queries: rt_trace_rays closest hit and any hit (tMax =
uINF), rt_trace_rays_multi at K = 0, 1, 4, 16, 32 without tMax, and once more at K = 4 with tMax = 1.5 times each ray's closest t (uINF on a miss).
Device times: torch.cuda events on the caller's stream around each call, after warm-up (the call makes that stream wait for the query).  Every
figure also as a ratio to the closest-hit query of the same visit."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import opengl_raytracing_amd as rt  # noqa: E402
import scenes  # noqa: E402
from query_time import primary_rays, timed  # noqa: E402

W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_hit_time.json"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    nodes, tris = scenes.bunny_bvh()
    cam = scenes.camera("closeup")
    cam.aspect = W / H
    u = rt.frame_uniforms(rt.default_render_params(), cam, W, H, 1, True, nodes.shape[0], tris.shape[0], env_loaded=False)
    out = []

    def record(r, **kw):
        r.update(kw, rays=W * H)
        r["mrays_per_s"] = r["rays"] / (r["ms_median"] * 1e3)
        if out:
            r["over_closest"] = r["ms_median"] / out[0]["ms_median"]
        print(json.dumps(r), flush=True)
        out.append(r)

    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        o, d = primary_rays(torch, u, W, H, dev)
        q = dict(eps=u.eps, inf=u.inf)
        closest = ren.trace_rays(o, d, **q)
        record(timed(torch, lambda: ren.trace_rays(o, d, **q), a.calls), case="rt_trace_rays: closest hit", hit_rays=int((closest.prim >= 0).sum()))
        far = torch.full((W * H,), float(u.inf), device=dev)
        record(timed(torch, lambda: ren.trace_rays(o, d, far, any_hit=True, **q), a.calls), case="rt_trace_rays: any hit, tMax = uINF")
        for K in (0, 1, 4, 16, 32):
            m = ren.trace_rays_multi(o, d, max_hits=K, **q)
            record(timed(torch, lambda: ren.trace_rays_multi(o, d, max_hits=K, **q), a.calls), case=f"rt_trace_rays_multi: K = {K}, no tMax", K=K,
                   hits_total=int(m.count.sum()), hits_max=int(m.count.max()), rays_beyond_K=int((m.count > K).sum()))
            del m
        tm = torch.where(closest.prim >= 0, closest.t * 1.5, far).contiguous()
        m = ren.trace_rays_multi(o, d, tm, max_hits=4, **q)
        record(timed(torch, lambda: ren.trace_rays_multi(o, d, tm, max_hits=4, **q), a.calls), case="rt_trace_rays_multi: K = 4, tMax = 1.5 x the closest t", K=4,
               hits_total=int(m.count.sum()), hits_max=int(m.count.max()))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
