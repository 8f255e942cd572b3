"""Times rt_query_nearest (Renderer.nearest_points on torch device tensors) against rt_trace_rays on as many rays, in one visit.

    python tools/nearest_time.py [--calls N] [--out profiles/nearest_time.json]

Scene: the bench mesh (bunny stand-in, 81 920 triangles).  Point sets of 1920 x 1080 = 2 073 600 points each: the hit points of the close-up primary
rays displaced 0.01 along the face normal, in pixel order (coherent, near the surface; a pixel whose ray misses takes the hit point before it in scan
order); the same points shuffled; uniform random points in twice the root box.  Each set without a limit and with max_dist = 0.05.  Device times:
torch.cuda events on the caller's stream around each call, after warm-up (the call makes that stream wait for the query), the median of the calls.
Every figure also as a ratio to the closest-hit ray query of the same visit on the primary rays, with the mean number of boxes visited per point."""
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
OFFSET, MAX_DIST = 0.01, 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_time.json"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    nodes, tris = scenes.bunny_bvh()
    cam = scenes.camera("closeup")
    cam.aspect = W / H
    u = rt.frame_uniforms(rt.default_render_params(), cam, W, H, 1, True, nodes.shape[0], tris.shape[0], env_loaded=False)
    N = W * H
    out = []

    def record(r, **kw):
        r.update(kw)
        r["mpoints_per_s"] = N / (r["ms_median"] * 1e3)
        if out:
            r["over_closest_hit"] = r["ms_median"] / out[0]["ms_median"]
        print(json.dumps(r), flush=True)
        out.append(r)

    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        o, d = primary_rays(torch, u, W, H, dev)
        q = dict(eps=u.eps, inf=u.inf)
        hits = ren.trace_rays(o, d, normals=True, **q)
        record(timed(torch, lambda: ren.trace_rays(o, d, **q), a.calls), case="rt_trace_rays: closest hit, the primary rays", rays=N,
               hit_rays=int((hits.prim >= 0).sum()))
        hit = hits.prim >= 0
        at = torch.cummax(torch.where(hit, torch.arange(N, device=dev), torch.full((N,), -1, device=dev)), 0).values
        at = torch.where(at >= 0, at, torch.nonzero(hit)[0, 0])              # pixels before the first hit take the first
        surface = (o + d * hits.t[:, None] + hits.normal * OFFSET)[at].contiguous()
        g = torch.Generator(device=dev).manual_seed(5)
        shuffled = surface[torch.randperm(N, device=dev, generator=g)].contiguous()
        lo, hi = (torch.tensor(nodes[0, k:k + 3], device=dev) for k in (0, 4))
        box = ((lo + hi) * 0.5 + (torch.rand((N, 3), device=dev, generator=g) - 0.5) * 2.0 * (hi - lo)).contiguous()
        limit = torch.full((N,), MAX_DIST, device=dev)
        for name, pts in (("surface points in pixel order", surface), ("surface points shuffled", shuffled), ("uniform in 2 x the root box", box)):
            for md in (None, limit):
                r = ren.nearest_points(pts, md, visits=True)
                stats = dict(points=N, max_dist=None if md is None else MAX_DIST, answered=int((r.prim >= 0).sum()),
                             visits_mean=float(r.visits.double().mean()), visits_max=int(r.visits.max()))
                del r
                record(timed(torch, lambda: ren.nearest_points(pts, md), a.calls),
                       case=f"rt_query_nearest: {name}, {'no limit' if md is None else f'max_dist = {MAX_DIST}'}", **stats)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
