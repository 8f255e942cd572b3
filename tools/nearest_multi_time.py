"""Times rt_query_nearest_multi (Renderer.nearest_points_multi on torch device tensors) against rt_query_nearest on the same points, in
one visit.

    python tools/nearest_multi_time.py [--calls N] [--out profiles/nearest_multi_time.json]

Scene and point sets as tools/nearest_time.py: the bench mesh (bunny stand-in, 81 920 triangles) and 1920 x 1080 = 2 073 600 points each of surface
points in pixel order, the same shuffled, and uniform random points in twice the root box.  Per set K = 1, 4, 16 and 32 without counts and without a
limit (the walk culls against its K-th best), and with counts at max_dist = 0.05 (it culls against the limit alone).  Device times: torch.cuda events
on the caller's stream around each call, after warm-up, the median of the calls.  Every figure also as a ratio to rt_query_nearest on the same points
and the same limit, with the mean and the largest number of boxes visited per point."""
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
KS = (1, 4, 16, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_multi_time.json"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    nodes, tris = scenes.bunny_bvh()
    cam = scenes.camera("closeup")
    cam.aspect = W / H
    u = rt.frame_uniforms(rt.default_render_params(), cam, W, H, 1, True, nodes.shape[0], tris.shape[0], env_loaded=False)
    N = W * H
    out = []

    def record(r, base=None, **kw):
        r.update(kw)
        r["mpoints_per_s"] = N / (r["ms_median"] * 1e3)
        if base is not None:
            r["over_query_nearest"] = r["ms_median"] / base["ms_median"]
        print(json.dumps(r), flush=True)
        out.append(r)
        return r

    def visits(r):
        return dict(visits_mean=float(r.visits.double().mean()), visits_max=int(r.visits.max()))

    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        o, d = primary_rays(torch, u, W, H, dev)
        hits = ren.trace_rays(o, d, normals=True, eps=u.eps, inf=u.inf)
        hit = hits.prim >= 0
        at = torch.cummax(torch.where(hit, torch.arange(N, device=dev), torch.full((N,), -1, device=dev)), 0).values
        at = torch.where(at >= 0, at, torch.nonzero(hit)[0, 0])              # pixels before the first hit take the first
        surface = (o + d * hits.t[:, None] + hits.normal * OFFSET)[at].contiguous()
        del hits, o, d
        g = torch.Generator(device=dev).manual_seed(5)
        shuffled = surface[torch.randperm(N, device=dev, generator=g)].contiguous()
        lo, hi = (torch.tensor(nodes[0, k:k + 3], device=dev) for k in (0, 4))
        box = ((lo + hi) * 0.5 + (torch.rand((N, 3), device=dev, generator=g) - 0.5) * 2.0 * (hi - lo)).contiguous()
        limit = torch.full((N,), MAX_DIST, device=dev)
        for name, pts in (("surface points in pixel order", surface), ("surface points shuffled", shuffled), ("uniform in 2 x the root box", box)):
            for md, counts in ((None, False), (limit, True)):
                how = "no limit, no counts" if md is None else f"max_dist = {MAX_DIST}, counts"
                r = ren.nearest_points(pts, md, visits=True)
                stats = dict(points=N, max_dist=None if md is None else MAX_DIST, answered=int((r.prim >= 0).sum()), **visits(r))
                del r
                base = record(timed(torch, lambda: ren.nearest_points(pts, md), a.calls), case=f"rt_query_nearest: {name}, {how}", **stats)
                for K in KS:
                    r = ren.nearest_points_multi(pts, K, md, counts=counts, visits=True)
                    stats = dict(points=N, K=K, counts=counts, max_dist=None if md is None else MAX_DIST, records=int((r.prim >= 0).sum()), **visits(r))
                    if counts:
                        stats.update(count_mean=float(r.count.double().mean()), count_max=int(r.count.max()))
                    del r
                    record(timed(torch, lambda: ren.nearest_points_multi(pts, K, md, counts=counts), a.calls), base,
                           case=f"rt_query_nearest_multi: K = {K}, {name}, {how}", **stats)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
