"""Times rt_query_boxes on torch device tensors, and rt_query_nearest_multi's radius count on the same centres for orientation, in
one visit.

    python tools/box_time.py [--calls N] [--out profiles/box_time.json]

Scene and centres as tools/nearest_time.py: the bench mesh (bunny stand-in, 81 920 triangles) and 1920 x 1080 = 2 073 600 points each of surface
points in pixel order, the same shuffled, and uniform random points in twice the root box.  Boxes are cubes about the centres with half-extents of
0.01, 0.05 and 0.2 of the root box's diagonal.  The work of a box grows with the rows it overlaps, so the larger extents take every 16th and every
256th centre (`boxes` in each record says how many).  Per set and extent: the counts alone (one call), and the exact list in two passes -- count,
torch.cumsum, list -- into arrays allocated beforehand, so that no host wait lies between the events; where the lists of a set would hold more than
2^28 entries the list is not run and the record says so.  Device times: torch.cuda events on the caller's stream around each form, after warm-up, the
median of the calls.  The counts alone also as a ratio to rt_query_nearest_multi with counts, K = 0 and max_dist = the half-extent."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import opengl_raytracing_amd as rt  # noqa: E402
import scenes  # noqa: E402
from query_time import primary_rays, timed  # noqa: E402

W, H = 1920, 1080
OFFSET = 0.01
EXTENTS = ((0.01, 1), (0.05, 16), (0.2, 256))       # (half-extent / root diagonal, take every n-th centre)
LIST_MAX = 1 << 28


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_time.json"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    L = rt.lib()
    nodes, tris = scenes.bunny_bvh()
    cam = scenes.camera("closeup")
    cam.aspect = W / H
    u = rt.frame_uniforms(rt.default_render_params(), cam, W, H, 1, True, nodes.shape[0], tris.shape[0], env_loaded=False)
    N = W * H
    diag = float(np.linalg.norm(nodes[0, 4:7].astype(np.float64) - nodes[0, 0:3].astype(np.float64)))
    out = []

    def record(r, **kw):
        r.update(kw)
        r["mboxes_per_s"] = r["boxes"] / (r["ms_median"] * 1e3)
        print(json.dumps(r), flush=True)
        out.append(r)
        return r

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
        uniform = ((lo + hi) * 0.5 + (torch.rand((N, 3), device=dev, generator=g) - 0.5) * 2.0 * (hi - lo)).contiguous()
        ext = torch.cuda.ExternalStream(ren.stream(), device=dev)
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

        def query(boxes, n, offsets, prims, counts, visits=None):
            cur = torch.cuda.current_stream(dev)
            ext.wait_stream(cur)
            rc = L.rt_query_boxes(ren._h, P(boxes), 6, n, P(offsets), 0, P(prims), P(counts), P(visits))
            assert rc == rt.RT_OK, L.rt_last_error(ren._h)
            cur.wait_stream(ext)

        for name, pts in (("surface points in pixel order", surface), ("surface points shuffled", shuffled), ("uniform in 2 x the root box", uniform)):
            for frac, step in EXTENTS:
                ctr = pts[::step].contiguous()
                n = ctr.shape[0]
                half = frac * diag
                boxes = torch.cat([ctr - half, ctr + half], 1).contiguous()
                counts = torch.zeros(n, dtype=torch.int32, device=dev)
                visits = torch.zeros(n, dtype=torch.int32, device=dev)
                query(boxes, n, None, None, counts, visits)
                total = int(counts.sum(dtype=torch.int64))
                stats = dict(boxes=n, half_extent=frac, count_mean=total / n, count_max=int(counts.max()), visits_mean=float(visits.double().mean()),
                             visits_max=int(visits.max()), listed=total)
                # a form that takes seconds per call is timed over fewer calls
                probe = timed(torch, lambda: query(boxes, n, None, None, counts), 1, warmup=1)
                calls = a.calls if probe["ms_median"] < 500 else 3
                limit = torch.full((n,), half, device=dev)
                near = timed(torch, lambda: ren.nearest_points_multi(ctr, 0, limit), calls)
                alone = record(timed(torch, lambda: query(boxes, n, None, None, counts), calls), case=f"the counts alone: {name}, half-extent {frac} of the diagonal", **stats)
                alone["nearest_multi_radius_count_ms"] = near["ms_median"]
                alone["over_nearest_multi_radius_count"] = alone["ms_median"] / near["ms_median"]
                print(json.dumps({"ratio to the radius count": alone["over_nearest_multi_radius_count"], "radius count ms": near["ms_median"]}), flush=True)
                if total > LIST_MAX:
                    out.append(dict(calls=0, ms_median=None, case=f"count, scan, list: {name}, half-extent {frac} of the diagonal -- not run, the lists hold "
                                                                  f"{total} entries", **stats))
                    print(json.dumps(out[-1]), flush=True)
                    continue
                offsets = torch.zeros(n + 1, dtype=torch.int32, device=dev)
                prims = torch.empty(total, dtype=torch.int32, device=dev)

                def two_pass():
                    query(boxes, n, None, None, counts)
                    offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64).to(torch.int32)
                    query(boxes, n, offsets, prims, None)

                record(timed(torch, two_pass, calls), case=f"count, scan, list: {name}, half-extent {frac} of the diagonal", **stats)
                del prims
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
