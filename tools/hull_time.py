"""Times rt_pick_rects and rt_query_hulls on torch device tensors, and rt_query_boxes counting on the hulls' [lo, hi] for orientation, in
one visit.

    python tools/hull_time.py [--calls N] [--out profiles/hull_time.json]

Scene as tools/tri_time.py: the bench mesh (bunny stand-in, 81 920 triangles) in the close-up camera's 1920 x 1080 view.  Two kinds of queries:
  * rect frusta: the frame tiled by squares of 1, 8 and 64 pixels (2 073 600, 32 400 and 510 rects; where the width does not divide the frame the
    last row reaches past it), from the eye to the far side of the scene, in pixel order and shuffled -- through rt_pick_rects, which makes the
    frusta on the device first;
  * oriented boxes: 2 073 600 boxes with half-extents of 0.005 of the root diagonal, turned at random, about the surface points of
    tools/nearest_time.py (in pixel order and shuffled) -- through rt_query_hulls.
Per case: the counts alone (one call), and the exact list in two passes -- count, torch.cumsum, list -- into arrays allocated beforehand, so that no
host wait lies between the events; the mean and largest count and `visits`, the entries listed.  Beside each, rt_query_boxes counting on the hulls'
[lo, hi] boxes with its `visits`: what the six-normal node test saves in visits, and the ratio of the times.  Device times: torch.cuda events on the
caller's stream around each form, after warm-up, the median of the calls."""
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
WIDTHS = (1, 8, 64)                                  # pixels
HALF = 0.005                                         # of the root diagonal
LIST_MAX = 1 << 28


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hull_time.json"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    L = rt.lib()
    nodes, tris = scenes.bunny_bvh()
    cam = scenes.camera("closeup")
    cam.aspect = W / H
    u = rt.frame_uniforms(rt.default_render_params(), cam, W, H, 1, True, nodes.shape[0], tris.shape[0], env_loaded=False)
    N = W * H
    lo64, hi64 = nodes[0, 0:3].astype(np.float64), nodes[0, 4:7].astype(np.float64)
    diag = float(np.linalg.norm(hi64 - lo64))
    out = []

    def record(r, **kw):
        r.update(kw)
        r["mqueries_per_s"] = r["queries"] / (r["ms_median"] * 1e3)
        print(json.dumps(r), flush=True)
        out.append(r)
        return r

    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        ext = torch.cuda.ExternalStream(ren.stream(), device=dev)
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

        def ordered(call):
            cur = torch.cuda.current_stream(dev)
            ext.wait_stream(cur)
            assert call() == rt.RT_OK, L.rt_last_error(ren._h)
            cur.wait_stream(ext)

        def boxes_q(boxes, n, counts, visits=None):
            ordered(lambda: L.rt_query_boxes(ren._h, P(boxes), 6, n, None, 0, None, P(counts), P(visits)))

        def case(name, n, hulls_q, corners):
            """hulls_q(offsets, prims, counts, visits): the query in one of its forms; corners: the hulls [n,24], filled by the first call."""
            counts = torch.zeros(n, dtype=torch.int32, device=dev)
            visits = torch.zeros(n, dtype=torch.int32, device=dev)
            bcounts = torch.zeros(n, dtype=torch.int32, device=dev)
            bvisits = torch.zeros(n, dtype=torch.int32, device=dev)
            hulls_q(None, None, counts, visits)
            c = corners.reshape(n, 8, 3)
            boxes = torch.cat([c.min(1).values, c.max(1).values], 1).contiguous()
            boxes_q(boxes, n, bcounts, bvisits)
            total, btotal = int(counts.sum(dtype=torch.int64)), int(bcounts.sum(dtype=torch.int64))
            stats = dict(queries=n, count_mean=total / n, count_max=int(counts.max()), visits_mean=float(visits.double().mean()), visits_max=int(visits.max()),
                         listed=total, box_count_mean=btotal / n, box_visits_mean=float(bvisits.double().mean()), box_visits_max=int(bvisits.max()))
            stats["visits_over_box_visits"] = stats["visits_mean"] / max(stats["box_visits_mean"], 1e-9)
            box = timed(torch, lambda: boxes_q(boxes, n, bcounts), a.calls)
            alone = record(timed(torch, lambda: hulls_q(None, None, counts, None), a.calls), case=f"the counts alone: {name}", **stats)
            alone["box_counts_ms"] = box["ms_median"]
            alone["over_box_counts"] = alone["ms_median"] / box["ms_median"]
            print(json.dumps({"box counts ms": box["ms_median"], "ratio to the box counts": alone["over_box_counts"]}), flush=True)
            if total > LIST_MAX:
                out.append(dict(calls=0, ms_median=None, case=f"count, scan, list: {name} -- not run, the lists hold {total} entries", **stats))
                print(json.dumps(out[-1]), flush=True)
                return
            offsets = torch.zeros(n + 1, dtype=torch.int32, device=dev)
            prims = torch.empty(max(total, 1), dtype=torch.int32, device=dev)

            def two_pass():
                hulls_q(None, None, counts, None)
                offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64).to(torch.int32)
                hulls_q(offsets, prims, None, None)

            record(timed(torch, two_pass, a.calls), case=f"count, scan, list: {name}", **stats)

        g = torch.Generator(device=dev).manual_seed(5)
        # ---- rect frusta: the frame tiled by squares, from the eye to the far side of the scene
        for w in WIDTHS:
            ys, xs = torch.meshgrid(torch.arange(0, H, w, device=dev, dtype=torch.float32), torch.arange(0, W, w, device=dev, dtype=torch.float32), indexing="ij")
            tiles = torch.stack([xs, ys, xs + w, ys + w], -1).reshape(-1, 4).contiguous()
            n = tiles.shape[0]
            for order, rects in (("in pixel order", tiles), ("shuffled", tiles[torch.randperm(n, device=dev, generator=g)].contiguous())):
                corners = torch.zeros((n, 24), dtype=torch.float32, device=dev)

                def rects_q(offsets, prims, counts, visits, rects=rects, corners=corners, n=n):
                    ordered(lambda: L.rt_pick_rects(ren._h, C.byref(u), P(rects), 4, n, 0.0, -1.0, P(corners), P(offsets), 0, P(prims), P(counts), P(visits)))

                case(f"rect frusta of {w} x {w} pixels, {order}", n, rects_q, corners)
        # ---- oriented boxes about surface points
        o, d = primary_rays(torch, u, W, H, dev)
        hits = ren.trace_rays(o, d, normals=True, eps=u.eps, inf=u.inf)
        hit = hits.prim >= 0
        at = torch.cummax(torch.where(hit, torch.arange(N, device=dev), torch.full((N,), -1, device=dev)), 0).values
        at = torch.where(at >= 0, at, torch.nonzero(hit)[0, 0])              # pixels before the first hit take the first
        surface = (o + d * hits.t[:, None] + hits.normal * OFFSET)[at].contiguous()
        del hits, o, d
        shuffled = surface[torch.randperm(N, device=dev, generator=g)].contiguous()
        for name, pts in (("surface points in pixel order", surface), ("surface points shuffled", shuffled)):
            e1 = torch.nn.functional.normalize(torch.randn((N, 3), device=dev, generator=g), dim=1)
            e2 = torch.nn.functional.normalize(torch.linalg.cross(e1, torch.randn((N, 3), device=dev, generator=g)), dim=1)
            e3 = torch.linalg.cross(e1, e2)
            h = HALF * diag
            hulls = torch.cat([pts + h * ((1 if k & 1 else -1) * e1 + (1 if k & 2 else -1) * e2 + (1 if k & 4 else -1) * e3) for k in range(8)], 1).contiguous()
            del e1, e2, e3

            def hulls_q(offsets, prims, counts, visits, hulls=hulls):
                ordered(lambda: L.rt_query_hulls(ren._h, P(hulls), 24, N, P(offsets), 0, P(prims), P(counts), P(visits)))

            case(f"oriented boxes, half-extent {HALF} of the diagonal: {name}", N, hulls_q, hulls)
            del hulls
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
