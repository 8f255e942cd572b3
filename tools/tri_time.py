"""Times rt_query_tris on torch device tensors, and rt_query_boxes counting on the boxes of the same queries for orientation, in one
visit.

    python tools/tri_time.py [--calls N] [--out profiles/tri_time.json]

Scene as tools/box_time.py: the bench mesh (bunny stand-in, 81 920 triangles).  Two kinds of queries:
  * the mesh against a moved copy of itself: the mesh's own 81 920 rows as query triangles (a, b, c by the definition's adds), translated along the
    root box's diagonal by 0, 0.001, 0.01 and 0.1 of its length, in row order and shuffled;
  * many small triangles: 1920 x 1080 = 2 073 600 triangles with edges of 0.01 of the diagonal, centred on the three point sets of
    tools/nearest_time.py (surface points in pixel order, the same shuffled, uniform random points in twice the root box).
Per case: the counts alone (one call), and the exact list in two passes -- count, torch.cumsum, list -- into arrays allocated beforehand, so that no
host wait lies between the events; the mean and largest count and `visits`, the entries listed.  Beside each, rt_query_boxes counting on the queries'
[qlo, qhi] boxes, and the ratio.  Device times: torch.cuda events on the caller's stream around each form, after warm-up, the median of the calls."""
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
SHIFTS = (0.0, 0.001, 0.01, 0.1)                     # of the root diagonal
EDGE = 0.01                                          # of the root diagonal
LIST_MAX = 1 << 28


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tri_time.json"))
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

        def query(fn, q, stride, n, offsets, prims, counts, visits=None):
            cur = torch.cuda.current_stream(dev)
            ext.wait_stream(cur)
            rc = fn(ren._h, P(q), stride, n, P(offsets), 0, P(prims), P(counts), P(visits))
            assert rc == rt.RT_OK, L.rt_last_error(ren._h)
            cur.wait_stream(ext)

        def case(name, q):
            n = q.shape[0]
            boxes = torch.cat([torch.minimum(torch.minimum(q[:, 0:3], q[:, 3:6]), q[:, 6:9]), torch.maximum(torch.maximum(q[:, 0:3], q[:, 3:6]), q[:, 6:9])], 1).contiguous()
            counts = torch.zeros(n, dtype=torch.int32, device=dev)
            visits = torch.zeros(n, dtype=torch.int32, device=dev)
            bcounts = torch.zeros(n, dtype=torch.int32, device=dev)
            query(L.rt_query_tris, q, 9, n, None, None, counts, visits)
            query(L.rt_query_boxes, boxes, 6, n, None, None, bcounts)
            total, btotal = int(counts.sum(dtype=torch.int64)), int(bcounts.sum(dtype=torch.int64))
            stats = dict(queries=n, count_mean=total / n, count_max=int(counts.max()), visits_mean=float(visits.double().mean()), visits_max=int(visits.max()),
                         listed=total, box_count_mean=btotal / n)
            box = timed(torch, lambda: query(L.rt_query_boxes, boxes, 6, n, None, None, bcounts), a.calls)
            alone = record(timed(torch, lambda: query(L.rt_query_tris, q, 9, n, None, None, counts), a.calls), case=f"the counts alone: {name}", **stats)
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
                query(L.rt_query_tris, q, 9, n, None, None, counts)
                offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64).to(torch.int32)
                query(L.rt_query_tris, q, 9, n, offsets, prims, None)

            record(timed(torch, two_pass, a.calls), case=f"count, scan, list: {name}", **stats)

        # ---- the mesh against a moved copy of itself
        own = torch.from_numpy(rt.rows_as_tris(tris)).to(dev)
        g = torch.Generator(device=dev).manual_seed(5)
        perm = torch.randperm(own.shape[0], device=dev, generator=g)
        step = torch.tensor(((hi64 - lo64) / diag).astype(np.float32), device=dev)          # the unit diagonal
        for shift in SHIFTS:
            moved = (own + (step * float(shift * diag)).repeat(3)).contiguous()
            case(f"the mesh's own rows moved by {shift} of the diagonal, in row order", moved)
            case(f"the mesh's own rows moved by {shift} of the diagonal, shuffled", moved[perm].contiguous())
        del own, moved
        # ---- many small triangles about the three point sets
        o, d = primary_rays(torch, u, W, H, dev)
        hits = ren.trace_rays(o, d, normals=True, eps=u.eps, inf=u.inf)
        hit = hits.prim >= 0
        at = torch.cummax(torch.where(hit, torch.arange(N, device=dev), torch.full((N,), -1, device=dev)), 0).values
        at = torch.where(at >= 0, at, torch.nonzero(hit)[0, 0])              # pixels before the first hit take the first
        surface = (o + d * hits.t[:, None] + hits.normal * OFFSET)[at].contiguous()
        del hits, o, d
        shuffled = surface[torch.randperm(N, device=dev, generator=g)].contiguous()
        lo, hi = (torch.tensor(nodes[0, k:k + 3], device=dev) for k in (0, 4))
        uniform = ((lo + hi) * 0.5 + (torch.rand((N, 3), device=dev, generator=g) - 0.5) * 2.0 * (hi - lo)).contiguous()
        # one shape for all: three points on a circle of radius edge / sqrt(3) about the centre, in a random plane
        r = EDGE * diag / np.sqrt(3.0)
        for name, pts in (("surface points in pixel order", surface), ("surface points shuffled", shuffled), ("uniform in 2 x the root box", uniform)):
            e1 = torch.nn.functional.normalize(torch.randn((N, 3), device=dev, generator=g), dim=1)
            e2 = torch.nn.functional.normalize(torch.linalg.cross(e1, torch.randn((N, 3), device=dev, generator=g)), dim=1)
            corners = [pts + r * (np.cos(t) * e1 + np.sin(t) * e2) for t in (0.0, 2 * np.pi / 3, 4 * np.pi / 3)]
            case(f"small triangles, edge {EDGE} of the diagonal: {name}", torch.cat(corners, 1).contiguous())
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
