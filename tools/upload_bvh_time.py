"""Wall time of rt_upload_bvh -- host packing (csrc/rt_scene_pack.cpp) plus the copies to the device -- on the bench mesh and on the 1 M-triangle scene.

    python tools/upload_bvh_time.py [--reps N] [--sizes bunny,1m] [--out FILE]

One process, one context per size: the tree is built once on the host, then uploaded `--reps` times after two warm-up uploads.  The call synchronises
the context before it frees the previous scene and its copies are synchronous, so the host clock around the call is the whole of it.  Median with
min .. max; the environment (RT_QNODES, RT_FUSED, RT_IMPLICIT, ...) is the caller's."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import opengl_raytracing_amd as rt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="bunny,1m")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"upload_bvh_time.py --reps {args.reps}: wall time of rt_upload_bvh (call .. return), one context per size"]
    for s in [x for x in args.sizes.split(",") if x]:
        v, f = rt.meshgen.bunny_standin(6) if s == "bunny" else rt.meshgen.million_triangle_scene()
        nodes, tris = rt.build_bvh(rt.gather_triangles(v, f, np.eye(4, dtype=np.float32).reshape(-1)))
        ms = []
        with rt.Renderer() as r:
            for k in range(-2, args.reps):
                r.synchronize()
                t0 = time.perf_counter()
                r.upload_bvh(nodes, tris)
                t1 = time.perf_counter()
                if k >= 0:
                    ms.append((t1 - t0) * 1e3)
            info = r.scene_info()
        lines.append(f"  {'bench mesh' if s == 'bunny' else '1 M scene':<10s} {tris.shape[0]:8d} triangles, {info.nNodes:7d} nodes, flags {info.flags}: "
                     f"median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f}   max {max(ms):9.3f}   (n = {len(ms)})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
