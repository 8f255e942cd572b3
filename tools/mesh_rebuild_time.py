"""Times one animation step of the dynamic mesh (rt_mesh_rebuild) against the parent route for the same step.

    python tools/mesh_rebuild_time.py [--reps N] [--out profiles/r07_mesh_rebuild.txt] [--sizes bunny,1m]

Per size (the bench mesh -- bunny stand-in, 81 920 triangles -- and the 1 M-triangle scene, where the quantised any-hit form is in use and the
rebuild pays its one allowed host wait), alternating the routes in one process, `--reps` repetitions each after warm-up:
  * parent route: host gather (rt_gather_triangles_checked) + rt_build_bvh_gpu + rt_upload_bvh, wall clock from the first call to rt_synchronize;
    and rt_build_bvh_gpu alone (it synchronises itself);
  * rt_mesh_rebuild: wall clock from the call to rt_synchronize, and device time between torch events recorded on the library stream around it.
Medians and spread (min .. max) are reported; the condition of the issue is `rebuild median wall < rt_build_bvh_gpu-alone median wall`.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import opengl_raytracing_amd as rt  # noqa: E402


def step_model(k):
    M = np.eye(4)
    c, s = np.cos(0.05 * k), np.sin(0.05 * k)
    M[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    M[:3, 3] = [0.0, 0.01 * k, 0.0]
    return np.ascontiguousarray((M @ rt.default_bvh_transform().reshape(4, 4).T).T, dtype=np.float32).reshape(-1)


def fmt(name, ms):
    return f"  {name:<52s} median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f}   max {max(ms):9.3f}   (n = {len(ms)})"


def measure(name, v, f, reps, lines):
    import torch
    dev = torch.device("cuda", 0)
    wall_parent, wall_build, wall_gather, wall_upload, wall_rebuild, dev_rebuild = [], [], [], [], [], []
    with rt.Renderer() as a, rt.Renderer() as b:
        b.mesh_upload(v, f)
        ext = torch.cuda.ExternalStream(b.stream(), device=dev)
        for k in range(-3, reps):       # k < 0: warm-up (code objects, rocPRIM's kernels, the allocator)
            M = step_model(k)
            # parent route
            a.synchronize()
            t0 = time.perf_counter()
            t9 = rt.gather_triangles(v, f, M)
            t1 = time.perf_counter()
            ng, tg = a.build_bvh_gpu(t9)
            t2 = time.perf_counter()
            a.upload_bvh(ng, tg)
            a.synchronize()
            t3 = time.perf_counter()
            # device rebuild
            b.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t4 = time.perf_counter()
            e0.record(ext)
            b.mesh_rebuild(M)
            e1.record(ext)
            b.synchronize()
            t5 = time.perf_counter()
            if k >= 0:
                wall_gather.append((t1 - t0) * 1e3); wall_build.append((t2 - t1) * 1e3); wall_upload.append((t3 - t2) * 1e3)
                wall_parent.append((t3 - t0) * 1e3); wall_rebuild.append((t5 - t4) * 1e3); dev_rebuild.append(e0.elapsed_time(e1))
        mi, si = b.mesh_info(), b.scene_info()
    lines.append(f"{name}: {np.asarray(f).size // 3} triangles, {si.nNodes} nodes; quantised any-hit form {'in use' if mi.hostSyncs else 'not in use'}")
    lines.append(fmt("parent route (gather + build_bvh_gpu + upload), wall", wall_parent))
    lines.append(fmt("  host gather, wall", wall_gather))
    lines.append(fmt("  rt_build_bvh_gpu alone, wall", wall_build))
    lines.append(fmt("  rt_upload_bvh + synchronize, wall", wall_upload))
    lines.append(fmt("rt_mesh_rebuild, wall (call .. rt_synchronize)", wall_rebuild))
    lines.append(fmt("rt_mesh_rebuild, device (events on the library stream)", dev_rebuild))
    mr, mb, mp = statistics.median(wall_rebuild), statistics.median(wall_build), statistics.median(wall_parent)
    lines.append(f"  rebuild / build_bvh_gpu alone = {mr / mb:.3f}   rebuild / parent route = {mr / mp:.4f}   (parent route / rebuild = {mp / mr:.1f}x)")
    lines.append(f"  RtMeshInfo: rebuilds {mi.rebuilds}, allocations {mi.allocations} (all in rt_mesh_upload), hostSyncs {mi.hostSyncs}, "
                 f"scratch {mi.scratchBytes / 2**20:.1f} MiB, scene {mi.sceneBytes / 2**20:.1f} MiB")
    lines.append(f"  condition (rebuild median wall < rt_build_bvh_gpu alone median wall): {'MET' if mr < mb else 'MISSED'}")
    lines.append("")
    return mr < mb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="bunny,1m")
    args = ap.parse_args()
    lines = [f"mesh_rebuild_time.py --reps {args.reps}: one animation step, routes alternated in one process, wall clock by time.perf_counter", ""]
    ok = True
    for s in args.sizes.split(","):
        v, f = rt.meshgen.bunny_standin(6) if s == "bunny" else rt.meshgen.million_triangle_scene()
        ok = measure("bench mesh" if s == "bunny" else "1 M scene", v, f, max(args.reps, 10), lines) and ok
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
