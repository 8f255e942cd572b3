"""Times what keeping the previous pose of the dynamic mesh adds to an update and to a frame.

    python tools/mesh_motion_time.py [--reps N] [--sizes bunny,1m] [--frames N] [--out profiles/r20_mesh_motion.txt]

Per size (the bench mesh -- bunny stand-in, 81 920 triangles -- and the 1 M-triangle scene), in one process and on one context, device time between
events recorded on the library stream around the call, the positions rewritten before every step:
  - a device-to-device copy of the triangle array (nTris x 48 bytes): the traffic floor of anything that keeps a second copy of the rows;
  - rt_mesh_refit and rt_mesh_rebuild with motion disabled, then with motion enabled (the refit copies the rows it is about to rewrite; the rebuild
    files the old rows by input triangle before its sorts and hands them out in the new order behind them), and rt_mesh_motion_latch.
Frame cost (--frames, bench mesh only): one 1080p / 4 spp frame with cameraMoved = 1 behind a refit, wall time from the call to the return of
rt_synchronize, on two contexts that differ only in rt_mesh_motion_enable, alternated.
`--reps` repetitions each after three of warm-up; medians with min .. max.  There is no condition: the figures are reported."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import opengl_raytracing_amd as rt  # noqa: E402


def fmt(name, ms):
    return f"  {name:<58s} median {statistics.median(ms):9.4f} ms   min {min(ms):9.4f}   max {max(ms):9.4f}   (n = {len(ms)})"


def timed(b, stream, reps, before, call):
    import torch
    out = []
    for k in range(-3, reps):       # k < 0: warm-up
        before(k)
        b.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        b.synchronize()
        if k >= 0:
            out.append(e0.elapsed_time(e1))
    return out


def measure(name, v, f, reps, lines):
    import torch
    dev = torch.device("cuda", 0)
    v = np.ascontiguousarray(v, np.float32)
    n = np.asarray(f).size // 3
    poses = [v, (v * np.float32(1.01) + np.float32(0.003)).astype(np.float32)]
    M = rt.default_bvh_transform()
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_rebuild(M)
        stream = torch.cuda.ExternalStream(b.stream(), device=dev)
        lines.append(f"{name}: {n} triangles ({n * 48 / 1e6:.2f} MB of rows), {v.shape[0]} vertices")
        src = torch.empty(n * 12, dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)
        torch.cuda.synchronize()

        def copy():
            with torch.cuda.stream(stream):
                dst.copy_(src)
        floor = timed(b, stream, reps, lambda k: None, copy)
        lines.append(fmt("device-to-device copy of nTris x 48 bytes, device", floor))
        move = lambda k: b.mesh_set_positions(poses[k % 2])      # noqa: E731
        med = {}
        for motion in (False, True):
            b.mesh_motion_enable(motion)
            tag = "motion on " if motion else "motion off"
            for what, call in (("rt_mesh_refit", lambda: b.mesh_refit(M)), ("rt_mesh_rebuild", lambda: b.mesh_rebuild(M))):
                ms = timed(b, stream, reps, move, call)
                med[(what, motion)] = statistics.median(ms)
                lines.append(fmt(f"{what}, {tag}, device", ms))
        lines.append(fmt("rt_mesh_motion_latch, device", timed(b, stream, reps, lambda k: None, b.mesh_motion_latch)))
        fl = statistics.median(floor)
        for what in ("rt_mesh_refit", "rt_mesh_rebuild"):
            off, on = med[(what, False)], med[(what, True)]
            lines.append(f"    {what}: motion adds {on - off:+.4f} ms ({(on / off - 1) * 100:+.1f} %), {(on - off) / fl:.2f} copies of the triangle array")
        mi = b.mesh_info()
        lines.append(f"  RtMeshInfo: allocations {mi.allocations}, hostSyncs {mi.hostSyncs}, scratchBytes {mi.scratchBytes}")
        lines.append("")
        torch.cuda.current_stream(dev).wait_stream(stream)


def frame_cost(reps, lines):
    W, H = 1920, 1080
    v, f = rt.meshgen.bunny_standin(6)
    v = np.ascontiguousarray(v, np.float32)
    poses = [v, (v * np.float32(1.01) + np.float32(0.003)).astype(np.float32)]
    M = rt.default_bvh_transform()
    L = rt.bvh_layout(np.asarray(f).size // 3)
    p = rt.default_render_params()
    p.sppPerFrame = 4
    cam = rt.closeup_camera()
    cam.aspect = W / H
    before = rt.closeup_camera()
    before.aspect = W / H
    before.pos[2] += 0.05
    prev = rt.mat4_mul(rt.camera_proj(before), rt.camera_view(before))
    ctx = {}
    for motion in (False, True):
        b = rt.Renderer()
        b.resize(W, H)
        b.mesh_upload(v, f)
        b.mesh_motion_enable(motion)
        b.mesh_rebuild(M)
        ctx[motion] = b
    ms = {False: [], True: []}
    for k in range(-3, reps):
        for motion in (False, True):
            b = ctx[motion]
            b.mesh_set_positions(poses[k % 2])
            b.mesh_refit(M)
            u = rt.frame_uniforms(p, cam, W, H, k + 3, True, L.nNodes, L.nTris, prev_vp=prev, env_loaded=False)
            b.synchronize()
            t0 = time.perf_counter()
            b.render_frame(u)
            b.synchronize()
            if k >= 0:
                ms[motion].append((time.perf_counter() - t0) * 1e3)
    for b in ctx.values():
        b.close()
    lines.append(f"frame cost: bench mesh, {W} x {H}, 4 spp, cameraMoved = 1, behind a refit; rt_render_frame + rt_synchronize, wall, contexts alternated")
    lines.append(fmt("motion off", ms[False]))
    lines.append(fmt("motion on", ms[True]))
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    lines.append(f"    motion adds {on - off:+.4f} ms ({(on / off - 1) * 100:+.2f} %); spread of the motion-off frames {max(ms[False]) - min(ms[False]):.4f} ms")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--frames", type=int, default=20, help="repetitions of the frame-cost measurement (0: skip it)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="bunny,1m")
    args = ap.parse_args()
    lines = [f"mesh_motion_time.py --reps {args.reps} --frames {args.frames}: one context per size, one process", ""]
    for s in [x for x in args.sizes.split(",") if x]:
        v, f = rt.meshgen.bunny_standin(6) if s == "bunny" else rt.meshgen.million_triangle_scene()
        measure("bench mesh" if s == "bunny" else "1 M scene", v, f, max(args.reps, 1), lines)
    if args.frames > 0:
        frame_cost(args.frames, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
