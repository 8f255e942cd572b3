"""Times what keeping per-vertex colours of the dynamic mesh adds to an update, the hit query, and a frame shaded with them.

    python tools/mesh_colors_time.py [--reps N] [--sizes bunny,1m] [--frames N] [--out profiles/r22_mesh_colors.txt]

Per size (the bench mesh -- bunny stand-in, 81 920 triangles -- and the 1 M-triangle scene), in one process and on one context, device time between
events recorded on the library stream around the call, the positions rewritten before every step:
  - rt_mesh_refit and rt_mesh_rebuild with colours disabled, then enabled (random colours): the difference is k_corner_rows<ColorAttr> (and the order array,
    which a rebuild, and the first refit behind one, derives for itself);
  - rt_mesh_colors_refresh, the gather alone;
  - rt_mesh_hit_colors on the hits of a 1920 x 1080 pick, device tensors.
Frame cost (--frames, bench mesh only): one 1080p / 4 spp frame behind a refit, wall time from the call to the return of rt_synchronize, on two
contexts that differ only in rt_mesh_colors_enable (random colours), alternated.
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
    W, H = 1920, 1080
    with rt.Renderer() as b:
        b.resize(W, H)
        b.mesh_upload(v, f)
        b.mesh_rebuild(M)
        stream = torch.cuda.ExternalStream(b.stream(), device=dev)
        lines.append(f"{name}: {n} triangles, {v.shape[0]} vertices; {(v.shape[0] * 16 + n * 48) / 1e6:.2f} MB for the two arrays")
        colors = np.random.default_rng(1).uniform(0.05, 1.0, (v.shape[0], 3)).astype(np.float32)
        move = lambda k: b.mesh_set_positions(poses[k % 2])      # noqa: E731
        med = {}
        for on in (False, True):
            b.mesh_colors_enable(on)
            if on:
                b.mesh_set_colors(colors)
            tag = "colours on " if on else "colours off"
            for what, call in (("rt_mesh_refit", lambda: b.mesh_refit(M)), ("rt_mesh_rebuild", lambda: b.mesh_rebuild(M))):
                ms = timed(b, stream, reps, move, call)
                med[(what, on)] = statistics.median(ms)
                lines.append(fmt(f"{what}, {tag}, device", ms))
        for what in ("rt_mesh_refit", "rt_mesh_rebuild"):
            off, on = med[(what, False)], med[(what, True)]
            lines.append(f"    {what}: colours add {on - off:+.4f} ms ({(on / off - 1) * 100:+.1f} %)")
        lines.append(fmt("rt_mesh_colors_refresh, device", timed(b, stream, reps, lambda k: None, b.mesh_colors_refresh)))
        L = rt.bvh_layout(n)
        cam = rt.closeup_camera()
        cam.aspect = W / H
        u = rt.frame_uniforms(rt.default_render_params(), cam, W, H, 0, True, L.nNodes, L.nTris, env_loaded=False)
        xy = torch.from_numpy(np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)).to(dev)
        h = b.pick(u, xy, normals=False, points=False)
        torch.cuda.synchronize()
        hits = int((h.prim >= 0).sum().item())
        lines.append(fmt(f"rt_mesh_hit_colors, {W * H} records ({hits} hits), device", timed(b, stream, reps, lambda k: None, lambda: b.mesh_hit_colors(h.record))))
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
    ctx = {}
    colors = np.random.default_rng(1).uniform(0.05, 1.0, (v.shape[0], 3)).astype(np.float32)
    for on in (False, True):
        b = rt.Renderer()
        b.resize(W, H)
        b.mesh_upload(v, f)
        if on:
            b.mesh_colors_enable()
            b.mesh_set_colors(colors)
        b.mesh_rebuild(M)
        ctx[on] = b
    ms = {False: [], True: []}
    for k in range(-3, reps):
        for on in (False, True):
            b = ctx[on]
            b.mesh_set_positions(poses[k % 2])
            b.mesh_refit(M)
            u = rt.frame_uniforms(p, cam, W, H, k + 3, True, L.nNodes, L.nTris, env_loaded=False)
            b.synchronize()
            t0 = time.perf_counter()
            b.render_frame(u)
            b.synchronize()
            if k >= 0:
                ms[on].append((time.perf_counter() - t0) * 1e3)
    for b in ctx.values():
        b.close()
    lines.append(f"frame cost: bench mesh, {W} x {H}, 4 spp, behind a refit; rt_render_frame + rt_synchronize, wall, contexts alternated")
    lines.append(fmt("colours off", ms[False]))
    lines.append(fmt("colours on", ms[True]))
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    lines.append(f"    colours add {on - off:+.4f} ms ({(on / off - 1) * 100:+.2f} %); spread of the colours-off frames {max(ms[False]) - min(ms[False]):.4f} ms")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--frames", type=int, default=20, help="repetitions of the frame-cost measurement (0: skip it)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="bunny,1m")
    args = ap.parse_args()
    lines = [f"mesh_colors_time.py --reps {args.reps} --frames {args.frames}: one context per size, one process", ""]
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
