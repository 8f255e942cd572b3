"""Times rt_mesh_morph against the only path a host that links the library alone had before it: blend on the CPU and push every
vertex through rt_mesh_set_positions.

    python tools/mesh_morph_time.py [--reps N] [--sizes bunny,1m] [--out profiles/r17_mesh_morph.txt]
    python tools/mesh_morph_time.py --baseline-only [...]      # only calls older than the morph: the same figures from a checkout without it

Per size (the bench mesh -- bunny stand-in, 81 920 triangles -- and the 1 M-triangle scene), in one process and on one context:
  - rt_mesh_set_positions + rt_synchronize, wall time from the call to the return of the synchronise: the cheapest leg of the host route (the CPU
    blend in front of it is not counted);
  - a device-to-device copy of the positions on the library stream, device time between events: the traffic floor of any kernel that rewrites them;
  - per configuration, rt_mesh_morph to the positions under a weight table that changes every step (written on the device), device time between
    events recorded on the library stream around the call.  Configurations: 64 targets that each touch 10 % of the vertices, as windows of the
    vertex array (regions: neighbours in memory share targets) and as random subsets (scattered: the padding of the sliced layout shows); one
    dense target.
`--reps` repetitions each after three of warm-up; medians with min .. max.  Reported per configuration, without a bound: the bytes the kernel must
move (padded records x 16 + 24 per vertex), the padding ratio paddedEntries / entries, and the bytes per second the median amounts to.
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


def fmt(name, ms):
    return f"  {name:<58s} median {statistics.median(ms):9.4f} ms   min {min(ms):9.4f}   max {max(ms):9.4f}   (n = {len(ms)})"


def targets(nv, kind):
    """(target_first, vert_idx, deltas) of one configuration"""
    rng = np.random.default_rng(nv)
    if kind == "dense":
        sets = [np.arange(nv)]
    elif kind == "regions":
        sets = [(np.arange(nv // 10) + (t * nv) // 64) % nv for t in range(64)]
    else:
        sets = [np.sort(rng.choice(nv, nv // 10, replace=False)) for _ in range(64)]
    first = np.concatenate([[0], np.cumsum([s.size for s in sets])]).astype(np.int32)
    vi = np.concatenate(sets).astype(np.uint32)
    return first, vi, rng.normal(0, 0.01, (vi.size, 3)).astype(np.float32)


def measure(name, v, f, kinds, reps, lines, baseline_only):
    import torch
    dev = torch.device("cuda", 0)
    v = np.ascontiguousarray(v, np.float32)
    nv = v.shape[0]
    other = (v * np.float32(1.001)).astype(np.float32)
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        stream = torch.cuda.ExternalStream(b.stream(), device=dev)
        lines.append(f"{name}: {nv} vertices ({nv * 12 / 1e6:.2f} MB of positions), {np.asarray(f).size // 3} triangles")
        wall = []
        for k in range(-3, reps):       # k < 0: warm-up
            b.synchronize()
            t0 = time.perf_counter()
            b.mesh_set_positions(other if k % 2 else v)
            b.synchronize()
            if k >= 0:
                wall.append((time.perf_counter() - t0) * 1e3)
        lines.append(fmt("rt_mesh_set_positions + rt_synchronize, wall", wall))
        base = statistics.median(wall)
        copy = []
        scratch = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for k in range(-3, reps):
            b.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                scratch.copy_(b.mesh_positions())
                e1.record(stream)
            b.synchronize()
            if k >= 0:
                copy.append(e0.elapsed_time(e1))
        lines.append(fmt("device-to-device copy of the positions, device", copy))
        floor = statistics.median(copy)
        for kind in ([] if baseline_only else kinds):
            tf, vi, d = targets(nv, kind)
            nt = tf.size - 1
            b.mesh_morph_upload(tf, vi, d, base=v)
            info = b.mesh_morph_info()
            tables = [torch.from_numpy(np.random.default_rng(k).uniform(0.1, 1.0, (nt, 1)).astype(np.float32)).to(dev) for k in range(4)]
            torch.cuda.synchronize()
            morph = []
            for k in range(-3, reps):
                with torch.cuda.stream(stream):
                    b.mesh_morph_weights().copy_(tables[k % 4])
                b.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                b.mesh_morph()
                e1.record(stream)
                b.synchronize()
                if k >= 0:
                    morph.append(e0.elapsed_time(e1))
            med = statistics.median(morph)
            must = info.paddedEntries * 16 + 24 * nv
            lines.append(fmt(f"rt_mesh_morph, {kind}: {nt} targets, {info.entries} entries, device", morph))
            lines.append(f"    at most {info.maxPerVertex} entries per vertex; padded records {info.paddedEntries} (padding ratio {info.paddedEntries / max(info.entries, 1):.3f}); "
                         f"bytes to move {must / 1e6:.2f} MB -> {must / (med * 1e-3) / 1e9:.1f} GB/s at the median; set_positions / morph {base / med:.1f}x   "
                         f"morph / copy {med / floor:.2f}")
        mi = b.mesh_info()
        lines.append(f"  RtMeshInfo: allocations {mi.allocations}, hostSyncs {mi.hostSyncs}")
        lines.append("")
        torch.cuda.current_stream(dev).wait_stream(stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="bunny,1m")
    ap.add_argument("--configs", default="regions,scattered,dense")
    ap.add_argument("--baseline-only", action="store_true", help="time rt_mesh_set_positions and the copy only: runs on a checkout without rt_mesh_morph")
    args = ap.parse_args()
    lines = [f"mesh_morph_time.py --reps {args.reps} --configs {args.configs}{' --baseline-only' if args.baseline_only else ''}: one context per size, one process", ""]
    for s in [x for x in args.sizes.split(",") if x]:
        v, f = rt.meshgen.bunny_standin(6) if s == "bunny" else rt.meshgen.million_triangle_scene()
        measure("bench mesh" if s == "bunny" else "1 M scene", v, f, [x for x in args.configs.split(",") if x], max(args.reps, 1), lines, args.baseline_only)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
