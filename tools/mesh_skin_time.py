"""Times rt_mesh_skin against the only path a host that links the library alone had before it: deform on the CPU and push every
vertex through rt_mesh_set_positions.

    python tools/mesh_skin_time.py [--reps N] [--bones 1,64,4096] [--sizes bunny,1m] [--out profiles/r16_mesh_skin.txt]
    python tools/mesh_skin_time.py --baseline-only [...]      # only calls older than the skin: the same figures from a checkout without it

Per size (the bench mesh -- bunny stand-in, 81 920 triangles -- and the 1 M-triangle scene), in one process and on one context:
  - rt_mesh_set_positions + rt_synchronize, wall time from the call to the return of the synchronise: the cheapest leg of the host route (the CPU
    skinning in front of it is not counted);
  - a device-to-device copy of the positions on the library stream, device time between events: the traffic floor of any kernel that rewrites them;
  - per bone count, rt_mesh_skin under a bone table that changes every step (written on the device), device time between events recorded on the
    library stream around the call.  Every vertex has four influences of non-zero weight on neighbouring bones.
`--reps` repetitions each after three of warm-up; medians with min .. max.
Condition of the issue, per size and bone count: the skin's median device time is below the set_positions median (no margin: the baseline already
omits the CPU work).  skin / copy is recorded without a bound.
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


def skin_tables(nv, nb):
    """Four influences per vertex on the bones next to vertex * nb / nv, weights normalised: vertices that are neighbours in memory share bones, as
    the vertices of a skinned model do."""
    rng = np.random.default_rng(nv + nb)
    first = (np.arange(nv, dtype=np.int64) * nb) // nv
    bi = np.minimum(first[:, None] + np.arange(4)[None, :], nb - 1).astype(np.uint16)
    w = rng.uniform(0.1, 1.0, (nv, 4)).astype(np.float32)
    return bi, (w / w.sum(1, keepdims=True)).astype(np.float32)


def bone_tables(nb, k):
    """[nb,16] column-major: a small rotation about y and a translation, distinct per bone, another at every step k."""
    b = np.arange(nb, dtype=np.float64)
    ang = 0.02 * (k + 1) * (1.0 + b % 7) + 0.001 * b
    c, s = np.cos(ang), np.sin(ang)
    M = np.zeros((nb, 4, 4))
    M[:, 0, 0], M[:, 0, 2], M[:, 2, 0], M[:, 2, 2], M[:, 1, 1], M[:, 3, 3] = c, s, -s, c, 1.0, 1.0
    M[:, 0, 3], M[:, 1, 3] = 0.01 * (b % 5), 0.005 * ((b + k) % 3)
    return np.ascontiguousarray(np.transpose(M, (0, 2, 1)), np.float32).reshape(nb, 16)


def measure(name, v, f, bone_counts, reps, lines, baseline_only):
    import torch
    dev = torch.device("cuda", 0)
    v = np.ascontiguousarray(v, np.float32)
    nv = v.shape[0]
    other = (v * np.float32(1.001)).astype(np.float32)
    ok = True
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
        for nb in ([] if baseline_only else bone_counts):
            bi, w = skin_tables(nv, nb)
            b.mesh_skin_upload(bi, w, nb, rest=v)
            tables = [torch.from_numpy(bone_tables(nb, k)).to(dev) for k in range(4)]
            torch.cuda.synchronize()
            skin = []
            for k in range(-3, reps):
                with torch.cuda.stream(stream):
                    b.mesh_bones().copy_(tables[k % 4])
                b.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                b.mesh_skin()
                e1.record(stream)
                b.synchronize()
                if k >= 0:
                    skin.append(e0.elapsed_time(e1))
            med = statistics.median(skin)
            met = med < base
            ok = ok and met
            lines.append(fmt(f"rt_mesh_skin, {nb} bones, device (events on the library stream)", skin))
            lines.append(f"    set_positions / skin {base / med:.1f}x   skin / copy {med / floor:.2f}   condition (skin median {med:.4f} < set_positions median "
                         f"{base:.4f}): {'MET' if met else 'MISSED'}")
        mi = b.mesh_info()
        lines.append(f"  RtMeshInfo: allocations {mi.allocations} (rt_mesh_upload and rt_mesh_skin_upload), hostSyncs {mi.hostSyncs}")
        lines.append("")
        torch.cuda.current_stream(dev).wait_stream(stream)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="bunny,1m")
    ap.add_argument("--bones", default="1,64,4096")
    ap.add_argument("--baseline-only", action="store_true", help="time rt_mesh_set_positions and the copy only: runs on a checkout without rt_mesh_skin")
    args = ap.parse_args()
    lines = [f"mesh_skin_time.py --reps {args.reps} --bones {args.bones}{' --baseline-only' if args.baseline_only else ''}: one context per size, one process", ""]
    ok = True
    for s in [x for x in args.sizes.split(",") if x]:
        v, f = rt.meshgen.bunny_standin(6) if s == "bunny" else rt.meshgen.million_triangle_scene()
        ok = measure("bench mesh" if s == "bunny" else "1 M scene", v, f, [int(x) for x in args.bones.split(",")], max(args.reps, 1), lines, args.baseline_only) and ok
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
