"""Times rt_mesh_refit against rt_mesh_rebuild on the same animation step, and what frames cost on a tree that is refitted
instead of rebuilt.

    python tools/mesh_refit_time.py [--reps N] [--out profiles/r09_mesh_refit.txt] [--sizes bunny,1m | none] [--no-frames]
    python tools/mesh_refit_time.py --parts 1,64,4096 [--reps N] [--out profiles/r10_mesh_parts.txt] [--sizes bunny,1m]
    python tools/mesh_refit_time.py --quality [--reps N] [--out profiles/r12_mesh_quality.txt] [--sizes bunny,1m] [--no-frames]

Per size (the bench mesh -- bunny stand-in, 81 920 triangles -- and the 1 M-triangle scene, where the quantised any-hit form is in use and both
calls pay their one host wait), in one process and on one context: every step displaces the positions on the device, then runs rt_mesh_rebuild
and rt_mesh_refit over those positions, alternated, `--reps` repetitions each after warm-up.  Device time between torch events recorded on the
library stream around the call; wall time from the call to the return of rt_synchronize.  Medians with min .. max.
Condition of the issue: the refit's median device time is below the rebuild's and its whole range lies below the rebuild's minimum.

Informational (bench mesh only): ms per frame of the bench view (1920x1080, 4 spp, close-up camera, wavefront pipeline) on the tree after 1, 8
and 32 refit steps of the animation, and after random per-vertex displacements, against a tree rebuilt over the same positions on a second
context -- the price of not rebuilding.

--parts N[,N ...] measures the part-aware calls instead: per size and N, the mesh split into N equal parts with a distinct rigid
matrix per part that changes every step (written into the device table on the library stream), and rt_mesh_refit / rt_mesh_refit_parts /
rt_mesh_rebuild / rt_mesh_rebuild_parts alternated on one context.  Conditions: the refit_parts median is below the rebuild median and its whole
range below the rebuild minimum; the rebuild_parts median is at most the rebuild median plus that rebuild's own (max - min) spread of the run.
refit_parts / refit is recorded without a bound.

--quality measures the tree-quality path: per size, rt_mesh_rebuild, rt_mesh_refit, rt_mesh_refit + rt_mesh_measure and
rt_mesh_measure alone, alternated on one context.  Condition: the refit + measure median is below the rebuild median and its whole range below the
rebuild minimum.  Then (bench mesh only, unless --no-frames) the table of cost ratio against ms per frame: for the deformations of the frames table
above plus four interleaved parts drifting apart, the refitted and the rebuilt tree's cost over the cost of the first build (rt_mesh_quality) beside
their ms per frame.
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
import scenes  # noqa: E402


def step_delta(pos, ext, k):
    """One step of the test animation: a smooth displacement of 3 % of the mesh's extent (tests/test_gpu_mesh_refit.py::_sinus)."""
    return (np.float32(0.03) * ext * np.sin(np.float32(3.0) * pos / ext + np.float32(0.7 + k))).astype(np.float32)


def fmt(name, ms):
    return f"  {name:<52s} median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f}   max {max(ms):9.3f}   (n = {len(ms)})"


def measure(name, v, f, reps, lines):
    import torch
    dev = torch.device("cuda", 0)
    v = np.ascontiguousarray(v, np.float32)
    ext = np.float32((v.max(0) - v.min(0)).max())
    M = rt.default_bvh_transform()
    t = {k: [] for k in ("dev_rebuild", "wall_rebuild", "dev_refit", "wall_refit")}
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        stream = torch.cuda.ExternalStream(b.stream(), device=dev)
        delta = torch.from_numpy(step_delta(v, ext, 0) * np.float32(0.1)).to(dev)
        torch.cuda.synchronize()

        def timed(call, what, keep):
            b.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            call(M)
            e1.record(stream)
            b.synchronize()
            t1 = time.perf_counter()
            if keep:
                t["wall_" + what].append((t1 - t0) * 1e3); t["dev_" + what].append(e0.elapsed_time(e1))

        for k in range(-3, reps):       # k < 0: warm-up (code objects, rocPRIM's kernels)
            with torch.cuda.stream(stream):
                b.mesh_positions().add_(delta if k % 2 else -delta)
            timed(b.mesh_rebuild, "rebuild", k >= 0)
            timed(b.mesh_refit, "refit", k >= 0)
        mi, si = b.mesh_info(), b.scene_info()
        total, _ = b.mesh_refit_count()
        torch.cuda.current_stream(dev).wait_stream(stream)
    lines.append(f"{name}: {np.asarray(f).size // 3} triangles, {si.nNodes} nodes, {si.treeDepth} levels; quantised any-hit form "
                 f"{'in use (one host wait per call)' if mi.hostSyncs else 'not in use (no host wait)'}")
    lines.append(fmt("rt_mesh_rebuild, device (events on the library stream)", t["dev_rebuild"]))
    lines.append(fmt("rt_mesh_refit,   device (events on the library stream)", t["dev_refit"]))
    lines.append(fmt("rt_mesh_rebuild, wall (call .. rt_synchronize)", t["wall_rebuild"]))
    lines.append(fmt("rt_mesh_refit,   wall (call .. rt_synchronize)", t["wall_refit"]))
    dr, df = statistics.median(t["dev_rebuild"]), statistics.median(t["dev_refit"])
    wr, wf = statistics.median(t["wall_rebuild"]), statistics.median(t["wall_refit"])
    ok = df < dr and max(t["dev_refit"]) < min(t["dev_rebuild"])
    lines.append(f"  rebuild / refit: device {dr / df:.1f}x   wall {wr / wf:.1f}x      RtMeshInfo: rebuilds {mi.rebuilds}, refits {total}, allocations "
                 f"{mi.allocations} (all in rt_mesh_upload), hostSyncs {mi.hostSyncs}")
    lines.append(f"  condition (refit median < rebuild median, refit max {max(t['dev_refit']):.3f} < rebuild min {min(t['dev_rebuild']):.3f}, device): "
                 f"{'MET' if ok else 'MISSED'}")
    lines.append("")
    return ok


def rigid_models(n_parts, k):
    """[n_parts,16] column-major: the default BVH transform after a rotation about y and a small translation, distinct per part, another at every step k."""
    p = np.arange(n_parts, dtype=np.float64)
    ang = 0.02 * (k + 1) * (1.0 + p % 7) + 0.001 * p
    c, s = np.cos(ang), np.sin(ang)
    R = np.zeros((n_parts, 4, 4))
    R[:, 0, 0], R[:, 0, 2], R[:, 2, 0], R[:, 2, 2], R[:, 1, 1], R[:, 3, 3] = c, s, -s, c, 1.0, 1.0
    R[:, 0, 3], R[:, 1, 3] = 0.01 * (p % 5), 0.005 * ((p + k) % 3)
    D = np.asarray(rt.default_bvh_transform(), np.float64).reshape(4, 4).T
    return np.ascontiguousarray(np.transpose(D @ R, (0, 2, 1)), np.float32).reshape(n_parts, 16)


def measure_parts(name, v, f, n_parts, reps, lines):
    import torch
    dev = torch.device("cuda", 0)
    v = np.ascontiguousarray(v, np.float32)
    n = np.asarray(f).size // 3
    pf = np.linspace(0, n, n_parts + 1).astype(np.int32)
    M = rt.default_bvh_transform()
    calls = ("refit", "refit_parts", "rebuild", "rebuild_parts")
    t = {c: [] for c in calls}
    with rt.Renderer() as b:
        b.mesh_upload_parts(v, f, pf)
        stream = torch.cuda.ExternalStream(b.stream(), device=dev)
        tables = [torch.from_numpy(rigid_models(n_parts, k)).to(dev) for k in range(4)]
        torch.cuda.synchronize()
        run = {"refit": lambda: b.mesh_refit(M), "refit_parts": b.mesh_refit_parts, "rebuild": lambda: b.mesh_rebuild(M), "rebuild_parts": b.mesh_rebuild_parts}
        b.mesh_rebuild(M)
        for k in range(-3, reps):       # k < 0: warm-up
            with torch.cuda.stream(stream):
                b.mesh_part_matrices().copy_(tables[k % 4])
            for c in calls:
                b.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run[c]()
                e1.record(stream)
                b.synchronize()
                if k >= 0:
                    t[c].append(e0.elapsed_time(e1))
        mi = b.mesh_info()
        total, _ = b.mesh_refit_count()
        torch.cuda.current_stream(dev).wait_stream(stream)
    lines.append(f"{name}, {n_parts} parts: {n} triangles; device time between events on the library stream; quantised any-hit form "
                 f"{'in use (one host wait per call)' if mi.hostSyncs else 'not in use (no host wait)'}")
    for c in calls:
        lines.append(fmt("rt_mesh_" + c, t[c]))
    med = {c: statistics.median(t[c]) for c in calls}
    spread = max(t["rebuild"]) - min(t["rebuild"])
    ok_refit = med["refit_parts"] < med["rebuild"] and max(t["refit_parts"]) < min(t["rebuild"])
    ok_rebuild = med["rebuild_parts"] <= med["rebuild"] + spread
    lines.append(f"  refit_parts / refit {med['refit_parts'] / med['refit']:.3f}   rebuild_parts / rebuild {med['rebuild_parts'] / med['rebuild']:.3f}   "
                 f"rebuild / refit_parts {med['rebuild'] / med['refit_parts']:.1f}x      RtMeshInfo: rebuilds {mi.rebuilds}, refits {total}, allocations "
                 f"{mi.allocations} (all in the upload), hostSyncs {mi.hostSyncs}")
    lines.append(f"  condition (refit_parts median < rebuild median, refit_parts max {max(t['refit_parts']):.3f} < rebuild min {min(t['rebuild']):.3f}): "
                 f"{'MET' if ok_refit else 'MISSED'}")
    lines.append(f"  condition (rebuild_parts median {med['rebuild_parts']:.3f} <= rebuild median {med['rebuild']:.3f} + its spread {spread:.3f}): "
                 f"{'MET' if ok_rebuild else 'MISSED'}")
    lines.append("")
    return ok_refit and ok_rebuild


def frame_cost(lines, steps=(1, 8, 32), frames=48, batch=8):
    """ms per frame of the bench view on a refitted tree against a rebuilt one over the same positions."""
    import torch
    dev = torch.device("cuda", 0)
    v, f = rt.meshgen.bunny_standin(6)
    v = np.ascontiguousarray(v, np.float32)
    ext = np.float32((v.max(0) - v.min(0)).max())
    M = rt.default_bvh_transform()
    W, H = 1920, 1080
    p = rt.default_render_params()
    p.sppPerFrame = 4
    cam = scenes.camera("closeup", aspect=W / H)
    L = rt.bvh_layout(np.asarray(f).size // 3)
    us = [rt.frame_uniforms(p, cam, W, H, k, True, L.nNodes, L.nTris) for k in range(frames + batch)]

    def ms_per_frame(r):
        # warm-up: after a change of scene the frames re-learn their share of bounce hits and re-size their ray arenas (device-wide waits and
        # allocations of gigabytes, tens of ms per frame while it lasts); four batches let that finish.  Then the better of two timed passes.
        for _ in range(4):
            r.render_frames(us[:batch])
        r.synchronize()
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            for k in range(batch, batch + frames, batch):
                r.render_frames(us[k:k + batch])
            r.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / frames
            best = ms if best is None else min(best, ms)
        return best

    lines.append(f"frames on a refitted tree (informational): bench view {W}x{H}, {p.sppPerFrame} spp, {frames} frames in batches of {batch} after 32 of warm-up, wall / frame, better of two passes")
    with rt.Renderer() as b, rt.Renderer() as c:     # b is refitted step by step, c is rebuilt over the same positions; both made and warmed up first
        for r in (b, c):
            r.upload_env(scenes.env_faces("Sky_01"))
            r.resize(W, H)
            r.mesh_upload(v, f)
            r.mesh_rebuild(M)
        stream = torch.cuda.ExternalStream(b.stream(), device=dev)
        lines.append(f"  undeformed mesh, rebuilt: context b {ms_per_frame(b):8.3f} ms   context c {ms_per_frame(c):8.3f} ms")
        pos, done = v, 0
        for n in steps:
            for k in range(done, n):     # refit steps on top of the first rebuild's tree
                d = step_delta(pos, ext, k)
                pos = (pos + d).astype(np.float32)
                dd = torch.from_numpy(d).to(dev)
                torch.cuda.current_stream(dev).synchronize()
                with torch.cuda.stream(stream):
                    b.mesh_positions().add_(dd)
                torch.cuda.current_stream(dev).wait_stream(stream)
                b.mesh_refit(M)
            done = n
            c.mesh_set_positions(pos)
            c.mesh_rebuild(M)
            refitted, rebuilt = ms_per_frame(b), ms_per_frame(c)
            lines.append(f"  after {n:2d} refit steps: refitted tree {refitted:8.3f} ms   rebuilt {rebuilt:8.3f} ms   ratio {refitted / rebuilt:.3f}")
        for frac in (0.02, 0.1):         # and where a refit does cost: every vertex displaced at random, neighbours torn apart
            noisy = (pos + np.random.default_rng(1).normal(0, frac * ext, pos.shape)).astype(np.float32)
            for r, update in ((b, b.mesh_refit), (c, c.mesh_rebuild)):
                r.mesh_set_positions(noisy)
                update(M)
            refitted, rebuilt = ms_per_frame(b), ms_per_frame(c)
            lines.append(f"  random displacement, sigma {frac:4.2f} of the extent: refitted tree {refitted:8.3f} ms   rebuilt {rebuilt:8.3f} ms   ratio {refitted / rebuilt:.3f}")
    lines.append("")


def measure_quality(name, v, f, reps, lines):
    """Device time of rebuild, refit, refit + measure and measure alone, alternated on one context."""
    import torch
    dev = torch.device("cuda", 0)
    v = np.ascontiguousarray(v, np.float32)
    ext = np.float32((v.max(0) - v.min(0)).max())
    M = rt.default_bvh_transform()
    calls = ("rebuild", "refit", "refit_measure", "measure")
    t = {c: [] for c in calls}
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        stream = torch.cuda.ExternalStream(b.stream(), device=dev)
        delta = torch.from_numpy(step_delta(v, ext, 0) * np.float32(0.1)).to(dev)
        torch.cuda.synchronize()

        def refit_measure():
            b.mesh_refit(M)
            b.mesh_measure()

        run = {"rebuild": lambda: b.mesh_rebuild(M), "refit": lambda: b.mesh_refit(M), "refit_measure": refit_measure, "measure": b.mesh_measure}
        for k in range(-3, reps):       # k < 0: warm-up
            with torch.cuda.stream(stream):
                b.mesh_positions().add_(delta if k % 2 else -delta)
            for c in calls:
                b.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run[c]()
                e1.record(stream)
                b.synchronize()
                if k >= 0:
                    t[c].append(e0.elapsed_time(e1))
        q = b.mesh_quality(wait=True)
        mi, si = b.mesh_info(), b.scene_info()
        torch.cuda.current_stream(dev).wait_stream(stream)
    lines.append(f"{name}: {np.asarray(f).size // 3} triangles, {si.nNodes} nodes; device time between events on the library stream; quantised any-hit form "
                 f"{'in use (one host wait per update)' if mi.hostSyncs else 'not in use (no host wait)'}")
    for c, label in zip(calls, ("rt_mesh_rebuild", "rt_mesh_refit", "rt_mesh_refit + rt_mesh_measure", "rt_mesh_measure alone")):
        lines.append(fmt(label, t[c]))
    med = {c: statistics.median(t[c]) for c in calls}
    ok = med["refit_measure"] < med["rebuild"] and max(t["refit_measure"]) < min(t["rebuild"])
    lines.append(f"  rebuild / (refit + measure) {med['rebuild'] / med['refit_measure']:.1f}x   (refit + measure) - refit {med['refit_measure'] - med['refit']:.3f} ms      "
                 f"measurements skipped {q.skipped}, allocations {mi.allocations} (all in rt_mesh_upload), hostSyncs {mi.hostSyncs} (the updates' own)")
    lines.append(f"  condition (refit + measure median < rebuild median, refit + measure max {max(t['refit_measure']):.3f} < rebuild min {min(t['rebuild']):.3f}): "
                 f"{'MET' if ok else 'MISSED'}")
    lines.append("")
    return ok


def quality_frames(lines, steps=(1, 8, 32), frames=48, batch=8):
    """Cost ratio (rt_mesh_quality) beside ms per frame of the bench view: a refitted tree against one rebuilt over the same positions."""
    v, f = rt.meshgen.bunny_standin(6)
    v = np.ascontiguousarray(v, np.float32)
    tri = np.asarray(f, np.uint32).reshape(-1, 3)
    nparts = 4
    runs = [tri[p::nparts] for p in range(nparts)]          # four parts interleaved in space: triangle i in part i % 4
    f = np.concatenate(runs).reshape(-1)
    pf = np.concatenate([[0], np.cumsum([r.shape[0] for r in runs])]).astype(np.int32)
    ext = np.float32((v.max(0) - v.min(0)).max())
    D = np.asarray(rt.default_bvh_transform(), np.float64).reshape(4, 4).T
    W, H = 1920, 1080
    p = rt.default_render_params()
    p.sppPerFrame = 4
    cam = scenes.camera("closeup", aspect=W / H)
    L = rt.bvh_layout(tri.shape[0])
    us = [rt.frame_uniforms(p, cam, W, H, k, True, L.nNodes, L.nTris) for k in range(frames + batch)]

    def table(drift):
        """The matrix table: the default transform, part p moved by p * drift * extent along x in object space."""
        T = np.tile(np.eye(4), (nparts, 1, 1))
        T[:, 0, 3] = np.arange(nparts) * drift * float(ext)
        return np.ascontiguousarray(np.transpose(D @ T, (0, 2, 1)), np.float32).reshape(nparts, 16)

    def ms_per_frame(r):
        for _ in range(4):               # 32 frames of warm-up: the frames re-learn their bounce share and re-size their arenas after a change of scene
            r.render_frames(us[:batch])
        r.synchronize()
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            for k in range(batch, batch + frames, batch):
                r.render_frames(us[k:k + batch])
            r.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / frames
            best = ms if best is None else min(best, ms)
        return best

    lines.append(f"cost ratio against frame time: bench mesh in {nparts} interleaved parts, bench view {W}x{H}, {p.sppPerFrame} spp, {frames} frames in batches of "
                 f"{batch} after 32 of warm-up, wall / frame, better of two passes; cost = rt_mesh_quality's, over the cost of the first build")
    rows = []
    with rt.Renderer() as b, rt.Renderer() as c:     # b is refitted, c is rebuilt over the same positions and matrices
        for r in (b, c):
            r.upload_env(scenes.env_faces("Sky_01"))
            r.resize(W, H)
            r.mesh_upload_parts(v, f, pf)
            r.mesh_set_part_matrices(table(0.0))
            r.mesh_rebuild_parts()
            r.mesh_measure()
        base = b.mesh_quality(wait=True).cost.cost
        lines.append(f"  first build: cost {base:.3f} (inner {b.mesh_quality().cost.inner:.3f}, leaf {b.mesh_quality().cost.leaf:.3f})   "
                     f"context b {ms_per_frame(b):8.3f} ms   context c {ms_per_frame(c):8.3f} ms")

        def row(label):
            b.mesh_refit_parts(); b.mesh_measure()
            c.mesh_rebuild_parts(); c.mesh_measure()
            qb, qc = b.mesh_quality(wait=True).cost.cost / base, c.mesh_quality(wait=True).cost.cost / base
            mb, mc = ms_per_frame(b), ms_per_frame(c)
            agree = (qb > qc) == (mb > mc)
            rows.append((qb / qc, mb / mc))
            lines.append(f"  {label:<44s} refitted: cost {qb:7.3f}  {mb:8.3f} ms   rebuilt: cost {qc:7.3f}  {mc:8.3f} ms   cost ratio {qb / qc:6.3f}  "
                         f"time ratio {mb / mc:6.3f}  {'same side of 1' if agree else 'OPPOSITE sides of 1'}")

        pos, done = v, 0
        for n in steps:
            for k in range(done, n):
                pos = (pos + step_delta(pos, ext, k)).astype(np.float32)
            done = n
            for r in (b, c):
                r.mesh_set_positions(pos)
            row(f"smooth animation, {n} steps of 3 % of the extent")
        for frac in (0.02, 0.1):
            noisy = (pos + np.random.default_rng(1).normal(0, frac * ext, pos.shape)).astype(np.float32)
            for r in (b, c):
                r.mesh_set_positions(noisy)
            row(f"random displacement, sigma {frac:4.2f} of the extent")
        for r in (b, c):                 # back to the rest pose and a fresh tree, then the parts drift apart
            r.mesh_set_positions(v)
            r.mesh_rebuild_parts()
        for drift in (0.05, 0.25, 1.0):
            for r in (b, c):
                r.mesh_set_part_matrices(table(drift))
            row(f"parts {drift:4.2f} of the extent apart")
    order = sorted(rows)
    monotone = all(order[i][1] <= order[i + 1][1] for i in range(len(order) - 1))
    lines.append(f"  rows ordered by cost ratio: time ratios {' '.join(f'{t:.3f}' for _, t in order)} -- {'ascending too' if monotone else 'NOT ascending'}")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="bunny,1m")
    ap.add_argument("--no-frames", action="store_true")
    ap.add_argument("--parts", default=None, help="comma-separated part counts: time the part-aware calls against the single-matrix ones instead")
    ap.add_argument("--quality", action="store_true", help="time rt_mesh_measure and print the table of cost ratio against frame time")
    args = ap.parse_args()
    if args.quality:
        lines = [f"mesh_refit_time.py --quality --reps {args.reps}: rebuild, refit, refit + measure and measure alternated on one context, one process", ""]
        ok = True
        for s in [x for x in args.sizes.split(",") if x and x != "none"]:
            v, f = rt.meshgen.bunny_standin(6) if s == "bunny" else rt.meshgen.million_triangle_scene()
            ok = measure_quality("bench mesh" if s == "bunny" else "1 M scene", v, f, max(args.reps, 1), lines) and ok
        if not args.no_frames:
            quality_frames(lines)
        text = "\n".join(lines)
        print(text)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")
        return 0 if ok else 1
    if args.parts:
        lines = [f"mesh_refit_time.py --parts {args.parts} --reps {args.reps}: refit, refit_parts, rebuild and rebuild_parts alternated on one context, one process", ""]
        ok = True
        for s in [x for x in args.sizes.split(",") if x and x != "none"]:
            v, f = rt.meshgen.bunny_standin(6) if s == "bunny" else rt.meshgen.million_triangle_scene()
            for n_parts in [int(x) for x in args.parts.split(",")]:
                ok = measure_parts("bench mesh" if s == "bunny" else "1 M scene", v, f, n_parts, max(args.reps, 1), lines) and ok
        text = "\n".join(lines)
        print(text)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")
        return 0 if ok else 1
    lines = [f"mesh_refit_time.py --reps {args.reps}: rebuild and refit alternated on one context, one process", ""]
    ok = True
    for s in [x for x in args.sizes.split(",") if x and x != "none"]:
        v, f = rt.meshgen.bunny_standin(6) if s == "bunny" else rt.meshgen.million_triangle_scene()
        ok = measure("bench mesh" if s == "bunny" else "1 M scene", v, f, max(args.reps, 1), lines) and ok
    if not args.no_frames:
        frame_cost(lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
