#!/usr/bin/env python3
"""bench.py -- Mray/s of the ray-trace hot path on MI355X (BASELINE.json metric).

One "step" = one frame of the hot path (rt_render_frames through the C ABI) over the synthetic
workload of BASELINE.json configs[1]: procedural bunny stand-in (81 920 triangles, median-split
BVH), 1920x1080, 4 spp, one bounce (GI) + AO, Sky_01 environment, default RenderParams, static
camera, frame indices continuing from the warm-up.  Inputs are resident in HBM before the timed
region.  Headline camera = the close-up of SURVEY.md 8d (mesh ~45 % of the frame); the
reference's default camera (mesh < 1 % of the frame) is reported beside it in "default_camera".
`--obj a.obj [--obj b.obj]` renders a supplied mesh (e.g. the Stanford bunny the reference loads at
src/app/application.cpp:260-272) through the same loader / default transform / builder instead.

N > 1: one process per GPU.  `python bench.py --gpus N` starts them itself (a torch.distributed.run
child process, before anything here touches a GPU); under an outer torch.distributed.run the
RANK / WORLD_SIZE environment is used as is.  The frame's 16x16 tiles are dealt round-robin to the
ranks (the frame is fixed, so this is STRONG scaling), every rank holds a BVH replica, and each
batch of frames ends with one RCCL gather of COLOR0 to rank 0 over xGMI plus the un-tiling
kernel.  value = rays of the whole frame / max-over-ranks time.

A "ray" is one traceBVH / traceBVHShadow call of the reference's shader for this frame
(SURVEY.md 8d), counted by the library's work counters in a separate, untimed pass and checked
against the oracle's count on the CPU sample.

A plain run does what the headline figure needs and nothing else: set-up, warm-up, the timed
steps, the work counters (over the first COUNT_FRAMES timed frames), `--dump-outputs DIR` if given,
and the JSON line.  `--full` adds every side measurement and check below, as one line.

Self-check (--full): the timed run submits frames in batches (rt_render_frames); afterwards the same
frame indices are rendered again one rt_render_frame at a time and the COLOR0 targets of the last
frame are compared (sha256).  A mismatch ends the run with a non-zero exit code.  Also under --full:
work counters over every timed frame, stage spans and the roofline, the one-launch-set-in-flight and
merged-access passes, parity of the last timed frame against the oracle, the reference's default
camera, the CPU baseline and run B of BASELINE configs[2].

--dump-outputs DIR: the four render targets of the last timed frame, as a caller of rt_render_frames
receives them (half floats, written as float32 DIR/<target>.npy of shape [H, W, C]); frames whose
targets exceed DUMP_BUDGET_BYTES are written as a fixed, seeded sample of pixels ([K, C] per target,
flat pixel indices y * W + x in DIR/pixel_index.npy).  The inputs depend on the arguments only.
"""
import argparse
import hashlib
import json
import os
import signal
import socket
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
# The binding bound of the traversal kernels when the BVH is cache-resident: the vector L1 (TCP) retires at most ONE cache access per
# clock and CU (tools/gather.hip under rocprofv3 --pmc, profiles/r02_gather_microbench_pmc.txt: 0.80-0.99 measured for divergent
# 16-byte lane-loads of every record shape; lanes that read the same 16 bytes are merged into one access).
CUS, PEAK_CLOCK_HZ = 256, 2.4e9
L1_ACCESS_PEAK_G = CUS * PEAK_CLOCK_HZ / 1e9
W, H, SPP = 1920, 1080, 4
COUNT_FRAMES = 16                    # plain run: timed frames the work counters are taken over (--full: all of them)
DUMP_BUDGET_BYTES = 60 * 2**20       # --dump-outputs: all files together stay below 64 MB
DUMP_SEED = 20240601


TRAVERSAL_SOURCES = ("rt_wave.hip", "rt_wave.hpp", "rt_api.hip", "rt_frame.hpp", "rt_device_shade.hpp", "rt_device_math.hpp", "rt_device_analytic.hpp")


def kernel_source_sha():
    """sha256 over the sources that determine the wavefront pipeline's launches (its kernels, the headers they include, and the host file that lays
    out the trees and queues): ties a committed PMC traffic figure to the code it was measured on.  The megakernel, the hybrid extension's passes, the
    present pass and the GPU tree builder are not on the benchmarked path and do not enter."""
    h = hashlib.sha256()
    for name in sorted(TRAVERSAL_SOURCES):
        f = ROOT / "opengl-raytracing_amd" / "csrc" / name
        h.update(f.name.encode())
        h.update(f.read_bytes())
    return h.hexdigest()


def usable_cores():
    """CPU threads this process may really use: affinity, capped by the cgroup CPU quota (the GPU box gives 16 of 256)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed frames (default 200: a timed region of ~0.4 s)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--subdiv", type=int, default=6, help="icosphere subdivisions of the bunny stand-in (6 = 81 920 tris)")
    ap.add_argument("--obj", action="append", default=[], help="render this .obj instead of the stand-in (repeat to merge several files into one "
                    "triangle soup): rt_load_obj -> rt_gather_triangles_checked with the reference's default transform -> rt_build_bvh")
    ap.add_argument("--pipeline", default="auto", choices=["auto", "mega", "wave"])
    ap.add_argument("--full", action="store_true", help="every side measurement and check beside the headline figure (see the module docstring); "
                    "a plain run does only what the headline needs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the render targets of the last timed frame as DIR/<target>.npy "
                    "(float32; a fixed, seeded pixel sample when the frame is larger than the budget)")
    ap.add_argument("--cpu-seconds", type=float, default=None, help="budget of EACH oracle (CPU baseline) sample -- one thread, then all cores; 0 = skip "
                    "(default: 10 with --full, else 0)")
    ap.add_argument("--no-default-camera", action="store_true")
    ap.add_argument("--batch", type=int, default=8, help="frames per rt_render_frames call: consecutive frames of the static camera share one set of "
                    "kernel launches (bit-identical to frame-by-frame rendering: checked in every --full run, see config.batched_equals_frame_by_frame); "
                    "1 = one rt_render_frame per step")
    ap.add_argument("--no-frame-by-frame", action="store_true", help="skip the frame-by-frame pass (and with it the self-check); used under rocprofv3 so "
                    "that the kernel statistics hold batched launches only")
    ap.add_argument("--no-diagnostics", action="store_true", help="skip the one-launch-set-in-flight and merged-access passes (roofline block reduced)")
    ap.add_argument("--gather-every", type=int, default=1, help="N > 1 GPUs: gather COLOR0 to rank 0 every k-th frame (1 = every batch; a static "
                    "camera's history is tile-local, so BASELINE configs[4] needs one gather per 32 accumulated frames)")
    ap.add_argument("--force-gather", action="store_true", help="rehearsal on one GPU: run the N > 1 code path (process group, communicator, "
                    "gather per batch) with a world of one (self-launched like N > 1 unless an outer launcher set WORLD_SIZE)")
    ap.add_argument("--gather", default="native", choices=["native", "torch"], help="N > 1: the library's own RCCL communicator (C ABI) or torch.distributed")
    ap.add_argument("--rehearse-one-gpu", action="store_true", help="N > 1 ranks as N processes that all render on GPU 0, with a gloo process group and "
                    "host-staged gathers (RCCL refuses two ranks on one device): the multi-process code path on a one-GPU box.  Rank 0 also renders the "
                    "frame alone and compares it with the assembled one (config.assembled_equals_single_rank).  Not a measurement")
    ap.add_argument("--launch", action="store_true", help="start the rank(s) through the self-launcher even for --gpus 1 (rehearsal of the N > 1 start-up "
                    "on a one-GPU box, together with --force-gather)")
    ap.add_argument("--dry-launch", action="store_true", help="--gpus N > 1 without WORLD_SIZE: print the child command / environment as JSON and exit")
    ap.add_argument("--launch-timeout", type=float, default=1500.0, help="self-launched run: seconds before the launcher ends all ranks")
    ap.add_argument("--rank-timeout", type=float, default=1200.0, help="N > 1: seconds after which a rank dumps its stacks and exits (watchdog)")
    # other BASELINE.json configurations, for side measurements (the default line is configs[1], the one `metric` is quoted on)
    ap.add_argument("--size", default="1920x1080", help="framebuffer WxH (configs[3]: 3840x2160)")
    ap.add_argument("--spp", type=int, default=4, help="samples per pixel and frame (configs[2-3]: 16, configs[4]: 64)")
    ap.add_argument("--scene", default="bunny", choices=["bunny", "1m"], help="1m = configs[4]'s 1M-triangle multi-object scene")
    ap.add_argument("--hybrid", action="store_true", help="EXTENSION (not in the reference; SURVEY 8d config 3 run B): the analytic scene "
                    "(floor, glass / mirror / diffuse spheres) with the mesh added to it, reference default camera")
    ap.add_argument("--gi-bounces", type=int, default=1, help="EXTENSION: diffuse bounces of the analytic / hybrid GI path (configs[2]: 4)")
    ap.add_argument("--parity-window", default=None, help="WxH of the oracle window around the frame centre that the last timed frame is compared "
                    "with after the timed run (full history chain from frame 0, all host threads); 0 = skip the parity block (default: 256x128 with "
                    "--full, else 0)")
    ap.add_argument("--no-run-b", action="store_true", help="skip the short side measurement of BASELINE configs[2] as written (\"run B\": bunny + glass + mirror, "
                    "16 spp, 4 bounces -- the labelled hybrid EXTENSION) that the default line carries in `extension_run_b`")
    ap.add_argument("--n1-ms", type=float, default=None, help="N > 1: ms_per_step of the same workload on one GPU -> config.multi_gpu.efficiency_vs_n1")
    return ap.parse_args(argv)


def dump_outputs(out_dir, targets, names):
    """targets: [H, W, C] uint16 half bit patterns -> out_dir/<name>.npy as float32 (exact).  Above DUMP_BUDGET_BYTES: the same fixed, seeded
    sample of pixels from every target ([K, C]), with their flat indices y * W + x in out_dir/pixel_index.npy (float64, exact)."""
    import numpy as np
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    arrs = [np.ascontiguousarray(t).view(np.float16).astype(np.float32) for t in targets]
    h, w = arrs[0].shape[:2]
    px_bytes = sum(a.shape[2] for a in arrs) * 4
    if h * w * px_bytes > DUMP_BUDGET_BYTES:
        k = DUMP_BUDGET_BYTES // (px_bytes + 8)
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(h * w, size=k, replace=False))
        np.save(out_dir / "pixel_index.npy", idx.astype(np.float64))
        arrs = [a.reshape(h * w, -1)[idx] for a in arrs]
    for a, name in zip(arrs, names):
        np.save(out_dir / ("%s.npy" % name), a)


def free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_plan(args, argv):
    """Child command + environment of a self-launched N-GPU run (nothing here has touched a GPU: torch is not even imported)."""
    child_argv = [a for a in argv if a not in ("--dry-launch", "--launch")]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % args.gpus, "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), str(ROOT / "bench.py")] + child_argv
    env = {"HSA_ENABLE_IPC_MODE_LEGACY": "0", "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS", "4")}
    return cmd, env


def self_launch(args, argv):
    """`python bench.py --gpus N` (N > 1) without a launcher: start one fresh process per GPU through torch.distributed.run as a CHILD
    (never an exec: this process stays what it is), relay rank 0's JSON line, return non-zero if any rank failed or the run timed out."""
    cmd, env = launch_plan(args, argv)
    if args.dry_launch:
        print(json.dumps({"cmd": cmd, "env": env, "ranks": args.gpus, "launch_timeout_s": args.launch_timeout}))
        return 0
    proc = subprocess.Popen(cmd, cwd=str(ROOT), env=dict(os.environ, **env), stdout=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, _ = proc.communicate(timeout=args.launch_timeout)
    except subprocess.TimeoutExpired:
        for sig in (signal.SIGTERM, signal.SIGKILL):          # the whole session: launcher + every rank
            try:
                os.killpg(proc.pid, sig)
            except ProcessLookupError:
                break
            try:
                proc.wait(timeout=15)
                break
            except subprocess.TimeoutExpired:
                continue
        sys.stderr.write("bench.py: the %d-rank run exceeded --launch-timeout %.0f s and was stopped\n" % (args.gpus, args.launch_timeout))
        return 124
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    for ln in out.splitlines():
        if not ln.startswith("{"):
            sys.stderr.write(ln + "\n")
    if proc.returncode != 0:
        sys.stderr.write("bench.py: torch.distributed.run exited with %d\n" % proc.returncode)
        return proc.returncode
    if len(lines) != 1:
        sys.stderr.write("bench.py: expected one JSON line from rank 0, got %d\n" % len(lines))
        return 1
    print(lines[0])
    return 0


def main():
    argv = sys.argv[1:]
    args = parse_args(argv)
    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or args.launch or args.force_gather):
        raise SystemExit(self_launch(args, argv))
    if args.dry_launch:
        raise SystemExit("bench.py: --dry-launch needs --gpus N > 1 and no WORLD_SIZE in the environment")
    # a plain run: no side measurements or checks unless asked for one by value (--cpu-seconds S, --parity-window WxH)
    if args.cpu_seconds is None:
        args.cpu_seconds = 10.0 if args.full else 0.0
    if args.parity_window is None:
        args.parity_window = "256x128" if args.full else "0"
    if not args.full:
        args.no_default_camera = args.no_diagnostics = args.no_run_b = args.no_frame_by_frame = True
    global W, H, SPP
    W, H = (int(v) for v in args.size.lower().split("x"))
    SPP = args.spp

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC for RCCL between processes: before anything initialises HIP
    import numpy as np
    import torch
    import torch.distributed as dist
    import opengl_raytracing_amd as rt
    from opengl_raytracing_amd.dist_gather import FrameGatherer, NativeGatherer
    import scenes

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    args.gpus = world
    if args.rehearse_one_gpu:
        local_rank = 0                 # every rank on GPU 0
        args.gather = "torch"          # the library's own communicator is RCCL
    torch.cuda.set_device(local_rank)
    multi = world > 1 or args.force_gather      # the tile-parallel code path (process group, communicator, gathers)
    if multi:
        import faulthandler
        faulthandler.dump_traceback_later(args.rank_timeout, exit=True)   # per-rank watchdog: a rank stuck in a collective ends itself
        if args.rehearse_one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    pipeline = {"auto": rt.RT_PIPELINE_AUTO, "mega": rt.RT_PIPELINE_MEGAKERNEL, "wave": rt.RT_PIPELINE_WAVEFRONT}[args.pipeline]
    mesh_desc = None
    if args.obj:
        # the reference's start-up: Model(path) -> gather_model_triangles(model, app.bvhTransform) -> build_bvh (src/scene/bvh.cpp:249-274),
        # several files merged into one triangle soup first (multi-object scenes, BASELINE configs[4])
        soups = []
        for path in args.obj:
            v_, f_ = rt.load_obj(path)
            soups.append(rt.gather_triangles(v_, f_))
        nodes, tris = rt.build_bvh(np.concatenate(soups, 0))
        mesh_desc = "%s (%d tris, rt_load_obj -> default transform -> median-split BVH)" % (" + ".join(Path(p).name for p in args.obj), tris.shape[0])
    elif args.scene == "1m":
        v, fidx = rt.meshgen.million_triangle_scene()
        nodes, tris = rt.build_bvh(rt.gather_triangles(v, fidx, np.eye(4, dtype=np.float32).reshape(-1)))
    else:
        nodes, tris = scenes.bunny_bvh(args.subdiv)
    faces = scenes.env_faces("Sky_01")
    params = rt.default_render_params()
    params.sppPerFrame = SPP
    npix = W * H
    B = max(1, min(args.batch, 16))

    gather_path = {"path": "library-owned RCCL communicator (rt_comm_init / rt_gather_frame)", "gather_every": args.gather_every,
                   "when": "after each batch of frames (its last frame), and after the last timed frame"}

    def make_renderer(count, pipe=None):
        # work counters (reference units) come from the reference-shaped megakernel; the timed run uses `pipeline`
        r = rt.Renderer(device=local_rank, rank=rank, world_size=world,
                        pipeline=rt.RT_PIPELINE_MEGAKERNEL if count else (pipeline if pipe is None else pipe), count_work=count)
        r.upload_bvh(nodes, tris)
        r.upload_env(faces)
        r.resize(W, H)
        if args.gi_bounces != 1:
            r.set_extension(gi_bounces=args.gi_bounces)
        return r

    def uniforms(cam, frame):
        return rt.frame_uniforms(params, cam, W, H, frame, rt.RT_SCENE_HYBRID if args.hybrid else True, nodes.shape[0], tris.shape[0])

    def color_hash(ren):
        """sha256 of this rank's COLOR0 target (RGBA16F bit patterns, row-major; pixels of other ranks' tiles read as zero)."""
        return hashlib.sha256(np.ascontiguousarray(ren.read_target(rt.RT_TARGET_COLOR)).tobytes()).hexdigest()

    def run_camera(cam, steps, warmup, timed_stage=True, check=False):
        """-> dict(seconds, counters summed over the timed frames, stage times, ...)"""
        # untimed counting pass over the same frame indices (work counters slow the kernels down); a plain run counts the first
        # COUNT_FRAMES timed frames, so that its cost does not grow with --steps
        n_count = steps if args.full else min(steps, COUNT_FRAMES)
        rc = make_renderer(True)
        for f in range(warmup):
            rc.render_frame(uniforms(cam, f))
        rc.reset_counters()
        for f in range(warmup, warmup + n_count):
            rc.render_frame(uniforms(cam, f))
        cnt = rc.counters()
        rc.close()

        ren = make_renderer(False)
        gatherer = None
        if multi:
            # the exchange runs inside the library (rt_comm_init / rt_gather_frame: RCCL behind the C ABI).  If its communicator
            # cannot be brought up on this node the run falls back to the same exchange issued through torch.distributed -- on
            # every rank alike -- and says so in the JSON line.
            ok = torch.ones(1, device="cuda")
            if args.gather == "native":
                try:
                    gatherer = NativeGatherer(ren, gather_every=args.gather_every)
                except Exception as e:   # noqa: BLE001
                    gather_path["error"] = repr(e)[:300]
                    ok.zero_()
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if args.gather != "native" or ok.item() == 0:
                gatherer = FrameGatherer(ren, gather_every=args.gather_every)
                gather_path["path"] = ("torch.distributed (gloo, blocks staged through host memory): REHEARSAL, every rank on GPU 0" if args.rehearse_one_gpu
                                       else "torch.distributed (RCCL) on the library's device pointers")
        # setup, not a step: every frame lane (3-4 streams with their own ray-queue arenas) allocates on its first frame; do that
        # before the W warm-up steps so that a small W cannot push a multi-GB hipMalloc into the timed region.  Round 5: twelve batches instead of five --
        # the library gives the worst-case part of a ray arena back once it knows the scene's share of bounce hits (a lane's SECOND large launch set), and an
        # arena that was reallocated is used at least twice before anything is timed
        N_SETUP = int(os.environ.get("RT_BENCH_SETUP_BATCHES", "12"))
        setup_u = [uniforms(cam, f) for f in range(N_SETUP * B)]
        for b in range(N_SETUP):
            ren.render_frames(setup_u[b * B:(b + 1) * B])
            if gatherer:
                gatherer.after(B, last=True)
        ren.synchronize()
        ren.reset_accum()
        if gatherer:
            gatherer.frames = 0

        frames_u = [uniforms(cam, f) for f in range(warmup + steps)]   # inputs prepared outside the timed region

        def run_steps(f0, f1):
            """Frames f0..f1-1 in batches of B (the last one shorter): rt_render_frames, then -- tile-parallel -- the RCCL gather of COLOR0
            to rank 0 + un-tiling kernel for the batch's last frame, if a --gather-every boundary was crossed (default: every batch)."""
            # at most B frames per batch, dealt evenly (20 frames at B = 8: 7 + 7 + 6 rather than 8 + 8 + 4)
            if f1 <= f0:
                return
            nb = max(1, -(-(f1 - f0) // B))
            f = f0
            for b in range(nb):
                n = (f1 - f0) // nb + (1 if b < (f1 - f0) % nb else 0)
                ren.render_frames(frames_u[f:f + n])
                f += n
                if gatherer:
                    gatherer.after(n, last=(f == f1))

        run_steps(0, warmup)
        ren.synchronize()
        torch.cuda.synchronize()
        ren.traced_rays(reset=True)
        # Stage events (two hipEventRecord per stage and batch) stay out of the single-GPU timed region: each is host work between a batch's hit-count read-back and
        # its next launches, 1.5 % of the driver's 20-step run (1.692 -> 1.666 ms per step, three runs each).  The overlapped spans come from an untimed pass below;
        # a tile-parallel run keeps them in (its gather diagnostics are measured in the timed region, and N > 1 lines are not the headline).
        events_in_timed_region = timed_stage and multi
        if events_in_timed_region:
            ren.enable_stage_timing(True)
            if isinstance(gatherer, FrameGatherer):
                gatherer.timed = True
        comm0 = ren.comm_info() if multi else None
        if multi:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_steps(warmup, warmup + steps)
        ren.synchronize()
        torch.cuda.synchronize()
        dt_own = time.perf_counter() - t0          # this rank alone: its frames and its share of the gathers (the line's per_rank_ms)
        if multi:
            dist.barrier()
        dt = time.perf_counter() - t0
        stages = ren.stage_times() if events_in_timed_region else None
        traced = ren.traced_rays()
        info = ren.scene_info()
        batched_hash = color_hash(ren) if check else None
        mem = ren.memory_info()
        comm = ren.comm_info() if multi else None
        if comm is not None:        # gathers of the timed region only
            comm.gathers -= comm0.gathers
            comm.gatherBytes -= comm0.gatherBytes
        gather_py = gatherer.timing() if (multi and hasattr(gatherer, "timing")) else None
        # what the parity block compares with the oracle: one GPU -- all four targets of the last timed frame; tile-parallel -- the COLOR0
        # frame rank 0 assembled from every rank's tiles in the last gather (so the exchange itself is inside the comparison)
        final_targets = None
        if (parity_wanted or args.dump_outputs) and timed_stage:
            if multi:
                final_targets = [gatherer.frame_halfs()] if rank == 0 else None
            else:
                final_targets = ren.read_all()
        stage_frames, stage_traced = steps, traced
        if timed_stage and not events_in_timed_region and args.full:
            # the same batches once more, untimed, with the stage events on: spans of the stages while launch sets overlap (the targets have been read above)
            n_extra = min(2 * B, warmup + steps)
            ren.traced_rays(reset=True)
            ren.enable_stage_timing(True)
            for f_ in range(0, n_extra, B):
                ren.render_frames(frames_u[f_:min(f_ + B, n_extra)])
            ren.synchronize()
            stages = ren.stage_times()
            stage_frames, stage_traced = n_extra, ren.traced_rays()
        assembled_same = None
        if args.rehearse_one_gpu and gatherer is not None and world > 1:
            # rank 0: the frame the ranks' tiles were assembled into == the same frames rendered by one context that owns every tile
            asm = gatherer.frame_halfs() if rank == 0 else None
            if rank == 0:
                solo = rt.Renderer(device=local_rank, rank=0, world_size=1, pipeline=pipeline)
                solo.upload_bvh(nodes, tris)
                solo.upload_env(faces)
                solo.resize(W, H)
                if args.gi_bounces != 1:
                    solo.set_extension(gi_bounces=args.gi_bounces)
                for f in range(0, warmup + steps, B):
                    solo.render_frames(frames_u[f:min(f + B, warmup + steps)])
                solo.synchronize()
                ref = np.ascontiguousarray(solo.read_target(rt.RT_TARGET_COLOR)).view("<u2").reshape(asm.shape)
                solo.close()
                assembled_same = bool(np.array_equal(ref, asm))
        ren.close()

        # Self-check + comparison figure: the same frame indices, one rt_render_frame per frame (three frames in flight).  Frames
        # 0 .. warmup+steps-1 of a fresh accumulation, as above, so the last frame's COLOR0 must equal the batched run's bit for bit.
        fbf_ms, fbf_hash = None, None
        if check:
            r2 = make_renderer(False)
            for u2 in frames_u[:warmup]:
                r2.render_frame(u2)
            r2.synchronize()
            t2 = time.perf_counter()
            for u2 in frames_u[warmup:]:
                r2.render_frame(u2)
            r2.synchronize()
            fbf_ms = (time.perf_counter() - t2) / max(steps, 1) * 1e3
            fbf_hash = color_hash(r2)
            r2.close()

        tt = torch.tensor([dt], dtype=torch.float64, device="cuda")
        cc = torch.tensor(list(cnt.to_dict().values()), dtype=torch.int64, device="cuda")
        same = torch.tensor([1 if batched_hash == fbf_hash else 0], dtype=torch.int64, device="cuda")
        if multi:
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dist.all_reduce(cc, op=dist.ReduceOp.SUM)
            dist.all_reduce(same, op=dist.ReduceOp.MIN)
        total = rt.RtCounters(*[int(v) for v in cc.tolist()])
        tr = torch.tensor([traced.rays, traced.frames], dtype=torch.int64, device="cuda")
        if multi:
            dist.all_reduce(tr, op=dist.ReduceOp.SUM)
        frames_all = max(int(tr[1].item()) // world, 1)
        traced_per_frame = int(tr[0].item()) // frames_all if traced.frames else 0
        return {"seconds": float(tt.item()), "seconds_own": dt_own, "memory": mem, "stage_frames": stage_frames, "stage_traced": stage_traced, "events_in_timed_region": bool(events_in_timed_region), "comm": comm, "gather_py": gather_py, "final_targets": final_targets, "frames_u": frames_u,
                "counters": total, "local_counters": cnt, "stages": stages,
                "traced_per_frame": traced_per_frame, "traced": traced, "scene_info": info, "counted_frames": n_count,
                "batched_hash": batched_hash, "fbf_hash": fbf_hash, "fbf_ms": fbf_ms, "same": bool(same.item()) if check else None,
                "assembled_same": assembled_same}

    if args.hybrid:
        # the mesh stands among the analytic objects, seen from the reference's default camera (include/app/state.h:129-131)
        M = np.eye(4, dtype=np.float32)
        M[0, 3], M[1, 3], M[2, 3] = -0.1, 1.0, -0.5
        v_, f_ = rt.meshgen.bunny_standin(args.subdiv)
        nodes, tris = rt.build_bvh(rt.gather_triangles(v_, f_, M.T.reshape(-1)))
    cam_kind = "default" if args.hybrid else "closeup"
    check = not args.no_frame_by_frame
    pw = [int(v) for v in args.parity_window.lower().split("x")] if args.parity_window not in ("0", "", "0x0") else None
    parity_wanted = pw is not None
    res = run_camera(scenes.camera(cam_kind), args.steps, args.warmup, check=check)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, res["final_targets"], ("color", "motion", "gpos", "gnrm")[:len(res["final_targets"])])

    # ---- diagnostics, untimed, single GPU: (1) one launch set in flight (RT_LANES=1) in the SAME batched mode as the timed run: what each
    # stage costs when it has the GPU to itself -- with 3-4 batches in flight an event span also contains the time a kernel shares the GPU
    # with other batches' kernels; this pass gives the kernels' own durations, which is what rocprofv3's kernel trace reports
    # (profiles/r05_*kernel_stats*.csv).  (2) the same with the instrumented traversal kernels (RT_TRACE_STATS=2): gather loads after merging the
    # lanes of a wave that stand on the same record -- the unit the vector L1's one-access-per-clock ceiling applies to.
    serial, merged = None, None
    if world == 1 and not args.hybrid and not args.no_diagnostics:
        saved = {k: os.environ.get(k) for k in ("RT_LANES", "RT_TRACE_STATS")}
        cam1 = scenes.camera(cam_kind)
        us1 = [uniforms(cam1, f) for f in range(4 * B)]
        try:
            os.environ["RT_LANES"] = "1"
            r1 = make_renderer(False)
            r1.render_frames(us1[:B])
            r1.render_frames(us1[B:2 * B])
            r1.synchronize()
            r1.traced_rays(reset=True)
            r1.enable_stage_timing(True)
            r1.render_frames(us1[2 * B:3 * B])
            r1.render_frames(us1[3 * B:])
            serial = {"stages": r1.stage_times()["stages"], "traced": r1.traced_rays(), "frames": 2 * B}
            r1.close()
            os.environ["RT_TRACE_STATS"] = "2"
            r3 = make_renderer(False)
            r3.render_frames(us1[:B])
            r3.synchronize()
            r3.traced_rays(reset=True)
            r3.render_frames(us1[B:2 * B])
            merged = r3.traced_rays()
            r3.close()
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    rays = res["counters"].rays * args.steps / res["counted_frames"]      # reference rays of the timed frames
    mray = rays / res["seconds"] / 1e6
    ms_per_step = res["seconds"] / args.steps * 1e3

    # ---- roofline of the dominant kernel
    roofline = None
    st = res["stages"]
    if st and st["stages"]:
        src = serial if serial else {"stages": st["stages"], "traced": res["stage_traced"], "frames": res["stage_frames"]}
        name, dom = max(src["stages"].items(), key=lambda kv: kv[1]["ms"])
        launches = max(int(dom["launches"]), 1)
        avg_ms = dom["ms"] / launches                  # HIP events around each launch of this kernel, on the stream it runs on
        tr = src["traced"]
        info = res["scene_info"]
        # (1) HBM roofline, the contract's: ALGORITHMIC bytes of one launch in THIS implementation's layout = what it has to move through HBM
        # at least once: the ray records it reads (32-byte origin/direction + 4-byte tMax; 4 bytes of pixel slot for a primary ray), the
        # results it writes (1 byte per any-hit ray, 8 per closest-hit ray) and the BVH arrays it walks, once (every re-read of
        # a node is served by L1 / L2 / Infinity Cache or is waste).
        # trace_ao (round 4): the AO rays of a hit are one packet -- one 16-byte origin for its four rays, 16-byte direction + 4-byte tMax in and 1 byte out per ray
        rays_k = {"trace_primary": tr.primary, "trace_shadow": tr.shadow + tr.bounceShadow, "trace_gi": tr.bounce, "trace_ao": tr.ao}
        rec_k = {"trace_primary": 4 + 8, "trace_shadow": 36 + 1, "trace_gi": 36 + 8, "trace_ao": 4 + 16 + 4 + 1}
        bvh_k = {"trace_primary": info.bytesNodes2 + info.bytesPairs, "trace_shadow": info.bytesNodes4 + info.bytesPairs,
                 "trace_gi": info.bytesNodes2 + info.bytesPairs, "trace_ao": info.bytesNodes4 + info.bytesPairs}
        if name in rays_k:
            rays_per_launch = rays_k[name] / launches
            bytes_per_launch = rays_per_launch * rec_k[name] + bvh_k[name]
            attribution = ("%d B per ray traced (record in, result out) x %.0f rays per launch + the BVH arrays this kernel walks, once (%d B)"
                           % (rec_k[name], rays_per_launch, bvh_k[name]))
        else:
            frames_per_launch = src["frames"] / launches
            bytes_per_launch = (npix // world) * 36.0 * frames_per_launch
            attribution = "36 B per pixel (8 B history read + 28 B of target writes) x %.1f frames per launch" % frames_per_launch
        achieved = bytes_per_launch / (avg_ms * 1e-3) / 1e9
        # the SURVEY 8d figure (REFERENCE layout: 48 B per nodeFetch / triFetch of the reference's loop for the rays this kernel traces) is kept
        # beside it without a fraction: it is not a traffic figure of this implementation (4x fewer rays are traversed, a node visit is one
        # 64 / 112-byte record instead of 3 x 48 B) and exceeds the HBM peak on cache-resident scenes.
        lc = res["local_counters"]
        fetch_rest = lc.nodeFetch + lc.triFetch - lc.fetchPrimary - lc.fetchShadow - lc.fetchAO
        per_kind = {"trace_primary": lc.fetchPrimary, "trace_shadow": lc.fetchShadow + lc.fetchAO, "trace_gi": fetch_rest}
        ref_layout = None
        if name in per_kind:
            ref_bytes = 48.0 * per_kind[name] / res["counted_frames"] * (src["frames"] / launches)
            ref_layout = {"algorithmic_bytes_per_launch": ref_bytes, "bytes_per_s_GB": ref_bytes / (avg_ms * 1e-3) / 1e9, "frac": None,
                          "note": "SURVEY 8d units (48 B x the reference loop's nodeFetch + triFetch for these rays, megakernel counting pass); "
                                  "not bytes this implementation moves, so no fraction of a hardware peak is formed from it"}
        # HBM bytes of that kernel per launch from the PMC passes of tools/r03_profile.sh (round 5: tag r05fin, summarised by tools/r05_summarize.py) (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate
        # passes over THIS command in its batched mode, gfx950 2x fetch correction).  PMC cannot be collected inside this run: the figure is
        # accepted only when the kernel sources it was measured on are the ones running now, else it is dropped.
        traffic, traffic_src = None, None
        kmap = {"trace_shadow": "DualQueueSrc, true", "trace_gi": "QueueSrc, false", "trace_primary": "PrimarySrc", "trace_ao": "k_trace_packets"}
        tj = ROOT / "profiles" / ("r05_traffic_%s.json" % ("1m" if args.scene == "1m" else "bunny"))
        if world == 1 and tj.exists() and name in kmap and (W, H, SPP, B) == (1920, 1080, 4, 8) and not args.obj:
            tjd = json.load(open(tj))
            if tjd.get("kernel_source_sha256") == kernel_source_sha():
                for k, v in tjd["kernels"].items():
                    if kmap[name] in k and v.get("launches_with_rays"):
                        traffic = v["hbm_bytes_corrected"] / v["launches_with_rays"]
                        traffic_src = {"kind": "profiled_offline", "file": str(tj.relative_to(ROOT)), "measured_at_commit": tjd.get("commit"),
                                       "kernel_source_sha256": tjd.get("kernel_source_sha256"), "mode": tjd.get("mode"),
                                       "tcp_accesses_per_clk_per_cu_pmc": v.get("tcp_accesses_per_clk_per_cu")}
            else:
                traffic_src = {"kind": "stale", "file": str(tj.relative_to(ROOT)),
                               "note": "kernel sources changed since the PMC passes; figure dropped"}
        # (2) what binds these kernels when the BVH is cache-resident: the vector L1 retires at most one cache access per clock and CU.  The
        # traversal kernels count the 16-byte per-lane node / triangle loads they issue; the instrumented pass counts them after merging the
        # lanes of a wave that read the same record (one access).  frac = merged accesses / launch duration / (256 CUs x 2.4 GHz) <= 1.
        l1 = None
        gl = {"trace_primary": tr.gatherLoadsPrimary, "trace_shadow": tr.gatherLoadsShadow, "trace_gi": tr.gatherLoadsBounce}
        if name in gl and merged is not None:   # (the packet launch has no instrumented build: every record it fetches is fetched once per packet by construction)
            mg = {"trace_primary": (merged.mergedLoadsPrimary, merged.gatherLoadsPrimary), "trace_shadow": (merged.mergedLoadsShadow, merged.gatherLoadsShadow),
                  "trace_gi": (merged.mergedLoadsBounce, merged.gatherLoadsBounce)}[name]
            if mg[1] > 0 and mg[0] > 0:
                factor = mg[0] / mg[1]
                lane_loads = gl[name] / launches
                acc = lane_loads * factor
                rate = acc / (avg_ms * 1e-3) / 1e9
                l1 = {"unit": "G L1 cache accesses/s (16 B each, lanes on the same record merged)", "lane_loads_per_launch": lane_loads,
                      "merge_factor": factor, "accesses_per_launch": acc, "achieved": rate, "peak": L1_ACCESS_PEAK_G, "frac": rate / L1_ACCESS_PEAK_G,
                      "peak_source": "one TCP cache access per clock and CU x 256 CUs x 2.4 GHz (profiles/r02_gather_microbench_pmc.txt: 0.80-0.99 measured "
                                     "with divergent 16-byte lane-loads; lanes reading the same 16 bytes count once)",
                      "merge_factor_source": "counted by the instrumented traversal kernels over one batch of this workload (distinct records per wave "
                                             "step / lanes); the PMC figure of the same launches is in profiles/r05_derived.txt"}
        roofline = {"bound": "hbm", "kernel": name, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                    "traffic_frac_of_peak": (traffic / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if traffic else None,
                    "avg_launch_ms": avg_ms, "launches": launches, "frames_per_launch": src["frames"] / launches,
                    "algorithmic_bytes_per_launch": bytes_per_launch, "attribution": attribution,
                    "bvh_bytes": {"nodes_2wide": info.bytesNodes2, "nodes_4wide": info.bytesNodes4, "triangle_pairs": info.bytesPairs,
                                  "nodes_4wide_form": ("quantised: 64 B per node + 32 B of exact box per leaf (any-hit trees beyond 4 MB, DESIGN.md 4.2)"
                                                       if info.bytesNodes4 != info.nWide4 * 128 else "exact: 128 B per node (112 B read)")},
                    "cache_resident": bool(info.bytesNodes2 + info.bytesNodes4 + info.bytesPairs < 32 * 2**20),
                    "reference_layout": ref_layout, "l1_gather": l1,
                    "avg_launch_ms_source": ("HIP events around the launches of an untimed pass with ONE launch set in flight (RT_LANES=1), same batching as "
                                             "the timed run; every launch traced rays" if serial else "HIP events, untimed pass after the timed region (N > 1: the timed region); "
                                             "launch sets of several batches overlap: spans include time shared with other kernels"),
                    "note": "hbm frac = compulsory bytes of the launch / its duration / 8 TB/s.  With the BVH resident in L2 / Infinity Cache "
                            "(cache_resident) HBM is not what bounds the kernel -- a low frac is expected; the binding bound is the L1 access "
                            "rate (l1_gather), see DESIGN.md 4.3"}

    headline = (args.scene, W, H, SPP, args.hybrid, bool(args.obj)) == ("bunny", 1920, 1080, 4, False, False)
    if args.obj:
        mesh = mesh_desc
    elif args.scene == "bunny":
        mesh = "procedural bunny stand-in (icosphere subdiv %d, %d tris, median-split BVH)" % (args.subdiv, tris.shape[0])
    else:
        mesh = "1M-triangle multi-object scene (%d tris, median-split BVH)" % tris.shape[0]
    if not args.hybrid:
        workload = "%s%s, %dx%d, %d spp, GI 1 bounce + AO 4, Sky_01 env, close-up camera (-2,1.5,1.0)" % (
            "configs[1]: " if headline else ("configs[1] with a supplied mesh: " if args.obj and (W, H, SPP) == (1920, 1080, 4) else "variant: "), mesh, W, H, SPP)
    else:
        workload = ("variant: %s inside the reference's analytic scene (floor, diffuse / glass / mirror spheres, light marker) -- EXTENSION mode=hybrid, "
                    "not expressible in the reference -- %dx%d, %d spp, %d GI bounces + AO 4, Sky_01 env, reference default camera" % (mesh, W, H, SPP, args.gi_bounces))
    out = {
        "metric": "Mray/s @1080p 4spp bunny BVH" if (headline or (args.obj and (W, H, SPP, args.hybrid) == (1920, 1080, 4, False))) else
                  "Mray/s @%dx%d %dspp %s%s" % (W, H, SPP, args.scene, " + analytic scene, %d GI bounces (extension, not in the reference)" % args.gi_bounces if args.hybrid else " BVH"),
        "value": mray, "unit": "Mray/s", "value_traversed": res["traced_per_frame"] * args.steps / res["seconds"] / 1e6,
        "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic" if not args.obj else "supplied .obj",
        "config": {"workload": workload,
                   "pipeline": args.pipeline, "tiles": "16x16 round-robin over ranks" if world > 1 else "single GPU",
                   "gather": gather_path if multi else None,
                   "frames_per_launch_set": B,
                   "batching": "rt_render_frames: consecutive frames of the static camera (they differ in uFrameIndex and uJitter only) share one set of "
                               "kernel launches; every frame is fully rendered",
                   "batched_equals_frame_by_frame": res["same"],
                   "assembled_equals_single_rank": res["assembled_same"],
                   "color0_sha256": res["batched_hash"], "color0_sha256_frame_by_frame": res["fbf_hash"],
                   "self_check": ("COLOR0 of frame %d (last timed frame) after the batched run == after one rt_render_frame per frame over the same frame "
                                  "indices, sha256 of the RGBA16F bits%s" % (args.warmup + args.steps - 1, ", every rank its own tiles" if world > 1 else "")) if check else None,
                   "ms_per_step_frame_by_frame": res["fbf_ms"],
                   "rays_per_frame": res["counters"].rays // res["counted_frames"], "msample_per_s": npix * SPP * args.steps / res["seconds"] / 1e6,
                   "hit_pixels": res["counters"].hitPixels // res["counted_frames"],
                   "rays_counted_frames": res["counted_frames"],
                   "full": bool(args.full),
                   "rays_traversed_per_frame": res["traced_per_frame"],
                   "ray_accounting": "value counts the reference shader's traceBVH/traceBVHShadow calls (SURVEY 8d); "
                                     "identical rays (SPP copies of the primary and AO rays) are traversed once and disk-light "
                                     "shadow rays of exactly zero weight are not traversed: rays_traversed_per_frame"},
        "roofline": roofline,
    }
    mi = res["memory"]
    out["config"]["hbm"] = {"in_use_GB": (mi.deviceTotalBytes - mi.deviceFreeBytes) / 1e9, "total_GB": mi.deviceTotalBytes / 1e9,
                            "ray_queue_arenas_GB": mi.queueArenaBytes / 1e9, "ray_queue_arenas": mi.queueArenas, "frame_lanes": mi.lanes,
                            "per_lane_frame_arrays_GB": mi.frameArrayBytes / 1e9, "hybrid_arena_GB": mi.hybridArenaBytes / 1e9,
                            "what": "hipMemGetInfo on this rank's device right after the timed run (this context + the runtime's own allocations); "
                                    "the ray-queue arenas are shared by the frame lanes (RT_ARENAS) and sized for one batch of frames each"}
    # how the stage spans relate to the timed region: rounds 1-3 recorded the stage events INSIDE it (about 1.5 % of a 20-step run); since round 4 a
    # single-GPU run records them in an untimed pass over `stage_frames` frames that continues the timed run's history -- ms_per_step lines are comparable from
    # round 4 on, and with rounds 1-3 only after that 1.5 %
    out["config"]["stage_events_in_timed_region"] = bool(res.get("events_in_timed_region", False))
    out["config"]["stage_frames"] = int(res["stage_frames"])
    if st:
        out["stage_ms_per_frame"] = {k: v["ms"] / res["stage_frames"] for k, v in st["stages"].items()}
        out["stage_ms_note"] = ("HIP-event spans of an untimed pass over the same batches (N > 1: of the timed region); consecutive batches overlap on four streams, "
                                "so spans add up to more than ms_per_step")
    if serial:
        out["stage_ms_per_frame_one_launch_set_in_flight"] = {k: v["ms"] / serial["frames"] for k, v in serial["stages"].items()}

    # ---- multi-GPU: what each rank did, gathered over the ranks, so that ONE line explains an N-GPU figure (no scaling curve has been measured
    # anywhere yet: SCALE_r01-r03 were skipped).  per_rank_ms: every rank's own time from the common start to the end of its own work (its
    # frames + its side of the gathers), before the closing barrier; gather: HIP events around each rt_gather_frame on the stream it runs on.
    if multi:
        g_stage = (st or {"stages": {}})["stages"].get("gather")
        gp = res["gather_py"]
        own = [res["seconds_own"] / args.steps * 1e3,
               (g_stage["ms"] if g_stage else (gp["ms"] if gp else 0.0)),
               float(g_stage["launches"] if g_stage else (gp["gathers"] if gp else 0)),
               float(res["comm"].gatherBytes if g_stage else (gp["bytes"] if gp else 0)),
               float(res["comm"].commWorld), float(res["comm"].commRank),
               1.0 if "error" in gather_path else 0.0, float(local_rank)]
        mine = torch.tensor(own, dtype=torch.float64, device="cuda")
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        rows = [[float(v) for v in t.tolist()] for t in allr]
        ms_r = [r[0] for r in rows]
        root = rows[0]
        g_ms = root[1] / max(root[2], 1.0)
        out["config"]["multi_gpu"] = {
            "per_rank_ms": {"min": min(ms_r), "max": max(ms_r), "mean": sum(ms_r) / len(ms_r), "values": ms_r,
                            "what": "per step; each rank's own host clock from the common start (barrier) to the end of its own frames and gathers"},
            "imbalance": max(ms_r) / (sum(ms_r) / len(ms_r)),
            "gather_ms_per_batch": g_ms, "gathers": int(root[2]), "gather_bytes": int(root[3] / max(root[2], 1.0)),
            "gather_GBps": (root[3] / max(root[2], 1.0)) / (g_ms * 1e-3) / 1e9 if g_ms > 0 else None,
            "gather_what": "rank 0: HIP events on the gathered frame's stream from the moment that stream reaches the exchange to the end of the "
                           "un-tiling kernel (so it includes waiting for the slowest sender); bytes = what rank 0 receives per gather",
            "gather_ms_per_batch_by_rank": [r[1] / max(r[2], 1.0) for r in rows],
            "rccl_world": [int(r[4]) for r in rows], "rccl_rank": [int(r[5]) for r in rows],
            "rccl_world_what": "ncclCommCount / ncclCommUserRank of the library's communicator on every rank (-1: no communicator on that rank -- "
                               "the exchange then ran through torch.distributed, see config.gather.path)",
            "fallback": [bool(r[6]) for r in rows], "device": [int(r[7]) for r in rows],
            "efficiency_vs_n1": (args.n1_ms / ms_per_step / world) if args.n1_ms else None,
            "scaling_curve": "not measured in any round so far; this line is one point",
        }

    # ---- parity of the timed frames (BASELINE.json's metric has an RMSE leg): the last timed frame -- warm-up + steps frames deep in the
    # accumulation -- against the oracle (oracle/: the scalar CPU restatement of shaders/rt, the checker) on a window around the frame centre,
    # the whole history chain rendered by the oracle on all host threads.  Untimed.  rmse >= 1e-4 on any target ends the run with exit code 4.
    # The reference's own precision anchor is the fp16 targets (rt.frag:29-38, src/render/accum.cpp:10); HIP == oracle is asserted bit for bit
    # in tests/, so bit_diff is expected to be 0 and rmse exactly 0.
    parity = None
    if parity_wanted and rank == 0 and res["final_targets"] is not None:
        import oracle as orc
        t_p = time.perf_counter()
        x0 = max(0, min(W - pw[0], W // 2 - pw[0] // 2)); y0 = max(0, min(H - pw[1], H // 2 - pw[1] // 2))
        x1, y1 = min(W, x0 + pw[0]), min(H, y0 + pw[1])
        prev, want = None, None
        for u_f in res["frames_u"]:
            want, _ = orc.render(u_f, nodes, tris, faces, prev, region=(x0, y0, x1, y1), nthreads=usable_cores(), gi_bounces=args.gi_bounces)
            prev = want[0]
        names = ("color", "motion", "gpos", "gnrm")
        per = {}
        for g_t, w_t, nm in zip(res["final_targets"], want, names):
            c_ = orc.compare(np.ascontiguousarray(g_t[y0:y1, x0:x1]), np.ascontiguousarray(w_t[y0:y1, x0:x1]))
            per[nm] = {"rmse": c_["rmse"], "max_abs": c_["max_abs"], "outliers_gt_1e-2": c_["outliers"], "bit_diff": c_["bit_diff"]}
        worst = max(v["rmse"] for v in per.values())
        parity = {"vs": "oracle", "window": [x0, y0, x1, y1], "frame": args.warmup + args.steps - 1, "frames_chained": len(res["frames_u"]),
                  "targets": per, "rmse": worst, "max_abs": max(v["max_abs"] for v in per.values()),
                  "outliers_gt_1e-2": sum(v["outliers_gt_1e-2"] for v in per.values()), "bit_diff": sum(v["bit_diff"] for v in per.values()),
                  "tolerance": "rmse < 1e-4 per target (north_star); values are RGBA16F / RG16F half floats compared as floats",
                  "compared": ("COLOR0 of the frame rank 0 assembled from all ranks' tiles (last gather)" if multi else
                               "all four targets of the last timed frame, as left by the batched timed run"),
                  "oracle_seconds": time.perf_counter() - t_p, "ok": bool(worst < 1e-4)}
    out["parity"] = parity

    if not args.no_default_camera and not args.hybrid:
        d = run_camera(scenes.camera("default"), args.steps, args.warmup, timed_stage=False)
        out["default_camera"] = {"value": d["counters"].rays * args.steps / d["counted_frames"] / d["seconds"] / 1e6, "unit": "Mray/s",
                                 "ms_per_step": d["seconds"] / args.steps * 1e3, "rays_per_frame": d["counters"].rays // d["counted_frames"],
                                 "hit_pixels": d["counters"].hitPixels // d["counted_frames"]}

    if rank == 0 and world == 1 and args.cpu_seconds > 0:
        import tempfile
        import oracle as orc
        cores = usable_cores()
        cam = scenes.camera(cam_kind)
        u = uniforms(cam, args.warmup)
        # the oracle's traversal + shade loop compiled -O3 -march=native on THIS host (bit-identical to the -O2 checker
        # build: tests/test_oracle_kat.py), (a) one thread -- the scalar figure the >= 10x target refers to -- (b) all usable cores.
        with tempfile.TemporaryDirectory() as tmp:
            Ln = orc.load(orc.build_native(tmp))
            order = sorted(range(0, H, 16), key=lambda y: abs(y + 8 - H // 2))   # 16-row bands outward from the middle of the frame

            def sample(nthreads, rows):
                rays_cpu, dt, bands = 0, 0.0, 0
                for y in order:
                    for y0 in range(y, min(y + 16, H), rows):
                        t0 = time.perf_counter()
                        _, c1 = orc.render(u, nodes, tris, faces, None, region=(0, y0, W, min(y0 + rows, H)), nthreads=nthreads, L=Ln, gi_bounces=args.gi_bounces)
                        dt += time.perf_counter() - t0
                        rays_cpu += c1.rays
                        bands += 1
                        if dt >= args.cpu_seconds:
                            return rays_cpu, dt, bands
                return rays_cpu, dt, bands

            r1, t1, b1 = sample(1, 2)
            rn, tn, bn = sample(cores, 16)
        what = "oracle (scalar fp32 C++ restatement of shaders/rt, g++ -O3 -march=native -ffp-contract=off), %dx%d/%dspp close-up frame %d" % (W, H, SPP, args.warmup)
        out["cpu_baseline"] = {"value": rn / tn / 1e6, "unit": "Mray/s", "cores": cores, "kind": "port",
                               "sample": f"{what}: {bn} 16-row bands around the middle, {rn} rays in {tn:.1f} s on {cores} threads",
                               "single_thread": {"value": r1 / t1 / 1e6, "unit": "Mray/s", "cores": 1,
                                                 "sample": f"{b1} 2-row bands around the middle, {r1} rays in {t1:.1f} s on 1 thread"},
                               "frame_seconds_estimate": {"threads_1": rays / args.steps / (r1 / t1), "threads_all": rays / args.steps / (rn / tn)},
                               "note": "the CPU traces every reference ray; the GPU pipeline skips duplicates (config.ray_accounting), so compare "
                                       "frame times (frame_seconds_estimate vs ms_per_step), or value_traversed, not the two Mray/s figures"}
    # ---- BASELINE configs[2] AS WRITTEN ("bunny + glass + mirror materials ..., 16 spp, 4 bounces": run B).  The reference cannot express it (rt.frag:84-163: its BVH
    # mode has no analytic objects or materials, its analytic mode no mesh, both one bounce), so it exists here only as the labelled hybrid EXTENSION, with
    # parity against this repository's own oracle.  The --full line carries a short measurement of it so that the record shows both runs; configs[2] / [3] are
    # still REPORTED as run A (`--spp 16`).  A child process of this command (the same bench.py with --hybrid); its failure does not fail the line.
    if rank == 0 and world == 1 and headline and not args.no_run_b:
        cmd = [sys.executable, str(ROOT / "bench.py"), "--full", "--hybrid", "--spp", "16", "--gi-bounces", "4", "--steps", "4", "--warmup", "2", "--cpu-seconds", "0",
               "--no-default-camera", "--no-frame-by-frame", "--no-diagnostics", "--no-run-b", "--parity-window", "32x16"]
        try:
            r_b = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=240)
            lines_b = [ln for ln in r_b.stdout.splitlines() if ln.startswith("{")]
            if r_b.returncode == 0 and len(lines_b) == 1:
                b_ = json.loads(lines_b[0])
                out["extension_run_b"] = {"what": "EXTENSION, not in the reference: BASELINE configs[2] as written (run B) through the staged hybrid pipeline; parity vs this repository's own oracle",
                                          "workload": b_["config"]["workload"], "metric": b_["metric"], "ms_per_step": b_["ms_per_step"], "value": b_["value"], "unit": b_["unit"],
                                          "steps": b_["steps"], "stage_ms_per_frame": b_.get("stage_ms_per_frame"), "hbm": b_["config"].get("hbm"),
                                          "parity": {k: b_["parity"][k] for k in ("vs", "window", "frames_chained", "rmse", "bit_diff", "ok")} if b_.get("parity") else None,
                                          "command": " ".join(cmd[1:])}
            else:
                out["extension_run_b"] = {"error": "exit code %d" % r_b.returncode, "stderr_tail": r_b.stderr[-300:]}
        except Exception as e:   # noqa: BLE001
            out["extension_run_b"] = {"error": repr(e)[:300]}
    if multi:
        import faulthandler
        faulthandler.cancel_dump_traceback_later()
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out))
    if check and res["same"] is False:
        sys.stderr.write("bench.py: batched frames differ from frame-by-frame rendering (COLOR0 %s vs %s)\n" % (res["batched_hash"], res["fbf_hash"]))
        raise SystemExit(3)
    if parity is not None and not parity["ok"]:
        sys.stderr.write("bench.py: the timed frame differs from the oracle: %s\n" % json.dumps(parity["targets"]))
        raise SystemExit(4)
    if rank == 0 and res.get("assembled_same") is False:
        sys.stderr.write("bench.py: the frame assembled from the ranks' tiles differs from the single-rank frame\n")
        raise SystemExit(3)


if __name__ == "__main__":
    main()
