"""Sparse answers of the wavefront frames' trace launches.

The generators write the miss answer beside every primary and any-hit ray they record -- primTri = -1 (k_primary), occ1 = 0 (k_gen_direct), occ2 = 0 (k_gen_gi /
k_gen_gi_listed) -- and such a ray stores only a hit or an occlusion when it retires.  (The bounce queue's launches store every answer: pre-filling giTri was
measured and gained nothing)  What can go wrong is a stale answer surviving in an array that is used
again, so the cases use the arrays again in every way the pipeline does: frame after frame, batch after frames, chunk after chunk, another view after one with
many hits, the overflow answers beside a sparse occ2, the other readers and writers of the AO slots, the permuted bounce queue.

Every frame case is tests/test_gpu_queue_diet.py's: three frames of 160 x 96 at 2 spp, frame by frame and as one batch, against the oracle chained from frame
to frame, bit for bit on all four targets; its two scenes (two_mesh: thousands of bounce hits and occluded AO rays, closeup: nearly all misses) and its oracle
frames, computed once for both files.
"""
import ctypes as C

import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scenes
import test_gpu_queue_diet as qd

W, H = qd.W, qd.H
FRAMES, SPP = 3, 2


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in qd.VARS:
        monkeypatch.delenv(v, raising=False)


# ---------------------------------------------------------------- 1. both bounce paths, both scenes

@pytest.mark.gpu
@pytest.mark.parametrize("probe", ["1", "0"])
@pytest.mark.parametrize("scene", list(qd.SCENES))
def test_frames_equal_the_oracle_on_both_bounce_paths(orc, monkeypatch, scene, probe):
    """Behind a bounce probe and behind the closest-hit bounce launch (QueueSrc with both kinds of store in one frame: occlusions only, every closest hit)."""
    out, spp = qd._run(orc, monkeypatch, scene, {"RT_BOUNCE_PROBE": probe})
    for gl, bp, _ in out:
        assert (bp.probeLaunches > 0) == (probe == "1") and (bp.closestLaunches > 0) == (probe == "0"), (scene, probe)
    if scene == "two_mesh":
        assert out[0][0].shaded > 1000, out[0][0].shaded      # bounce hits whose answers had to be stored


# ---------------------------------------------------------------- 2. a view full of hits and occlusions, then one that is nearly all misses

def _hit(target):          # gpos.w = 1 (fp16) on a hit
    return target[2][:, :, 3] == 0x3C00


@pytest.mark.gpu
def test_stale_answers_of_another_view_do_not_survive(orc, monkeypatch):
    """One renderer with one launch set in flight (RT_LANES=1: two lanes that take turns, so each lane's arrays see both views): three frames of two_mesh, then
    three frames of closeup -- uploaded as qd._prepare does -- equal the oracle; then closeup as one batch behind a batch from a moved camera, without another
    upload.  Precondition, from the oracle's frames: among the pixels that are hits in both views the hit answer (the hit point, G-buffer position) differs at a
    quarter at least, and so does the colour -- the only place the oracle's frames show the occlusion and bounce answers --, and some pixels are a hit in one
    view only; otherwise the arrays could hold the right answers by accident.  (The two views show different meshes, so both shares are near one.)"""
    monkeypatch.setenv("RT_LANES", "1")
    first, second = qd._oracle(orc, "two_mesh"), qd._oracle(orc, "closeup")
    both = _hit(first[-1]) & _hit(second[-1])
    differ = (first[-1][2] != second[-1][2]).any(axis=2) & both
    shaded = (first[-1][0] != second[-1][0]).any(axis=2) & both
    only_first = _hit(first[-1]) & ~_hit(second[-1])
    print(f"hits in both views {int(both.sum())}, hit point differs at {int(differ.sum())}, colour at {int(shaded.sum())}; hits of the first view only {int(only_first.sum())}")
    assert both.sum() > 1000 and 4 * differ.sum() >= both.sum() and 4 * shaded.sum() >= both.sum() and only_first.sum() > 0
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r:
        assert r.memory_info().lanes == 2      # RT_LANES=1: serial frames over the two COLOR0 buffers
        qd._prepare(r, "two_mesh")
        for f, u in enumerate(qd._uniforms("two_mesh")):
            r.render_frame(u)
            qd._equal(r.read_all(), first[f], orc, f"two_mesh frame {f}")
        qd._prepare(r, "closeup")
        r.reset_accum()
        for f, u in enumerate(qd._uniforms("closeup")):
            r.render_frame(u)
            qd._equal(r.read_all(), second[f], orc, f"closeup after two_mesh, frame {f}")
        # the same once more as a batch behind frames of a moved camera (no upload in between)
        r.reset_accum()
        r.render_frames(qd._uniforms("closeup", moved=True))
        r.reset_accum()
        r.render_frames(qd._uniforms("closeup"))
        qd._equal(r.read_all(), second[-1], orc, "closeup batch after a moved camera")


# ---------------------------------------------------------------- 3. chunk after chunk

@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(qd.SCENES))
def test_chunks_use_the_arrays_again(orc, monkeypatch, scene):
    budget = qd.OPTIONS["chunked"]["RT_QUEUE_BUDGET_MB"]
    out, spp = qd._run(orc, monkeypatch, scene, {"RT_BOUNCE_PROBE": "1", "RT_QUEUE_BUDGET_MB": budget})
    (gl, bp, hits), (glb, _, _) = out
    per_frame = hits // FRAMES                                           # (hits of the three frames differ by the jitter only)
    plan = rt.wave_plan(W * H, spp, rt.default_render_params().aoSamples, hits=per_frame)      # options from the environment, as the lanes read them
    assert plan.options["budgetBytes"] == int(budget) << 20
    print(f"{scene}: {hits} hits in {FRAMES} frames, chunk {plan.chBudget} hits, {plan.nChunks} chunks per frame, bounce launches {bp.probeLaunches}")
    assert plan.nChunks >= 2
    assert bp.probeLaunches >= 2 * FRAMES and glb.listedLaunches >= 2     # frame by frame: two chunks per frame at least; the batch is cut too


# ---------------------------------------------------------------- 4. overflow answers beside a sparse occ2

@pytest.mark.gpu
def test_overflow_answers_beside_sparse_occ2(orc, monkeypatch):
    out, spp = qd._run(orc, monkeypatch, "two_mesh", {"RT_Q2_CAP": "64"}, stale=True)
    assert out[0][0].shaded > 64 * FRAMES                                # pairs beyond the queue: k_gen_gi_overflow wrote their answers


# ---------------------------------------------------------------- 5. the other writers and readers of the arrays

@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"RT_PACKET_AO": "1"}, {"RT_DENSE_TAKE": "0"}, {"RT_BIN_GI": "1"}], ids=["packet_ao", "dense_take_0", "bin_gi"])
def test_queue_options(orc, monkeypatch, env):
    out, _ = qd._run(orc, monkeypatch, "two_mesh", env)
    assert out[0][0].shaded > 1000


# ---------------------------------------------------------------- 6. rt_debug_trace kinds 2 - 4: their arrays are pre-filled by the entry

def _debug_rays(nodes, tris, n=384, seed=17):
    """n rays (a multiple of four) in packets of four that share an origin: packets aimed at the mesh, packets that point away from it from outside its box (known
    misses, about half) and a negative tMax -- an empty slot -- in every fifth ray."""
    rng = np.random.default_rng(seed)
    v0, e1, e2 = tris[:, 0:3], tris[:, 4:7], tris[:, 8:11]
    pts = np.concatenate([v0, v0 + e1, v0 + e2])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    mid, ext = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    P = n // 4
    org = np.repeat(mid + rng.normal(size=(P, 3)) / np.linalg.norm(rng.normal(size=(P, 3)), axis=1, keepdims=True) * ext, 4, axis=0)
    org = (mid + (org - mid) / np.linalg.norm(org - mid, axis=1, keepdims=True) * ext).astype(np.float32)      # on a sphere around the box
    toward = (mid + rng.uniform(-0.3, 0.3, (n, 3)) * (hi - lo)) - org
    d = toward / np.linalg.norm(toward, axis=1, keepdims=True)
    away = (np.arange(n) // 4) % 2 == 1
    d[away] = -d[away]                                                   # leaves the sphere: never meets the box
    tmax = rng.uniform(0.5, 3.0, n).astype(np.float32) * np.float32(ext)
    dead = np.arange(n) % 5 == 3
    tmax[dead] = np.float32(-1.0)
    return org, d.astype(np.float32), tmax, away, dead


def _debug_trace_into(r, kind, org, d, tmax, fill=0xCD):
    out = np.full((org.shape[0], 7), fill, np.uint8).repeat(4, axis=1).view(np.float32).copy()     # every byte 0xCD
    assert out.shape == (org.shape[0], 7) and (out.view(np.uint8) == fill).all()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    o, dd, t = np.ascontiguousarray(org, np.float32), np.ascontiguousarray(d, np.float32), np.ascontiguousarray(tmax, np.float32)
    r._check(rt.lib().rt_debug_trace(r._h, kind, fp(o), fp(dd), fp(t), 1e-4, 1e30, fp(out), o.shape[0]))
    return out


@pytest.mark.gpu
def test_debug_trace_answers_every_ray(orc):
    """Kinds 2 - 4 hand the frame's sources (QueueSrc, PacketSrc) device arrays of their own: misses, root-box misses and empty slots must read the documented
    answer (kind 2: t = inf, triangle -1; kinds 3 / 4: 0, an empty slot too) whatever the caller's output held before.  The host output is all overwritten by the
    entry, so the 0xCD fill alone cannot show a missing pre-fill of the DEVICE arrays; for that every checked call follows a call of the same kind and size
    whose rays are all aimed at the mesh with a long reach (most of them occluded): a device allocation handed out again then holds ones where the checked call
    has misses and empty slots."""
    nodes, tris = scenes.bunny_bvh(3)
    u = rt.frame_uniforms(rt.default_render_params(), rt.default_camera(), 64, 64, 0, True, nodes.shape[0], tris.shape[0])
    org, d, tmax, away, dead = _debug_rays(nodes, tris)
    n = org.shape[0]
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r:
        r.upload_bvh(nodes, tris)
        aimed = np.where(away[:, None], -d, d).astype(np.float32)
        reach = np.full(n, 1e30, np.float32)
        closest = _debug_trace_into(r, 2, org, d, tmax)
        assert _debug_trace_into(r, 3, org, aimed, reach)[:, 0].sum() > n // 2
        anyhit = _debug_trace_into(r, 3, org, d, tmax)
        assert _debug_trace_into(r, 4, org, aimed, reach)[:, 0].sum() > n // 2
        packets = _debug_trace_into(r, 4, org, d, tmax)
    hits = occluded = 0
    for i in range(n):
        hit, t, _, nn, _ = orc.trace_bvh(u, nodes, tris, org[i], d[i])
        hits += bool(hit)
        assert not (hit and away[i]), i
        if hit:
            assert closest[i, 0].view(np.uint32) == np.float32(t).view(np.uint32) and closest[i, 1] >= 0, i
            tri = int(closest[i, 1])                                     # the triangle the oracle's normal belongs to (as tests/test_gpu_parity.py checks it)
            g = np.cross(tris[tri, 4:7].astype(np.float64), tris[tri, 8:11].astype(np.float64))
            assert abs(abs(float(np.dot(g / np.linalg.norm(g), nn.astype(np.float64)))) - 1.0) < 1e-4, (i, tri)
        else:
            assert closest[i, 0] == np.float32(1e30) and closest[i, 1] == -1.0, (i, closest[i, :2])
        occ = (not dead[i]) and bool(orc.trace_bvh_shadow(u, nodes, tris, org[i], d[i], tmax[i]))
        occluded += occ
        assert anyhit[i, 0] == np.float32(occ) and packets[i, 0] == np.float32(occ), (i, dead[i], anyhit[i, 0], packets[i, 0], occ)
    assert (closest[:, 2:] == 0).all() and (anyhit[:, 1:] == 0).all() and (packets[:, 1:] == 0).all()
    print(f"{n} rays: {hits} hit, {occluded} occluded, {int(away.sum())} point away, {int(dead.sum())} empty slots")
    assert hits > n // 8 and occluded > n // 16 and away.sum() >= n // 2 - 4 and dead.sum() > n // 8
    assert (anyhit[dead, 0] == 0).all() and (packets[dead, 0] == 0).all()


# ---------------------------------------------------------------- 7. nothing is traced differently

@pytest.mark.gpu
@pytest.mark.parametrize("probe", ["1", "0"])
def test_two_mesh_counters_equal_the_cpu(orc, monkeypatch, probe):
    """Hit pixels from the frame's own G-buffer and casting (hit, sample) pairs from the frame's random numbers (qd.bounce_casts), per frame, against
    rt_get_traced_rays and rt_debug_bounce_probe: the launches trace the rays they traced before."""
    monkeypatch.setenv("RT_BOUNCE_PROBE", probe)
    us, wants = qd._uniforms("two_mesh"), qd._oracle(orc, "two_mesh")
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r:
        qd._prepare(r, "two_mesh")
        for f, u in enumerate(us):
            r.render_frame(u)
            got = r.read_all()
            qd._equal(got, wants[f], orc, f"two_mesh frame {f}")
            hit = _hit(got)
            cast, near = qd.bounce_casts(hit, f, SPP)
            bp, tr = r.bounce_probe(reset=True), r.traced_rays(reset=True)
            print(f"frame {f}: hits {int(hit.sum())} / {tr.hitPixels}, casting pairs CPU {int(cast.sum())} (near the threshold {near}), bounce rays {tr.bounce}, "
                  f"probed {bp.probed}, re-traced {bp.retraced}, candidates {tr.candidatePixels}, primary {tr.primary}")
            assert tr.hitPixels == hit.sum() and tr.frames == 1
            assert tr.primary == tr.candidatePixels >= tr.hitPixels
            assert abs(int(cast.sum()) - int(tr.bounce)) <= near, (int(cast.sum()), tr.bounce, near)
            if probe == "1":
                assert bp.probed == tr.bounce and 0 < bp.retraced < bp.probed and bp.closestLaunches == 0
            else:
                assert bp.probed == 0 and bp.retraced == 0 and bp.probeLaunches == 0 and bp.closestLaunches > 0
