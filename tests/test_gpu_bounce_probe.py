"""RT_BOUNCE_PROBE: the bounce rays walked any-hit first with tMax = uINF, misses answered there, hits re-traced closest-hit.

Under RT_BOUNCE_PROBE=0, 1 and auto every case renders the oracle's frames bit for bit (so the three modes also equal each other).  Each case
checks through rt_debug_builds that the probe ran exactly where it may (the RT_BUILD_BOUNCE_PROBE bit of the any-hit half) and, through
rt_debug_bounce_probe, that it walked every bounce ray (=1), wrote the misses itself and handed the hits to the re-trace.
"""
import functools

import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scenes

pytestmark = pytest.mark.gpu

PROBE_BIT = rt.RT_BUILD_BOUNCE_PROBE << rt.RT_BUILD_ANY_SHIFT
VARS = ("RT_BOUNCE_PROBE", "RT_BIN_GI", "RT_QUEUE_BUDGET_MB", "RT_ANYHIT_TREE", "RT_Q2_CAP", "RT_LANES", "RT_CHUNKS_FROM_SLOTS")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)


def _floor_and_wall(y0, n=24, half=2.0):
    """Axis-parallel geometry: a floor grid in the plane y = y0 (flat leaf boxes) and a wall in the plane z = -half (flat in z)."""
    g = np.linspace(-half, half, n + 1, dtype=np.float32)
    tris = []
    for i in range(n):
        for k in range(n):
            a, b, c, d = (g[i], g[k]), (g[i + 1], g[k]), (g[i + 1], g[k + 1]), (g[i], g[k + 1])
            tris += [[a[0], y0, a[1], b[0], y0, b[1], c[0], y0, c[1]], [a[0], y0, a[1], c[0], y0, c[1], d[0], y0, d[1]]]
            tris += [[a[0], y0 + a[1] + half, -half, b[0], y0 + b[1] + half, -half, c[0], y0 + c[1] + half, -half],
                     [a[0], y0 + a[1] + half, -half, c[0], y0 + c[1] + half, -half, d[0], y0 + d[1] + half, -half]]
    return np.array(tris, np.float32)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "bench":                 # bench.py's mesh: the bunny stand-in at subdivision 6 (81 920 triangles)
        return scenes.bunny_bvh(6)
    v, f = rt.meshgen.bunny_standin(4)
    a = rt.gather_triangles(v, f)
    if name == "facing":                # two copies facing each other: many bounce rays hit the other copy (the re-trace carries load)
        b = a.copy()
        b[:, 0] += np.float32(0.7); b[:, 2] += np.float32(0.5)
        b[:, 3] += np.float32(0.7); b[:, 5] += np.float32(0.5)
        b[:, 6] += np.float32(0.7); b[:, 8] += np.float32(0.5)
        return rt.build_bvh(np.concatenate([a, b], 0))
    if name == "floor":                 # the bunny on an axis-parallel floor in front of a wall: flat boxes, grazing bounce rays
        y0 = float(a[:, 1::3].min())
        return rt.build_bvh(np.concatenate([a, _floor_and_wall(y0)], 0))
    raise KeyError(name)


def _uniforms(mesh, W, H, frames, spp, gi=True, moving=False):
    nodes, tris = _mesh(mesh)
    p = rt.default_render_params()
    p.sppPerFrame = spp
    if not gi:
        p.enableGI = 0
    us, prev_vp = [], None
    for f in range(frames):
        cam = scenes.camera("closeup", aspect=W / H)
        if moving:
            cam.pos[0] += 0.03 * f; cam.yaw += 0.7 * f
        vp = rt.mat4_mul(rt.camera_proj(cam), rt.camera_view(cam))
        us.append(rt.frame_uniforms(p, cam, W, H, f, True, nodes.shape[0], tris.shape[0], prev_vp=prev_vp if moving else None))
        prev_vp = vp
    return us


@functools.lru_cache(maxsize=None)
def _oracle(orc, mesh, W, H, frames, spp, gi, moving):
    nodes, tris = _mesh(mesh)
    wants, prev = [], None
    for u in _uniforms(mesh, W, H, frames, spp, gi, moving):
        want, _ = orc.render(u, nodes, tris, scenes.tiny_env(8), prev, nthreads=16)
        wants.append(want)
        prev = want[0]
    return wants


def _equal(got, want, orc, what):
    for g, w, n in zip(got, want, ("color", "motion", "gpos", "gnrm")):
        st = orc.compare(g, w)
        assert st["bit_diff"] == 0, f"{what}/{n}: not bit-identical: {st}"


def _run(orc, monkeypatch, mode, mesh, *, W=128, H=72, frames=3, spp=2, gi=True, moving=False, env=None):
    """Renders the frames frame by frame and as one batch under RT_BOUNCE_PROBE=mode, both against the oracle; returns the build bits,
    the probe counts and the traced rays of the frame-by-frame renderer."""
    for k, v in dict(env or {}, RT_BOUNCE_PROBE=mode).items():
        monkeypatch.setenv(k, v)
    nodes, tris = _mesh(mesh)
    us = _uniforms(mesh, W, H, frames, spp, gi, moving)
    wants = _oracle(orc, mesh, W, H, frames, spp, gi, moving)
    what = f"{mesh} RT_BOUNCE_PROBE={mode} {env or ''}"
    collapsed = (env or {}).get("RT_ANYHIT_TREE") != "sah"   # the probe's exactness needs the any-hit tree to be the binary one collapsed
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r, rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as rb:
        for x in (r, rb):
            x.upload_bvh(nodes, tris); x.upload_env(scenes.tiny_env(8)); x.resize(W, H)
            x.debug_build_bits(reset=True); x.bounce_probe(reset=True); x.traced_rays(reset=True)
        for f, u in enumerate(us):
            r.render_frame(u)
            _equal(r.read_all(), wants[f], orc, f"{what} frame {f}")
        rb.render_frames(us)
        _equal(rb.read_all(), wants[-1], orc, f"{what} batch of {frames}")
        bits, bp, tr = r.debug_build_bits(), r.bounce_probe(), r.traced_rays()
        bitsB, bpB, trB = rb.debug_build_bits(), rb.bounce_probe(), rb.traced_rays()
    assert tr.bounce == trB.bounce, what                 # each bounce ray counted once, probed or not
    for b, p, t in ((bits, bp, tr), (bitsB, bpB, trB)):
        assert p.retraced <= p.probed <= t.bounce, (what, p.probed, p.retraced, t.bounce)
        assert bool(b & PROBE_BIT) == (p.probeLaunches > 0), what
        if mode == "1" and gi and collapsed:            # every bounce launch probed, every bounce ray walked any-hit first
            assert p.closestLaunches == 0 and p.probeLaunches > 0 and p.probed == t.bounce > 0, (what, p.probed, t.bounce)
        if mode == "0" or not gi or not collapsed:
            assert p.probeLaunches == 0 and p.probed == 0 and not b & PROBE_BIT, what
    return bits, bp, tr


@pytest.mark.parametrize("mode", ["0", "1", "auto"])
def test_bench_mesh(orc, monkeypatch, mode):
    _run(orc, monkeypatch, mode, "bench")


@pytest.mark.parametrize("mode", ["0", "1", "auto"])
def test_bounce_hits_retraced(orc, monkeypatch, mode):
    """Two meshes facing each other: a large share of the bounce rays hit, so the re-trace launch does real work."""
    _, bp, tr = _run(orc, monkeypatch, mode, "facing", spp=3)
    if mode == "1":
        assert bp.retraced > 0.01 * bp.probed, (bp.retraced, bp.probed)   # the probe found the hits and handed them on


@pytest.mark.parametrize("mode", ["0", "1", "auto"])
def test_axis_parallel_and_grazing(orc, monkeypatch, mode):
    """Flat leaf boxes (a floor and a wall in coordinate planes), grazing bounce rays along the floor, rays that leave into the sky (tMax = uINF)."""
    _, bp, _ = _run(orc, monkeypatch, mode, "floor", spp=2)
    if mode == "1":
        assert bp.retraced > 0 and bp.probed > bp.retraced


@pytest.mark.parametrize("mode", ["0", "1", "auto"])
def test_moving_camera(orc, monkeypatch, mode):
    _run(orc, monkeypatch, mode, "floor", frames=3, moving=True)


@pytest.mark.parametrize("mode", ["0", "1", "auto"])
def test_gi_off(orc, monkeypatch, mode):
    _, bp, _ = _run(orc, monkeypatch, mode, "bench", gi=False)
    assert bp.probeLaunches == 0 and bp.closestLaunches == 0


@pytest.mark.parametrize("mode", ["0", "1", "auto"])
def test_bin_gi(orc, monkeypatch, mode):
    """RT_BIN_GI=1: the bounce queue addressed through giPerm; the probe and the re-trace work on queue addresses and keep it."""
    _run(orc, monkeypatch, mode, "facing", env={"RT_BIN_GI": "1"})


@pytest.mark.parametrize("mode", ["0", "1", "auto"])
def test_chunked(orc, monkeypatch, mode):
    """RT_QUEUE_BUDGET_MB=1: several chunks per launch set, one probe (and hit list) per chunk.  Eight frames frame by frame: lanes see a second
    launch set, so the share of bounce hits is known and auto probes."""
    _, bp, _ = _run(orc, monkeypatch, mode, "bench", W=160, H=96, frames=8, env={"RT_QUEUE_BUDGET_MB": "1"})
    if mode == "auto":
        assert bp.probeLaunches > 0 and bp.closestLaunches > 0, (bp.probeLaunches, bp.closestLaunches)


@pytest.mark.parametrize("mode", ["1", "auto"])
def test_sah_tree_never_probes(orc, monkeypatch, mode):
    """RT_ANYHIT_TREE=sah walks a different tree, where a triangle's hit may fall a rounding outside its leaf's box: the probe must not run."""
    _, bp, _ = _run(orc, monkeypatch, mode, "bench", env={"RT_ANYHIT_TREE": "sah", "RT_QUEUE_BUDGET_MB": "1"}, W=160, H=96, frames=6)
    assert bp.probeLaunches == 0 and bp.probed == 0 and bp.closestLaunches > 0


def test_share_forgotten_on_new_scene(orc, monkeypatch):
    """auto: a context that learnt one scene's share of bounce hits starts the next scene (rt_upload_bvh) and a new frame size (rt_resize) with the
    closest-hit launch alone -- nothing known yet."""
    monkeypatch.setenv("RT_BOUNCE_PROBE", "auto")
    monkeypatch.setenv("RT_QUEUE_BUDGET_MB", "1")
    nodes, tris = _mesh("bench")
    us = _uniforms("bench", 160, 96, 8, 2)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r:
        r.upload_bvh(nodes, tris); r.upload_env(scenes.tiny_env(8)); r.resize(160, 96)
        for u in us:
            r.render_frame(u)
        assert r.bounce_probe(reset=True).probeLaunches > 0
        for again in (lambda: r.upload_bvh(nodes, tris), lambda: r.resize(160, 96)):
            again()
            r.bounce_probe(reset=True)
            r.render_frame(us[0])
            bp = r.bounce_probe(reset=True)
            assert bp.probeLaunches == 0 and bp.closestLaunches > 0, (bp.probeLaunches, bp.closestLaunches)
