"""The disk-light skip of the wavefront shading stages: a wave whose hits all satisfy diskUnlit (rt_device_shade.hpp) does not evaluate
the four disk samples.

* the predicate against the production code: rt_debug_disk_unlit evaluates diskUnlit(hp, N) and, for the same pair, diskSample for all four samples
  of 64 (pixel, frame) seeds.  No pair that the test calls unlit may have a sample with geom != 0 or a computed dot(N, L) above zero.  The inputs
  straddle the predicate's threshold by +-1e-2 (half on either side by construction; checked on the CPU in float64 first).
* frames: three scenes -- most hits unlit, most hits lit, bounce hits with shadow queue 2 overflowing -- bit-identical to the oracle frame by frame
  and batched, on one frame lane and on four, and under the queue options; rt_debug_disk_skip says which path ran.
"""
import functools

import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scenes

# diskUnlit's constants (rt_device_shade.hpp) and the light's centre (rt_lighting.glsl:29)
K_R, K_TAU = 1.21, 1e-4
LIGHT_C = np.array([0.0, 5.0, -3.0])
W, H = 160, 96
VARS = ("RT_BOUNCE_PROBE", "RT_BIN_GI", "RT_QUEUE_BUDGET_MB", "RT_Q2_CAP", "RT_LANES", "RT_ARENAS", "RT_DENSE_TAKE", "RT_PACKET_AO", "RT_CHUNKS_FROM_SLOTS")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "two_mesh":   # two copies facing each other: bounce rays hit the other copy
        v, f = rt.meshgen.bunny_standin(4)
        a = rt.gather_triangles(v, f)
        b = a.copy()
        b[:, 0] += np.float32(0.7); b[:, 2] += np.float32(0.5)
        return rt.build_bvh(np.concatenate([a, b]).astype(np.float32))
    return scenes.bunny_bvh(3)


def _margin64(hp, n):
    """Left side minus right side of diskUnlit in float64, on the float32 inputs."""
    hp, n = hp.astype(np.float64), n.astype(np.float64)
    v = LIGHT_C - hp
    ln, lv = np.linalg.norm(n, axis=1), np.linalg.norm(v, axis=1)
    return np.sum(n * v, axis=1) + K_R * ln + K_TAU * ln * (lv + K_R)


def threshold_pairs(count=120_000, seed=17):
    """(hp, N, m): hp in the root boxes of the test scenes (grown by a quarter), N a unit vector placed so that diskUnlit's left side minus its right
    side is m, uniform in [-1e-2, 1e-2]: cos(theta) = (m - R - tau (|v| + R)) / |v| against v = c - hp, the rest of N along a random direction normal to v."""
    rng = np.random.default_rng(seed)
    boxes = []
    for name in ("bunny", "two_mesh"):
        nodes, _ = _mesh(name)
        lo, hi = nodes[0, 0:3].astype(np.float64), nodes[0, 4:7].astype(np.float64)
        boxes.append((lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo)))
    which = rng.integers(0, len(boxes), count)
    lo = np.array([boxes[k][0] for k in which]); hi = np.array([boxes[k][1] for k in which])
    hp = lo + rng.random((count, 3)) * (hi - lo)
    v = LIGHT_C - hp
    lv = np.linalg.norm(v, axis=1)
    assert lv.min() > 3.0          # so that the expression below is a cosine
    m = rng.uniform(-1e-2, 1e-2, count)
    cos = (m - K_R - K_TAU * (lv + K_R)) / lv
    sin = np.sqrt(1.0 - cos * cos)
    w = np.cross(v, rng.normal(size=(count, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    n = cos[:, None] * v / lv[:, None] + sin[:, None] * w
    return hp.astype(np.float32), n.astype(np.float32), m


def special_pairs(seed=23):
    """(hp, N, expected): axis-parallel normals, components of denormal size, normals that are not unit vectors, |N| = 0, NaN and infinities.
    expected: True = must be called unlit, False = must not, None = either."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    hp, n, exp = [], [], []
    nodes, _ = _mesh("bunny")
    lo, hi = nodes[0, 0:3].astype(np.float64), nodes[0, 4:7].astype(np.float64)
    pts = (lo + rng.random((64, 3)) * (hi - lo)).astype(f32)
    tiny = [f32(1e-40), f32(-1e-42), f32(1.4e-45), f32(-0.0), f32(0.0)]
    for p in pts:
        v = LIGHT_C - p.astype(np.float64)
        away = (-v / np.linalg.norm(v)).astype(f32)
        for a in range(3):
            for s in (1.0, -1.0):
                e = np.zeros(3, f32); e[a] = s
                hp.append(p); n.append(e); exp.append(None)
                for t in tiny:            # the other two components of denormal size / signed zero
                    d = np.full(3, t, f32); d[a] = s
                    hp.append(p); n.append(d); exp.append(None)
        hp.append(p); n.append(away); exp.append(True)              # squarely facing away
        hp.append(p); n.append(-away); exp.append(False)            # squarely facing the light
        for scale in (0.25, 4.0, 1e-20, 1e20, 1e-42):              # not a normalised vector: today's path
            hp.append(p); n.append((away.astype(np.float64) * scale).astype(f32)); exp.append(False)
        hp.append(p); n.append(np.zeros(3, f32)); exp.append(False)
        for bad in (np.nan, np.inf, -np.inf):
            for a in range(3):
                d = away.copy(); d[a] = bad
                hp.append(p); n.append(d); exp.append(False)
                q = p.copy(); q[a] = bad
                hp.append(q); n.append(away); exp.append(False)
        hp.append((p.astype(np.float64) * 1e30).astype(f32)); n.append(away); exp.append(None)   # |c - hp|^2 overflows
    return np.array(hp, f32), np.array(n, f32), exp


def test_threshold_pairs_fall_on_both_sides():
    """The generator's promise, checked where no GPU is needed: in float64 at least a quarter of the pairs satisfy the predicate and at least a quarter
    do not, and the margin the float32 inputs realise is the drawn one up to rounding."""
    hp, n, m = threshold_pairs()
    got = _margin64(hp, n)
    assert hp.shape[0] >= 100_000
    assert np.abs(got - m).max() < 1e-5, np.abs(got - m).max()
    assert (got < 0).mean() >= 0.25 and (got >= 0).mean() >= 0.25, ((got < 0).mean(), (got >= 0).mean())
    assert got.min() < -9e-3 and got.max() > 9e-3


@pytest.mark.gpu
def test_unlit_pairs_have_no_live_disk_sample():
    hp, n, m = threshold_pairs()
    shp, sn, exp = special_pairs()
    u = rt.frame_uniforms(rt.default_render_params(), rt.default_camera(), 64, 64, 0, True, 1, 1)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r:
        unlit, lit, md = r.debug_disk_unlit(u, np.concatenate([hp, shp]), np.concatenate([n, sn]), seeds=64)
    k = hp.shape[0]
    share = unlit[:k].mean()
    print(f"threshold pairs: {k}, unlit {share:.4f}; largest dot(N, L) among unlit pairs {md[unlit].max():.3e}; special pairs {len(exp)}, unlit {unlit[k:].mean():.4f}")
    bad = np.flatnonzero(unlit & lit)
    assert bad.size == 0, (bad[:8], md[bad[:8]])
    assert not np.any(md[unlit] > 0.0), md[unlit].max()            # (-0.0 passes; NaN cannot be unlit)
    assert share >= 0.25 and 1.0 - share >= 0.25, share
    # the float32 test agrees with the float64 one outside the band that rounding can move
    m64 = _margin64(hp, n)
    clear = np.abs(m64) > 1e-5
    assert np.array_equal(unlit[:k][clear], (m64 < 0)[clear])
    for i, e in enumerate(exp):
        assert e is None or bool(unlit[k + i]) == e, (i, shp[i], sn[i], e)
    # the pairs just above the threshold are what the margins give away: most of them are in fact dead
    print(f"pairs not called unlit whose samples are all dead: {(~unlit[:k] & ~lit[:k]).mean():.4f}")


# ---------------------------------------------------------------- frames

def _camera(scene):
    cam = scenes.camera("closeup", aspect=W / H)
    if scene == "lightside":   # the mesh seen from the light's side
        nodes, _ = _mesh("bunny")
        c = 0.5 * (nodes[0, 0:3] + nodes[0, 4:7])
        cam.pos[0], cam.pos[1], cam.pos[2] = float(c[0]), float(c[1]), float(c[2]) - 3.0
        cam.yaw = 90.0
    return cam


SCENES = {"closeup": "bunny", "lightside": "bunny", "two_mesh": "two_mesh"}


def _uniforms(scene, frames=3, spp=2):
    nodes, tris = _mesh(SCENES[scene])
    p = rt.default_render_params()
    p.sppPerFrame = spp
    return [rt.frame_uniforms(p, _camera(scene), W, H, f, True, nodes.shape[0], tris.shape[0]) for f in range(frames)]


@functools.lru_cache(maxsize=None)
def _oracle(orc, scene):
    nodes, tris = _mesh(SCENES[scene])
    wants, prev = [], None
    for u in _uniforms(scene):
        want, _ = orc.render(u, nodes, tris, scenes.tiny_env(8), prev, nthreads=16)
        wants.append(want)
        prev = want[0]
    return wants


def _equal(got, want, orc, what):
    for g, w, n in zip(got, want, ("color", "motion", "gpos", "gnrm")):
        st = orc.compare(g, w)
        assert st["bit_diff"] == 0, f"{what}/{n}: not bit-identical: {st}"


def _run(orc, monkeypatch, scene, env):
    env = dict(env)
    if scene == "two_mesh":
        env.setdefault("RT_Q2_CAP", "64")     # shadow queue 2 overflows: k_gen_gi_overflow shades bounce hits too
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nodes, tris = _mesh(SCENES[scene])
    us, wants = _uniforms(scene), _oracle(orc, scene)
    what = f"{scene} {env}"
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r, rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as rb:
        for x in (r, rb):
            x.upload_bvh(nodes, tris); x.upload_env(scenes.tiny_env(8)); x.resize(W, H)
            x.disk_skip(reset=True)           # switches the counting on
        for f, u in enumerate(us):
            r.render_frame(u)
            _equal(r.read_all(), wants[f], orc, f"{what} frame {f}")
        rb.render_frames(us)
        _equal(rb.read_all(), wants[-1], orc, f"{what} batch")
        ds, dsb = r.disk_skip(), rb.disk_skip()
        hits = r.traced_rays().hitPixels
    for d in (ds, dsb):
        assert d.directSkipped <= d.directUnlit <= d.directPairs and d.giSkipped <= d.giUnlit <= d.giPairs, what
        assert d.directWavesSkipped <= d.directWaves and d.giWavesSkipped <= d.giWaves, what
    assert ds.directPairs == dsb.directPairs == 2 * hits > 0, (what, ds.directPairs, dsb.directPairs, hits)   # every (hit, sample) pair of the three frames
    assert ds.directUnlit == dsb.directUnlit and ds.giPairs == dsb.giPairs and ds.giUnlit == dsb.giUnlit, what
    print(f"{what}: direct pairs {ds.directPairs} unlit {ds.directUnlit / ds.directPairs:.3f} skipped {ds.directSkipped / ds.directPairs:.3f} "
          f"(batched {dsb.directSkipped / dsb.directPairs:.3f}) waves {ds.directWavesSkipped}/{ds.directWaves} | "
          f"gi pairs {ds.giPairs} unlit {ds.giUnlit / max(ds.giPairs, 1):.3f} skipped {ds.giSkipped / max(ds.giPairs, 1):.3f} waves {ds.giWavesSkipped}/{ds.giWaves}")
    return ds, dsb


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", ["1", "4"])
@pytest.mark.parametrize("scene", list(SCENES))
def test_frames_equal_the_oracle(orc, monkeypatch, scene, lanes):
    ds, dsb = _run(orc, monkeypatch, scene, {"RT_LANES": lanes})
    for d in (ds, dsb):
        share = d.directSkipped / d.directPairs
        if scene == "closeup":
            assert share > 0.5, share         # the skip ran
        if scene == "lightside":
            assert share < 0.5, share         # the loop ran
        if scene == "two_mesh":
            assert d.giPairs > 0              # bounce hits were shaded


OPTIONS = {
    "chunked": {"RT_QUEUE_BUDGET_MB": "1"},
    "dense_take_0": {"RT_DENSE_TAKE": "0"},
    "bin_gi": {"RT_BIN_GI": "1"},
    "packet_ao": {"RT_PACKET_AO": "1"},
    "no_bounce_probe": {"RT_BOUNCE_PROBE": "0"},
}


@pytest.mark.gpu
@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("scene", list(SCENES))
def test_frames_equal_the_oracle_under_queue_options(orc, monkeypatch, scene, option):
    _run(orc, monkeypatch, scene, OPTIONS[option])
