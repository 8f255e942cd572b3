"""Every kept traversal and scheduler option of the wavefront pipeline ("Environment knobs") against the oracle, bit for bit.

Each case sets its variables before the Renderer is created and asserts, through rt_debug_builds, the k_trace / k_trace_packets build that
launch_trace chose -- a test that passes because the variable was ignored is worth nothing.  Ray by ray: rt_debug_trace kinds 2 / 3 launch the
build a frame launches under the same environment (tune_from_env), kind 4 the packet kernel of RT_PACKET_AO.  Frames: two renderers, one
frame by frame and one batch (rt_render_frames), all four targets against orc.render.
"""
import functools

import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scenes

pytestmark = pytest.mark.gpu

# every variable a case sets, deleted first so that no case inherits one (e.g. from a stress run over the whole suite)
OPTION_VARS = ("RT_COOP", "RT_FUSED", "RT_IMPLICIT", "RT_NEAR_FIRST", "RT_QNODES", "RT_QNODES_SPARSE_BOXES", "RT_ANYHIT_TREE", "RT_LEAFB",
               "RT_LEAFB_CLOSEST", "RT_QUAD_REFILL", "RT_REFILL_MIN", "RT_GUIDED", "RT_CHUNK", "RT_MIN_SEARCH", "RT_CHUNK_PRIMARY", "RT_GRID_PCT",
               "RT_GRID_PCT_PRIMARY", "RT_REVERSE", "RT_DENSE_TAKE", "RT_PACKET_AO", "RT_BIN_GI", "RT_Q2_CAP", "RT_Q2_PREDICT", "RT_CU_SPLIT",
               "RT_SHADE_PRIORITY", "RT_TRACE_STATS", "RT_TRACE_TIMING", "RT_QUEUE_BUDGET_MB", "RT_DEBUG_SKIP_TRAVERSAL", "RT_CHUNKS_FROM_SLOTS", "RT_ARENAS")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in OPTION_VARS:
        monkeypatch.delenv(v, raising=False)


def _set(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _builds(closest, any_):
    b = lambda s: frozenset({"k_trace"} | set(s)) if s is not None else frozenset()
    return {"closest": b(closest), "any": b(any_)}


def _assert_targets_equal(got, want, orc, what):
    for g, w, n in zip(got, want, ["color", "motion", "gpos", "gnrm"]):
        st = orc.compare(g, w)
        assert st["bit_diff"] == 0, f"{what}/{n}: not bit-identical: {st}"


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "one_leaf":
        nodes, tris = scenes.one_leaf_mesh()
        assert nodes.shape[0] == 1
        return nodes, tris
    if name == "million":
        v, f = rt.meshgen.million_triangle_scene()
        return rt.build_bvh(rt.gather_triangles(v, f, np.eye(4, dtype=np.float32).reshape(-1)))
    if name == "two_mesh":   # test_shadow_queue_2_overflow_is_traced_in_place: two copies facing each other, bounce rays hit the other
        v, f = rt.meshgen.bunny_standin(4)
        a = rt.gather_triangles(v, f)
        b = a.copy()
        b[:, 0] += np.float32(0.7); b[:, 2] += np.float32(0.5)
        return rt.build_bvh(np.concatenate([a, b]).astype(np.float32))
    return scenes.bunny_bvh(4)   # 5120 triangles, depth-12 tree


def _uniforms(nodes, tris):
    return rt.frame_uniforms(rt.default_render_params(), rt.default_camera(), 64, 64, 0, True, nodes.shape[0], tris.shape[0])


# ---------------------------------------------------------------- ray by ray (kinds 2 / 3)

@functools.lru_cache(maxsize=None)
def _adversarial(mesh):
    """The rays of scenes.adversarial_rays and the oracle's answers to them (computed once per mesh, shared by every option)."""
    import oracle as orc
    nodes, tris = _mesh(mesh)
    u = _uniforms(nodes, tris)
    org, dirs, tmax = scenes.adversarial_rays(nodes, tris)
    N = org.shape[0]
    hit = np.zeros(N, bool); t = np.zeros(N, np.float32); nn = np.zeros((N, 3), np.float32); occ = np.zeros(N, bool)
    for i in range(N):
        h, t_, _, n_, _ = orc.trace_bvh(u, nodes, tris, org[i], dirs[i])
        hit[i], t[i], nn[i] = h, t_, n_
        occ[i] = orc.trace_bvh_shadow(u, nodes, tris, org[i], dirs[i], tmax[i])
    return org, dirs, tmax, hit, t, nn, occ


RAY_CASES = {   # id: (mesh, environment, extra bits of the closest-hit build, of the any-hit build)
    "coop": ("bunny", {"RT_COOP": "1"}, {"COOP"}, set()),
    "coop_fused": ("bunny", {"RT_COOP": "1", "RT_FUSED": "1"}, {"COOP"}, set()),                    # fused yields to COOP
    "coop_implicit": ("bunny", {"RT_COOP": "1", "RT_IMPLICIT": "1"}, {"COOP"}, {"IMPL"}),          # (implicit closest-hit records yield to COOP too)
    "near": ("bunny", {"RT_NEAR_FIRST": "1"}, set(), {"NEAR"}),
    "near_qnodes2": ("bunny", {"RT_NEAR_FIRST": "1", "RT_QNODES": "2"}, set(), {"NEAR"}),          # near-first walks the exact nodes
    "near_sah": ("bunny", {"RT_NEAR_FIRST": "1", "RT_ANYHIT_TREE": "sah"}, set(), {"NEAR"}),
    "leafb4": ("bunny", {"RT_LEAFB": "4"}, {"LEAFB4"}, {"LEAFB4"}),
    "leafb4_implicit": ("bunny", {"RT_LEAFB": "4", "RT_IMPLICIT": "1"}, {"IMPL"}, {"LEAFB4"}),     # implicit any-hit needs leafb < 4
    "leafb_closest4": ("bunny", {"RT_LEAFB_CLOSEST": "4"}, {"LEAFB4"}, set()),
    "quad_refill": ("bunny", {"RT_QUAD_REFILL": "1", "RT_REFILL_MIN": "8"}, set(), set()),
    "guided1": ("bunny", {"RT_GUIDED": "1"}, set(), set()),
    "guided2": ("bunny", {"RT_GUIDED": "2"}, set(), set()),
    "chunk_min_search": ("bunny", {"RT_CHUNK": "8", "RT_MIN_SEARCH": "64"}, set(), set()),
    "qnodes2_sparse_boxes": ("bunny", {"RT_QNODES": "2", "RT_QNODES_SPARSE_BOXES": "1"}, set(), {"QN2"}),
    "qnodes2_leafb4": ("bunny", {"RT_QNODES": "2", "RT_LEAFB": "4"}, {"LEAFB4"}, {"QN2"}),       # quantised wins over RT_LEAFB=4
    "one_leaf_coop": ("one_leaf", {"RT_COOP": "1"}, {"COOP"}, set()),
    "one_leaf_near": ("one_leaf", {"RT_NEAR_FIRST": "1"}, set(), {"NEAR"}),
}


@pytest.mark.parametrize("case", list(RAY_CASES))
def test_option_ray_by_ray_on_adversarial_rays(orc, monkeypatch, case):
    """rt_debug_trace kinds 2 / 3 under one option: the build it selects, answer by answer against the oracle's traceBVH / traceBVHShadow on the
    adversarial rays of test_wavefront_traversal_kernels_ray_by_ray_on_adversarial_rays."""
    mesh, env, want_closest, want_any = RAY_CASES[case]
    _set(monkeypatch, env)
    nodes, tris = _mesh(mesh)
    org, dirs, tmax, hit, t, nn, occ = _adversarial(mesh)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r:
        r.upload_bvh(nodes, tris)
        r.debug_builds(reset=True)
        closest = r.debug_trace(2, org, dirs)
        assert r.debug_builds() == _builds(want_closest, None), case
        anyhit = r.debug_trace(3, org, dirs, tmax)
        assert r.debug_builds() == _builds(None, want_any), case
    # closest hit: the same t bits, and the triangle the oracle's normal belongs to
    assert np.array_equal(closest[hit, 0].view(np.uint32), t[hit].view(np.uint32)), (case, np.flatnonzero(closest[hit, 0].view(np.uint32) != t[hit].view(np.uint32))[:8])
    assert np.all(closest[~hit, 0] == np.float32(1e30)), (case, np.flatnonzero(closest[~hit, 0] != np.float32(1e30))[:8])
    tri = closest[hit, 1].astype(np.int64)
    assert np.all(tri >= 0)
    g = np.cross(tris[tri, 4:7].astype(np.float64), tris[tri, 8:11].astype(np.float64))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    assert np.all(np.abs(np.abs(np.sum(g * nn[hit].astype(np.float64), axis=1)) - 1.0) < 1e-4), case
    bad = np.flatnonzero(anyhit[:, 0].astype(bool) != occ)
    assert bad.size == 0, (case, bad[:8])
    N = org.shape[0]
    assert mesh == "one_leaf" or (hit.sum() > N // 8 and occ.sum() > N // 16)


# ---------------------------------------------------------------- packets (kind 4)

def packet_rays(nodes, tris, packets, seed=5):
    """(origins, dirs, tmax) of `packets` packets of four any-hit rays that leave one point, as computeAO's do: origins are triangle vertices and
    edge midpoints offset along the normal by aoBias, directions spread over the hemisphere, tmax 0.05 - 1.5 times the root extent.  Mixed in:
    packets on box planes with axis-parallel directions, direction components of denormal size and -0.0, and packets with one to three live
    rays (tmax < 0 marks an empty slot)."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    lo, hi = nodes[:, 0:3], nodes[:, 4:7]
    ext = float((hi[0] - lo[0]).max())
    bias = f32(rt.default_render_params().aoBias)
    P = packets
    k = rng.integers(0, tris.shape[0], P)
    v0, e1, e2 = tris[k, 0:3], tris[k, 4:7], tris[k, 8:11]
    which = rng.integers(0, 4, P)    # vertex 0, midpoint of e1, of e2, of the third edge
    p = np.where((which == 0)[:, None], v0, np.where((which == 1)[:, None], v0 + f32(0.5) * e1,
                 np.where((which == 2)[:, None], v0 + f32(0.5) * e2, v0 + f32(0.5) * (e1 + e2)))).astype(f32)
    n = np.cross(e1, e2).astype(f32)
    n = (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)).astype(f32)
    n = np.where((rng.random(P) < 0.5)[:, None], n, -n).astype(f32)
    o = (p + n * bias).astype(f32)
    org = np.repeat(o, 4, axis=0)
    d = rng.normal(size=(P * 4, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    nn4 = np.repeat(n, 4, axis=0)
    d = np.where((np.sum(d * nn4, axis=1) < 0)[:, None], -d, d)
    dirs = d.astype(f32)
    tmax = (rng.uniform(0.05, 1.5, P * 4) * ext).astype(f32)
    # packets on box planes: origin coordinates from a node's corner, four axis-parallel directions
    q = rng.choice(P, P // 8, replace=False)
    for axis in range(3):
        sel = q[q % 3 == axis]
        kk = rng.integers(0, nodes.shape[0], sel.size)
        corner = np.where(rng.random((sel.size, 3)) < 0.5, lo[kk], hi[kk]).astype(f32)
        for r in range(4):
            org[sel * 4 + r] = corner
            dd = np.zeros((sel.size, 3), f32)
            ax = (axis + r) % 3
            dd[:, ax] = np.where(rng.random(sel.size) < 0.5, f32(-1.0), f32(1.0))
            dirs[sel * 4 + r] = dd
    # denormal and -0.0 direction components
    m = rng.random(P * 4) < 0.1
    comp = rng.integers(0, 3, P * 4)
    dirs[m, comp[m]] = np.where(rng.random(m.sum()) < 0.5, f32(1e-41), f32(-0.0))
    # packets with one, two and three live rays (also with slot 0 empty: the origin is still taken from it)
    live = rng.integers(1, 4, P)
    short = rng.random(P) < 0.25
    for i in np.flatnonzero(short):
        dead = rng.choice(4, 4 - live[i], replace=False)
        tmax[i * 4 + dead] = f32(-1.0)
    return org, dirs, tmax


PACKET_CASES = {   # id: (mesh, environment, packets, extra bits of the any-hit k_trace build of the same environment)
    "one_leaf": ("one_leaf", {}, 2000, set()),
    "bunny": ("bunny", {}, 4000, set()),
    "sah": ("bunny", {"RT_ANYHIT_TREE": "sah"}, 4000, set()),
    "million": ("million", {}, 3000, {"QN2"}),                  # launch_trace walks the quantised nodes, the packets the exact w4
}


@pytest.mark.parametrize("case", list(PACKET_CASES))
def test_packet_kernel_ray_by_ray(orc, monkeypatch, case):
    """rt_debug_trace kind 4: packets of four AO-like rays through k_trace_packets; every live ray equals the oracle's traceBVHShadow and kind 3's
    answer (the single-ray any-hit build of the same environment), an empty slot reads 0."""
    mesh, env, P, want_any = PACKET_CASES[case]
    _set(monkeypatch, env)
    nodes, tris = _mesh(mesh)
    u = _uniforms(nodes, tris)
    org, dirs, tmax = packet_rays(nodes, tris, P)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r:
        r.upload_bvh(nodes, tris)
        r.debug_builds(reset=True)
        pk = r.debug_trace(4, org, dirs, tmax)
        assert r.debug_builds() == {"closest": frozenset(), "any": frozenset({"PACKETS"})}
        single = r.debug_trace(3, org, dirs, tmax)
        assert r.debug_builds() == _builds(None, want_any)
        with pytest.raises(rt.RtError):
            r.debug_trace(4, org[:6], dirs[:6], tmax[:6])          # not whole packets
    live = tmax >= 0
    want = np.zeros(org.shape[0], bool)
    for i in np.flatnonzero(live):
        want[i] = orc.trace_bvh_shadow(u, nodes, tris, org[i], dirs[i], tmax[i])
    got = pk[:, 0].astype(bool)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (case, bad[:8], got[bad[:8]], want[bad[:8]])
    assert np.array_equal(pk[:, 0], single[:, 0])
    assert not got[~live].any()
    assert mesh == "one_leaf" or 0 < want.sum() < live.sum()


# ---------------------------------------------------------------- frames

W, H = 96, 64
DEFAULT = _builds(set(), set())


@functools.lru_cache(maxsize=None)
def _oracle_frames(mesh, W, H, frames, spp, ao):
    import oracle as orc
    nodes, tris = _mesh(mesh)
    faces = scenes.tiny_env(8)
    p = rt.default_render_params()
    p.sppPerFrame = spp
    if ao is not None:
        p.aoSamples = ao
    assert p.enableGI == 1 and p.enableAO == 1
    cam = scenes.camera("closeup", aspect=W / H)
    us = [rt.frame_uniforms(p, cam, W, H, f, True, nodes.shape[0], tris.shape[0]) for f in range(frames)]
    wants, prev = [], None
    for u in us:
        want, _ = orc.render(u, nodes, tris, faces, prev, nthreads=16)
        wants.append(want)
        prev = want[0]
    return us, wants


def _frames(orc, what, *, mesh="bunny", W=W, H=H, frames=3, spp=2, ao=None):
    """The frames frame by frame and as one batch against the oracle; returns (builds of the frame-by-frame renderer, its traced rays)."""
    nodes, tris = _mesh(mesh)
    faces = scenes.tiny_env(8)
    us, wants = _oracle_frames(mesh, W, H, frames, spp, ao)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r, rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as rb:
        for x in (r, rb):
            x.upload_bvh(nodes, tris); x.upload_env(faces); x.resize(W, H)
            x.debug_builds(reset=True)
        for f, u in enumerate(us):
            r.render_frame(u)
            _assert_targets_equal(r.read_all(), wants[f], orc, f"{what} frame={f}")
        rb.render_frames(us)
        _assert_targets_equal(rb.read_all(), wants[-1], orc, f"{what} batch of {frames}")
        builds = r.debug_builds()
        assert rb.debug_builds() == builds, what
        tr = r.traced_rays()
    return builds, tr


PACKET_AO_CASES = {   # id: (environment, aoSamples, frame size, expected builds)
    "ao1": ({}, 1, (W, H), _builds(set(), {"PACKETS"})),
    "ao3": ({}, 3, (W, H), _builds(set(), {"PACKETS"})),
    "ao4": ({}, 4, (W, H), _builds(set(), {"PACKETS"})),
    "ao6": ({}, 6, (W, H), _builds(set(), {"PACKETS"})),
    "qnodes2": ({"RT_QNODES": "2"}, 3, (W, H), _builds(set(), {"PACKETS", "QN2"})),
    "implicit": ({"RT_IMPLICIT": "1"}, 3, (W, H), _builds({"IMPL"}, {"PACKETS", "IMPL"})),
    "sah": ({"RT_ANYHIT_TREE": "sah"}, 3, (W, H), _builds(set(), {"PACKETS"})),
    "chunked": ({"RT_QUEUE_BUDGET_MB": "1"}, 3, (160, 96), _builds(set(), {"PACKETS"})),   # 4096-hit chunks: two per frame
}


@pytest.mark.parametrize("case", list(PACKET_AO_CASES))
def test_packet_ao_frames(orc, monkeypatch, case):
    """RT_PACKET_AO=1: the AO rays of a hit as one packet (k_trace_packets), the any-hit launch behind the AO slots of queue 1.  aoSamples that are
    not multiples of four leave short packets; traced_rays().ao > 0 shows the packet kernel traced them."""
    env, ao, (w, h), want = PACKET_AO_CASES[case]
    _set(monkeypatch, dict(env, RT_PACKET_AO="1"))
    builds, tr = _frames(orc, f"RT_PACKET_AO {case}", W=w, H=h, ao=ao)
    assert builds == want, case
    assert tr.ao > 0 and tr.shadow > 0


FRAME_CASES = {   # id: (environment, mesh, frame size, spp, expected builds)
    "bin_gi": ({"RT_BIN_GI": "1"}, "bunny", (W, H), 2, DEFAULT),
    "bin_gi_chunked": ({"RT_BIN_GI": "1", "RT_QUEUE_BUDGET_MB": "1"}, "bunny", (160, 96), 2, DEFAULT),
    "bin_gi_q2_cap": ({"RT_BIN_GI": "1", "RT_Q2_CAP": "64"}, "two_mesh", (W, H), 3, DEFAULT),   # k_gen_gi_overflow reads through giPerm
    "coop": ({"RT_COOP": "1"}, "bunny", (W, H), 2, _builds({"COOP"}, set())),
    "leafb_closest4": ({"RT_LEAFB_CLOSEST": "4"}, "bunny", (W, H), 2, _builds({"LEAFB4"}, set())),
    "reverse0": ({"RT_REVERSE": "0"}, "bunny", (W, H), 2, DEFAULT),
    "dense_take0": ({"RT_DENSE_TAKE": "0"}, "bunny", (W, H), 2, DEFAULT),
    "guided1": ({"RT_GUIDED": "1"}, "bunny", (W, H), 2, DEFAULT),
    "grid_pct30": ({"RT_GRID_PCT": "30", "RT_GRID_PCT_PRIMARY": "30"}, "bunny", (W, H), 2, DEFAULT),
    "chunk8": ({"RT_CHUNK": "8", "RT_CHUNK_PRIMARY": "8"}, "bunny", (W, H), 2, DEFAULT),
}


@pytest.mark.parametrize("case", list(FRAME_CASES))
def test_option_frames(orc, monkeypatch, case):
    """Scheduler, sorting and build options on whole frames (GI and AO on): the build each selects, and the frames of the oracle."""
    env, mesh, (w, h), spp, want = FRAME_CASES[case]
    _set(monkeypatch, env)
    builds, tr = _frames(orc, case, mesh=mesh, W=w, H=h, spp=spp)
    assert builds == want, case
    assert tr.bounce > 0 and tr.shadow > 0


@pytest.mark.parametrize("env", [{"RT_CU_SPLIT": "2"}, {"RT_SHADE_PRIORITY": "-1"}, {"RT_SHADE_PRIORITY": "1"}, {"RT_ARENAS": "1"}],
                         ids=["cu_split2", "priority-1", "priority1", "arenas1"])
def test_shading_stream_options(orc, monkeypatch, env):
    """RT_CU_SPLIT / RT_SHADE_PRIORITY: the shading kernels on a second stream, cross-stream event hops at every stage; RT_ARENAS=1: one ray-queue
    arena handed from lane to lane.  Twelve batches of four frames with no synchronisation in between keep all lanes turning over; the last frame
    equals the oracle's."""
    _set(monkeypatch, env)
    Wd, Hd, K, NB = 96, 64, 4, 12
    nodes, tris = _mesh("bunny")
    faces = scenes.tiny_env(8)
    us, wants = _oracle_frames("bunny", Wd, Hd, K * NB, 2, None)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as r:
        r.upload_bvh(nodes, tris); r.upload_env(faces); r.resize(Wd, Hd)
        r.debug_builds(reset=True)
        for b in range(NB):
            r.render_frames(us[b * K:(b + 1) * K])
        _assert_targets_equal(r.read_all(), wants[-1], orc, f"{env} last of {K * NB}")
        assert r.debug_builds() == DEFAULT


def _production_counts(orc):
    _, tr = _frames(orc, "production")
    return tr


@pytest.mark.parametrize("env,want", [({"RT_TRACE_STATS": "1"}, _builds({"STATS"}, {"STATS"})), ({"RT_TRACE_STATS": "2"}, _builds({"STATS"}, {"STATS"})),
                                      ({"RT_TRACE_TIMING": "1"}, _builds({"TIMING"}, {"TIMING"}))], ids=["stats1", "stats2", "timing"])
def test_instrumented_builds(orc, monkeypatch, env, want):
    """RT_TRACE_STATS=1 / 2 and RT_TRACE_TIMING=1: the instrumented k_trace builds render the oracle's frames and trace the rays the production build
    traces.  Deterministic, hence compared: the ray counts of traced_rays() (candidate / hit pixels, primary, shadow, bounce, bounce-shadow, AO rays,
    frames) -- which rays exist depends on the frame only.  Not deterministic, hence only checked non-zero: the merged-load counters of the stats
    build (which lanes share a wave step depends on the scheduler's run-time dealing)."""
    prod = _production_counts(orc)
    _set(monkeypatch, env)
    builds, tr = _frames(orc, str(env))
    assert builds == want
    for f in ("candidatePixels", "hitPixels", "primary", "shadow", "bounce", "bounceShadow", "ao", "frames"):
        assert getattr(tr, f) == getattr(prod, f), (f, getattr(tr, f), getattr(prod, f))
    if "RT_TRACE_STATS" in env:
        assert tr.mergedLoadsPrimary > 0 and tr.mergedLoadsShadow > 0 and tr.mergedLoadsBounce > 0, (tr.mergedLoadsPrimary, tr.mergedLoadsShadow, tr.mergedLoadsBounce)
