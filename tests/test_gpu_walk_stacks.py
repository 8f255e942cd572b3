"""Every tree walk driven to the bound of its per-lane LDS stack, on the fixtures of tests/stack_cases.py: trees whose every box a ray
along the axis enters, at the depths where a stack size changes -- the floor of four entries (depths 4 / 5), the megakernel's compiled stacks of 16,
24 and 32 (depths 16 / 17, 24 / 25) and the deepest tree rt_upload_bvh accepts (32) -- and perfect trees (slabs) for the implicit forms.
tests/test_stack_cases_host.py shows on the CPU that the walks' models reach depth - 1 (closest hit) and anyStack (any hit) entries on these rays, so an
entry pushed past a stack, or a subtree dropped at a guard, shows here as a wrong answer: every comparison is bit or integer equality with the oracle,
the host definitions of the queries, and the counts the construction fixes.
"""
import functools
import math

import numpy as np
import pytest

import box_query_ref
import hull_query_ref
import opengl_raytracing_amd as rt
import scenes
import stack_cases as sc
import test_gpu_options as gpu_options
import trace_build_cases
import tri_query_ref

pytestmark = pytest.mark.gpu
f32 = np.float32
CLEARED = gpu_options.OPTION_VARS + ("RT_NEAREST_FAR_FIRST",)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in CLEARED:
        monkeypatch.delenv(v, raising=False)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------- ray by ray

RAY_FIXTURES = ("ladder4L", "ladder4R", "ladder5L", "ladder5R", "ladder32L", "ladder32R", "slab6", "slab7")
ENVS = {"none": {}, "qnodes2": {"RT_QNODES": "2"}, "fused": {"RT_FUSED": "1"}, "implicit": {"RT_IMPLICIT": "1"},
        "implicit_qnodes2": {"RT_IMPLICIT": "1", "RT_QNODES": "2"}, "sah": {"RT_ANYHIT_TREE": "sah"},
        "implicit_sah": {"RT_IMPLICIT": "1", "RT_ANYHIT_TREE": "sah"}, "coop": {"RT_COOP": "1"}, "near": {"RT_NEAR_FIRST": "1"}, "leafb4": {"RT_LEAFB": "4"}}
# what a slab's builds must show of the environment (a ladder has no implicit form): the extra bits of (closest, any)
SLAB_BITS = {"none": (set(), set()), "qnodes2": (set(), {"QN2"}), "fused": ({"FUSE"}, set()), "implicit": ({"IMPL"}, {"IMPL"}),
             "implicit_qnodes2": ({"IMPL"}, {"IMPL", "QN2"}), "sah": (set(), set()), "implicit_sah": ({"IMPL"}, {"IMPL"}), "coop": ({"COOP"}, set()),
             "near": (set(), {"NEAR"}), "leafb4": ({"LEAFB4"}, {"LEAFB4"})}


def _assert_closest(fx, r, oracle, t, tri, what):
    prim, t_want, _ = oracle
    hit = prim >= 0
    assert np.array_equal(_bits(t[hit]), _bits(t_want[hit])), (what, np.flatnonzero(_bits(t[hit]) != _bits(t_want[hit]))[:8])
    assert (t[~hit] == f32(1e30)).all(), (what, np.flatnonzero(t[~hit] != f32(1e30))[:8])
    want = np.where(r.first >= 0, fx.row[np.clip(r.first, 0, fx.n)], -1)          # the rung the construction names
    bad = np.flatnonzero(np.where(hit, tri, -1) != want)
    assert bad.size == 0, (what, bad[:8], tri[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("name", RAY_FIXTURES)
def test_ray_by_ray(orc, monkeypatch, name, env):
    """rt_debug_trace kinds 2, 3 and 4 -- k_trace closest-hit and any-hit, k_trace_packets -- under one environment: the builds rt.trace_build
    predicts; closest hit: t bit-equal to the oracle's and the triangle the construction names; any hit and packets: the oracle's answers."""
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, v)
    fx = sc.by_name(name)
    r, pk = sc.rays(fx), sc.packet_rays(fx)
    oracle, pk_occ = sc.oracle_answers(fx), sc.oracle_packet_answers(fx)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as ren:
        ren.upload_bvh(fx.nodes, fx.tris)
        forms = tuple(f for f, a in trace_build_cases.FORM_ARRAYS.items() if ren.debug_read_scene(a).size)
        depth = int(ren.scene_info().treeDepth)
        packed_depth, any_stack, packed_forms = trace_build_cases.scene_offers(fx.nodes, fx.tris)
        assert (packed_depth, packed_forms) == (depth, forms) and depth == fx.depth
        want = {kind: rt.trace_build(kind == "any", depth=depth, stats=False, any_stack=any_stack, forms=forms) for kind in ("closest", "any")}
        ren.debug_builds(reset=True)
        closest = ren.debug_trace(2, r.org, r.dirs)
        assert ren.debug_builds() == {"closest": frozenset({"k_trace"}) | want["closest"].bits, "any": frozenset()}, (name, env)
        anyhit = ren.debug_trace(3, r.org, r.dirs, r.tmax)
        assert ren.debug_builds() == {"closest": frozenset(), "any": frozenset({"k_trace"}) | want["any"].bits}, (name, env)
        packets = ren.debug_trace(4, pk.org, pk.dirs, pk.tmax)
        assert ren.debug_builds() == {"closest": frozenset(), "any": frozenset({"PACKETS"})}, (name, env)
    if fx.kind == "slab":            # the environment was not ignored
        assert (set(want["closest"].bits), set(want["any"].bits)) == SLAB_BITS[env], (name, env)
    assert want["closest"].stack == max(4, fx.depth) and want["any"].stack == max(4, any_stack)
    _assert_closest(fx, r, oracle, closest[:, 0], closest[:, 1].astype(np.int64), (name, env))
    bad = np.flatnonzero(anyhit[:, 0].astype(bool) != oracle[2])
    assert bad.size == 0, (name, env, bad[:8])
    bad = np.flatnonzero(packets[:, 0].astype(bool) != pk_occ)
    assert bad.size == 0, (name, env, bad[:8])
    assert 0 < oracle[2].sum() < r.org.shape[0] and 0 < pk_occ.sum() < pk.org.shape[0]


@pytest.mark.parametrize("name", ["ladder32L", "ladder32R"])
def test_trace_rays_on_the_deepest_tree(orc, name):
    """Renderer.trace_rays, closest and any hit, on the deepest tree an upload accepts."""
    fx = sc.by_name(name)
    r = sc.rays(fx)
    oracle = sc.oracle_answers(fx)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as ren:
        ren.upload_bvh(fx.nodes, fx.tris)
        hits = ren.trace_rays(r.org, r.dirs)
        occ = ren.trace_rays(r.org, r.dirs, r.tmax, any_hit=True)
    _assert_closest(fx, r, oracle, hits.t, hits.prim.astype(np.int64), name)
    assert np.array_equal(np.asarray(occ, bool), oracle[2])


# ---------------------------------------------------------------- frames

W = H = 32


def _camera(fx):
    """Three units beyond the far end and above the hypotenuse (y = z = 0.62), looking down the axis at (the middle rung's x, 1/2, 1/2), the field of
    view as narrow as the far end of the unit square: the primary rays stay inside the square over the whole length -- they enter every box, as the
    rays of stack_cases do -- and dip under the hypotenuse at different rungs, so the first rung a pixel sees ranges over the ladder."""
    back, off = 3.0, 0.62
    span = float(fx.x[-1] - fx.x[0])
    tilt = math.degrees(math.atan2(off - 0.5, back + span / 2.0))
    cam = rt.default_camera()
    cam.pos[0], cam.pos[1], cam.pos[2] = float(fx.x[-1]) + back, off, off
    cam.yaw, cam.pitch, cam.aspect = 180.0 + tilt, -tilt, W / H
    cam.fov = 2.0 * math.degrees(math.atan(0.42 / (span + back)))
    return cam


@functools.lru_cache(maxsize=None)
def _oracle_frames(name, mode, frames=2):
    import oracle as orc
    fx = sc.by_name(name)
    faces = scenes.tiny_env(8)
    p = rt.default_render_params()
    p.sppPerFrame = 2
    assert p.enableGI == 1 and p.enableAO == 1
    us = [rt.frame_uniforms(p, _camera(fx), W, H, f, mode, fx.nodes.shape[0], fx.tris.shape[0]) for f in range(frames)]
    wants, hit_pixels, prev = [], [], None
    for u in us:
        want, cnt = orc.render(u, fx.nodes, fx.tris, faces, prev, nthreads=16)
        wants.append(want)
        hit_pixels.append(cnt.hitPixels)
        prev = want[0]
    return us, wants, hit_pixels


def _render(orc, name, pipeline, mode=True, bounce_hits=None):
    """Two frames of the fixture against the oracle's, all four targets bit for bit -> the renderer's traced-ray tallies.  bounce_hits: a list that
    receives each frame's count of (hit, sample) pairs whose bounce ray hit the mesh (Renderer.gi_list, which makes the generator count)."""
    fx = sc.by_name(name)
    us, wants, hit_pixels = _oracle_frames(name, mode)
    assert min(hit_pixels) > W * H // 2, hit_pixels          # the mesh fills the view
    with rt.Renderer(pipeline=pipeline) as ren:
        ren.upload_bvh(fx.nodes, fx.tris); ren.upload_env(scenes.tiny_env(8)); ren.resize(W, H)
        if bounce_hits is not None:
            ren.gi_list(reset=True)
        for f, u in enumerate(us):
            ren.render_frame(u)
            gpu_options._assert_targets_equal(ren.read_all(), wants[f], orc, f"{name} frame={f}")
            if bounce_hits is not None:
                bounce_hits.append(int(ren.gi_list(reset=True).shaded))
        return ren.traced_rays()


@pytest.mark.parametrize("name", ["ladder16L", "ladder17R", "ladder24L", "ladder25R", "ladder32L", "ladder32R"])
def test_megakernel_frames(orc, name):
    """The megakernel with its compiled stacks of 16, 24 and 32 entries at the depths where the choice changes (16 / 17, 24 / 25) and at 32."""
    _render(orc, name, rt.RT_PIPELINE_MEGAKERNEL)


@pytest.mark.parametrize("name", ["ladder4L", "ladder5R", "ladder32L", "ladder32R"])
def test_wavefront_frames(orc, name):
    tr = _render(orc, name, rt.RT_PIPELINE_WAVEFRONT)
    assert tr.primary > 0 and tr.shadow > 0 and tr.bounce > 0


@pytest.mark.parametrize("name", ["ladder5R", "ladder32L"])
def test_wavefront_frames_with_a_small_shadow_queue_2(orc, monkeypatch, name):
    """RT_Q2_CAP=64: shadow queue 2 holds 64 (hit, sample) pairs, and the pairs beyond them trace their shadow rays in place, with the megakernel's any-hit
    walk on k_gen_gi_overflow's stack of max(depth, 4) entries.  Each frame's bounce rays hit the ladder more than 64 times, so the kernel has work; the
    frames are rendered as they are in production and once more with the generator counting."""
    monkeypatch.setenv("RT_Q2_CAP", "64")
    _render(orc, name, rt.RT_PIPELINE_WAVEFRONT)
    bounce_hits = []
    _render(orc, name, rt.RT_PIPELINE_WAVEFRONT, bounce_hits=bounce_hits)
    assert len(bounce_hits) == 2 and min(bounce_hits) > 64, bounce_hits


def test_hybrid_frame_on_the_deepest_tree(orc):
    _render(orc, "ladder32L", rt.RT_PIPELINE_AUTO, rt.RT_SCENE_HYBRID)


# ---------------------------------------------------------------- queries

QUERY_FIXTURES = ("ladder32L", "ladder32R", "slab7")


def _root_box(fx):
    return np.concatenate([fx.nodes[0, 0:3], fx.nodes[0, 4:7]]).astype(f32)


@pytest.mark.parametrize("name", QUERY_FIXTURES)
def test_overlap_queries(name):
    """Box, triangle and hull queries whose node test passes at every node, so that the walk defers a sibling at every level: lists, counts and
    `visits` against the host definitions and the reference walks; a sibling dropped at the `sp < stackEntries` guard changes all three."""
    fx = sc.by_name(name)
    n_nodes, n_tris = fx.nodes.shape[0], fx.tris.shape[0]
    x0, x1 = float(fx.x[0]) - 1.0, float(fx.x[-1]) + 1.0
    boxes = np.array([_root_box(fx),
                      [x0, 0.3, 0.3, x1, 0.3125, 0.3125],          # thin, along the axis, under the hypotenuse: every rung
                      [x0, 0.7, 0.7, x1, 0.75, 0.75]], f32)        # thin, beyond the hypotenuse: every node box, no rung
    qtris = np.array([[x0, 0.2, 0.2, x1, 0.2, 0.2, x1, 0.3, 0.25]], f32)              # a sliver that cuts every rung
    hulls = rt.box_corners(boxes[:1])
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as ren:
        ren.upload_bvh(fx.nodes, fx.tris)
        got = {"box": ren.box_overlaps(boxes, visits=True), "tri": ren.tri_overlaps(qtris, visits=True), "hull": ren.hull_overlaps(hulls, visits=True)}
    want = {"box": rt.box_overlaps(fx.nodes, fx.tris, boxes), "tri": rt.tri_overlaps(fx.nodes, fx.tris, qtris), "hull": rt.hull_overlaps(fx.nodes, fx.tris, hulls)}
    visits = {"box": box_query_ref.Walk(fx.nodes, n_tris, boxes).visits, "tri": tri_query_ref.Walk(fx.nodes, n_tris, qtris).visits,
              "hull": hull_query_ref.Walk(fx.nodes, n_tris, hulls).visits}
    for kind in got:
        g, w = got[kind], want[kind]
        assert np.array_equal(g.count, w.count) and np.array_equal(g.offsets, w.offsets) and np.array_equal(g.prims, w.prims), (name, kind)
        assert np.array_equal(g.visits, visits[kind]), (name, kind, g.visits, visits[kind])
    # what the construction fixes: every row for the root box, the thin box under the hypotenuse, the sliver and the hull; every node box tested
    assert got["box"].count.tolist() == [n_tris, n_tris, 0] and got["tri"].count.tolist() == [n_tris] and got["hull"].count.tolist() == [n_tris]
    assert (got["box"].visits == n_nodes).all() and (got["tri"].visits == n_nodes).all() and (got["hull"].visits == n_nodes).all()
    assert sorted(got["box"].prims[:n_tris].tolist()) == list(range(n_tris))


@pytest.mark.parametrize("far_first", [0, 1])
@pytest.mark.parametrize("name", QUERY_FIXTURES)
def test_nearest_queries(monkeypatch, name, far_first):
    """Nearest and K-nearest points from beyond both ends and beside the middle, the nearer and the farther child first."""
    monkeypatch.setenv("RT_NEAREST_FAR_FIRST", str(far_first))
    fx = sc.by_name(name)
    mid = float(fx.x[fx.n // 2])
    pts = np.array([[fx.x[0] - 2.0, 0.3, 0.3], [fx.x[-1] + 2.0, 0.3, 0.3], [mid + 0.01, 0.3, 0.3], [mid, 3.0, 0.5], [mid, 0.5, -3.0],
                    [fx.x[0] - 50.0, 2.0, 2.0], [fx.x[-1] + 50.0, -1.0, 0.2]], f32)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as ren:
        ren.upload_bvh(fx.nodes, fx.tris)
        one = ren.nearest_points(pts, visits=True)
        many = ren.nearest_points_multi(pts, 32, visits=True)
        culled = ren.nearest_points_multi(pts, 32, counts=False, visits=True)
    w1 = rt.nearest_points(fx.nodes, fx.tris, pts)
    wk = rt.nearest_points_multi(fx.nodes, fx.tris, pts, 32)
    assert np.array_equal(_bits(one.hits), _bits(w1.hits)) and np.array_equal(_bits(one.points), _bits(w1.points)), name
    for g in (many, culled):
        assert np.array_equal(_bits(g.hits), _bits(wk.hits)) and np.array_equal(_bits(g.points), _bits(wk.points)), name
    assert np.array_equal(many.count, wk.count) and (many.count == fx.n + 1).all()
    assert (many.visits == fx.nodes.shape[0]).all()                 # no limit, with counts: every box, whatever the order
    assert (one.visits >= 1).all() and (one.visits <= fx.nodes.shape[0]).all() and (culled.visits <= many.visits).all()
    # beyond an end the nearest rung is the end's; beside the middle, the middle's
    assert one.prim[:3].tolist() == [fx.row[0], fx.row[fx.n], fx.row[fx.n // 2]]


@pytest.mark.parametrize("name", QUERY_FIXTURES)
def test_multi_hit_queries(name):
    """The 32 nearest hits and the count of all of them, per ray: the multi-hit walk defers a sibling at every level on these rays."""
    fx = sc.by_name(name)
    r = sc.rays(fx)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_WAVEFRONT) as ren:
        ren.upload_bvh(fx.nodes, fx.tris)
        got = ren.trace_rays_multi(r.org, r.dirs, max_hits=32)
        limited = ren.trace_rays_multi(r.org, r.dirs, r.tmax, max_hits=32)
    want = rt.multi_hits(fx.nodes, fx.tris, r.org, r.dirs, max_hits=32)
    assert np.array_equal(_bits(got.hits), _bits(want.hits)) and np.array_equal(got.count, want.count), name
    assert np.array_equal(got.count, r.hits)                                        # what the construction fixes
    assert np.array_equal(limited.count, r.occluded.astype(np.int32))               # exactly one rung within the any-hit limit
    full = np.flatnonzero(r.hits == fx.n + 1)
    k = min(32, fx.n + 1)
    rungs = np.where((r.dirs[full, 0] > 0)[:, None], np.arange(k)[None], fx.n - np.arange(k)[None])
    assert np.array_equal(got.prim[full][:, :k], fx.row[rungs])
