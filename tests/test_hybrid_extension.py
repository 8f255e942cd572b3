"""EXTENSION beyond the reference (SURVEY.md 8d config 3 "run B"; BASELINE configs[2]: "bunny + glass + mirror materials ..., 4 bounces").
The reference cannot express that scene: its BVH mode has no analytic objects and no materials (rt.frag:84-106).  uUseBVH == 2
(RT_SCENE_HYBRID) renders the ANALYTIC branch of rt.frag with the BVH mesh added to the analytic scene as one more object (material id
5 = the default branch of getMaterial), and rt_set_extension(giBounces) lengthens the analytic GI path.  Parity is against this
repository's own oracle only -- there is nothing in the reference to compare with -- plus the one anchor the reference does give:
with an empty BVH and one bounce, hybrid mode IS the reference's analytic mode, bit for bit."""
import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scenes


def _mesh_in_front_of_the_spheres():
    """The bunny stand-in, scaled and moved between the camera and the analytic spheres (default camera at (0,2,8) looking down -z)."""
    v, f = rt.meshgen.bunny_standin(2)
    M = np.eye(4, dtype=np.float32)
    M[0, 0] = M[1, 1] = M[2, 2] = 1.0
    M[0, 3], M[1, 3], M[2, 3] = 0.1, 1.0, 0.0
    return rt.build_bvh(rt.gather_triangles(v, f, M.T.reshape(-1)))       # column-major


def test_oracle_hybrid_with_empty_bvh_is_the_analytic_mode(orc):
    W, H = 64, 48
    faces = scenes.tiny_env(8)
    p = orc.default_render_params()
    p.sppPerFrame = 2
    cam = orc.default_camera()
    cam.aspect = W / H
    ua = orc.frame_uniforms(p, cam, W, H, 3, False)
    uh = orc.frame_uniforms(p, cam, W, H, 3, 2)
    assert ua.useBVH == 0 and uh.useBVH == rt.RT_SCENE_HYBRID
    a, ca = orc.render(ua, env_faces=faces)
    b, cb = orc.render(uh, env_faces=faces)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert ca.raysAnalytic == cb.raysAnalytic


def test_oracle_hybrid_mesh_interacts_with_the_analytic_scene(orc):
    """The mesh occludes analytic objects, is reflected by the mirror sphere, casts shadows; more bounces add light."""
    W, H = 96, 64
    nodes, tris = _mesh_in_front_of_the_spheres()
    p = orc.default_render_params()
    p.enableEnvMap = 0
    cam = orc.default_camera()
    cam.aspect = W / H
    ua = orc.frame_uniforms(p, cam, W, H, 0, False, env_loaded=False)
    uh = orc.frame_uniforms(p, cam, W, H, 0, 2, nodes.shape[0], tris.shape[0], env_loaded=False)
    a, _ = orc.render(ua)
    h1, c1 = orc.render(uh, nodes, tris)
    h4, c4 = orc.render(uh, nodes, tris, gi_bounces=4)
    fa, f1, f4 = (orc.half_to_float(x[0])[:, :, :3] for x in (a, h1, h4))
    changed = np.abs(f1 - fa).max(axis=2) > 1e-3
    assert 0.02 < changed.mean() < 0.9                         # the mesh and its shadows / reflections changed part of the image
    assert c1.raysClosest > 0 and c1.raysAnalytic > W * H      # both kinds of scene query ran
    # gpos where the primary ray hit the mesh lies inside the mesh's box
    g = orc.half_to_float(h1[2])
    on_mesh = (np.abs(orc.half_to_float(h1[3])[:, :, :3] - orc.half_to_float(a[3])[:, :, :3]).max(axis=2) > 1e-3) & (g[:, :, 3] == 1.0)
    assert on_mesh.sum() > 50
    lo, hi = nodes[0, 0:3] - 0.02, nodes[0, 4:7] + 0.02
    pts = g[on_mesh][:, :3]
    assert ((pts >= lo) & (pts <= hi)).all(axis=1).mean() > 0.95
    assert c4.raysAnalytic > c1.raysAnalytic and f4.mean() > f1.mean()        # deeper paths: more rays, more light


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["staged", "mega"])
@pytest.mark.parametrize("bounces,spp,env", [(1, 2, True), (4, 1, True), (2, 3, False)])
def test_hip_hybrid_frames_match_the_oracle(orc, bounces, spp, env, pipeline):
    W, H = 96, 64
    nodes, tris = _mesh_in_front_of_the_spheres()
    faces = scenes.tiny_env(8) if env else None
    p = rt.default_render_params()
    p.sppPerFrame = spp
    p.enableEnvMap = int(env)
    cam = scenes.camera("default", aspect=W / H)
    # "staged" (RT_PIPELINE_AUTO): replayed shading passes + persistent traversal launches (csrc/rt_hybrid.hip); "mega": one thread per pixel
    with rt.Renderer(pipeline=rt.RT_PIPELINE_AUTO if pipeline == "staged" else rt.RT_PIPELINE_MEGAKERNEL) as r:
        r.upload_bvh(nodes, tris)
        r.upload_env(faces)
        r.resize(W, H)
        r.set_extension(gi_bounces=bounces)
        prev = None
        for frame in range(3):
            u = rt.frame_uniforms(p, cam, W, H, frame, rt.RT_SCENE_HYBRID, nodes.shape[0], tris.shape[0], env_loaded=env)
            assert u.useBVH == rt.RT_SCENE_HYBRID
            r.render_frame(u)
            want, _ = orc.render(u, nodes, tris, faces, prev, gi_bounces=bounces)
            for g, w, name in zip(r.read_all(), want, ("color", "motion", "gpos", "gnrm")):
                st = orc.compare(g, w)
                assert st["rmse"] < 1e-4 and st["bit_diff"] == 0, (bounces, frame, name, st)
            prev = want[0]
        with pytest.raises(rt.RtError):
            r.set_extension(gi_bounces=0)


@pytest.mark.gpu
def test_staged_hybrid_run_b_settings_whole_frame_against_the_oracle(orc):
    """Run B's own settings -- 1920x1080, 16 spp, four bounces, cube map -- on the staged pipeline, the whole frame of two accumulating frames against this
    repository's oracle, every target bit for bit (the other oracle checks of the extension are 96x64 frames and the 32x16 window of bench.py's run-B line):
    thousands of shading tiles per pass, every pass of the speculation / replay scheme, default capacity estimates."""
    W, H = 1920, 1080
    nodes, tris = _mesh_in_front_of_the_spheres()
    faces = scenes.tiny_env(16)
    p = rt.default_render_params()
    p.sppPerFrame = 16
    cam = scenes.camera("default", aspect=W / H)
    with rt.Renderer(pipeline=rt.RT_PIPELINE_AUTO) as r:
        r.upload_bvh(nodes, tris)
        r.upload_env(faces)
        r.resize(W, H)
        r.set_extension(gi_bounces=4)
        prev = None
        for frame in range(2):
            u = rt.frame_uniforms(p, cam, W, H, frame, rt.RT_SCENE_HYBRID, nodes.shape[0], tris.shape[0])
            r.render_frame(u)
            want, _ = orc.render(u, nodes, tris, faces, prev, gi_bounces=4, nthreads=16)
            for g, w, name in zip(r.read_all(), want, ("color", "motion", "gpos", "gnrm")):
                assert np.array_equal(g, w), (frame, name, orc.compare(g, w))
            prev = want[0]


@pytest.mark.gpu
def test_hip_hybrid_with_empty_bvh_is_the_analytic_mode(orc):
    W, H = 128, 80
    faces = scenes.tiny_env(8)
    p = rt.default_render_params()
    p.sppPerFrame = 2
    cam = scenes.camera("default", aspect=W / H)
    outs = []
    for mode in (False, rt.RT_SCENE_HYBRID):
        with rt.Renderer() as r:
            r.upload_env(faces)
            r.resize(W, H)
            for frame in range(2):
                r.render_frame(rt.frame_uniforms(p, cam, W, H, frame, mode))
            outs.append(r.read_all())
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


_STAGED_CODE = r'''
import sys, numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import opengl_raytracing_amd as rt, scenes
W, H, SPP, BOUNCES = (int(v) for v in sys.argv[1:5])
v, f = rt.meshgen.bunny_standin(3)
M = np.eye(4, dtype=np.float32); M[0, 3], M[1, 3], M[2, 3] = -0.1, 1.0, -0.5
nodes, tris = rt.build_bvh(rt.gather_triangles(v, f, M.T.reshape(-1)))
faces = scenes.tiny_env(8)
p = rt.default_render_params(); p.sppPerFrame = SPP
cam = scenes.camera("default", aspect=W / H)
outs = {}
for name, pipe in (("staged", rt.RT_PIPELINE_AUTO), ("mega", rt.RT_PIPELINE_MEGAKERNEL)):
    with rt.Renderer(pipeline=pipe) as r:
        r.upload_bvh(nodes, tris); r.upload_env(faces); r.resize(W, H); r.set_extension(gi_bounces=BOUNCES)
        for frame in range(3):
            r.render_frame(rt.frame_uniforms(p, cam, W, H, frame, rt.RT_SCENE_HYBRID, nodes.shape[0], tris.shape[0]))
        outs[name] = r.read_all()
        if name == "staged":
            st = r.stage_times() if False else None
for a, b in zip(outs["staged"], outs["mega"]):
    assert np.array_equal(a, b)
print("STAGED-OK")
'''


@pytest.mark.gpu
@pytest.mark.parametrize("budget_mb,w,h,spp,bounces,extra", [(8192, 640, 360, 4, 4, {}), (1, 320, 200, 3, 2, {}),
                                                             (8192, 320, 200, 4, 4, {"RT_HYBRID_RATIO_Q": "0.02", "RT_HYBRID_RATIO_L": "0.02"}),
                                                             (2, 320, 200, 2, 2, {"RT_HYBRID_RATIO_Q": "0.05", "RT_HYBRID_RATIO_L": "0.05"}),
                                                             (8192, 320, 200, 2, 2, {"RT_HYBRID_WAVES": "3"}), (8192, 320, 200, 2, 2, {"RT_HYBRID_WAVES": "5"}),
                                                             (8192, 320, 200, 2, 2, {"RT_HYBRID_WAVES": "6"})])
def test_staged_hybrid_equals_the_megakernel(budget_mb, w, h, spp, bounces, extra):
    """The staged hybrid pipeline against the megakernel on a frame that shows everything at once -- mesh, floor, diffuse / glass / mirror
    spheres, light marker, N bounces, three frames of accumulation -- bit for bit; the second case cuts the frame into some twenty chunks of
    pixel slots (1 MB of per-thread state + queue + log); the third and fourth start with capacity estimates fifty / twenty times too small for the
    dense queue and the log arena, so that the first passes outgrow them, only count, and the chunk is rendered again with enlarged arrays
    (round 4: memory follows the recorded queries; the estimates are the one thing that can be wrong) -- also in combination with chunking.  The
    last three run the other register budgets of the shading kernel (RT_HYBRID_WAVES = 3 / 5 / 6: other instantiations of k_hybrid_shade)."""
    import os
    import subprocess
    import sys
    # RT_HYBRID_CHECK=1: every staged-record, thread-list, queue and log store of the staged pipeline proves its index against the capacity its array
    # was allocated with and raises a flag instead of storing (rt_hybrid.hip hb_ok; the frame then ends with RT_ERR_STATE) -- the fence around the one
    # GPU memory fault this pipeline has produced, in an uncommitted working tree of round 4 at exactly the second parametrisation
    env = dict(os.environ, RT_QUEUE_BUDGET_MB=str(budget_mb), RT_HYBRID_CHECK="1", **extra)
    r = subprocess.run([sys.executable, "-c", _STAGED_CODE, str(w), str(h), str(spp), str(bounces)], cwd=str(scenes.ROOT), env=env, capture_output=True, text=True, timeout=900)
    assert "STAGED-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("RT_FUZZ_CASES", "8"))))
def test_random_hybrid_scenes_match_the_oracle_on_both_pipelines(orc, seed):
    """Randomised sweep of the hybrid extension: random mesh placement among the analytic objects (in front of, beside, inside the glass /
    mirror spheres' neighbourhood), cameras, toggles, materials, 1-4 bounces, 1-3 spp, ragged frame sizes, moving and static cameras;
    the staged pipeline and the megakernel must both equal the own oracle bit for bit on three consecutive frames."""
    rng = np.random.default_rng(9000 + seed)
    v, f = rt.meshgen.bunny_standin(int(rng.integers(0, 3)), seed=int(rng.integers(1 << 30)))
    M = np.eye(4, dtype=np.float32)
    M[0, 0] = M[1, 1] = M[2, 2] = float(rng.uniform(0.3, 1.2))
    M[0, 3], M[1, 3], M[2, 3] = float(rng.uniform(-1.5, 1.5)), float(rng.uniform(0.4, 1.6)), float(rng.uniform(-4.5, 1.0))
    nodes, tris = rt.build_bvh(rt.gather_triangles(v, f, M.T.reshape(-1)))
    W, H = int(rng.integers(17, 90)), int(rng.integers(17, 64))
    p = rt.default_render_params()
    p.sppPerFrame = int(rng.choice([1, 2, 3]))
    for name in ("enableGI", "enableAO", "enableTAA", "enableJitter", "sunEnabled", "skyEnabled", "pointLightEnabled", "enableEnvMap",
                 "matGlassEnabled", "matMirrorEnabled"):
        setattr(p, name, int(rng.random() < 0.8))
    p.aoSamples = int(rng.integers(1, 6))
    p.pointLightPos[0], p.pointLightPos[1], p.pointLightPos[2] = float(rng.normal(0, 1.5)), float(rng.uniform(0.5, 4.0)), float(rng.uniform(-5, 1))
    bounces = int(rng.integers(1, 5))
    moving = bool(rng.random() < 0.4)
    cams = []
    for k in range(3):
        c = scenes.camera("default", aspect=W / H)
        c.pos[0] += float(rng.normal(0, 0.6)); c.pos[1] += float(rng.normal(0, 0.4)); c.pos[2] += float(rng.normal(0, 1.0))
        c.yaw += float(rng.normal(0, 8)); c.pitch += float(rng.normal(0, 6)); c.fov = float(rng.uniform(35, 80))
        cams.append(c)
    faces = scenes.tiny_env(int(rng.choice([1, 4, 8])), seed=int(rng.integers(100))) if p.enableEnvMap else None
    for pipeline in (rt.RT_PIPELINE_AUTO, rt.RT_PIPELINE_MEGAKERNEL):
        with rt.Renderer(pipeline=pipeline) as r:
            r.upload_bvh(nodes, tris)
            r.upload_env(faces)
            r.resize(W, H)
            r.set_extension(gi_bounces=bounces)
            prev, prev_vp = None, None
            for frame in range(3):
                cam = cams[frame] if moving else cams[0]
                u = rt.frame_uniforms(p, cam, W, H, frame, rt.RT_SCENE_HYBRID, nodes.shape[0], tris.shape[0], prev_vp=prev_vp, env_loaded=faces is not None)
                prev_vp = rt.mat4_mul(rt.camera_proj(cam), rt.camera_view(cam))
                r.render_frame(u)
                want, _ = orc.render(u, nodes, tris, faces, prev, gi_bounces=bounces)
                for g, w_, name in zip(r.read_all(), want, ("color", "motion", "gpos", "gnrm")):
                    assert np.array_equal(g, w_), (seed, pipeline, frame, name, int(np.sum(g != w_)))
                prev = want[0]


@pytest.mark.gpu
@pytest.mark.parametrize("world,rank", [(3, 1), (8, 7)])
def test_staged_hybrid_on_a_tile_parallel_rank_equals_the_megakernel(world, rank):
    """One rank of a tile-parallel frame (16x16 tiles with tile % world == rank) renders the hybrid extension in stages: the same tiles as the
    megakernel, bit for bit, over three frames of accumulation."""
    W, H = 200, 120
    nodes, tris = _mesh_in_front_of_the_spheres()
    faces = scenes.tiny_env(8)
    p = rt.default_render_params()
    p.sppPerFrame = 2
    cam = scenes.camera("default", aspect=W / H)
    outs = []
    for pipe in (rt.RT_PIPELINE_AUTO, rt.RT_PIPELINE_MEGAKERNEL):
        with rt.Renderer(rank=rank, world_size=world, pipeline=pipe) as r:
            r.upload_bvh(nodes, tris)
            r.upload_env(faces)
            r.resize(W, H)
            r.set_extension(gi_bounces=2)
            for frame in range(3):
                r.render_frame(rt.frame_uniforms(p, cam, W, H, frame, rt.RT_SCENE_HYBRID, nodes.shape[0], tris.shape[0]))
            outs.append(r.read_all())
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert outs[0][0].any()
