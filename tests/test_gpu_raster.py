"""The raster preview on the device: rt_render_raster against tests/raster_ref.py bit for bit (RGBA8, primitive id, depth24), its
isolation from the ray pipeline, its errors, and rt_cli --raster."""
import os
import subprocess

import numpy as np
import pytest

import opengl_raytracing_amd as rt
from opengl_raytracing_amd import meshgen
import raster_ref as rr
import scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ground_quad(half=20.0):
    pos = np.array([[-half, 0, -half], [half, 0, -half], [half, 0, half], [-half, 0, half]], np.float32)
    return pos, np.array([0, 2, 1, 0, 3, 2], np.uint32)


def scene_meshes():
    b = meshgen.bunny_standin(6)
    s = meshgen.uv_sphere(32, 16)
    return {0: ground_quad(), 1: (b[0], b[1]), 2: (s[0], s[1])}


def check(ren, meshes, draws, view, proj, w, h, windows=None):
    got = ren.render_raster(draws, view, proj)
    for win in windows or [None]:
        want = rr.render(meshes, draws, view, proj, w, h, window=win)
        x0, y0, x1, y1 = (0, 0, w, h) if win is None else win
        for g, e, name in zip(got, want, ("rgba8", "prim_id", "depth24")):
            g = g[y0:y1, x0:x1]
            bad = np.argwhere(g != e)
            assert bad.size == 0, (name, win, bad[:5].tolist(), g[tuple(bad[0][:2])], e[tuple(bad[0][:2])])
    return got


def random_scene(rng):
    """Triangles of many kinds in front of, across and behind a random camera; several draws, some sharing a mesh."""
    n = int(rng.integers(1, 40))
    pts = []
    for _ in range(n):
        k = rng.integers(0, 8)
        if k == 0:   # small random
            c = rng.normal(0, 2, 3)
            pts.append(c + rng.normal(0, 0.6, (3, 3)))
        elif k == 1:   # huge: covers the frame
            c = rng.normal(0, 0.5, 3)
            pts.append(c + rng.normal(0, 60, (3, 3)))
        elif k == 2:   # degenerate: repeated vertex or collinear
            a, b = rng.normal(0, 2, 3), rng.normal(0, 2, 3)
            pts.append(np.stack([a, b, a if rng.random() < 0.5 else 0.5 * (a + b)]))
        elif k == 3:   # straddles the camera plane (near clip)
            c = rng.normal(0, 1, 3)
            pts.append(c + np.array([[0, 0, -12.0], [1, 0, 12.0], [0, 1, 12.0]]) * rng.uniform(0.2, 2))
        elif k == 4:   # non-finite
            t = rng.normal(0, 2, (3, 3))
            t[rng.integers(0, 3), rng.integers(0, 3)] = [np.inf, -np.inf, np.nan][rng.integers(0, 3)]
            pts.append(t)
        elif k == 5:   # shared edge: a quad as two triangles
            o, u, v = rng.normal(0, 2, 3), rng.normal(0, 1, 3), rng.normal(0, 1, 3)
            pts.append(np.stack([o, o + u, o + u + v])); pts.append(np.stack([o, o + u + v, o + v]))
        elif k == 6:   # grazing the guard band: far off to the side, close to the eye plane
            pts.append(np.array([[0, 0, 1e-3], [5e3, 1, 2], [0, 5e3, 3]]) * rng.choice([-1, 1], 3) + rng.normal(0, 0.1, (3, 3)))
        else:   # behind the camera
            pts.append(rng.normal(0, 1, (3, 3)) + np.array([0, 0, 30.0]))
    tri = np.concatenate([p.reshape(-1, 3) for p in pts]).astype(np.float32)
    idx = np.arange(tri.shape[0], dtype=np.uint32)
    if rng.random() < 0.5:
        idx = rng.permutation(idx).astype(np.uint32)
    k = max(1, tri.shape[0] // 6) * 3   # a second mesh: the first half of the triangles
    meshes = {0: (tri, idx), 1: (tri[:k].copy(), np.arange(k, dtype=np.uint32))}
    draws = [rt.raster_draw(0, None, rng.uniform(-0.2, 1.3, 3))]
    for _ in range(int(rng.integers(0, 3))):
        m = np.eye(4, dtype=np.float32)
        if rng.random() < 0.5:
            m[3, :3] = rng.normal(0, 0.5, 3)
        draws.append(rt.raster_draw(int(rng.integers(0, 2)), m.reshape(-1), rng.uniform(0, 1, 3)))
    if rng.random() < 0.5:   # equal-depth overlap: the same mesh with the same matrix again
        draws.append(rt.raster_draw(draws[0].mesh, list(draws[0].model), rng.uniform(0, 1, 3)))
    return meshes, draws


def test_fuzz_against_reference():
    rng = np.random.default_rng(20261016)
    sizes = [(97, 61), (300, 17), (128, 128), (33, 200), (16, 16)]
    with rt.Renderer() as ren:
        for it in range(200):
            w, h = sizes[it % len(sizes)]
            if (ren.width, ren.height) != (w, h):
                ren.resize(w, h)
            cam = rt.default_camera()
            cam.pos[0], cam.pos[1], cam.pos[2] = rng.normal(0, 1, 3) + [0, 0, 6]
            cam.yaw, cam.pitch, cam.fov, cam.aspect = -90 + rng.normal(0, 15), rng.normal(0, 10), rng.uniform(30, 100), w / h
            view, proj = rt.camera_view(cam), rt.camera_proj(cam)
            meshes, draws = random_scene(rng)
            for s, (p, i) in meshes.items():
                ren.raster_mesh(s, p, i)
            try:
                check(ren, meshes, draws, view, proj, w, h)
            except AssertionError as e:
                raise AssertionError(f"scene {it}: {e}") from None
            st = ren.raster_stats()
            assert st.trianglesSetUp + st.trianglesDropped == st.trianglesIn


def test_fuzz_past_the_bin_capacity():
    """Bins too small for the frame: the triangles past the capacity are rasterised from the triangle list; same frame."""
    rng = np.random.default_rng(7)
    with rt.Renderer() as ren:
        ren.resize(97, 61)
        ren.debug_raster_bin_capacity(37)
        for it in range(20):
            cam = rt.default_camera()
            cam.aspect = 97 / 61
            view, proj = rt.camera_view(cam), rt.camera_proj(cam)
            meshes, draws = random_scene(rng)
            for s, (p, i) in meshes.items():
                ren.raster_mesh(s, p, i)
            check(ren, meshes, draws, view, proj, 97, 61)
            st = ren.raster_stats()
            assert st.binCapacity == 37


@pytest.mark.parametrize("camera", ["default", "closeup"])
@pytest.mark.parametrize("light", ["on", "off", "orbit"])
def test_render_raster_scene_1080p(camera, light):
    W, H = 1920, 1080
    meshes = scene_meshes()
    p = rt.default_render_params()
    p.pointLightEnabled = int(light != "off")
    if light == "orbit":
        p.pointLightOrbitEnabled, p.pointLightYaw, p.pointLightPitch = 1, 60.0, 15.0
    cam = scenes.camera(camera, aspect=W / H)
    view, proj = rt.camera_view(cam), rt.camera_proj(cam)
    draws = rt.raster_scene_draws(p, 0, 1, 2)
    with rt.Renderer() as ren:
        ren.resize(W, H)
        for s, (pp, i) in meshes.items():
            ren.raster_mesh(s, pp, i)
        full = camera == "default" and light == "on"
        wins = None if full else [(0, 0, 256, 160), (700, 400, 1000, 700), (1200, 300, 1500, 650), (1800, 1000, 1920, 1080)]
        got = check(ren, meshes, draws, view, proj, W, H, windows=wins)
        prim = got[1]
        assert (prim != rr.BACKGROUND).any() and (prim == rr.BACKGROUND).any() or camera == "closeup"
        st = ren.raster_stats()
        assert st.trianglesIn == sum(m[1].size // 3 for m in [meshes[d.mesh] for d in draws])
        assert st.trianglesSetUp + st.trianglesDropped == st.trianglesIn and st.deviceMs > 0


def test_million_triangles_1080p_windows():
    W, H = 1920, 1080
    pos, idx = meshgen.million_triangle_scene()[:2]
    cam = scenes.camera("default", aspect=W / H)
    view, proj = rt.camera_view(cam), rt.camera_proj(cam)
    draws = [rt.raster_draw(0, None, (0.8, 0.7, 0.6))]
    with rt.Renderer() as ren:
        ren.resize(W, H)
        ren.raster_mesh(0, pos, idx)
        check(ren, {0: (pos, idx)}, draws, view, proj, W, H, windows=[(900, 500, 1000, 580), (300, 200, 380, 260), (1500, 700, 1560, 760)])
        st = ren.raster_stats()
        assert st.trianglesIn == idx.size // 3
        assert st.trianglesSetUp + st.trianglesDropped == st.trianglesIn
        assert st.binEntries >= st.trianglesSetUp // 4 and st.rasterBytes > 0


def test_deterministic_and_resize():
    meshes = scene_meshes()
    p = rt.default_render_params()
    draws = rt.raster_scene_draws(p, 0, 1, 2)
    with rt.Renderer() as ren:
        for s, (pp, i) in meshes.items():
            ren.raster_mesh(s, pp, i)
        for (w, h) in [(320, 180), (257, 129), (320, 180)]:
            cam = scenes.camera("default", aspect=w / h)
            view, proj = rt.camera_view(cam), rt.camera_proj(cam)
            ren.resize(w, h)
            a = ren.render_raster(draws, view, proj)
            b = ren.render_raster(draws, view, proj)
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
            want = rr.render(meshes, draws, view, proj, w, h)
            for x, y in zip(a, want):
                assert np.array_equal(x, y)
        ren.render_raster_async([], view, proj)
        rgba, prim, depth = ren.read_raster()
        assert (prim == rr.BACKGROUND).all() and (depth == rr.D24_MAX).all()
        assert (rgba.reshape(-1, 4) == [rr.unorm8(0.1), 0, rr.unorm8(0.2), 255]).all()


@pytest.mark.parametrize("pipeline", [rt.RT_PIPELINE_WAVEFRONT, rt.RT_PIPELINE_MEGAKERNEL])
def test_raster_leaves_ray_frames_alone(pipeline):
    W, H = 160, 96
    nodes, tris = scenes.bunny_bvh(3)
    p = rt.default_render_params()
    p.sppPerFrame = 1
    cam = scenes.camera("closeup", aspect=W / H)
    meshes = scene_meshes()
    draws = rt.raster_scene_draws(p, 0, 1, 2)
    view, proj = rt.camera_view(cam), rt.camera_proj(cam)

    def run(interleave):
        with rt.Renderer(pipeline=pipeline) as ren:
            ren.upload_bvh(nodes, tris)
            ren.resize(W, H)
            out = []
            for f in range(3):
                if interleave:
                    for s, (pp, i) in meshes.items():
                        ren.raster_mesh(s, pp, i)
                    ren.render_raster_async(draws, view, proj)
                ren.render_ray(p, cam, use_bvh=True)
                if interleave:
                    ren.render_raster(draws, view, proj)
                out.append((ren.read_target(rt.RT_TARGET_COLOR).copy(), ren.frame_index))
            return out, ren.memory_info()   # after the raster calls: they add nothing to the ray pipeline's memory

    a, mem_a = run(False)
    b, mem_b = run(True)
    for (ca, fa), (cb, fb) in zip(a, b):
        assert fa == fb and np.array_equal(ca, cb)
    for k in ("queueArenaBytes", "frameArrayBytes", "hybridArenaBytes", "queueArenas", "lanes"):
        assert getattr(mem_a, k) == getattr(mem_b, k)


def test_memory_info_unchanged_before_first_raster_call():
    with rt.Renderer() as ren:
        ren.resize(64, 48)
        m0 = ren.memory_info()
        st = ren.raster_stats()
        assert st.rasterBytes == 0
        ren.raster_mesh(0, *ground_quad())
        m1 = ren.memory_info()
        for k in ("queueArenaBytes", "frameArrayBytes", "hybridArenaBytes", "queueArenas", "lanes"):
            assert getattr(m0, k) == getattr(m1, k)


def test_read_after_resize_is_refused_until_rendered_again():
    """rt_read_raster fills buffers of the framebuffer's size: after rt_resize the old raster frame no longer fits them."""
    meshes = scene_meshes()
    draws = rt.raster_scene_draws(rt.default_render_params(), 0, 1, 2)
    with rt.Renderer() as ren:
        for s, (pp, i) in meshes.items():
            ren.raster_mesh(s, pp, i)
        ren.resize(320, 180)
        cam = scenes.camera("default", aspect=320 / 180)
        view, proj = rt.camera_view(cam), rt.camera_proj(cam)
        ren.render_raster(draws, view, proj)
        for (w, h) in [(64, 48), (640, 360)]:
            ren.resize(w, h)
            with pytest.raises(rt.RtError) as e:
                ren.read_raster()
            assert e.value.code == rt.RT_ERR_STATE and "render it again" in str(e.value)
        got = ren.render_raster(draws, view, proj)
        want = rr.render(meshes, draws, view, proj, 640, 360)
        for g, x in zip(got, want):
            assert g.shape[:2] == (360, 640) and np.array_equal(g, x)


def test_errors():
    view = proj = np.eye(4, dtype=np.float32).reshape(-1)
    with rt.Renderer() as ren:
        ren.raster_mesh(0, *ground_quad())
        with pytest.raises(rt.RtError) as e:
            ren.render_raster([rt.raster_draw(0)], view, proj)
        assert e.value.code == rt.RT_ERR_STATE
        ren.resize(32, 32)
        for bad in (-1, rt.RT_MAX_RASTER_MESHES):
            with pytest.raises(rt.RtError) as e:
                ren.raster_mesh(bad, *ground_quad())
            assert e.value.code == rt.RT_ERR_INVALID
            with pytest.raises(rt.RtError) as e:
                ren.render_raster([rt.raster_draw(bad)], view, proj)
            assert e.value.code == rt.RT_ERR_INVALID
        with pytest.raises(rt.RtError) as e:
            ren.raster_mesh(1, *ground_quad()[:1], np.array([0, 1, 4], np.uint32))
        assert e.value.code == rt.RT_ERR_INVALID and "nVerts" in str(e.value)
        with pytest.raises(rt.RtError) as e:
            ren.raster_mesh(1, ground_quad()[0], np.array([0, 1], np.uint32))
        assert e.value.code == rt.RT_ERR_INVALID
        ren.render_raster([rt.raster_draw(0)], view, proj)
        ren.raster_mesh(0, None)
        with pytest.raises(rt.RtError) as e:
            ren.render_raster([rt.raster_draw(0)], view, proj)
        assert e.value.code == rt.RT_ERR_STATE


def test_raster_refused_on_tile_parallel_ranks():
    with rt.Renderer(rank=0, world_size=2) as r:
        r.resize(64, 48)
        r.raster_mesh(0, *ground_quad())
        with pytest.raises(rt.RtError) as e:
            r.render_raster([rt.raster_draw(0)], np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32))
        assert e.value.code == rt.RT_ERR_UNSUPPORTED and "tile-parallel" in str(e.value)


def test_cli_raster_png_equals_render_raster(tmp_path):
    meshes = scene_meshes()
    paths = {}
    for name, slot in (("ground", 0), ("bunny", 1), ("sphere", 2)):
        paths[name] = str(tmp_path / f"{name}.obj")
        meshgen.write_obj(paths[name], *meshes[slot])
    W, H = 240, 135
    out = str(tmp_path / "raster.png")
    cli = os.path.join(ROOT, "opengl-raytracing_amd", "rt_cli")
    r = subprocess.run([cli, "--raster", "--obj", paths["bunny"], "--ground", paths["ground"], "--sphere", paths["sphere"], "--size", f"{W}x{H}",
                        "--out", out[:-4]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    png = rt.load_png(out)
    loaded = {s: rt.load_obj(paths[n]) for n, s in (("ground", 0), ("bunny", 1), ("sphere", 2))}
    cam = rt.default_camera()
    cam.aspect = W / H
    p = rt.default_render_params()
    with rt.Renderer() as ren:
        ren.resize(W, H)
        for s, (pp, i) in loaded.items():
            ren.raster_mesh(s, pp, i)
        rgba, _, _ = ren.render_raster(rt.raster_scene_draws(p, 0, 1, 2), rt.camera_view(cam), rt.camera_proj(cam))
    assert np.array_equal(png[::-1], rgba)
