"""The raster preview without a GPU: hand-computed cases of the rules (tests/raster_ref.py = DESIGN.md 11), the host-side draw list
of renderRaster (rt_raster_scene_draws) and the argument checks of the new entry points."""
import ctypes as C

import numpy as np

import opengl_raytracing_amd as rt
import raster_ref as rr

I16 = np.eye(4, dtype=np.float32).reshape(-1)
W = H = 8


def ndc_tri(pts, z=0.5, w=W, h=H):
    """Window-space points (pixels, y up) -> NDC positions for identity view / projection (exact for these coordinates)."""
    zs = z if isinstance(z, (list, tuple)) else [z] * len(pts)
    return np.array([[2.0 * x / w - 1.0, 2.0 * y / h - 1.0, zz] for (x, y), zz in zip(pts, zs)], np.float32)


def covered(pos, idx=None, w=W, h=H, draws=None, meshes=None):
    if meshes is None:
        idx = np.arange(pos.shape[0], dtype=np.uint32) if idx is None else idx
        meshes, draws = {0: (pos, idx)}, [(0, I16, (1, 1, 1))]
    _, prim, depth = rr.render(meshes, draws, I16, I16, w, h)
    return prim, depth


def cells(prim):
    ys, xs = np.nonzero(prim != rr.BACKGROUND)
    return set(zip(xs.tolist(), ys.tolist()))


def test_triangle_covered_pixel_set():
    prim, _ = covered(ndc_tri([(0, 0), (4, 0), (0, 4)]))
    # centres (i + .5, j + .5) with i + j < 3 are inside; i + j == 3 lies ON the hypotenuse, a right-hand edge: not owned
    assert cells(prim) == {(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (0, 2)}


def test_top_left_ownership_horizontal_edge():
    lower = ndc_tri([(0.25, 0.25), (6.25, 2.5), (0.25, 2.5)])   # its top edge runs through the centres of row 2
    upper = ndc_tri([(0.25, 2.5), (6.25, 2.5), (0.25, 5.0)])    # the same edge is its bottom edge
    low = cells(covered(lower)[0])
    up = cells(covered(upper)[0])
    assert {(i, 2) for i in range(6)} <= low
    assert not any(y == 2 for _, y in up)


def test_top_left_ownership_vertical_edge():
    left = ndc_tri([(0.25, 0.25), (2.5, 0.25), (2.5, 6.25)])    # right edge x = 2.5 through the centres of column 2
    right = ndc_tri([(2.5, 0.25), (6.0, 6.25), (2.5, 6.25)])    # left edge x = 2.5
    assert not any(x == 2 for x, _ in cells(covered(left)[0]))
    assert {(2, j) for j in range(1, 6)} <= cells(covered(right)[0])


def _count_cover(tris, w, h):
    count = np.zeros((h, w), np.int32)
    for t in tris:
        prim, _ = covered(t, w=w, h=h)
        count += prim != rr.BACKGROUND
    return count


def test_quad_diagonal_covers_each_pixel_once():
    q = [(0.3, 0.7), (7.1, 0.2), (7.6, 6.9), (0.1, 7.3)]
    count = _count_cover([ndc_tri([q[0], q[1], q[2]]), ndc_tri([q[0], q[2], q[3]])], W, H)
    assert count.max() == 1
    # every centre of this 8 x 8 frame lies strictly inside the quad except those cut off at its slanted borders
    inside = np.zeros((H, W), bool)
    for j in range(H):
        for i in range(W):
            x, y = i + 0.5, j + 0.5
            s = [(bx - ax) * (y - ay) - (by - ay) * (x - ax) for (ax, ay), (bx, by) in zip(q, q[1:] + q[:1])]
            inside[j, i] = all(v > 0 for v in s)
    assert (count[inside] == 1).all() and (count[~inside] == 0).all()


def test_fan_of_64_covers_each_pixel_once():
    n, size = 64, 64
    c = (31.3, 32.7)
    ang = np.arange(n + 1) * (2 * np.pi / n)
    ring = [(c[0] + 29.0 * np.cos(a), c[1] + 29.0 * np.sin(a)) for a in ang]
    # snap the ring to 1/256 pixel first so that the shared edges are identical for both neighbours
    ring = [(round(x * 256) / 256, round(y * 256) / 256) for x, y in ring]
    ring[-1] = ring[0]
    tris = [ndc_tri([c, ring[k], ring[k + 1]], w=size, h=size) for k in range(n)]
    count = _count_cover(tris, size, size)
    assert count.max() == 1
    # the polygon's interior: every centre inside it strictly
    poly = ring[:-1]
    for j in range(size):
        for i in range(size):
            x, y = i + 0.5, j + 0.5
            s = [(bx - ax) * (y - ay) - (by - ay) * (x - ax) for (ax, ay), (bx, by) in zip(poly, poly[1:] + poly[:1])]
            if all(v > 1e-6 for v in s):
                assert count[j, i] == 1, (i, j)


def test_triangle_crossing_the_near_plane():
    # identity projection: w = 1, near plane z >= -1.  z runs from -3 at (0,0) to 0.5 at the other two vertices:
    # z = -3 + 3.5 (x + y) / 8 >= -1  <=>  x + y >= 4.571; the hypotenuse x + y = 8 is not owned -> i + j in {4, 5, 6}
    pos = ndc_tri([(0, 0), (8, 0), (0, 8)], z=[-3.0, 0.5, 0.5])
    _, _, _, st = rr.render({0: (pos, np.arange(3, dtype=np.uint32))}, [(0, I16, (1, 1, 1))], I16, I16, W, H, return_stats=True)
    prim, depth = covered(pos)
    assert cells(prim) == {(i, j) for i in range(8) for j in range(8) if 4 <= i + j <= 6}
    assert st == {"in": 1, "dropped": 0, "clipped": 1, "set_up": 1}
    assert depth[prim != rr.BACKGROUND].max() < rr.D24_MAX


def test_triangle_behind_the_camera_is_dropped():
    cam = rt.default_camera()
    view, proj = rt.camera_view(cam), rt.camera_proj(cam)
    pos = np.array([[-1, 2, 9.0], [1, 2, 9.0], [0, 3, 9.5]], np.float32)   # behind the eye at z = 8 looking down -z
    rgba, prim, depth, st = rr.render({0: (pos, np.arange(3, dtype=np.uint32))}, [(0, I16, (1, 0, 0))], view, proj, 32, 18, return_stats=True)
    assert (prim == rr.BACKGROUND).all() and (depth == rr.D24_MAX).all()
    assert st["dropped"] == 1 and st["set_up"] == 0
    assert (rgba.reshape(-1, 4) == [rr.unorm8(0.1), 0, rr.unorm8(0.2), 255]).all()


def test_fragment_at_the_far_plane_is_rejected():
    far = ndc_tri([(0, 0), (8, 0), (0, 8)], z=1.0)
    assert (covered(far)[0] == rr.BACKGROUND).all()
    near_far = ndc_tri([(0, 0), (8, 0), (0, 8)], z=float(np.nextafter(np.float32(1.0), np.float32(0))))
    assert (covered(near_far)[0] == rr.BACKGROUND).all()   # z_w rounds to 1 - 2^-25: d24 = 0xFFFFFF fails the strict test
    assert (covered(ndc_tri([(0, 0), (8, 0), (0, 8)], z=0.99))[0] != rr.BACKGROUND).any()


def test_equal_depth_first_draw_wins_nearer_later_draw_wins():
    t = ndc_tri([(0, 0), (8, 0), (0, 8)], z=0.25)
    idx = np.arange(3, dtype=np.uint32)
    meshes = {0: (t, idx), 1: (ndc_tri([(0, 0), (8, 0), (0, 8)], z=0.2), idx)}
    rgba, prim, _ = rr.render(meshes, [(0, I16, (1, 0, 0)), (0, I16, (0, 1, 0))], I16, I16, W, H)
    drawn = prim != rr.BACKGROUND
    assert drawn.any() and (prim[drawn] == 0).all() and (rgba[drawn][:, :3] == [255, 0, 0]).all()
    rgba, prim, _ = rr.render(meshes, [(0, I16, (1, 0, 0)), (1, I16, (0, 1, 0))], I16, I16, W, H)
    assert (prim[drawn] == 1).all() and (rgba[drawn][:, :3] == [0, 255, 0]).all()


def test_scene_draws_match_render_raster():
    p = rt.default_render_params()
    d = rt.raster_scene_draws(p, 0, 1, 2)
    assert len(d) == 4 and [x.mesh for x in d] == [0, 1, 2, 2]
    assert np.array_equal(np.array(d[0].model, np.float32), I16)
    assert np.allclose(d[0].color, [0.1, 0.4, 0.1]) and np.allclose(d[1].color, [0.9] * 3) and np.allclose(d[2].color, [0.3, 0.6, 1.0])
    assert np.array_equal(np.array(d[1].model, np.float32), rt.default_bvh_transform())
    sphere = np.eye(4, dtype=np.float32)
    sphere[0, 0] = sphere[1, 1] = sphere[2, 2] = 0.5
    sphere[3, :3] = [2.0, 1.0, 0.0]   # column 3 of a column-major matrix
    assert np.array_equal(np.array(d[2].model, np.float32), sphere.reshape(-1))
    cam = rt.default_camera()
    view, proj = rt.camera_view(cam), rt.camera_proj(cam)
    for orbit in (0, 1):
        p.pointLightOrbitEnabled, p.pointLightYaw, p.pointLightPitch = orbit, 37.0, 21.0
        d = rt.raster_scene_draws(p, 0, 1, 2)
        u = rt.make_uniforms(p, cam, view, rt.mat4_mul(proj, view), rt.mat4_mul(proj, view), 64, 36)
        m = np.array(d[3].model, np.float32)
        assert np.array_equal(m[12:15], np.array(u.pointLightPos, np.float32)), orbit
        assert m[0] == m[5] == m[10] == np.float32(0.15) and m[15] == 1.0
        assert np.array_equal(np.array(d[3].color, np.float32), np.array(p.pointLightColor, np.float32) * np.float32(3.0))
    orbit_pos = np.array(rt.raster_scene_draws(p, 0, 1, 2)[3].model, np.float32)[12:15]
    assert not np.array_equal(orbit_pos, np.array(p.pointLightPos, np.float32))
    p.pointLightEnabled = 0
    d = rt.raster_scene_draws(p, 0, 1, 2)
    assert len(d) == 3
    assert [x.mesh for x in rt.raster_scene_draws(p, -1, 1, -1)] == [1]
    assert rt.raster_scene_draws(p, -1, -1, -1) == []


def test_raster_argument_validation_without_device():
    L = rt.lib()
    pos = np.zeros((3, 3), np.float32)
    idx = np.arange(3, dtype=np.uint32)
    assert L.rt_raster_mesh(None, 0, pos.ctypes.data_as(C.POINTER(C.c_float)), 3, idx.ctypes.data_as(C.POINTER(C.c_uint32)), 3) == rt.RT_ERR_INVALID
    assert L.rt_render_raster(None, None, 0, None, None) == rt.RT_ERR_INVALID
    assert L.rt_read_raster(None, None, None, None) == rt.RT_ERR_INVALID
    assert L.rt_get_raster_stats(None, None) == rt.RT_ERR_INVALID
    assert L.rt_debug_raster_bin_capacity(None, 0) == rt.RT_ERR_INVALID
    assert L.rt_raster_scene_draws(None, 0, 1, 2, None) == rt.RT_ERR_INVALID
    assert C.sizeof(rt.RtRasterDraw) == 4 * (1 + 16 + 3)
    assert C.sizeof(rt.RtRasterStats) == 8 * 8
