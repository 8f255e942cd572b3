"""Scene queries and pixel picking, host side (no GPU): the numpy restatement of tests/analytic_ref.py pinned to the oracle's own
frames (every pixel's primary answer is what GPOS / GNRM show, bit for bit at f16), and the C ABI of rt_trace_scene_rays / rt_pick_pixels."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import analytic_ref as ar
import opengl_raytracing_amd as rt

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
W, H = 64, 40


def _mesh(where):
    """The bunny stand-in between the camera and the spheres, or around the albedo sphere (partly inside it)."""
    v, f = rt.meshgen.bunny_standin(2)
    M = np.eye(4, dtype=np.float32)
    if where == "front":
        M[0, 3], M[1, 3], M[2, 3] = 0.1, 1.0, 0.0
    else:
        M[0, 0] = M[1, 1] = M[2, 2] = 1.6
        M[0, 3], M[1, 3], M[2, 3] = -1.2, 1.0, -3.5
    return rt.build_bvh(rt.gather_triangles(v, f, M.T.reshape(-1)))       # column-major


def _uniforms(orc, mode, frame, light, nodes=None, tris=None):
    p = orc.default_render_params()
    p.sppPerFrame = 1
    p.enableJitter = 1
    cam = orc.default_camera()
    cam.aspect = W / H
    args = (nodes.shape[0], tris.shape[0]) if nodes is not None else ()
    u = orc.frame_uniforms(p, cam, W, H, frame, mode, *args, env_loaded=False)
    u.pointLightEnabled = 1 if light else 0
    u.pointLightPos[:] = (0.35, 1.55, 3.0)       # the marker in view, in front of the spheres
    u.enableGI = u.enableAO = 0                  # GPOS / GNRM depend on the primary answer only
    return u


def _pick_all(u, nodes=None, tris=None):
    y, x = np.mgrid[0:H, 0:W]
    xy = np.stack([x.reshape(-1), y.reshape(-1)], axis=1).astype(np.int32)
    ro, rd = ar.pixel_rays(u, xy)
    if u.useBVH == rt.RT_SCENE_HYBRID and nodes is not None:
        return ar.trace_hybrid(u, nodes, tris, ro, rd)
    return ar.trace_analytic(u, ro, rd)


@pytest.mark.parametrize("case", ["analytic-light", "analytic-dark", "hybrid-front", "hybrid-inside", "hybrid-inside-dark"])
def test_restated_picks_are_the_oracle_frames(orc, case):
    mode, rest = case.split("-", 1)
    light = not rest.endswith("dark")
    nodes = tris = None
    if mode == "hybrid":
        nodes, tris = _mesh(rest.split("-")[0])
    u = _uniforms(orc, rt.RT_SCENE_HYBRID if mode == "hybrid" else 0, 3, light, nodes, tris)
    assert u.enableJitter == 1 and (u.jitter[0] != 0 or u.jitter[1] != 0)
    (_, _, gpos, gnrm), _ = orc.render(u, nodes, tris)
    a = _pick_all(u, nodes, tris)
    want_pos, want_nrm = ar.gbuffer(a)
    assert np.array_equal(want_pos.reshape(H, W, 4), gpos)
    assert np.array_equal(want_nrm.reshape(H, W, 4), gnrm)
    seen = set(np.unique(a.obj).tolist())
    assert {-1, rt.RT_OBJECT_FLOOR, 3} <= seen                                          # sky, floor and mirror sphere on screen
    assert (1 in seen) == (rest != "inside" and rest != "inside-dark")        # the albedo sphere, unless the mesh around it hides it
    assert (rt.RT_OBJECT_POINT_LIGHT in seen) == light
    if mode == "hybrid":
        assert (a.obj == rt.RT_OBJECT_MESH).sum() > 50


def test_hybrid_without_a_mesh_is_the_analytic_scene(orc):
    u = _uniforms(orc, rt.RT_SCENE_HYBRID, 1, True)
    (_, _, gpos, gnrm), _ = orc.render(u)
    a = _pick_all(u)
    assert not (a.obj == rt.RT_OBJECT_MESH).any()
    want_pos, want_nrm = ar.gbuffer(a)
    assert np.array_equal(want_pos.reshape(H, W, 4), gpos) and np.array_equal(want_nrm.reshape(H, W, 4), gnrm)


def test_restatement_flags_and_bounds(orc):
    u = _uniforms(orc, 0, 0, True)
    # a ray through the glass sphere's centre, from in front of it: skipping the glass reveals the floor behind it / the sky
    ro = np.array([[0.7, 1.0, -3.5]], f32)
    rd = ar.normalize(np.array([[0.0, -0.05, -1.0]], f32))
    assert ar.trace_analytic(u, ro, rd).obj[0] == 2
    assert ar.trace_analytic(u, ro, rd, include_glass=False).obj[0] == rt.RT_OBJECT_FLOOR
    # the marker only when asked for and enabled
    m = np.array(list(u.pointLightPos), f32)
    rd = ar.normalize((m - np.array([0.0, 2.0, 8.0], f32))[None, :])
    ro = np.array([[0.0, 2.0, 8.0]], f32)
    assert ar.trace_analytic(u, ro, rd).obj[0] == rt.RT_OBJECT_POINT_LIGHT
    assert ar.trace_analytic(u, ro, rd, include_marker=False).obj[0] != rt.RT_OBJECT_POINT_LIGHT
    u.pointLightEnabled = 0
    assert ar.trace_analytic(u, ro, rd).obj[0] != rt.RT_OBJECT_POINT_LIGHT
    # tMax: inclusive, negative = empty
    a = ar.trace_analytic(u, ro, rd)
    t = a.t[0]
    for tm, hit in ((t, True), (np.nextafter(t, f32(np.inf)), True), (np.nextafter(t, f32(0)), False), (f32(-1), False)):
        assert (ar.bounded(u, a, np.array([tm], f32)).obj[0] >= 0) == hit
    # a ray starting inside a sphere takes the far root
    a = ar.trace_analytic(u, np.array([[-1.2, 1.0, -3.5]], f32), np.array([[1.0, 0.0, 0.0]], f32))
    assert a.obj[0] == 1 and abs(a.t[0] - 1.0) < 1e-6


# ---------------------------------------------------------------- C ABI

NEW = ("rt_trace_scene_rays", "rt_trace_scene_rays_host", "rt_pick_pixels", "rt_pick_pixels_host")


def test_header_declares_the_scene_query_entries():
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "rt_mi355.h").read_text(), flags=re.S)
    consts = {"RT_QUERY_SKIP_GLASS": 1, "RT_QUERY_SKIP_MARKER": 2, "RT_OBJECT_FLOOR": 0, "RT_OBJECT_ALBEDO_SPHERE": 1, "RT_OBJECT_GLASS_SPHERE": 2,
              "RT_OBJECT_MIRROR_SPHERE": 3, "RT_OBJECT_POINT_LIGHT": 4, "RT_OBJECT_MESH": 5}
    for name, v in consts.items():
        assert re.search(rf"#define {name} {v}\b", code), name
        assert getattr(rt, name) == v
    assert re.search(r"#define RT_OBJECT_NONE \(-1\)", code) and rt.RT_OBJECT_NONE == -1
    # the scene flags keep their own names and values
    assert rt.RT_SCENE_HYBRID == 2 and "RT_QUERY_SKIP_GLASS" not in rt.__dict__.get("RT_SCENE_BITS", {})
    L = rt.lib()
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", code), name
        assert name in rt.SIGNATURES and hasattr(L, name)
    assert (ar.FLOOR, ar.MARKER, ar.MESH) == (rt.RT_OBJECT_FLOOR, rt.RT_OBJECT_POINT_LIGHT, rt.RT_OBJECT_MESH)


def test_null_context_is_invalid():
    L = rt.lib()
    u = rt.RtUniforms()
    for fn in (L.rt_trace_scene_rays, L.rt_trace_scene_rays_host):
        assert fn(None, C.byref(u), 0, 0, None, 3, None, 3, None, 0, None, None, None, None, None) == rt.RT_ERR_INVALID
    for fn in (L.rt_pick_pixels, L.rt_pick_pixels_host):
        assert fn(None, C.byref(u), None, 0, None, None, None, None) == rt.RT_ERR_INVALID


def test_python_argument_errors_come_before_any_device_work():
    """Renderer methods refuse malformed arrays before they reach the library (no context needed to see it)."""
    ren = object.__new__(rt.Renderer)      # no RtContext: any library call would fail with a different error
    ren._h = C.c_void_p()
    u = rt.RtUniforms()
    o = np.zeros((4, 3), f32)
    with pytest.raises(rt.RtError, match="any-hit queries need tmax"):
        ren.trace_scene_rays(u, o, o, any_hit=True)
    with pytest.raises(rt.RtError, match="float32"):
        ren.trace_scene_rays(u, o.astype(np.float64), o)
    with pytest.raises(rt.RtError, match="k >= 3"):
        ren.trace_scene_rays(u, o[:, :2].copy(), o)
    with pytest.raises(rt.RtError, match="tmax must be"):
        ren.trace_scene_rays(u, o, o, tmax=np.zeros(3, f32))
    with pytest.raises(rt.RtError, match="int32"):
        ren.pick(u, np.zeros((4, 2), np.int64))
    with pytest.raises(rt.RtError, match="int32"):
        ren.pick(u, np.zeros((4, 3), np.int32))
