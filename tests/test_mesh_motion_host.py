"""rt_hit_motion, the host definition of the dynamic mesh's object motion, without a GPU: against its float32 numpy restatement
(tests/motion_ref.py) bit for bit, its refusals, the exports, a null context to every new entry, and its meaning against the oracle -- a mesh placed
rigidly under M0 and then M1 moves, at every primary hit, as the reference's own MOTION target does when the previous view-projection carries the
rigid motion instead."""
import ctypes as C

import numpy as np
import pytest

import analytic_ref
import motion_ref
import opengl_raytracing_amd as rt
from test_gpu_mesh_refit import COORDS

f32 = np.float32
NEW_SYMBOLS = ("rt_mesh_motion_enable", "rt_mesh_motion_latch", "rt_mesh_hit_prev_points", "rt_mesh_hit_prev_points_host", "rt_hit_motion")
INT_MAX = 2 ** 31 - 1


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def records(t, prim, u, v):
    rec = np.zeros((len(prim), 4), f32)
    rec[:, 0], rec[:, 2], rec[:, 3] = t, u, v
    rec[:, 1] = np.asarray(prim, np.int32).view(f32)
    return rec


def uniforms(seed=0):
    """A uniform block whose two view-projections differ: a camera that stepped sideways and turned a little."""
    p, cam = rt.default_render_params(), rt.default_camera()
    prev = rt.mat4_mul(rt.camera_proj(cam), rt.camera_view(cam))
    cam.pos[0] += 0.21 + 0.01 * seed
    cam.yaw += 1.5
    u = rt.frame_uniforms(p, cam, 64, 48, 0, True, 1, 1, prev_vp=prev)
    assert list(u.prevViewProj) != list(u.currViewProj)
    return u


def case(n, n_tris=37, seed=5, scale=0.02):
    """n hits on n_tris rows whose previous pose differs a little in every geometry float; padding words differ too and must not matter."""
    rng = np.random.default_rng(seed + n)
    T = rng.uniform(-2, 2, (n_tris, 12)).astype(f32)
    P = (T + rng.normal(0, scale, T.shape)).astype(f32)
    T[:, 3::4], P[:, 3::4] = 0, 7
    prim = rng.integers(0, n_tris, n).astype(np.int32)
    a, b = rng.uniform(0, 1, n).astype(f32), rng.uniform(0, 1, n).astype(f32)
    x = (T[prim, 0:3] + T[prim, 4:7] * a[:, None] + T[prim, 8:11] * b[:, None] + np.array([0, 1, -4], f32)).astype(f32)
    return T, P, records(rng.uniform(1, 9, n), prim, a, b), x


def check(u, T, P, rec, x):
    prev, mo = rt.hit_motion(u, T, P, rec, x)
    rp, rm = motion_ref.hit_motion(u, T, P, rec, x)
    assert (bits(prev) == bits(rp)).all() and (bits(mo) == bits(rm)).all()
    only_prev, none = rt.hit_motion(None, T, P, rec, x, want=("prev",))
    assert none is None and (bits(only_prev) == bits(prev)).all()
    none, only_mo = rt.hit_motion(u, T, P, rec, x, want=("motion",))
    assert none is None and (bits(only_mo) == bits(mo)).all()
    return prev, mo


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_equals_the_numpy_definition(n):
    u = uniforms(n)
    T, P, rec, x = case(n)
    prev, mo = check(u, T, P, rec, x)
    assert (bits(prev) != bits(x)).any() and np.abs(mo).max() > 1e-3


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_unchanged_rows_hand_the_point_back(n):
    u = uniforms()
    T, _, rec, x = case(n)
    T[0, COORDS] = [-0.0, 0.0, -0.0, 1.0, -0.0, 0.0, 0.0, -0.0, 1.0]    # -0 coordinates: -0 == +0 as floats, not as bits
    x[::3] = [-0.0, 0.5, -0.0]                                           # x + (+0) would turn -0 into +0
    rec[::5, 2] = np.inf                                                 # 0 * inf would turn the delta into NaN
    P = T.copy()
    P[:, 3::4] = 9                                                       # the padding words are not geometry
    prev, mo = check(u, T, P, rec, x)
    assert (bits(prev) == bits(x)).all()
    two = (motion_ref.ndc_from_world(x, list(u.currViewProj)) - motion_ref.ndc_from_world(x, list(u.prevViewProj))).astype(f32)
    assert (bits(mo) == bits(two)).all()                                 # exactly the reference's motion of one world point
    P[0, 0] = 0.0                                                        # T has -0 there: one bit differs, so the delta form applies
    prev2, _ = check(u, T, P, rec, x)
    hit0 = motion_ref.prims(rec) == 0
    if hit0.any():
        assert (bits(prev2[hit0]) == bits((x[hit0] + f32(0.0)).astype(f32))).all() or not np.isfinite(rec[hit0, 2]).all()


@pytest.mark.parametrize("coord", COORDS)
def test_rows_differing_in_one_float(coord):
    u = uniforms()
    T, _, rec, x = case(65)
    P = T.copy()
    P[:, coord] = np.nextafter(P[:, coord], f32(np.inf))                 # one ulp in one float of every row
    P[5, coord] = T[5, coord] + f32(0.75)
    prev, _ = check(u, T, P, rec, x)
    axis = coord % 4
    others = [c for c in range(3) if c != axis]
    assert (bits(prev[:, others]) == bits((x[:, others] + f32(0.0)).astype(f32))).all()   # only the component of that float moves
    big = motion_ref.prims(rec) == 5
    if coord < 3 and big.any():
        assert np.allclose(prev[big, axis] - x[big, axis], 0.75, atol=1e-5)


def test_prims_outside_the_mesh_give_zeros():
    u = uniforms()
    T, P, rec, x = case(64, n_tris=11)
    bad = np.array([-1, 11, INT_MAX, -INT_MAX - 1, 12, -2], np.int32)
    rec[:6, 1] = bad.view(f32)
    prev, mo = check(u, T, P, rec, x)
    assert (bits(prev[:6]) == 0).all() and (bits(mo[:6]) == 0).all()
    assert (bits(prev[6:]) != 0).any()
    # nothing is read out of bounds: the same call on exactly-sized copies, the last row's hits included
    rec[6, 1] = np.array([10], np.int32).view(f32)[0]
    check(u, T.copy(), P.copy(), rec.copy(), x.copy())


def _raw(u, T, P, n_tris, rec, x, n, prev, mo):
    fp = C.POINTER(C.c_float)

    def ptr(a):
        return None if a is None else a.ctypes.data_as(fp)
    return rt.lib().rt_hit_motion(None if u is None else C.addressof(u), ptr(T), ptr(P), n_tris, None if rec is None else C.c_void_p(rec.ctypes.data), ptr(x), n,
                                  ptr(prev), ptr(mo))


def test_refusals():
    u = uniforms()
    T, P, rec, x = case(9)
    prev, mo = np.zeros((9, 3), f32), np.zeros((9, 2), f32)
    nt = T.shape[0]
    assert _raw(u, T, P, nt, rec, x, 9, prev, mo) == rt.RT_OK
    assert _raw(u, T, P, nt, rec, x, 9, prev, None) == rt.RT_OK and _raw(u, T, P, nt, rec, x, 9, None, mo) == rt.RT_OK
    assert _raw(None, T, P, nt, rec, x, 9, prev, None) == rt.RT_OK                 # no uniforms needed without motion
    assert _raw(u, T, P, nt, rec, x, 0, prev, mo) == rt.RT_OK                      # no hits: nothing to do
    assert _raw(u, T, P, nt, None, None, 0, prev, mo) == rt.RT_OK
    assert _raw(u, T, P, nt, rec, x, 9, None, None) == rt.RT_ERR_INVALID           # both outputs null
    assert _raw(None, T, P, nt, rec, x, 9, prev, mo) == rt.RT_ERR_INVALID          # motion without uniforms
    assert _raw(u, None, P, nt, rec, x, 9, prev, mo) == rt.RT_ERR_INVALID          # a null required array, each of the four
    assert _raw(u, T, None, nt, rec, x, 9, prev, mo) == rt.RT_ERR_INVALID
    assert _raw(u, T, P, nt, None, x, 9, prev, mo) == rt.RT_ERR_INVALID
    assert _raw(u, T, P, nt, rec, None, 9, prev, mo) == rt.RT_ERR_INVALID
    assert _raw(u, T, P, 0, rec, x, 9, prev, mo) == rt.RT_ERR_INVALID              # nTris <= 0
    assert _raw(u, T, P, -3, rec, x, 9, prev, mo) == rt.RT_ERR_INVALID
    assert _raw(u, T, P, nt, rec, x, -1, prev, mo) == rt.RT_ERR_INVALID            # n < 0
    for call in (lambda: rt.hit_motion(u, T, P[:-1], rec, x), lambda: rt.hit_motion(u, T, P, rec, x[:-1]), lambda: rt.hit_motion(u, T, P, rec[:, :3], x),
                 lambda: rt.hit_motion(None, T, P, rec, x), lambda: rt.hit_motion(u, T, P, rec, x, want=())):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt.RT_ERR_INVALID


def test_symbols_are_exported_and_declared():
    L = rt.lib()
    for name in NEW_SYMBOLS:
        assert name in rt.SIGNATURES, name
        assert getattr(L, name) is not None, name
    assert rt.RT_SCENE_ARRAY_PREV_TRIS == 13
    for method in ("mesh_motion_enable", "mesh_motion_latch", "mesh_prev_tris", "mesh_hit_prev_points"):
        assert callable(getattr(rt.Renderer, method)), method


def test_null_context():
    L = rt.lib()
    rec, x, out = np.zeros((4, 4), f32), np.zeros((4, 3), f32), np.zeros((4, 3), f32)
    args = (C.c_void_p(rec.ctypes.data), C.c_void_p(x.ctypes.data), 4, C.c_void_p(out.ctypes.data))
    calls = {
        "rt_mesh_motion_enable": lambda: L.rt_mesh_motion_enable(None, 1),
        "rt_mesh_motion_latch": lambda: L.rt_mesh_motion_latch(None),
        "rt_mesh_hit_prev_points": lambda: L.rt_mesh_hit_prev_points(None, *args),
        "rt_mesh_hit_prev_points_host": lambda: L.rt_mesh_hit_prev_points_host(None, *args),
    }
    assert set(calls) == set(NEW_SYMBOLS) - {"rt_hit_motion"}
    for name, call in calls.items():
        assert call() == rt.RT_ERR_INVALID, name
    size = C.c_size_t(1)
    assert L.rt_debug_read_scene(None, rt.RT_SCENE_ARRAY_PREV_TRIS, None, 0, C.byref(size)) == rt.RT_ERR_INVALID


# ---------------------------------------------------------------- semantics against the oracle
W, H = 64, 48
# Largest |rt_hit_motion - MOTION target of the oracle| over the 472 hit pixels of the scene below, measured on the CPU: 1.209e-4, where
# the largest motion is 0.2605 NDC (8.3 pixels).  The two agree in real arithmetic; what separates them is the target's half precision -- half an ulp of
# binary16 is 2^-13 = 1.22e-4 for a motion in [0.25, 0.5) -- and, far below that, the fp32 rounding of prevVP . M0 . M1^-1.  A sign, transposition or
# ordering error is off by the motion itself, a thousand times as much.
MEASURED_MAX_ABS = 1.209e-4


def _rigid(angle_deg, axis, t, s=0.9):
    a = np.radians(angle_deg)
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    M = np.eye(4)
    M[:3, :3] = R * s
    M[:3, 3] = t
    return M                                                             # row-major 4x4 in float64; column-major float32 for the library: M.T.reshape(-1)


def test_rigid_motion_matches_the_oracles_motion_target(orc):
    v, f = rt.meshgen.icosphere(3)
    assert f.size // 3 == 1280
    M0, M1 = _rigid(10, (0.2, 1, 0.1), (-0.25, 0.95, 2.6), 1.5), _rigid(24, (0.1, 1, -0.2), (0.15, 1.1, 2.8), 1.5)
    col = lambda M: np.ascontiguousarray(M.T, f32).reshape(-1)           # noqa: E731
    t9_now, t9_before = rt.gather_triangles(v, f, col(M1)), rt.gather_triangles(v, f, col(M0))
    nodes, tris, order = rt.build_bvh_order(t9_now)
    prev = np.zeros_like(tris)
    prev[:, COORDS] = t9_before[order]
    p, cam = rt.default_render_params(), rt.default_camera()
    cam.aspect = W / H
    p.enableJitter = 0
    view, vp = rt.camera_view(cam), rt.mat4_mul(rt.camera_proj(cam), rt.camera_view(cam))
    u = rt.make_uniforms(p, cam, view, vp, vp, W, H, 0, True, True, False, nodes.shape[0], tris.shape[0], False)
    # the oracle's primary hits: its own traceBVH along the frame's primary rays, u, v by triHit's operations
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)
    ro, rd = analytic_ref.pixel_rays(u, xy)
    hits = [orc.trace_bvh_prim(u, nodes, tris, ro[i], rd[i]) for i in range(xy.shape[0])]
    prim = np.array([h[0] for h in hits], np.int32)
    t = np.array([h[1] for h in hits], f32)
    hit = prim >= 0
    assert hit.sum() >= 200
    with np.errstate(all="ignore"):
        pts = np.where(hit[:, None], (ro + (rd * t[:, None]).astype(f32)).astype(f32), f32(0))
        T = tris[np.where(hit, prim, 0)]
        pvec = analytic_ref.cross(rd, T[:, 8:11])
        inv = (f32(1.0) / analytic_ref.dot(T[:, 4:7], pvec)).astype(f32)
        tvec = (ro - T[:, 0:3]).astype(f32)
        a = (analytic_ref.dot(tvec, pvec) * inv).astype(f32)
        b = (analytic_ref.dot(rd, analytic_ref.cross(tvec, T[:, 4:7])) * inv).astype(f32)
    _, mo = rt.hit_motion(u, tris, prev, records(t, prim, np.where(hit, a, 0), np.where(hit, b, 0)), pts)
    # the reference's rule with the rigid motion folded into the previous view-projection: prevVP . M0 . M1^-1
    vp64 = np.asarray(vp, np.float64).reshape(4, 4).T
    prev_vp = np.ascontiguousarray((vp64 @ M0 @ np.linalg.inv(M1)).T, f32).reshape(-1)
    u2 = rt.make_uniforms(p, cam, view, vp, prev_vp, W, H, 0, True, True, False, nodes.shape[0], tris.shape[0], False)
    (_, motion, gpos, _), _ = orc.render(u2, nodes, tris, None)
    want = orc.half_to_float(motion).reshape(-1, 2)
    assert (orc.half_to_float(gpos).reshape(-1, 4)[:, 3] == hit).all()   # the same pixels hit
    assert (want[~hit] == 4.0).all()
    diff = np.abs(mo[hit].astype(np.float64) - want[hit])
    pixels = np.abs(want[hit] * np.array([W, H]) / 2).max()
    print(f"hit pixels {hit.sum()}, largest motion {np.abs(want[hit]).max():.4f} NDC = {pixels:.1f} pixels, largest |hit_motion - oracle| {diff.max():.3e}")
    assert pixels > 3.0                                                  # the mesh moves by several pixels
    assert diff.max() <= 2 * MEASURED_MAX_ABS
