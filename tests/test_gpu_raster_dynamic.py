"""Raster draws of the dynamic mesh (rt_raster_mesh_dynamic).  A draw naming a slot bound to the mesh is, by definition, the run of
static draws -- one per non-empty part -- that tests/raster_dynamic_ref.py writes out; every comparison below is bit for bit on RGBA8, primitive id
and depth24, with no tolerance.  The conditions that keep a case honest (something is visible, several parts show, the clipper and the drop paths
run) are asserted on the numpy reference's own output before the device is compared."""
import ctypes as C
import functools

import numpy as np
import pytest

import opengl_raytracing_amd as rt
from opengl_raytracing_amd import meshgen
import raster_dynamic_ref as rd
import raster_ref as rr
import scenes
from test_raster_dynamic_host import part_colors, part_models, soup, split

pytestmark = pytest.mark.gpu

W, H = 97, 61
SLOT = 1                                                   # the bound slot, between the ground quad (0) and the sphere (2)
CAMERAS = {"outside": (0.0, 0.0, 6.0), "inside": (0.0, 0.0, 0.5)}
NS = (1, 9, 100, 1000)
SPLITS = ("one", "singles", "uneven")


def _have_torch():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def _camera(name, w=W, h=H):
    cam = rt.default_camera()
    cam.pos[0], cam.pos[1], cam.pos[2] = CAMERAS[name]
    cam.yaw, cam.pitch, cam.fov, cam.aspect = -90.0, 0.0, 60.0, w / h
    return cam


def _view_proj(name, w=W, h=H):
    cam = _camera(name, w, h)
    return rt.camera_view(cam), rt.camera_proj(cam)


def _trs(angle, scale, t):
    """rotation about z x non-uniform scale, then a translation; column-major 16 floats"""
    M = np.eye(4)
    c, s = np.cos(angle), np.sin(angle)
    M[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.diag(scale)
    M[:3, 3] = t
    return np.ascontiguousarray(M.T, dtype=np.float32).reshape(-1)


DRAW_MODEL = _trs(0.2, (0.9, 1.1, 1.0), (0.1, -0.2, 0.3))                      # the bound draw's own model: not the identity
GROUND_MODEL = _trs(0.0, (1.0, 1.0, 1.0), (0.0, -3.0, 0.0))
SPHERE_MODEL = _trs(0.0, (0.6, 0.6, 0.6), (2.6, 1.6, 1.0))
STATIC = {0: (np.array([[-20, 0, -20], [20, 0, -20], [20, 0, 20], [-20, 0, 20]], np.float32), np.array([0, 2, 1, 0, 3, 2], np.uint32)),
          2: tuple(np.ascontiguousarray(a) for a in meshgen.uv_sphere(8, 4)[:2])}
N_GROUND, N_SPHERE = 2, STATIC[2][1].size // 3


def _draws(model=DRAW_MODEL):
    return [rt.raster_draw(0, GROUND_MODEL, (0.3, 0.5, 0.2)), rt.raster_draw(SLOT, model, (0.9, 0.4, 0.1)), rt.raster_draw(2, SPHERE_MODEL, (0.2, 0.3, 0.9))]


def _upload_static(ren):
    for s, (p, i) in STATIC.items():
        ren.raster_mesh(s, p, i)


def _same_frame(got, want, tag):
    for g, e, name in zip(got, want[:3], ("rgba8", "prim_id", "depth24")):
        bad = np.argwhere(np.asarray(g) != np.asarray(e))
        assert bad.size == 0, (tag, name, len(bad), bad[:4].tolist(), np.asarray(g)[tuple(bad[0][:2])], np.asarray(e)[tuple(bad[0][:2])])


def _same_counts(st, stats, tag):
    assert (st.trianglesIn, st.trianglesDropped, st.trianglesClipped, st.trianglesSetUp) == (stats["in"], stats["dropped"], stats["clipped"], stats["set_up"]), tag
    assert st.trianglesSetUp + st.trianglesDropped == st.trianglesIn


def _reference(v, f, pf, table, colors, camera, draws=None, w=W, h=H, parts=True):
    view, proj = _view_proj(camera, w, h)
    bound = {SLOT: rd.Bound(parts=parts, colors=colors)}
    return rd.render(STATIC, draws or _draws(), bound, (v, f, pf, table), view, proj, w, h)


@functools.lru_cache(maxsize=None)
def _parts_case(n, name, camera, colored):
    """Inputs and the expanded reference's frame for one case of the parts contract: computed once, read only."""
    v, f = soup(n)
    pf = split(name, n)
    k = pf.size - 1
    table = part_models(k)
    colors = part_colors(k) if colored else None
    want = _reference(v, f, pf, table, colors, camera)
    rgba, prim, depth, stats, bases = want
    assert bases == [0, N_GROUND, N_GROUND + n] and stats["in"] == n + N_GROUND + N_SPHERE
    part, _ = rd.prim_parts(prim, bases[1], pf)
    if camera == "outside":
        assert (part >= 0).any(), "the frame shows no triangle of the bound draw"
        if n >= 100 and name != "one":
            assert len(set(part[part >= 0].tolist())) >= 3, "fewer than three parts show"
        assert (prim < N_GROUND).any() and ((prim >= N_GROUND + n) & (prim != rr.BACKGROUND)).any()      # the static draws around it show too
    if camera == "inside" and n == 1000:
        assert stats["clipped"] >= 50 and stats["dropped"] >= 50 and stats["set_up"] >= 50, stats
    for a in (v, f, pf, table, rgba, prim, depth):
        a.setflags(write=False)
    return v, f, pf, table, colors, want


# ---------------------------------------------------------------- 1: single-matrix contract
@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("n", NS)
def test_single_matrix_contract(n, camera):
    v, f = soup(n)
    view, proj = _view_proj(camera)
    draws = [rt.raster_draw(SLOT, DRAW_MODEL, (0.9, 0.4, 1.7))]
    want = rd.render({}, draws, {SLOT: rd.Bound()}, (v, f, np.array([0, n], np.int32), None), view, proj, W, H)
    if camera == "outside":
        assert (want[1] != rr.BACKGROUND).any()
    with rt.Renderer() as ren:
        ren.resize(W, H)
        ren.mesh_upload(v, f)
        ren.raster_mesh_dynamic(SLOT)
        got = ren.render_raster(draws, view, proj)
        _same_frame(got, want, (n, camera, "reference"))
        st = ren.raster_stats()
        _same_counts(st, want[3], (n, camera))
        ren.raster_mesh(3, v, f)                                   # the device's own static route over the same arrays
        got2 = ren.render_raster([rt.raster_draw(3, DRAW_MODEL, (0.9, 0.4, 1.7))], view, proj)
        _same_frame(got2, got, (n, camera, "static route"))
        s2 = ren.raster_stats()
        for key in ("trianglesIn", "trianglesDropped", "trianglesClipped", "trianglesSetUp", "binEntries", "binCapacity"):
            assert getattr(st, key) == getattr(s2, key), key


# ---------------------------------------------------------------- 2: parts contract
@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("name", SPLITS)
@pytest.mark.parametrize("n", NS)
def test_parts_contract(n, name, camera):
    view, proj = _view_proj(camera)
    with rt.Renderer() as ren:
        ren.resize(W, H)
        _upload_static(ren)
        for colored in (False, True):
            v, f, pf, table, colors, want = _parts_case(n, name, camera, colored)
            if not colored:
                ren.mesh_upload_parts(v, f, pf)
                ren.mesh_set_part_matrices(table)
                ren.raster_mesh_dynamic(SLOT, parts=True)
            else:
                ren.raster_part_colors(SLOT, colors)
            got = ren.render_raster(_draws(), view, proj)
            _same_frame(got, want, (n, name, camera, colored))
            _same_counts(ren.raster_stats(), want[3], (n, name, camera, colored))
            part, tri = rt.raster_prim_parts(got[1], want[4][1], pf)
            vis = part >= 0
            assert np.array_equal(pf[part[vis]] + tri[vis], got[1][vis].astype(np.int64) - N_GROUND)
            if colored:                                           # each visible pixel has its part's colour: the part is the one the frame drew
                packed = np.array([rr.pack_rgba(c) for c in colors], np.uint32)
                assert np.array_equal(got[0].view(np.uint32)[..., 0][vis], packed[part[vis]])


@functools.lru_cache(maxsize=None)
def _standin():
    v, f = meshgen.bunny_standin(5)[:2]
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.uint32).reshape(-1)


@pytest.mark.parametrize("k,colored", [(40, False), (40, True), (4096, True)])
def test_parts_contract_standin(k, colored):
    w, h = 160, 96
    v, f = _standin()
    n = f.size // 3
    assert n == 20480
    pf = np.linspace(0, n, k + 1).astype(np.int32)
    table = part_models(k)
    colors = part_colors(k) if colored else None
    want = _reference(v, f, pf, table, colors, "outside", w=w, h=h)
    part, _ = rd.prim_parts(want[1], want[4][1], pf)
    if k == 40:
        assert set(part[part >= 0].tolist()) == set(range(40)), "the stand-in must show all 40 parts"
    view, proj = _view_proj("outside", w, h)
    with rt.Renderer() as ren:
        ren.resize(w, h)
        _upload_static(ren)
        ren.mesh_upload_parts(v, f, pf)
        ren.mesh_set_part_matrices(table)
        ren.raster_mesh_dynamic(SLOT, parts=True, colors=colors)
        got = ren.render_raster(_draws(), view, proj)
        _same_frame(got, want, ("standin", k, colored))
        _same_counts(ren.raster_stats(), want[3], ("standin", k))
        gp, _ = rt.raster_prim_parts(got[1], want[4][1], pf)
        assert np.array_equal(gp, part)


# ---------------------------------------------------------------- 3: non-finite data
def test_non_finite_positions_and_matrix():
    n, name = 100, "uneven"
    v, f, pf, table, colors, clean = _parts_case(n, name, "outside", True)
    v2, t2 = v.copy(), table.copy()
    tri = f.reshape(-1, 3)
    v2[tri[5, 1], 0] = np.inf
    v2[tri[40, 2], 2] = np.nan
    p_bad = int(np.searchsorted(pf, 60, "right") - 1)             # the part of triangle 60: not empty
    assert pf[p_bad + 1] > pf[p_bad]
    t2[p_bad, 13] = np.inf
    want = _reference(v2, f, pf, t2, colors, "outside")
    assert want[3]["dropped"] > clean[3]["dropped"]
    view, proj = _view_proj("outside")
    with rt.Renderer() as ren:
        ren.resize(W, H)
        _upload_static(ren)
        ren.mesh_upload_parts(v2, f, pf)
        ren.mesh_set_part_matrices(t2)
        ren.raster_mesh_dynamic(SLOT, parts=True, colors=colors)
        got = ren.render_raster(_draws(), view, proj)
        _same_frame(got, want, "non-finite")
        st = ren.raster_stats()
        _same_counts(st, want[3], "non-finite")
        assert st.trianglesDropped == want[3]["dropped"]


# ---------------------------------------------------------------- 4: follows the device
def _write_rows(ren, tensor_of, sel, new):
    """rows new[k] into rows sel[k] of a device array of the mesh, on the library stream through torch"""
    import torch
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(np.ascontiguousarray(new, np.float32)).to(dev)
    ix = torch.from_numpy(np.asarray(sel, np.int64)).to(dev)
    torch.cuda.current_stream(dev).synchronize()
    ext = torch.cuda.ExternalStream(ren.stream(), device=dev)
    with torch.cuda.stream(ext):
        tensor_of().index_copy_(0, ix, d)
    torch.cuda.current_stream(dev).wait_stream(ext)               # `d` and `ix` stay tied to torch's own stream


def test_follows_the_device():
    n, name = 100, "uneven"
    v, f, pf, table, colors, want0 = _parts_case(n, name, "outside", True)
    k = pf.size - 1
    view, proj = _view_proj("outside")
    rng = np.random.default_rng(4)
    with rt.Renderer() as ren:
        ren.resize(W, H)
        _upload_static(ren)
        ren.mesh_upload_parts(v, f, pf)
        ren.mesh_set_part_matrices(table)
        ren.raster_mesh_dynamic(SLOT, parts=True, colors=colors)
        _same_frame(ren.render_raster(_draws(), view, proj), want0, "first")
        pos, cur = np.array(v), np.array(table)
        marks = []

        def step(tag):
            want = _reference(pos, f, pf, cur, colors, "outside")
            assert not all(np.array_equal(a, b) for a, b in zip(want[:3], want0[:3])), (tag, "the state did not change the frame")
            _same_frame(ren.render_raster(_draws(), view, proj), want, tag)
            i = ren.mesh_info()
            marks.append((ren.raster_stats().rasterBytes, i.allocations, i.hostSyncs))

        pos = (pos + rng.normal(0, 0.2, pos.shape)).astype(np.float32)       # positions from the host
        ren.mesh_set_positions(pos)
        step("mesh_set_positions")
        if _have_torch():                                                    # positions written on the device
            sel = np.arange(0, pos.shape[0], 3)
            pos[sel] = (pos[sel] + rng.normal(0, 0.3, (sel.size, 3))).astype(np.float32)
            _write_rows(ren, ren.mesh_positions, sel, pos[sel])
            step("positions on the device")
        other = part_models(k, shift=k + 3)
        sel = np.arange(1, k, 2)
        cur[sel] = other[sel]
        if _have_torch():                                                    # every second matrix through the device table ...
            _write_rows(ren, ren.mesh_part_matrices, sel, cur[sel])
        else:
            for p in sel:
                ren.mesh_set_part_matrices(cur[p:p + 1], first=int(p))
        step("matrices on the device")
        cur[0:k:4] = other[0:k:4]                                            # ... and others through mesh_set_part_matrices
        for p in range(0, k, 4):
            ren.mesh_set_part_matrices(cur[p:p + 1], first=p)
        step("mesh_set_part_matrices")
        assert len(set(marks)) == 1, marks                                   # no allocation, no host wait, from the second bound call on


# ---------------------------------------------------------------- 5: back to back, no host wait
def test_back_to_back_without_a_host_wait():
    n, name = 1000, "uneven"
    v, f, pf, table, colors, _ = _parts_case(n, name, "outside", True)
    k = pf.size - 1
    rng = np.random.default_rng(5)
    A = (v + rng.normal(0, 0.2, v.shape)).astype(np.float32)
    B = (v + rng.normal(0, 0.2, v.shape)).astype(np.float32)
    T1 = part_models(k, shift=k + 3)
    want = _reference(A, f, pf, T1, colors, "outside")
    assert not np.array_equal(want[1], _reference(B, f, pf, T1, colors, "outside")[1])
    assert not np.array_equal(want[1], _reference(A, f, pf, table, colors, "outside")[1])
    view, proj = _view_proj("outside")
    p = rt.default_render_params()
    p.sppPerFrame = 1
    cam = _camera("outside")

    def run(raster):
        with rt.Renderer() as ren:
            ren.resize(W, H)
            ren.mesh_upload_parts(v, f, pf)
            ren.mesh_set_part_matrices(table)
            ren.mesh_rebuild_parts()
            ren.render_ray(p, cam, use_bvh=True)                     # the first frame runs on the stream rt_stream() starts as: the next one moves it
            if raster:
                _upload_static(ren)
                ren.raster_mesh_dynamic(SLOT, parts=True, colors=colors)
                ren.render_raster(_draws(), view, proj)              # sizes the raster buffers: the calls below allocate nothing
            ren.synchronize()
            s0 = ren.stream()
            ren.mesh_set_positions(A)
            ren.render_ray(p, cam, use_bvh=True)                     # rt_stream() moves to another lane
            moved = ren.stream() != s0
            ren.mesh_set_part_matrices(T1)
            if raster:
                ren.render_raster_async(_draws(), view, proj)
            ren.mesh_set_positions(B)
            ren.mesh_refit_parts()
            ren.render_ray(p, cam, use_bvh=True)
            frame = ren.read_raster() if raster else None
            return frame, ren.read_target(rt.RT_TARGET_COLOR).copy(), ren.frame_index, moved

    got, ray_a, fi_a, moved = run(True)
    assert moved, "the ray frame did not move rt_stream(): the case does not cross lanes"
    _same_frame(got, want, "state A")
    _, ray_b, fi_b, _ = run(False)
    assert fi_a == fi_b and np.array_equal(ray_a, ray_b)


def test_writes_after_a_lane_change_wait_for_the_raster_call():
    """The other half of the ordering: a raster call of the stand-in, then a ray frame that moves rt_stream() to another lane, then at once new
    positions and matrices on that lane.  The raster frame is the one of the state before them."""
    w, h, k = 160, 96, 40
    v, f = _standin()
    n = f.size // 3
    pf = np.linspace(0, n, k + 1).astype(np.int32)
    T0, T1 = part_models(k), part_models(k, shift=k + 3)
    colors = part_colors(k)
    B = (v * np.float32(0.5)).astype(np.float32)
    want = _reference(v, f, pf, T0, colors, "outside", w=w, h=h)
    assert not np.array_equal(want[1], _reference(B, f, pf, T1, colors, "outside", w=w, h=h)[1])
    view, proj = _view_proj("outside", w, h)
    p = rt.default_render_params()
    p.sppPerFrame = 1
    cam = _camera("outside", w, h)
    with rt.Renderer() as ren:
        ren.resize(w, h)
        _upload_static(ren)
        ren.mesh_upload_parts(v, f, pf)
        ren.mesh_set_part_matrices(T0)
        ren.mesh_rebuild_parts()
        ren.raster_mesh_dynamic(SLOT, parts=True, colors=colors)
        ren.render_ray(p, cam, use_bvh=True)
        ren.render_raster(_draws(), view, proj)                      # sizes the raster buffers
        for _ in range(3):
            s0 = ren.stream()
            ren.render_raster_async(_draws(), view, proj)
            ren.render_ray(p, cam, use_bvh=True)
            assert ren.stream() != s0
            ren.mesh_set_positions(B)
            ren.mesh_set_part_matrices(T1)
            _same_frame(ren.read_raster(), want, "the state before the writes")
            ren.mesh_set_positions(v)
            ren.mesh_set_part_matrices(T0)


# ---------------------------------------------------------------- 6: isolation
@pytest.mark.parametrize("pipeline", [rt.RT_PIPELINE_WAVEFRONT, rt.RT_PIPELINE_MEGAKERNEL])
def test_bound_raster_leaves_the_ray_path_alone(pipeline):
    n, name = 100, "uneven"
    v, f, pf, table, colors, want = _parts_case(n, name, "outside", True)
    view, proj = _view_proj("outside")
    p = rt.default_render_params()
    p.sppPerFrame = 1
    cam = _camera("outside")
    xy = np.stack(np.meshgrid(np.arange(8, W, 12), np.arange(6, H, 10)), -1).reshape(-1, 2).astype(np.int32)
    T1 = part_models(pf.size - 1, shift=pf.size + 2)
    want1 = _reference(v, f, pf, T1, colors, "outside")

    def run(interleave):
        with rt.Renderer(pipeline=pipeline) as ren:
            ren.resize(W, H)
            ren.mesh_upload_parts(v, f, pf)
            ren.mesh_set_part_matrices(table)
            if interleave:
                _upload_static(ren)
                ren.raster_mesh_dynamic(SLOT, parts=True, colors=colors)
                _same_frame(ren.render_raster(_draws(), view, proj), want, "before the first rebuild")      # no tree is needed
            ren.mesh_rebuild_parts()
            out = []
            for step in range(3):
                if interleave:
                    ren.render_raster_async(_draws(), view, proj)
                ren.render_ray(p, cam, use_bvh=True)
                if step == 1:
                    ren.mesh_set_part_matrices(T1)
                    ren.mesh_rebuild_parts()
                else:
                    ren.mesh_refit_parts()
                if interleave:
                    _same_frame(ren.render_raster(_draws(), view, proj), want1 if step >= 1 else want, ("interleaved", step))
                u = rt.frame_uniforms(p, cam, W, H, ren.frame_index, True, ren.n_nodes, ren.n_tris)
                hits = ren.pick(u, xy)
                out.append((ren.read_target(rt.RT_TARGET_COLOR).copy(), ren.frame_index, np.array(hits.record), np.array(hits.object)))
            return out, ren.memory_info()

    a, mem_a = run(False)
    b, mem_b = run(True)
    for (ca, fa, ha, oa), (cb, fb, hb, ob) in zip(a, b):
        assert fa == fb and np.array_equal(ca, cb)
        assert np.array_equal(ha.view(np.uint32), hb.view(np.uint32)) and np.array_equal(oa, ob)
    assert any((h[:, 0] < 1e29).any() for _, _, h, _ in a), "no pick hit the mesh"
    for key in ("queueArenaBytes", "frameArrayBytes", "hybridArenaBytes", "queueArenas", "lanes"):
        assert getattr(mem_a, key) == getattr(mem_b, key)


# ---------------------------------------------------------------- 7: past the bin capacity
def test_past_the_bin_capacity():
    v, f, pf, table, colors, want = _parts_case(100, "uneven", "outside", True)
    view, proj = _view_proj("outside")
    with rt.Renderer() as ren:
        ren.resize(W, H)
        ren.debug_raster_bin_capacity(37)
        _upload_static(ren)
        ren.mesh_upload_parts(v, f, pf)
        ren.mesh_set_part_matrices(table)
        ren.raster_mesh_dynamic(SLOT, parts=True, colors=colors)
        _same_frame(ren.render_raster(_draws(), view, proj), want, "bins of 37 pairs")
        st = ren.raster_stats()
        assert st.binCapacity == 37 and st.binEntries > 37


# ---------------------------------------------------------------- 8: raster_targets
def test_raster_targets():
    v, f, pf, table, colors, want = _parts_case(100, "uneven", "outside", True)
    view, proj = _view_proj("outside")
    with rt.Renderer() as ren:
        with pytest.raises(rt.RtError) as e:
            ren.raster_targets(as_torch=False)
        assert e.value.code == rt.RT_ERR_STATE
        ren.resize(W, H)
        _upload_static(ren)
        ren.mesh_upload_parts(v, f, pf)
        ren.mesh_set_part_matrices(table)
        ren.raster_mesh_dynamic(SLOT, parts=True, colors=colors)
        with pytest.raises(rt.RtError) as e:
            ren.raster_targets(as_torch=False)
        assert e.value.code == rt.RT_ERR_STATE
        ren.render_raster_async(_draws(), view, proj)
        if _have_torch():
            import torch
            rgba, prim, depth = ren.raster_targets(as_torch=True)          # no host wait: torch's stream waits for the library's
            assert rgba.is_cuda and tuple(rgba.shape) == (H, W, 4) and tuple(prim.shape) == (H, W) and rgba.dtype == torch.uint8
            g = (rgba.cpu().numpy(), prim.cpu().numpy().view(np.uint32), depth.cpu().numpy().view(np.uint32))
            _same_frame(g, want, "torch views")
            a, b, c = ren.raster_targets(as_torch=True)
            assert (a.data_ptr(), b.data_ptr(), c.data_ptr()) == (rgba.data_ptr(), prim.data_ptr(), depth.data_ptr())     # views, not copies
        _same_frame(ren.raster_targets(as_torch=False), want, "numpy copies")
        _same_frame(ren.read_raster(), want, "read_raster")
        ren.resize(64, 48)
        for as_torch in ([False, True] if _have_torch() else [False]):
            with pytest.raises(rt.RtError) as e:
                ren.raster_targets(as_torch=as_torch)
            assert e.value.code == rt.RT_ERR_STATE and "render it again" in str(e.value)
        view2, proj2 = _view_proj("outside", 64, 48)
        ren.render_raster_async(_draws(), view2, proj2)
        got = ren.raster_targets(as_torch=False)
        _same_frame(got, _reference(v, f, pf, table, colors, "outside", w=64, h=48), "after resize")


# ---------------------------------------------------------------- 9: lifetime and refusals
def test_lifetime_and_refusals():
    v, f, pf, table, colors, want = _parts_case(100, "uneven", "outside", True)
    k = pf.size - 1
    view, proj = _view_proj("outside")
    with rt.Renderer() as ren:
        ren.resize(W, H)
        _upload_static(ren)
        for bad in (-1, rt.RT_MAX_RASTER_MESHES):
            with pytest.raises(rt.RtError) as e:
                ren.raster_mesh_dynamic(bad)
            assert e.value.code == rt.RT_ERR_INVALID
            with pytest.raises(rt.RtError) as e:
                ren.raster_part_colors(bad, colors)
            assert e.value.code == rt.RT_ERR_INVALID
        assert rt.lib().rt_raster_mesh_dynamic(ren._h, SLOT, 2) == rt.RT_ERR_INVALID
        assert rt.lib().rt_raster_mesh_dynamic(ren._h, SLOT, -1) == rt.RT_ERR_INVALID
        with pytest.raises(rt.RtError) as e:
            ren.raster_part_colors(0, colors)                          # a slot that holds an uploaded mesh
        assert e.value.code == rt.RT_ERR_INVALID
        with pytest.raises(rt.RtError) as e:
            ren.raster_part_colors(5, colors)                          # an empty slot
        assert e.value.code == rt.RT_ERR_INVALID
        ren.raster_mesh_dynamic(5)                                     # bound, but not in parts mode
        with pytest.raises(rt.RtError) as e:
            ren.raster_part_colors(5, colors)
        assert e.value.code == rt.RT_ERR_INVALID and "RT_RASTER_BIND_PARTS" in str(e.value)
        ren.raster_mesh_dynamic(SLOT, parts=True)
        c = np.ascontiguousarray(colors, np.float32)
        assert rt.lib().rt_raster_part_colors(ren._h, SLOT, c.ctypes.data_as(C.POINTER(C.c_float)), -1) == rt.RT_ERR_INVALID
        # no mesh: RT_ERR_STATE
        with pytest.raises(rt.RtError) as e:
            ren.render_raster(_draws(), view, proj)
        assert e.value.code == rt.RT_ERR_STATE and "no mesh" in str(e.value)
        # the mesh arrives after the binding; a bound slot goes through rt_raster_scene_draws like any other
        ren.mesh_upload_parts(v, f, pf)
        ren.mesh_set_part_matrices(table)
        ren.raster_part_colors(SLOT, colors)
        _same_frame(ren.render_raster(_draws(), view, proj), want, "bound before the upload")
        scene = rt.raster_scene_draws(rt.default_render_params(), 0, SLOT, 2)
        ws = rd.render(STATIC, scene, {SLOT: rd.Bound(parts=True, colors=colors)}, (v, f, pf, table), view, proj, W, H)
        _same_frame(ren.render_raster(scene, view, proj), ws, "rt_raster_scene_draws")
        # two slots bound at once, one in each mode, in one call
        both = _draws() + [rt.raster_draw(5, _trs(0.5, (0.5, 0.5, 0.5), (-2.0, 1.0, 0.0)), (1.0, 1.0, 0.0))]
        wb = rd.render(STATIC, both, {SLOT: rd.Bound(parts=True, colors=colors), 5: rd.Bound()}, (v, f, pf, table), view, proj, W, H)
        _same_frame(ren.render_raster(both, view, proj), wb, "two bound slots")
        # a second upload with another triangle count and part count: the same binding draws the new mesh; the stale colour table is refused
        v2, f2 = soup(9)
        pf2 = split("singles", 9)
        ren.mesh_upload_parts(v2, f2, pf2)
        ren.mesh_set_part_matrices(part_models(9))
        kept = ren.read_raster()
        with pytest.raises(rt.RtError) as e:
            ren.render_raster(_draws(), view, proj)
        assert e.value.code == rt.RT_ERR_STATE and "colour table" in str(e.value)
        _same_frame(ren.read_raster(), kept, "the previous frame after a refused call")
        ren.raster_part_colors(SLOT, None)
        w2 = _reference(v2, f2, pf2, part_models(9), None, "outside")
        _same_frame(ren.render_raster(_draws(), view, proj), w2, "second upload")
        # plain mesh_upload is one part: parts mode draws it under draw.model x table[0]
        ren.mesh_upload(v2, f2)
        ren.mesh_set_part_matrices(part_models(1))
        w3 = _reference(v2, f2, np.array([0, 9], np.int32), part_models(1), None, "outside")
        _same_frame(ren.render_raster(_draws(), view, proj), w3, "mesh_upload is one part")
        # upload_bvh releases the mesh
        nodes, tris = scenes.bunny_bvh(2)
        ren.upload_bvh(nodes, tris)
        with pytest.raises(rt.RtError) as e:
            ren.render_raster(_draws(), view, proj)
        assert e.value.code == rt.RT_ERR_STATE
        ren.render_raster([_draws()[0], _draws()[2]], view, proj)      # static draws go on working
        # raster_mesh on a bound slot replaces the binding; None unbinds
        ren.raster_mesh(SLOT, *STATIC[2])
        ren.render_raster(_draws(), view, proj)
        with pytest.raises(rt.RtError) as e:
            ren.raster_part_colors(SLOT, colors)
        assert e.value.code == rt.RT_ERR_INVALID
        ren.raster_mesh_dynamic(SLOT)                                  # binding a slot that holds a mesh frees the mesh
        ren.raster_mesh(SLOT, None)
        ren.mesh_upload(v2, f2)
        with pytest.raises(rt.RtError) as e:
            ren.render_raster(_draws(), view, proj)
        assert e.value.code == rt.RT_ERR_STATE and "empty mesh slot" in str(e.value)
    with rt.Renderer(rank=0, world_size=2) as r:                       # a tile-parallel context refuses the render as before
        r.resize(64, 48)
        r.raster_mesh_dynamic(SLOT)
        with pytest.raises(rt.RtError) as e:
            r.render_raster([rt.raster_draw(SLOT)], np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32))
        assert e.value.code == rt.RT_ERR_UNSUPPORTED and "tile-parallel" in str(e.value)
