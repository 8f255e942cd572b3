"""The previous pose of the dynamic mesh and the object motion of its hits on the device.  Contract: with motion enabled, row i of
mesh_prev_tris() is, byte for byte, the row input triangle mesh_order()[i] had in the triangle array before the most recent update (the new rows after the
mesh's first rebuild and after a latch); mesh_hit_prev_points equals hit_motion (rt_hit_motion, pinned to numpy by tests/test_mesh_motion_host.py) bit for
bit; frames of the mesh's scene write f16(hit_motion(...)) of the pixel's own pick into MOTION on both pipelines and change nothing else; with motion
disabled, or latched, every frame is what it was.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import opengl_raytracing_amd as rt
import scenes
from mesh_fixtures import bones as _bones, placed_turned as _placed_turned, turn as _turn
from test_gpu_dynamic_mesh import _mesh, _model, _ntris
from test_gpu_mesh_refit import _set_qnodes

pytestmark = pytest.mark.gpu

f32 = np.float32
IDENT = np.eye(4, dtype=f32).reshape(-1)
W, H = 64, 48
TARGETS = ("color", "motion", "gpos", "gnrm")


def _dev():
    return torch.device("cuda", 0)


def _same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def _rows(b, n):
    """The current rows of the triangle array (padding dropped) as float32 [n,12]."""
    return b.debug_read_scene("tris").view(f32).reshape(-1, 12)[:n].copy()


def _refused(call, code=rt.RT_ERR_INVALID):
    with pytest.raises(rt.RtError) as e:
        call()
    assert e.value.code == code
    return str(e.value)


# ---------------------------------------------------------------- 1: prevTris replayed on the host
class _Replay:
    """Follows the device through updates from what debug_read_scene("tris") and mesh_order() show before and after each of them."""

    def __init__(self, b, n):
        self.b, self.n, self.tris, self.order, self.reordered = b, n, None, None, 0

    def after(self, what, latched=False):
        b, n = self.b, self.n
        tris, order, prev = _rows(b, n), b.mesh_order(as_torch=False).copy(), b.mesh_prev_tris()
        assert prev.shape == (n, 12), (what, prev.shape)
        if self.tris is None or latched:
            want = tris                                             # the first rebuild has no old rows; a latch copies the current ones
        else:
            row_of = np.empty(n, np.int64)
            row_of[self.order] = np.arange(n)                       # old row of every input triangle
            want = self.tris[row_of[order]]
            self.reordered += int(not np.array_equal(order, self.order))
        assert _same(prev, want), (what, int((prev.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()))
        self.tris, self.order = tris, order


@pytest.mark.parametrize("qnodes", [None, "0", "2"])
@pytest.mark.parametrize("mesh", [1, 9, 63, 65, 257, 1000, "parts"])
def test_prev_tris_replayed_on_the_host(monkeypatch, mesh, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    parts = mesh == "parts"
    v, f = _mesh(300 if parts else mesh)
    v = np.ascontiguousarray(v, f32)
    n = _ntris(f)
    rng = np.random.default_rng(11)
    with rt.Renderer() as b:
        if parts:
            b.mesh_upload_parts(v, f, [0, 100, 220, 300])
            mats = lambda k: np.stack([_turn(k), _turn(k + 2), _turn(-k)])          # noqa: E731
            rebuild = lambda k: (b.mesh_set_part_matrices(mats(k)), b.mesh_rebuild_parts())      # noqa: E731
            refit = lambda k: (b.mesh_set_part_matrices(mats(k)), b.mesh_refit_parts())          # noqa: E731
            update = lambda k, above: (b.mesh_set_part_matrices(mats(k)), b.mesh_update(parts=True, rebuild_above=above))[1]      # noqa: E731
        else:
            b.mesh_upload(v, f)
            rebuild = lambda k: b.mesh_rebuild(_turn(k))                            # noqa: E731
            refit = lambda k: b.mesh_refit(_turn(k))                                # noqa: E731
            update = lambda k, above: b.mesh_update(_turn(k), rebuild_above=above)  # noqa: E731
        assert b.mesh_prev_tris().size == 0                         # not enabled: no array
        b.mesh_motion_enable()                                      # no tree is needed to enable
        assert b.mesh_prev_tris().size == 0                         # ... and there is no scene to read before the first rebuild
        r = _Replay(b, n)
        rebuild(0); r.after("first rebuild")
        refit(1); r.after("refit")
        b.mesh_set_positions((v + rng.normal(0, 0.05, v.shape)).astype(f32))
        refit(1); r.after("refit of moved positions")
        rebuild(3); r.after("rebuild, reordered")
        if n >= 63:
            assert r.reordered == 1, "the rebuild kept every triangle in its row: the case does not reorder"
        b.mesh_motion_latch(); r.after("latch", latched=True)
        actions = []
        b.synchronize()
        actions.append(update(4, 1e9)); r.after("update 1")         # no measured baseline yet: a rebuild
        b.synchronize()
        b.mesh_set_positions((v + rng.normal(0, 1.5, v.shape)).astype(f32))
        actions.append(update(4, 1e9)); r.after("update 2")         # far below the threshold: a refit, of a badly scattered mesh
        b.synchronize()
        actions.append(update(5, 1.0)); r.after("update 3")         # at the threshold: whatever costs more than the baseline is rebuilt
        assert actions[:2] == ["rebuild", "refit"], actions
        if n >= 257:
            assert actions[2] == "rebuild", actions
        b.mesh_motion_enable(False)
        assert b.mesh_prev_tris().size == 0
        b.mesh_motion_enable()                                      # a tree exists: enabling latches
        r.after("enable with a tree", latched=True)


# ---------------------------------------------------------------- the animated mesh of the frame and query tests
@functools.lru_cache(maxsize=None)
def _bend_mesh():
    """The small stand-in (1280 triangles) with two bones blended along x, read only."""
    v, f = rt.meshgen.bunny_standin(3)
    v = np.ascontiguousarray(v, f32)
    f = np.ascontiguousarray(f, np.uint32).reshape(-1)
    x = v[:, 0]
    t = np.clip((x - x.min()) / (x.max() - x.min()) * f32(2.0) - f32(0.5), 0, 1).astype(f32)
    w = np.zeros((v.shape[0], 4), f32)
    w[:, 0], w[:, 1] = f32(1.0) - t, t
    bi = np.zeros((v.shape[0], 4), np.uint16)
    bi[:, 1] = 1
    for a in (v, f, bi, w):
        a.setflags(write=False)
    return v, f, bi, w


def _skin_step(b, k):
    b.mesh_set_bones(_bones(k))
    b.mesh_skin()


def _animated(b, motion):
    v, f, bi, w = _bend_mesh()
    b.upload_env(scenes.tiny_env(8))
    b.resize(W, H)
    b.mesh_upload(v, f)
    b.mesh_skin_upload(bi, w, 2, rest=v)
    if motion:
        b.mesh_motion_enable()
    b.mesh_rebuild(_model("default"))


def _params(spp):
    p = rt.default_render_params()
    p.sppPerFrame = spp
    return p


def _uniforms(spp, frame, moved=True, use_bvh=True, n=None):
    """A frame of the close-up camera.  moved: the previous view-projection is that of a camera a step to the side, so the reference's own motion is
    non-zero and the resolve reprojects; else a static camera."""
    p, cam = _params(spp), scenes.camera("closeup", aspect=W / H)
    L = rt.bvh_layout(n or _ntris(_bend_mesh()[1]))
    prev = None
    if moved:
        before = scenes.camera("closeup", aspect=W / H)
        before.pos[2] += 0.07
        before.yaw -= 0.8
        prev = rt.mat4_mul(rt.camera_proj(before), rt.camera_view(before))
    u = rt.frame_uniforms(p, cam, W, H, frame, use_bvh, L.nNodes, L.nTris, prev_vp=prev)
    assert u.cameraMoved == int(moved)
    return u


def _xy():
    return np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)


def _expected_motion(b, u, tris, prev):
    """(hit mask [H,W], MOTION as halfs [H,W,2]) from the pick of every pixel: f16(hit_motion) at hits, (4, 4) at misses under cameraMoved, else zero."""
    h = b.pick(u, _xy())
    hit = h.prim >= 0
    _, mo = rt.hit_motion(u, tris, prev, h.record, h.point, want=("motion",))
    want = np.where(hit[:, None], mo, f32(4.0) if u.cameraMoved == 1 else f32(0.0)).astype(np.float16)
    return hit.reshape(H, W), want.view(np.uint16).reshape(H, W, 2)


# ---------------------------------------------------------------- 2: the device query
def test_hit_prev_points_equal_the_host_definition():
    v, f, _, _ = _bend_mesh()
    n = _ntris(f)
    rng = np.random.default_rng(3)
    with rt.Renderer() as b:
        _animated(b, True)
        _skin_step(b, 2)
        b.mesh_refit(_model("default"))
        tris, prev = _rows(b, n), b.mesh_prev_tris()
        assert not _same(tris, prev)
        u = _uniforms(1, 0)
        # pixels, misses included: host arrays and device tensors
        h = b.pick(u, _xy())
        assert (h.prim >= 0).sum() >= 200 and (h.prim < 0).sum() >= 200
        want, _ = rt.hit_motion(None, tris, prev, h.record, h.point, want=("prev",))
        got = b.mesh_hit_prev_points(h, h.point)
        assert _same(got, want) and not _same(got[h.prim >= 0], h.point[h.prim >= 0]) and (got[h.prim < 0].view(np.uint32) == 0).all()
        ht = b.pick(u, torch.from_numpy(_xy()).to(_dev()))
        got_t = b.mesh_hit_prev_points(ht, ht.point)
        torch.cuda.synchronize()
        assert _same(ht.record.cpu().numpy(), h.record) and _same(got_t.cpu().numpy(), want)
        # rays: 1, 63, 64, 65 and 2049 of them, aimed at triangles from all around (some miss); points = origin + dir * t
        k = rng.integers(0, n, 2049)
        target = (tris[k, 0:3] + (tris[k, 4:7] + tris[k, 8:11]) / 3).astype(f32)
        org = (target + rng.normal(0, 1, target.shape) * 2).astype(f32)
        dirs = target - org
        dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(f32)
        dirs[::7] = -dirs[::7]                                      # ... and some of them the other way
        for m in (1, 63, 64, 65, 2049):
            r = b.trace_rays(org[:m], dirs[:m])
            with np.errstate(all="ignore"):
                pts = (org[:m] + (dirs[:m] * r.t[:, None]).astype(f32)).astype(f32)
            want, _ = rt.hit_motion(None, tris, prev, r.record, pts, want=("prev",))
            assert _same(b.mesh_hit_prev_points(r, pts), want), m
            rt_ = b.trace_rays(torch.from_numpy(org[:m]).to(_dev()), torch.from_numpy(dirs[:m]).to(_dev()))
            got_t = b.mesh_hit_prev_points(rt_.record, torch.from_numpy(pts).to(_dev()))
            torch.cuda.synchronize()
            assert _same(got_t.cpu().numpy(), want), m
        assert (r.prim >= 0).sum() > 500 and (r.prim < 0).sum() > 50
        # stale records: prims outside the mesh answer zeros
        rec = h.record.copy()
        rec[:4, 1] = np.array([n, 2 ** 31 - 1, -2, -2 ** 31], np.int32).view(f32)
        assert (b.mesh_hit_prev_points(rec, h.point)[:4].view(np.uint32) == 0).all()
        assert b.mesh_hit_prev_points(rec[:0], h.point[:0]).shape == (0, 3)
        b.mesh_motion_latch()                                       # latched: every hit point stays where it is
        got = b.mesh_hit_prev_points(h, h.point)
        assert _same(got[h.prim >= 0], h.point[h.prim >= 0])


# ---------------------------------------------------------------- 3: frames
@functools.lru_cache(maxsize=None)
def _frame_run(pipeline, spp, motion):
    """The stages of the frame test on one context -> {stage: targets, ...}; with motion also {stage + "/want": (hit mask, expected MOTION)}."""
    n = _ntris(_bend_mesh()[1])
    out = {}
    with rt.Renderer(pipeline=pipeline) as b:
        _animated(b, motion)
        u = _uniforms(spp, 0)

        def frame(stage, uu=u):
            b.reset_accum()
            b.render_frame(uu)
            out[stage] = b.read_all()
            if motion and uu.useBVH == 1:
                out[stage + "/want"] = _expected_motion(b, uu, _rows(b, n), b.mesh_prev_tris())

        frame("latched")                                            # after the first rebuild: previous pose == current pose
        _skin_step(b, 2)
        b.mesh_refit(_model("default"))
        frame("refit")
        frame("hybrid", _uniforms(spp, 0, use_bvh=rt.RT_SCENE_HYBRID))
        _skin_step(b, 3)
        b.mesh_rebuild(_placed_turned())                            # turned where it stands: the rows are reordered and the mesh moves a long way
        out["order"] = b.mesh_order(as_torch=False).copy()
        frame("rebuild")
        if motion:
            b.mesh_motion_latch()
        frame("latched again")
    return out


@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("pipeline", [rt.RT_PIPELINE_WAVEFRONT, rt.RT_PIPELINE_MEGAKERNEL])
def test_frames(pipeline, spp):
    on, off = _frame_run(pipeline, spp, True), _frame_run(pipeline, spp, False)
    for stage in ("latched", "latched again", "hybrid"):           # latched, and the hybrid scene: all four targets are the motion-off frame's
        for name, x, y in zip(TARGETS, on[stage], off[stage]):
            assert _same(x, y), (stage, name)
    for stage in ("latched", "refit", "rebuild", "latched again"):
        hit, want = on[stage + "/want"]
        motion = on[stage][1]
        assert hit.sum() >= 200 and (~hit).sum() >= 200, stage
        assert _same(motion[hit], want[hit]), (stage, int((motion[hit] != want[hit]).any(axis=1).sum()))
        assert (motion[~hit] == np.float16(4.0).view(np.uint16)).all(), stage
        assert _same(on[stage][2], off[stage][2]) and _same(on[stage][3], off[stage][3]), stage      # GPOS and GNRM do not change
        assert ((on[stage][2][..., 3] != 0) == hit).all(), stage
    for stage in ("refit", "rebuild"):                             # the mesh did move: object motion differs from the reference's
        hit, _ = on[stage + "/want"]
        assert (on[stage][1][hit] != off[stage][1][hit]).any(axis=1).sum() >= 100, stage
    first = _frame_run(rt.RT_PIPELINE_WAVEFRONT, spp, True)["order"]
    assert not np.array_equal(first, np.arange(first.size))


@pytest.mark.parametrize("spp", [1, 2])
def test_wavefront_equals_megakernel(spp):
    wave, mega = _frame_run(rt.RT_PIPELINE_WAVEFRONT, spp, True), _frame_run(rt.RT_PIPELINE_MEGAKERNEL, spp, True)
    for stage in ("latched", "refit", "hybrid", "rebuild", "latched again"):
        for name, x, y in zip(TARGETS, wave[stage], mega[stage]):
            assert _same(x, y), (stage, name)


# ---------------------------------------------------------------- 4: a batch of static-camera frames
@pytest.mark.parametrize("spp", [1, 2])
def test_render_frames_equals_single_calls(spp):
    n = _ntris(_bend_mesh()[1])
    with rt.Renderer() as b:
        _animated(b, True)
        _skin_step(b, 2)
        b.mesh_refit(_model("default"))
        us = [_uniforms(spp, k, moved=False) for k in range(4)]
        prev0 = b.mesh_prev_tris()
        b.reset_accum()
        for u in us:
            b.render_frame(u)
        single = b.read_all()
        b.reset_accum()
        b.render_frames(us)
        batch = b.read_all()
        for name, x, y in zip(TARGETS, batch, single):
            assert _same(x, y), name
        hit, want = _expected_motion(b, us[3], _rows(b, n), b.mesh_prev_tris())
        assert _same(batch[1][hit], want[hit]) and (batch[1][~hit] == 0).all()
        assert (batch[1][hit] != 0).any(axis=1).sum() >= 100       # a static camera, a moving mesh: MOTION is the object's
        assert _same(b.mesh_prev_tris(), prev0) and not _same(_rows(b, n), prev0)      # frames change no mesh state


# ---------------------------------------------------------------- 5: ordering across lanes
def test_call_order_holds_across_lanes(monkeypatch):
    """update, frame, latch, frame, update, frame -- each call on whatever lane stream() has reached, without a host synchronise, and behind every frame
    the previous points of its pixels asked for on the device; everything equals a run that synchronises after every call."""
    _set_qnodes(monkeypatch, "0")                                  # no quantised form: the updates have no host wait of their own
    n = _ntris(_bend_mesh()[1])
    xy = torch.from_numpy(_xy()).to(_dev())
    torch.cuda.synchronize()

    def run(sync):
        with rt.Renderer() as b:
            _animated(b, True)
            b.synchronize()
            wait = b.synchronize if sync else (lambda: None)
            asked, streams = [], set()

            def frame(k):
                u = _uniforms(1, k)
                b.render_frame(u); wait()
                streams.add(b.stream())
                h = b.pick(u, xy); wait()
                asked.append((h.record, b.mesh_hit_prev_points(h, h.point))); wait()

            _skin_step(b, 2); wait()
            b.mesh_refit(_model("default")); wait()
            frame(0)
            b.mesh_motion_latch(); wait()
            frame(1)
            _skin_step(b, 4); wait()
            b.mesh_refit(_model("default")); wait()
            frame(2)
            assert b.mesh_info().hostSyncs == 0
            b.synchronize()
            return b.read_all(), b.mesh_prev_tris(), _rows(b, n), [(r.cpu().numpy().copy(), p.cpu().numpy().copy()) for r, p in asked], streams

    targets_s, prev_s, tris_s, asked_s, _ = run(True)
    targets_a, prev_a, tris_a, asked_a, streams = run(False)
    assert len(streams) > 1, "the frames did not move stream(): the case does not cross lanes"
    for name, x, y in zip(TARGETS, targets_a, targets_s):
        assert _same(x, y), name
    assert _same(prev_a, prev_s) and _same(tris_a, tris_s) and not _same(prev_s, tris_s)
    for k, ((ra, pa), (rs, ps)) in enumerate(zip(asked_a, asked_s)):
        assert _same(ra, rs) and _same(pa, ps), k
    hit = asked_s[1][0][:, 1].copy().view(np.int32) >= 0
    pts = lambda k: asked_s[k][1][hit]                              # noqa: E731
    assert not _same(pts(0), pts(1)) and not _same(pts(1), pts(2))  # moved, latched, moved again: the three frames saw three previous poses


# ---------------------------------------------------------------- 6: render_ray keeps the frame state itself
def test_render_ray_latches_behind_the_moved_frame():
    n = _ntris(_bend_mesh()[1])
    p, cam = _params(1), scenes.camera("closeup", aspect=W / H)
    view = rt.camera_view(cam)
    vp = rt.mat4_mul(rt.camera_proj(cam), view)
    L = rt.bvh_layout(n)

    def uniforms(frame, moved):
        return rt.make_uniforms(p, cam, view, vp, vp, W, H, frame, moved, True, False, L.nNodes, L.nTris, True)

    def sequence(motion, frames=False):
        out = []
        with rt.Renderer() as b:
            _animated(b, motion)
            b.render_ray(p, cam, use_bvh=True)                     # frame 0, behind the first rebuild
            out.append((b.read_all(), None))
            _skin_step(b, 2)
            b.mesh_refit(_model("default"))
            tris, prev = _rows(b, n), b.mesh_prev_tris()
            if frames:
                b.render_ray_frames(p, cam, 3, use_bvh=True)       # frames 1 - 3 in one call: the first moved, the rest batched
                out.append((b.read_all(), None))
                return out, b.mesh_prev_tris(), tris
            b.render_ray(p, cam, use_bvh=True)                     # frame 1: after an update
            out.append((b.read_all(), _expected_motion(b, uniforms(1, True), tris, prev) if motion else None))
            latched = b.mesh_prev_tris()
            b.render_ray(p, cam, use_bvh=True)                     # frame 2: nothing moved
            out.append((b.read_all(), None))
            return out, latched, tris

    on, latched, tris = sequence(True)
    assert _same(latched, tris)                                    # the call latched behind frame 1
    hit, want = on[1][1]
    motion1 = on[1][0][1]
    assert hit.sum() >= 200 and _same(motion1[hit], want[hit]) and (motion1[hit] != 0).any(axis=1).sum() >= 100      # rendered as moved, object motion
    assert (motion1[~hit] == np.float16(4.0).view(np.uint16)).all()
    assert (on[2][0][1] == 0).all()                                # frame 2: a static camera's motion, the reference's
    # with motion disabled the sequence is the uniform-level one of a static camera
    off, _, _ = sequence(False)
    with rt.Renderer() as b:
        _animated(b, False)
        b.render_frame(uniforms(0, False))
        assert all(_same(x, y) for x, y in zip(b.read_all(), off[0][0]))
        _skin_step(b, 2)
        b.mesh_refit(_model("default"))
        for k in (1, 2):
            b.render_frame(uniforms(k, False))
            assert all(_same(x, y) for x, y in zip(b.read_all(), off[k][0])), k
    # rt_render_ray_frames: the first frame moved and latched, the others behind it -- the targets of three single calls
    three, latched3, tris3 = sequence(True, frames=True)
    assert _same(latched3, tris3)
    with rt.Renderer() as b:
        _animated(b, True)
        b.render_ray(p, cam, use_bvh=True)
        _skin_step(b, 2)
        b.mesh_refit(_model("default"))
        for _ in range(3):
            b.render_ray(p, cam, use_bvh=True)
        assert all(_same(x, y) for x, y in zip(b.read_all(), three[1][0]))


# ---------------------------------------------------------------- 7: counters
@pytest.mark.parametrize("qnodes", ["0", "2"])
def test_no_allocation_no_host_wait(monkeypatch, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    v, f, bi, w = _bend_mesh()
    n = _ntris(f)
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_skin_upload(bi, w, 2, rest=v)
        before = b.mesh_info()
        b.mesh_motion_enable()
        mi0 = b.mesh_info()
        assert mi0.allocations == before.allocations + 2           # the previous rows and the old rows by input triangle
        assert mi0.scratchBytes == before.scratchBytes + 2 * n * 48 and mi0.hostSyncs == 0
        for k in range(20):
            _skin_step(b, k)
            b.mesh_update(rebuild_above=1.0 if k % 3 == 0 else 1.5)
            assert b.mesh_info().hostSyncs == (0 if qnodes == "0" else k + 1)      # the quantised form's status read alone
            b.mesh_motion_latch()
            mi = b.mesh_info()
            assert mi.allocations == mi0.allocations and mi.hostSyncs == (0 if qnodes == "0" else k + 1)
        assert _same(b.mesh_prev_tris(), _rows(b, n))
        b.mesh_motion_enable(False)                                # released: the bytes are given back
        assert b.mesh_info().scratchBytes == before.scratchBytes


# ---------------------------------------------------------------- 8: state and refusals
def test_state_and_refusals():
    v, f, _, _ = _bend_mesh()
    rec, pts = np.zeros((4, 4), f32), np.zeros((4, 3), f32)

    def calls(b):
        return {"mesh_motion_latch": b.mesh_motion_latch, "mesh_hit_prev_points": lambda: b.mesh_hit_prev_points(rec, pts),
                "mesh_hit_prev_points (device)": lambda: b.mesh_hit_prev_points(torch.from_numpy(rec).to(_dev()), torch.from_numpy(pts).to(_dev()))}

    with rt.Renderer() as b:
        assert "no mesh" in _refused(b.mesh_motion_enable)         # no mesh
        for name, call in calls(b).items():
            _refused(call)
        b.mesh_upload(v, f)
        for name, call in calls(b).items():                        # a mesh, motion not enabled, no tree
            _refused(call)
        b.mesh_rebuild()
        for name, call in calls(b).items():                        # a tree, motion not enabled
            assert "rt_mesh_motion_enable" in _refused(call), name
        assert b.mesh_prev_tris().size == 0
        b.mesh_upload(v, f)
        b.mesh_motion_enable()
        for name, call in calls(b).items():                        # enabled, before the first rebuild
            assert "rebuild" in _refused(call), name
        b.mesh_rebuild()
        for name, call in calls(b).items():
            call()
        _refused(lambda: b.mesh_hit_prev_points(rec, pts[:3]))     # as many points as hits
        _refused(lambda: b.mesh_hit_prev_points(rec.astype(np.float64), pts))
        b.mesh_motion_enable(False)                                # released on request ...
        for name, call in calls(b).items():
            _refused(call)
        b.mesh_motion_enable()
        b.mesh_upload(v, f)                                        # ... with the mesh by mesh_upload ...
        b.mesh_rebuild()
        for name, call in calls(b).items():
            assert "rt_mesh_motion_enable" in _refused(call), name
        b.mesh_motion_enable()
        nodes, tris12 = rt.build_bvh(rt.gather_triangles(v, f, IDENT))
        b.upload_bvh(nodes, tris12)                                # ... and by upload_bvh
        assert "no mesh" in _refused(b.mesh_motion_enable)
        for name, call in calls(b).items():
            _refused(call)
        assert b.debug_read_scene(rt.RT_SCENE_ARRAY_PREV_TRIS).size == 0 and b.scene_info().nTris == _ntris(f)
