"""Per-vertex colours of the dynamic mesh on the device.  Contract: with colours enabled, debug_read_scene("color rows") is, bit for
bit, what color_rows (rt_color_rows, pinned to numpy by tests/test_mesh_colors_host.py) makes of mesh_order(), the indices and mesh_colors(), behind
every kind of update and behind mesh_colors_refresh; mesh_hit_colors equals hit_colors bit for bit; frames of the mesh's scene shade the primary and the
bounce hit with those colours on both pipelines while GPOS, GNRM and MOTION stay; a mesh whose colours are all 0.85 -- the constant the colours replace --
renders the disabled frame on all four targets, a channel pinned to 0.85 renders the disabled frame's channel, and a red ceiling takes green and blue
out of the floor under it; with colours disabled every frame is what it was.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import opengl_raytracing_amd as rt
import scenes
from mesh_fixtures import random_colors as _random_colors
from test_gpu_dynamic_mesh import _mesh, _model, _ntris
from test_gpu_mesh_motion import H, TARGETS, W, _dev, _placed_turned, _refused, _rows, _same, _skin_step, _turn, _xy
from test_gpu_mesh_normals import _flat, _sphere, _two_bone_skin
from test_gpu_mesh_refit import _set_qnodes

pytestmark = pytest.mark.gpu

f32 = np.float32
IDENT = np.eye(4, dtype=f32).reshape(-1)
GREY = f32(0.85)
PIPELINES = [rt.RT_PIPELINE_WAVEFRONT, rt.RT_PIPELINE_MEGAKERNEL]


def _device_colors(b):
    """mesh_colors() as float32 [V,4], read after everything enqueued."""
    t = b.mesh_colors()
    b.synchronize()
    return t.cpu().numpy().copy()


def _check_rows(b, f, what):
    order = b.mesh_order(as_torch=False).copy()
    colors = _device_colors(b)
    rows = b.debug_read_scene("color rows").view(f32).reshape(-1, 12)
    want = rt.color_rows(order, f, colors)
    assert rows.shape == (_ntris(f), 12) and _same(rows, want), (what, int((rows.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()))
    assert _same(rows, b.mesh_color_rows())
    return order, rows


# ---------------------------------------------------------------- 1: the rows replayed on the host behind every kind of update
@pytest.mark.parametrize("qnodes", [None, "0", "2"])
@pytest.mark.parametrize("mesh", [1, 9, 63, 65, 257, 1000, "parts"])
def test_rows_equal_the_host_definition(monkeypatch, mesh, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    parts = mesh == "parts"
    v, f = _mesh(300 if parts else mesh)
    v, f = np.ascontiguousarray(v, f32), np.ascontiguousarray(f, np.uint32).reshape(-1)
    n, nv = _ntris(f), v.shape[0]
    bi, w = _two_bone_skin(v)
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
        b.mesh_skin_upload(bi, w, 2, rest=v)
        assert b.debug_read_scene("color rows").size == 0           # not enabled: no array
        b.mesh_colors_enable()                                      # no tree is needed to enable
        assert b.debug_read_scene("color rows").size == 0           # ... and there is no scene to read before the first rebuild
        got = _device_colors(b)
        assert got.shape == (nv, 4) and _same(got, np.tile(np.array([GREY, GREY, GREY, 0], f32), (nv, 1)))
        if parts:
            b.mesh_set_colors(rt.vertex_colors_from_parts(f, [0, 100, 220, 300], [[0.9, 0.1, 0.1], [0.1, 0.8, 0.2], [0.2, 0.3, 0.95]], nv))
        else:
            b.mesh_set_colors(_random_colors(nv, 1))
        rebuild(0); first, rows0 = _check_rows(b, f, "first rebuild")
        assert not _same(rows0, rt.color_rows(first, f, np.full((nv, 3), GREY, f32)))
        refit(1); _check_rows(b, f, "refit")
        b.mesh_set_colors(_random_colors(nv, 2))
        assert _same(b.mesh_color_rows(), rows0)                    # writing colours alone leaves the rows as they were
        b.mesh_colors_refresh()
        _, rows1 = _check_rows(b, f, "set colours, refresh")
        assert not _same(rows1, rows0)                              # ... the refresh moves them, with no update
        b.mesh_set_colors(_random_colors(max(nv // 2, 1), 3), first=nv - max(nv // 2, 1))       # a range that ends at the last vertex
        _skin_step(b, 3)
        refit(1); _check_rows(b, f, "skin step, refit")
        rebuild(3); order, _ = _check_rows(b, f, "rebuild, reordered")
        if n >= 63:
            assert not np.array_equal(order, first), "the rebuild kept every triangle in its row: the case does not reorder"
        actions = []
        b.synchronize()
        actions.append(update(4, 1e9)); _check_rows(b, f, "update 1")                # no measured baseline yet: a rebuild
        b.synchronize()
        b.mesh_set_positions((v + np.random.default_rng(11).normal(0, 1.5, v.shape)).astype(f32))
        t = b.mesh_colors()                                         # the caller's own write, on stream()'s stream
        with torch.cuda.stream(torch.cuda.ExternalStream(b.stream(), device=_dev())):
            t[:, :3] = torch.from_numpy(_random_colors(nv, 4)).to(_dev())
        actions.append(update(4, 1e9)); _check_rows(b, f, "update 2")                # far below the threshold: a refit
        b.synchronize()
        actions.append(update(5, 1.0)); _check_rows(b, f, "update 3")                # at the threshold
        assert actions[:2] == ["rebuild", "refit"] and actions[2] in ("rebuild", "refit"), actions   # the third: whichever the measured costs say
        # ... and the rebuild side of mesh_update right behind a refit, whatever the costs: a tree of an explicit rebuild has no measured baseline
        rebuild(6)
        refit(7)
        b.mesh_set_colors(_random_colors(nv, 6))
        assert update(8, 1e9) == "rebuild"
        _check_rows(b, f, "update 4: a rebuild behind a refit")
        b.mesh_colors_enable(False)
        assert b.debug_read_scene("color rows").size == 0
        b.mesh_colors_enable()                                      # a tree exists: enabling fills the rows at once, with the initial colour
        _, rows = _check_rows(b, f, "enable with a tree")
        assert _same(rows, np.tile(np.array([GREY, GREY, GREY, 0], f32), (n, 3)))
        b.mesh_set_colors(_random_colors(nv, 5))
        b.mesh_colors_refresh()
        before, _, rows5 = b.mesh_info().allocations, *_check_rows(b, f, "colours set again")
        b.mesh_colors_enable()                                      # already enabled: colours and rows stay, nothing is allocated
        assert b.mesh_info().allocations == before and _same(_check_rows(b, f, "enable while enabled")[1], rows5) and not _same(rows5, rows)


# ---------------------------------------------------------------- the scenes of the frame and query tests
def _uniforms(spp, frame, n, moved=True, use_bvh=True, gi=1, ao=1, taa=1):
    p, cam = rt.default_render_params(), scenes.camera("closeup", aspect=W / H)
    p.sppPerFrame, p.enableGI, p.enableAO, p.enableTAA = spp, gi, ao, taa
    L = rt.bvh_layout(n)
    prev = None
    if moved:
        before = scenes.camera("closeup", aspect=W / H)
        before.pos[2] += 0.07
        before.yaw -= 0.8
        prev = rt.mat4_mul(rt.camera_proj(before), rt.camera_view(before))
    u = rt.frame_uniforms(p, cam, W, H, frame, use_bvh, L.nNodes, L.nTris, prev_vp=prev)
    assert u.cameraMoved == int(moved) and u.enableGI == gi and u.enableAO == ao
    return u


def _animated(b, colors=None, normals=False, motion=False):
    """The skinned icosphere in front of the close-up camera; colors: None = never enabled, else [V,3]."""
    v, f, bi, w = _sphere()
    b.upload_env(scenes.tiny_env(8))
    b.resize(W, H)
    b.mesh_upload(v, f)
    b.mesh_skin_upload(bi, w, 2, rest=v)
    if colors is not None:
        b.mesh_colors_enable()
        b.mesh_set_colors(colors)
    if normals:
        b.mesh_normals_enable()
    if motion:
        b.mesh_motion_enable()
    b.mesh_rebuild(_model("default"))


def _flat_scene(b, colors=None):
    """The floor and the ceiling of the flat anchor (tests/test_gpu_mesh_normals.py): bounce and AO rays from one meet the other."""
    v, f = _flat()
    b.upload_env(scenes.tiny_env(8))
    b.resize(W, H)
    b.mesh_upload(v, f)
    if colors is not None:
        b.mesh_colors_enable()
        if not isinstance(colors, str):
            b.mesh_set_colors(colors)
    b.mesh_rebuild(IDENT)


def _frame(b, u):
    b.reset_accum()
    b.render_frame(u)
    return b.read_all()


# ---------------------------------------------------------------- 2: the device query
def test_hit_colors_equal_the_host_definition():
    v, f, _, _ = _sphere()
    n, nv = _ntris(f), v.shape[0]
    rng = np.random.default_rng(3)
    with rt.Renderer() as b:
        _animated(b, _random_colors(nv, 5))
        _skin_step(b, 2)
        b.mesh_refit(_model("default"))
        tris, order, colors = _rows(b, n), b.mesh_order(as_torch=False).copy(), _device_colors(b)
        u = _uniforms(1, 0, n)
        h = b.pick(u, _xy())                                        # pixels, misses included: host arrays and device tensors
        hit = h.prim >= 0
        assert hit.sum() >= 200 and (~hit).sum() >= 200
        want = rt.hit_colors(tris, order, f, colors, h.record)
        got = b.mesh_hit_colors(h)
        assert _same(got, want) and (got[~hit].view(np.uint32) == 0).all() and (got[hit] > 0).all()
        ht = b.pick(u, torch.from_numpy(_xy()).to(_dev()))
        got_t = b.mesh_hit_colors(ht)
        torch.cuda.synchronize()
        assert _same(ht.record.cpu().numpy(), h.record) and _same(got_t.cpu().numpy(), want)
        k = rng.integers(0, n, 2049)                                # rays: 1, 63, 64, 65 and 2049 of them, aimed at triangles from all around
        target = (tris[k, 0:3] + (tris[k, 4:7] + tris[k, 8:11]) / 3).astype(f32)
        org = (target + rng.normal(0, 1, target.shape) * 2).astype(f32)
        dirs = target - org
        dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(f32)
        dirs[::7] = -dirs[::7]                                      # ... and some of them the other way
        for m in (1, 63, 64, 65, 2049):
            r = b.trace_rays(org[:m], dirs[:m])
            want = rt.hit_colors(tris, order, f, colors, r.record)
            assert _same(b.mesh_hit_colors(r), want), m
            rt_ = b.trace_rays(torch.from_numpy(org[:m]).to(_dev()), torch.from_numpy(dirs[:m]).to(_dev()))
            got_t = b.mesh_hit_colors(rt_.record)
            torch.cuda.synchronize()
            assert _same(got_t.cpu().numpy(), want), m
        assert (r.prim >= 0).sum() > 500 and (r.prim < 0).sum() > 50
        rec = h.record.copy()                                       # stale records: prims outside the mesh answer zeros
        rec[:4, 1] = np.array([n, 2 ** 31 - 1, -2, -2 ** 31], np.int32).view(f32)
        assert (b.mesh_hit_colors(rec)[:4].view(np.uint32) == 0).all()
        got_t = b.mesh_hit_colors(torch.from_numpy(rec).to(_dev()))
        torch.cuda.synchronize()
        assert _same(got_t.cpu().numpy(), rt.hit_colors(tris, order, f, colors, rec))
        assert b.mesh_hit_colors(rec[:0]).shape == (0, 3)


# ---------------------------------------------------------------- 3: the grey anchor
@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_grey_anchor_frames_are_the_disabled_frames(pipeline, spp):
    """0.85 at every vertex is the constant the colours replace: the enabled frame is the disabled frame on all four targets, COLOR0 included, with GI and
    AO on -- every substitution site, tied to the oracle-pinned path without an oracle."""
    v, f = _flat()
    n, nv = _ntris(f), v.shape[0]
    u = _uniforms(spp, 0, n)

    def run(mode):
        with rt.Renderer(pipeline=pipeline) as b:
            _flat_scene(b, None if mode == "off" else "initial")
            if mode == "set":
                b.mesh_set_colors(np.full((nv, 3), GREY, f32))
                b.mesh_colors_refresh()
            if mode == "on-off":
                b.mesh_set_colors(_random_colors(nv, 9))
                b.mesh_colors_refresh()
                b.mesh_colors_enable(False)
            t = _frame(b, u)
            h = b.pick(u, _xy())
            return t, h

    off, h = run("off")
    hit = h.prim >= 0
    assert hit.sum() >= 200 and (~hit).sum() >= 200
    lit = off[0].reshape(-1, off[0].shape[-1])[hit]
    assert (lit[:, :3] != 0).any()
    for mode in ("initial", "set", "on-off"):
        got, _ = run(mode)
        for name, x, y in zip(TARGETS, got, off):
            assert _same(x, y), (mode, name)


# ---------------------------------------------------------------- 4: the channel anchor
@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_channel_anchor(pipeline, spp):
    """A first frame (no history), GI off (its luminance clamp couples channels), AO on: with one channel 0.85 at every vertex and the other two random,
    that channel of COLOR0 is the disabled frame's at every pixel."""
    v, f = _flat()
    n, nv = _ntris(f), v.shape[0]
    u = _uniforms(spp, 0, n, gi=0)

    def run(colors):
        with rt.Renderer(pipeline=pipeline) as b:
            _flat_scene(b, colors)
            return _frame(b, u)

    off = run(None)
    for ch in range(3):
        c = _random_colors(nv, 20 + ch)
        c[:, ch] = GREY
        got = run(c)
        assert _same(got[0][..., ch], off[0][..., ch]), ch
        others = [k for k in range(3) if k != ch]
        assert all(not _same(got[0][..., k], off[0][..., k]) for k in others), ch
        for name, x, y in list(zip(TARGETS, got, off))[1:]:
            assert _same(x, y), (ch, name)


# ---------------------------------------------------------------- 5: bleed
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_a_red_ceiling_takes_green_and_blue_out_of_the_floor(pipeline):
    v, f = _flat()
    n, nv = _ntris(f), v.shape[0]
    u = _uniforms(2, 0, n)
    colors = np.full((nv, 3), GREY, f32)
    colors[nv // 2:] = [GREY, 0, 0]                                 # the ceiling's vertices

    def run(c):
        with rt.Renderer(pipeline=pipeline) as b:
            _flat_scene(b, c)
            t = _frame(b, u)
            h = b.pick(u, _xy())
            return t, h, _rows(b, n)

    (on, h, tris), (off, _, _) = run(colors), run(None)
    hit = h.prim >= 0
    floor = np.zeros(hit.shape, bool)
    floor[hit] = tris[h.prim[hit], 1] == 1
    ceiling = hit & ~floor
    assert floor.sum() >= 100 and ceiling.sum() >= 100
    c_on, c_off = on[0].reshape(-1, on[0].shape[-1]).astype(np.float64), off[0].reshape(-1, off[0].shape[-1]).astype(np.float64)
    for ch in (1, 2):
        assert (c_on[floor, ch] <= c_off[floor, ch]).all(), ch     # the floor's own albedo is the constant: only the bounce changed
        assert (c_on[floor, ch] < c_off[floor, ch]).any(), ch
    assert (c_on[ceiling, 1:3] != c_off[ceiling, 1:3]).any(axis=1).sum() >= 100        # the ceiling's own pixels differ


# ---------------------------------------------------------------- 6: pipelines
@functools.lru_cache(maxsize=None)
def _frame_run(pipeline, spp, colored, normals):
    """Stages on one context with GI and AO on and motion enabled -> {stage: targets}."""
    v, f, _, _ = _sphere()
    n, nv = _ntris(f), v.shape[0]
    out = {}
    with rt.Renderer(pipeline=pipeline) as b:
        _animated(b, _random_colors(nv, 6) if colored else None, normals=normals, motion=True)
        out["rest"] = _frame(b, _uniforms(spp, 0, n))
        _skin_step(b, 2)
        b.mesh_refit(_model("default"))
        out["refit"] = _frame(b, _uniforms(spp, 0, n))
        out["hybrid"] = _frame(b, _uniforms(spp, 0, n, use_bvh=rt.RT_SCENE_HYBRID))
        out["analytic"] = _frame(b, _uniforms(spp, 0, n, use_bvh=False))
        _skin_step(b, 3)
        b.mesh_rebuild(_placed_turned())                            # turned where it stands: the rows are reordered
        out["rebuild"] = _frame(b, _uniforms(spp, 0, n))
        if colored:
            out["picked"] = b.mesh_hit_colors(b.pick(_uniforms(spp, 0, n), _xy()))
    return out


STAGES = ("rest", "refit", "rebuild")


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("spp", [1, 2])
def test_wavefront_equals_megakernel_and_only_color_changes(spp, normals):
    wave, mega = _frame_run(PIPELINES[0], spp, True, normals), _frame_run(PIPELINES[1], spp, True, normals)
    off = _frame_run(PIPELINES[0], spp, False, normals)
    for stage in STAGES + ("hybrid", "analytic"):
        for name, x, y in zip(TARGETS, wave[stage], mega[stage]):
            assert _same(x, y), (stage, name)
    for stage in STAGES:
        assert not _same(wave[stage][0], off[stage][0]), stage      # the shading follows the colours ...
        for name, x, y in list(zip(TARGETS, wave[stage], off[stage]))[1:]:
            assert _same(x, y), (stage, name)                       # ... MOTION, GPOS and GNRM do not
    for stage in ("hybrid", "analytic"):                            # the hybrid and the analytic scene are unchanged
        for name, x, y in zip(TARGETS, wave[stage], off[stage]):
            assert _same(x, y), (stage, name)
    assert (wave["picked"] > 0).all(axis=1).sum() >= 200


@pytest.mark.parametrize("spp", [1, 2])
def test_render_frames_equals_single_calls(spp):
    v, f, _, _ = _sphere()
    n, nv = _ntris(f), v.shape[0]
    with rt.Renderer() as b:
        _animated(b, _random_colors(nv, 7))
        _skin_step(b, 2)
        b.mesh_refit(_model("default"))
        us = [_uniforms(spp, k, n, moved=False) for k in range(4)]
        rows0 = b.mesh_color_rows()
        b.reset_accum()
        for u in us:
            b.render_frame(u)
        single = b.read_all()
        b.reset_accum()
        b.render_frames(us)
        batch = b.read_all()
        for name, x, y in zip(TARGETS, batch, single):
            assert _same(x, y), name
        assert _same(b.mesh_color_rows(), rows0)                    # frames change no mesh state


# ---------------------------------------------------------------- 7: ordering across lanes
def test_call_order_holds_across_lanes(monkeypatch):
    """set_colors, refresh, frame, update, frame -- each call on whatever lane stream() has reached, without a host synchronise, and behind every frame a
    pick and the colours of its pixels asked for on the device; everything equals a run that synchronises after every call."""
    _set_qnodes(monkeypatch, "0")                                   # no quantised form: the updates have no host wait of their own
    v, f, _, _ = _sphere()
    n, nv = _ntris(f), v.shape[0]
    xy = torch.from_numpy(_xy()).to(_dev())
    torch.cuda.synchronize()

    def run(sync):
        with rt.Renderer() as b:
            _animated(b, _random_colors(nv, 30))
            b.synchronize()
            wait = b.synchronize if sync else (lambda: None)
            asked, streams = [], set()

            def frame(k):
                u = _uniforms(1, k, n)
                b.render_frame(u); wait()
                streams.add(b.stream())
                h = b.pick(u, xy); wait()
                asked.append((h.record, b.mesh_hit_colors(h))); wait()

            b.mesh_set_colors(_random_colors(nv, 31)); wait()
            b.mesh_colors_refresh(); wait()
            frame(0)
            b.mesh_set_colors(_random_colors(nv, 32)); wait()
            _skin_step(b, 4); wait()
            b.mesh_rebuild(_placed_turned()); wait()
            frame(1)
            b.mesh_set_colors(_random_colors(nv, 33)); wait()
            b.mesh_colors_refresh(); wait()
            frame(2)
            assert b.mesh_info().hostSyncs == 0
            b.synchronize()
            return b.read_all(), b.mesh_color_rows(), [(r.cpu().numpy().copy(), p.cpu().numpy().copy()) for r, p in asked], streams

    targets_s, rows_s, asked_s, _ = run(True)
    targets_a, rows_a, asked_a, streams = run(False)
    assert len(streams) > 1, "the frames did not move stream(): the case does not cross lanes"
    for name, x, y in zip(TARGETS, targets_a, targets_s):
        assert _same(x, y), name
    assert _same(rows_a, rows_s)
    for k, ((ra, pa), (rs, ps)) in enumerate(zip(asked_a, asked_s)):
        assert _same(ra, rs) and _same(pa, ps), k
    assert not _same(asked_s[0][1], asked_s[1][1]) and not _same(asked_s[1][1], asked_s[2][1])     # three sets of colours


# ---------------------------------------------------------------- 8: counters
@pytest.mark.parametrize("qnodes", ["0", "2"])
def test_no_allocation_no_host_wait(monkeypatch, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    v, f, bi, w = _sphere()
    n, nv = _ntris(f), v.shape[0]
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_skin_upload(bi, w, 2, rest=v)
        before = b.mesh_info()
        b.mesh_colors_enable()
        mi0 = b.mesh_info()
        assert mi0.allocations == before.allocations + 2           # the vertex colours and the rows
        assert mi0.scratchBytes == before.scratchBytes + nv * 16 + n * 48 and mi0.hostSyncs == 0
        for k in range(20):
            b.mesh_set_colors(_random_colors(nv, 40 + k))
            if k % 4 == 1:                                         # (there is a tree from step 0 on)
                b.mesh_colors_refresh()
            _skin_step(b, k)
            b.mesh_update(rebuild_above=1.0 if k % 3 == 0 else 1.5)
            mi = b.mesh_info()
            assert mi.allocations == mi0.allocations and mi.hostSyncs == (0 if qnodes == "0" else k + 1)      # the quantised form's status read alone
        _check_rows(b, f, "after 20 steps")
        b.mesh_colors_enable(False)                                # released: the bytes are given back
        assert b.mesh_info().scratchBytes == before.scratchBytes


# ---------------------------------------------------------------- 9: state and refusals
def test_state_and_refusals():
    v, f, _, _ = _sphere()
    nv = v.shape[0]
    rec = np.zeros((4, 4), f32)
    grey = np.full((nv, 3), GREY, f32)

    def calls(b):
        return {"mesh_colors": b.mesh_colors, "mesh_set_colors": lambda: b.mesh_set_colors(grey), "mesh_colors_refresh": b.mesh_colors_refresh,
                "mesh_hit_colors": lambda: b.mesh_hit_colors(rec), "mesh_hit_colors (device)": lambda: b.mesh_hit_colors(torch.from_numpy(rec).to(_dev()))}

    with rt.Renderer() as b:
        assert "no mesh" in _refused(b.mesh_colors_enable)         # no mesh
        for name, call in calls(b).items():
            _refused(call)
        b.mesh_upload(v, f)
        for name, call in calls(b).items():                        # a mesh, colours not enabled, no tree
            _refused(call)
        b.mesh_rebuild()
        for name, call in calls(b).items():                        # a tree, colours not enabled
            assert "rt_mesh_colors_enable" in _refused(call), name
        assert b.mesh_color_rows().size == 0
        b.mesh_upload(v, f)
        b.mesh_colors_enable()
        b.mesh_colors()                                            # the array exists as soon as colours are enabled, and can be written ...
        b.mesh_set_colors(grey)
        for name, call in list(calls(b).items())[2:]:              # ... the gather and the query need a tree
            assert "rebuild" in _refused(call), name
        b.mesh_rebuild()
        for name, call in calls(b).items():
            call()
        for bad in (np.nan, np.inf, -np.inf, -1e-9):               # host colours that are non-finite or negative
            c = grey.copy()
            c[nv - 1, 2] = bad
            _refused(lambda: b.mesh_set_colors(c))
        z = grey.copy()
        z[0, 0], z[1, 1] = 0.0, -0.0                               # zero is a colour
        b.mesh_set_colors(z)
        _refused(lambda: b.mesh_set_colors(grey, first=1))         # past the last vertex
        _refused(lambda: b.mesh_set_colors(grey[:2], first=-1))
        _refused(lambda: b.mesh_set_colors(np.zeros(4, f32)))      # no multiple of three
        b.mesh_set_colors(grey[:0], first=nv)                      # nothing, at the end: fine
        _refused(lambda: b.mesh_hit_colors(rec[:, :3]))
        _refused(lambda: b.mesh_hit_colors(rec.astype(np.float64)))
        b.mesh_colors_enable(False)                                # released on request ...
        for name, call in calls(b).items():
            _refused(call)
        b.mesh_colors_enable()
        b.mesh_upload(v, f)                                        # ... with the mesh by mesh_upload ...
        b.mesh_rebuild()
        for name, call in calls(b).items():
            assert "rt_mesh_colors_enable" in _refused(call), name
        b.mesh_colors_enable()
        b.mesh_upload_parts(v, f, [0, 640, _ntris(f)])             # ... by mesh_upload_parts ...
        b.mesh_rebuild_parts()
        for name, call in calls(b).items():
            assert "rt_mesh_colors_enable" in _refused(call), name
        b.mesh_colors_enable()
        nodes, tris12 = rt.build_bvh(rt.gather_triangles(v, f, IDENT))
        b.upload_bvh(nodes, tris12)                                # ... and by upload_bvh
        assert "no mesh" in _refused(b.mesh_colors_enable)
        for name, call in calls(b).items():
            _refused(call)
        assert b.debug_read_scene(rt.RT_SCENE_ARRAY_COLOR_ROWS).size == 0 and b.scene_info().nTris == _ntris(f)
