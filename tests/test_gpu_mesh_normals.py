"""Smooth vertex normals of the dynamic mesh on the device.  Contract: with normals enabled, mesh_vertex_normals() and
debug_read_scene("normal rows") are, bit for bit, what vertex_normals (rt_vertex_normals, pinned to numpy by tests/test_mesh_normals_host.py) computes
from debug_read_scene("tris"), mesh_order() and the indices, behind every kind of update; mesh_hit_normals equals hit_normals bit for bit; frames of
the mesh's scene write f16(hit_normals) of the pixel's own pick into GNRM on both pipelines and shade with it, GPOS and MOTION stay, and on a flat mesh
-- where the smooth normal has the face normal's bits -- the enabled frame is the disabled one on all four targets; with normals disabled every frame
is what it was.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import opengl_raytracing_amd as rt
import scenes
from mesh_fixtures import flat as _flat, sphere as _sphere, two_bone_skin as _two_bone_skin
from test_gpu_dynamic_mesh import _mesh, _model, _ntris
from test_gpu_mesh_motion import H, TARGETS, W, _bones, _dev, _placed_turned, _refused, _rows, _same, _skin_step, _turn, _xy
from test_gpu_mesh_refit import _set_qnodes
from test_mesh_normals_host import _fan

pytestmark = pytest.mark.gpu

f32 = np.float32
IDENT = np.eye(4, dtype=f32).reshape(-1)


def _device_normals(b):
    """mesh_vertex_normals() as float32 [V,4], read after everything enqueued."""
    t = b.mesh_vertex_normals()
    b.synchronize()
    return t.cpu().numpy().copy()


def _check_against_the_host(b, f, nv, what):
    n = _ntris(f)
    tris, order = _rows(b, n), b.mesh_order(as_torch=False).copy()
    got = _device_normals(b)
    want = rt.vertex_normals(tris, order, f, nv)
    assert got.shape == (nv, 4) and (got[:, 3].view(np.uint32) == 0).all(), what
    assert _same(got[:, :3], want), (what, int((got[:, :3].view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()))
    rows = b.debug_read_scene("normal rows").view(f32).reshape(-1, 12)
    corners = np.asarray(f, np.int64).reshape(-1, 3)[order]
    assert rows.shape == (n, 12) and _same(rows, got[corners].reshape(n, 12)), what
    assert _same(rows, b.mesh_normal_rows())
    return order


# ---------------------------------------------------------------- 1: the normals replayed on the host behind every kind of update
@pytest.mark.parametrize("qnodes", [None, "0", "2"])
@pytest.mark.parametrize("mesh", [1, 9, 63, 65, 257, 1000, "fan", "parts"])
def test_normals_equal_the_host_definition(monkeypatch, mesh, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    parts = mesh == "parts"
    v, f = _fan() if mesh == "fan" else _mesh(300 if parts else mesh)
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
        assert b.debug_read_scene("normal rows").size == 0          # not enabled: no array
        b.mesh_normals_enable()                                     # no tree is needed to enable
        assert b.debug_read_scene("normal rows").size == 0          # ... and there is no scene to read before the first rebuild
        rebuild(0); first = _check_against_the_host(b, f, nv, "first rebuild")
        refit(1); _check_against_the_host(b, f, nv, "refit")
        _skin_step(b, 3)
        refit(1); _check_against_the_host(b, f, nv, "skin step, refit")
        rebuild(3); order = _check_against_the_host(b, f, nv, "rebuild, reordered")
        if n >= 63:
            assert not np.array_equal(order, first), "the rebuild kept every triangle in its row: the case does not reorder"
        actions = []
        b.synchronize()
        actions.append(update(4, 1e9)); _check_against_the_host(b, f, nv, "update 1")       # no measured baseline yet: a rebuild
        b.synchronize()
        b.mesh_set_positions((v + np.random.default_rng(11).normal(0, 1.5, v.shape)).astype(f32))
        actions.append(update(4, 1e9)); _check_against_the_host(b, f, nv, "update 2")       # far below the threshold: a refit, of a badly scattered mesh
        b.synchronize()
        actions.append(update(5, 1.0)); _check_against_the_host(b, f, nv, "update 3")       # at the threshold: whatever costs more than the baseline is rebuilt
        assert actions[:2] == ["rebuild", "refit"], actions
        if mesh == "fan":
            assert rt.debug_normal_pack(f, nv)["info"].maxPerVertex == 200
        b.mesh_normals_enable(False)
        assert b.debug_read_scene("normal rows").size == 0
        b.mesh_normals_enable()                                     # a tree exists: enabling computes the normals at once
        _check_against_the_host(b, f, nv, "enable with a tree")


# ---------------------------------------------------------------- the animated sphere of the frame and query tests
def _animated(b, normals, motion=False):
    v, f, bi, w = _sphere()
    b.upload_env(scenes.tiny_env(8))
    b.resize(W, H)
    b.mesh_upload(v, f)
    b.mesh_skin_upload(bi, w, 2, rest=v)
    if normals:
        b.mesh_normals_enable()
    if motion:
        b.mesh_motion_enable()
    b.mesh_rebuild(_model("default"))


def _uniforms(spp, frame, n, moved=True, use_bvh=True):
    """A frame of the close-up camera with GI and AO on.  moved: the previous view-projection is that of a camera a step to the side."""
    p, cam = rt.default_render_params(), scenes.camera("closeup", aspect=W / H)
    p.sppPerFrame, p.enableGI, p.enableAO = spp, 1, 1
    L = rt.bvh_layout(n)
    prev = None
    if moved:
        before = scenes.camera("closeup", aspect=W / H)
        before.pos[2] += 0.07
        before.yaw -= 0.8
        prev = rt.mat4_mul(rt.camera_proj(before), rt.camera_view(before))
    u = rt.frame_uniforms(p, cam, W, H, frame, use_bvh, L.nNodes, L.nTris, prev_vp=prev)
    assert u.cameraMoved == int(moved) and u.enableGI == 1 and u.enableAO == 1
    return u


def _host_state(b, f):
    n = _ntris(f)
    return _rows(b, n), b.mesh_order(as_torch=False).copy(), _device_normals(b)


def _expected_gnrm(b, u, f, state):
    """(hit mask [H,W], GNRM as halfs [H,W,4]) from the pick of every pixel: f16(hit_normals) and w = 0 at hits, zeros at misses."""
    tris, order, normals = state
    h = b.pick(u, _xy())
    hit = h.prim >= 0
    hn = rt.hit_normals(tris, order, f, normals, h.record)
    want = np.zeros((hit.size, 4), np.float16)
    want[:, :3] = np.where(hit[:, None], hn, f32(0.0)).astype(np.float16)
    return hit.reshape(H, W), want.view(np.uint16).reshape(H, W, 4)


# ---------------------------------------------------------------- 2: the device query
def test_hit_normals_equal_the_host_definition():
    v, f, _, _ = _sphere()
    n = _ntris(f)
    rng = np.random.default_rng(3)
    with rt.Renderer() as b:
        _animated(b, True)
        _skin_step(b, 2)
        b.mesh_refit(_model("default"))
        tris, order, normals = _host_state(b, f)
        u = _uniforms(1, 0, n)
        # pixels, misses included: host arrays and device tensors
        h = b.pick(u, _xy())
        hit = h.prim >= 0
        assert hit.sum() >= 200 and (~hit).sum() >= 200
        want = rt.hit_normals(tris, order, f, normals, h.record)
        got = b.mesh_hit_normals(h)
        assert _same(got, want) and (got[~hit].view(np.uint32) == 0).all()
        assert not _same(got[hit], h.normal[hit])                   # the pick's own normal output stays the face normal
        ht = b.pick(u, torch.from_numpy(_xy()).to(_dev()))
        got_t = b.mesh_hit_normals(ht)
        torch.cuda.synchronize()
        assert _same(ht.record.cpu().numpy(), h.record) and _same(got_t.cpu().numpy(), want)
        # rays: 1, 63, 64, 65 and 2049 of them, aimed at triangles from all around (some miss)
        k = rng.integers(0, n, 2049)
        target = (tris[k, 0:3] + (tris[k, 4:7] + tris[k, 8:11]) / 3).astype(f32)
        org = (target + rng.normal(0, 1, target.shape) * 2).astype(f32)
        dirs = target - org
        dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(f32)
        dirs[::7] = -dirs[::7]                                      # ... and some of them the other way
        for m in (1, 63, 64, 65, 2049):
            r = b.trace_rays(org[:m], dirs[:m])
            want = rt.hit_normals(tris, order, f, normals, r.record)
            assert _same(b.mesh_hit_normals(r), want), m
            rt_ = b.trace_rays(torch.from_numpy(org[:m]).to(_dev()), torch.from_numpy(dirs[:m]).to(_dev()))
            got_t = b.mesh_hit_normals(rt_.record)
            torch.cuda.synchronize()
            assert _same(got_t.cpu().numpy(), want), m
        assert (r.prim >= 0).sum() > 500 and (r.prim < 0).sum() > 50
        # stale records: prims outside the mesh answer zeros
        rec = h.record.copy()
        rec[:4, 1] = np.array([n, 2 ** 31 - 1, -2, -2 ** 31], np.int32).view(f32)
        assert (b.mesh_hit_normals(rec)[:4].view(np.uint32) == 0).all()
        assert b.mesh_hit_normals(rec[:0]).shape == (0, 3)


# ---------------------------------------------------------------- 3: frames
@functools.lru_cache(maxsize=None)
def _frame_run(pipeline, spp, mode):
    """The stages of the frame test on one context -> {stage: targets, ...}; mode "on" also {stage + "/want": (hit mask, expected GNRM)}.
    mode: "off" never enabled, "on" enabled before the first rebuild, "on-off" enabled, then disabled before the first frame."""
    f = _sphere()[1]
    n = _ntris(f)
    out = {}
    with rt.Renderer(pipeline=pipeline) as b:
        _animated(b, mode != "off")
        if mode == "on-off":
            b.mesh_normals_enable(False)
        u = _uniforms(spp, 0, n)

        def frame(stage, uu=u):
            b.reset_accum()
            b.render_frame(uu)
            out[stage] = b.read_all()
            if mode == "on" and uu.useBVH == 1:
                out[stage + "/want"] = _expected_gnrm(b, uu, f, _host_state(b, f))

        frame("rest")
        _skin_step(b, 2)
        b.mesh_refit(_model("default"))
        frame("refit")
        frame("hybrid", _uniforms(spp, 0, n, use_bvh=rt.RT_SCENE_HYBRID))
        _skin_step(b, 3)
        b.mesh_rebuild(_placed_turned())                            # turned where it stands: the rows are reordered
        out["order"] = b.mesh_order(as_torch=False).copy()
        frame("rebuild")
    return out


STAGES = ("rest", "refit", "rebuild")


@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("pipeline", [rt.RT_PIPELINE_WAVEFRONT, rt.RT_PIPELINE_MEGAKERNEL])
def test_frames(pipeline, spp):
    on, off, on_off = (_frame_run(pipeline, spp, m) for m in ("on", "off", "on-off"))
    for stage in STAGES:
        hit, want = on[stage + "/want"]
        gnrm = on[stage][3]
        assert hit.sum() >= 200 and (~hit).sum() >= 200, stage
        assert _same(gnrm[hit], want[hit]), (stage, int((gnrm[hit] != want[hit]).any(axis=1).sum()))      # f16(hit_normals(pick)) at every hit pixel
        assert (gnrm[~hit] == 0).all(), stage                                                              # ... and zero at misses
        assert _same(on[stage][1], off[stage][1]) and _same(on[stage][2], off[stage][2]), stage            # MOTION and GPOS do not change
        assert (gnrm[hit] != off[stage][3][hit]).any(axis=1).sum() >= 100, stage                           # the normal did: it is not the face normal
        assert not _same(on[stage][0], off[stage][0]), stage                                               # ... and the shading follows it
    for name, x, y in zip(TARGETS, on["hybrid"], off["hybrid"]):   # the hybrid scene keeps the face normal
        assert _same(x, y), name
    for stage in STAGES + ("hybrid",):                             # enabled, then disabled: never enabled
        for name, x, y in zip(TARGETS, on_off[stage], off[stage]):
            assert _same(x, y), (stage, name)
    assert not np.array_equal(on["order"], np.arange(on["order"].size))


@pytest.mark.parametrize("spp", [1, 2])
def test_wavefront_equals_megakernel(spp):
    wave, mega = _frame_run(rt.RT_PIPELINE_WAVEFRONT, spp, "on"), _frame_run(rt.RT_PIPELINE_MEGAKERNEL, spp, "on")
    for stage in STAGES + ("hybrid",):
        for name, x, y in zip(TARGETS, wave[stage], mega[stage]):
            assert _same(x, y), (stage, name)


@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("pipeline", [rt.RT_PIPELINE_WAVEFRONT, rt.RT_PIPELINE_MEGAKERNEL])
def test_flat_anchor_frames_are_the_disabled_frames(pipeline, spp):
    """On a flat mesh every vertex normal has the face normal's bits, so the blend hands exactly the reference's normal back at the primary hit and at
    the bounce hit: the enabled frame is the disabled frame on all four targets, COLOR0 included -- every substitution site, without an oracle."""
    v, f = _flat()
    n, nv = _ntris(f), v.shape[0]

    def run(enabled):
        with rt.Renderer(pipeline=pipeline) as b:
            b.upload_env(scenes.tiny_env(8))
            b.resize(W, H)
            b.mesh_upload(v, f)
            if enabled:
                b.mesh_normals_enable()
            b.mesh_rebuild(IDENT)
            u = _uniforms(spp, 0, n)
            b.reset_accum()
            b.render_frame(u)
            targets = b.read_all()
            if not enabled:
                return targets, None
            tris, order, normals = _host_state(b, f)
            h = b.pick(u, _xy())
            return targets, (tris, order, normals, h)

    on, (tris, order, normals, h) = run(True)
    off, _ = run(False)
    # the premise, on the host: (+0, +-1, +0) at every vertex, and hit_normals is the face normal bit for bit at every pixel
    want = np.zeros((nv, 3), f32)
    want[:nv // 2, 1], want[nv // 2:, 1] = 1, -1
    assert _same(normals[:, :3], want)
    hit = h.prim >= 0
    assert hit.sum() >= 200 and (~hit).sum() >= 200
    assert _same(rt.hit_normals(tris, order, f, normals, h.record)[hit], h.normal[hit])
    below = tris[h.prim[hit], 1] == 1
    assert below.sum() >= 100 and (~below).sum() >= 100            # the floor and the ceiling are both in view
    for name, x, y in zip(TARGETS, on, off):
        assert _same(x, y), name
    lit = off[0].reshape(-1, off[0].shape[-1])[hit]
    assert (lit[:, :3] != 0).any()


# ---------------------------------------------------------------- 4: a batch of static-camera frames
@pytest.mark.parametrize("spp", [1, 2])
def test_render_frames_equals_single_calls(spp):
    f = _sphere()[1]
    n = _ntris(f)
    with rt.Renderer() as b:
        _animated(b, True)
        _skin_step(b, 2)
        b.mesh_refit(_model("default"))
        us = [_uniforms(spp, k, n, moved=False) for k in range(4)]
        rows0 = b.mesh_normal_rows()
        b.reset_accum()
        for u in us:
            b.render_frame(u)
        single = b.read_all()
        b.reset_accum()
        b.render_frames(us)
        batch = b.read_all()
        for name, x, y in zip(TARGETS, batch, single):
            assert _same(x, y), name
        hit, want = _expected_gnrm(b, us[3], f, _host_state(b, f))
        assert _same(batch[3][hit], want[hit]) and (batch[3][~hit] == 0).all()
        assert _same(b.mesh_normal_rows(), rows0)                   # frames change no mesh state


# ---------------------------------------------------------------- 5: ordering across lanes
def test_call_order_holds_across_lanes(monkeypatch):
    """update, frame, update, frame -- each call on whatever lane stream() has reached, without a host synchronise, and behind every frame the normals
    of its pixels asked for on the device; everything equals a run that synchronises after every call."""
    _set_qnodes(monkeypatch, "0")                                  # no quantised form: the updates have no host wait of their own
    f = _sphere()[1]
    n = _ntris(f)
    xy = torch.from_numpy(_xy()).to(_dev())
    torch.cuda.synchronize()

    def run(sync):
        with rt.Renderer() as b:
            _animated(b, True)
            b.synchronize()
            wait = b.synchronize if sync else (lambda: None)
            asked, streams = [], set()

            def frame(k):
                u = _uniforms(1, k, n)
                b.render_frame(u); wait()
                streams.add(b.stream())
                h = b.pick(u, xy); wait()
                asked.append((h.record, b.mesh_hit_normals(h))); wait()

            _skin_step(b, 2); wait()
            b.mesh_refit(_model("default")); wait()
            frame(0)
            _skin_step(b, 4); wait()
            b.mesh_rebuild(_placed_turned()); wait()
            frame(1)
            _skin_step(b, 5); wait()
            b.mesh_refit(_placed_turned()); wait()
            frame(2)
            assert b.mesh_info().hostSyncs == 0
            b.synchronize()
            return b.read_all(), b.mesh_normal_rows(), [(r.cpu().numpy().copy(), p.cpu().numpy().copy()) for r, p in asked], streams

    targets_s, rows_s, asked_s, _ = run(True)
    targets_a, rows_a, asked_a, streams = run(False)
    assert len(streams) > 1, "the frames did not move stream(): the case does not cross lanes"
    for name, x, y in zip(TARGETS, targets_a, targets_s):
        assert _same(x, y), name
    assert _same(rows_a, rows_s)
    for k, ((ra, pa), (rs, ps)) in enumerate(zip(asked_a, asked_s)):
        assert _same(ra, rs) and _same(pa, ps), k
    assert not _same(asked_s[0][1], asked_s[1][1]) and not _same(asked_s[1][1], asked_s[2][1])     # three poses, three sets of normals


# ---------------------------------------------------------------- 6: normals and motion together
@pytest.mark.parametrize("pipeline", [rt.RT_PIPELINE_WAVEFRONT, rt.RT_PIPELINE_MEGAKERNEL])
def test_motion_is_the_motion_only_frames(pipeline):
    f = _sphere()[1]
    n = _ntris(f)

    def run(normals):
        with rt.Renderer(pipeline=pipeline) as b:
            _animated(b, normals, motion=True)
            _skin_step(b, 2)
            b.mesh_refit(_model("default"))
            u = _uniforms(1, 0, n)
            b.reset_accum()
            b.render_frame(u)
            t = b.read_all()
            want = _expected_gnrm(b, u, f, _host_state(b, f)) if normals else None
            return t, want

    both, (hit, want) = run(True)
    only, _ = run(False)
    assert _same(both[1], only[1]) and _same(both[2], only[2])     # MOTION (the object's) and GPOS are the motion-only frame's
    assert (both[1][hit] != 0).any(axis=1).sum() >= 100
    assert _same(both[3][hit], want[hit]) and not _same(both[3], only[3])


# ---------------------------------------------------------------- 7: counters
@pytest.mark.parametrize("qnodes", ["0", "2"])
def test_no_allocation_no_host_wait(monkeypatch, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    v, f, bi, w = _sphere()
    n, nv = _ntris(f), v.shape[0]
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_skin_upload(bi, w, 2, rest=v)
        before = b.mesh_info()
        b.mesh_normals_enable()
        mi0 = b.mesh_info()
        info = rt.debug_normal_pack(f, nv)["info"]
        assert mi0.allocations == before.allocations + 5           # adjacency, slice table, face vectors, vertex normals, corner rows
        assert mi0.scratchBytes == before.scratchBytes + info.bytes and mi0.hostSyncs == 0
        assert info.bytes == info.paddedEntries * 4 + (info.nSlices + 1) * 4 + n * 16 + nv * 16 + n * 48
        for k in range(20):
            _skin_step(b, k)
            b.mesh_update(rebuild_above=1.0 if k % 3 == 0 else 1.5)
            mi = b.mesh_info()
            assert mi.allocations == mi0.allocations and mi.hostSyncs == (0 if qnodes == "0" else k + 1)      # the quantised form's status read alone
        _check_against_the_host(b, f, nv, "after 20 steps")
        b.mesh_normals_enable(False)                               # released: the bytes are given back
        assert b.mesh_info().scratchBytes == before.scratchBytes


# ---------------------------------------------------------------- 8: state and refusals
def test_state_and_refusals():
    v, f, _, _ = _sphere()
    rec = np.zeros((4, 4), f32)

    def calls(b):
        return {"mesh_vertex_normals": b.mesh_vertex_normals, "mesh_hit_normals": lambda: b.mesh_hit_normals(rec),
                "mesh_hit_normals (device)": lambda: b.mesh_hit_normals(torch.from_numpy(rec).to(_dev()))}

    with rt.Renderer() as b:
        assert "no mesh" in _refused(b.mesh_normals_enable)        # no mesh
        for name, call in calls(b).items():
            _refused(call)
        b.mesh_upload(v, f)
        for name, call in calls(b).items():                        # a mesh, normals not enabled, no tree
            _refused(call)
        b.mesh_rebuild()
        for name, call in calls(b).items():                        # a tree, normals not enabled
            assert "rt_mesh_normals_enable" in _refused(call), name
        assert b.mesh_normal_rows().size == 0
        b.mesh_upload(v, f)
        b.mesh_normals_enable()
        b.mesh_vertex_normals()                                    # the array exists as soon as normals are enabled ...
        for name, call in list(calls(b).items())[1:]:              # ... the query needs a tree
            assert "rebuild" in _refused(call), name
        b.mesh_rebuild()
        for name, call in calls(b).items():
            call()
        _refused(lambda: b.mesh_hit_normals(rec[:, :3]))
        _refused(lambda: b.mesh_hit_normals(rec.astype(np.float64)))
        b.mesh_normals_enable(False)                               # released on request ...
        for name, call in calls(b).items():
            _refused(call)
        b.mesh_normals_enable()
        b.mesh_upload(v, f)                                        # ... with the mesh by mesh_upload ...
        b.mesh_rebuild()
        for name, call in calls(b).items():
            assert "rt_mesh_normals_enable" in _refused(call), name
        b.mesh_normals_enable()
        nodes, tris12 = rt.build_bvh(rt.gather_triangles(v, f, IDENT))
        b.upload_bvh(nodes, tris12)                                # ... and by upload_bvh
        assert "no mesh" in _refused(b.mesh_normals_enable)
        for name, call in calls(b).items():
            _refused(call)
        assert b.debug_read_scene(rt.RT_SCENE_ARRAY_NORMAL_ROWS).size == 0 and b.scene_info().nTris == _ntris(f)
