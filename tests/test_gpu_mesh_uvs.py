"""UVs and the albedo texture of the dynamic mesh on the device.  Contract: with UVs enabled, debug_read_scene("uv rows") is, bit for
bit, what uv_rows (rt_uv_rows, pinned to numpy by tests/test_mesh_uvs_host.py) makes of mesh_order(), the indices and mesh_uvs(), behind every kind of
update and behind mesh_uvs_refresh; mesh_hit_uvs equals hit_uvs and mesh_hit_texels equals sample_texture(hit_uvs) bit for bit for every texture size
and flag combination; frames of the mesh's scene multiply the albedo of the primary and the bounce hit by the texel on both pipelines while GPOS, GNRM
and MOTION stay; an all-255 texture -- the factor 1 -- renders the untextured frame on all four targets, a texture with a channel at 0 and the others
at 255 leaves the others' bits alone; without UVs or without a texture every frame is what it was.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import opengl_raytracing_amd as rt
from mesh_fixtures import random_texture as _random_texture, random_uvs as _random_uvs
from test_gpu_dynamic_mesh import _mesh, _model, _ntris
from test_gpu_mesh_colors import PIPELINES, _animated, _flat_scene, _frame, _random_colors, _uniforms
from test_gpu_mesh_motion import H, TARGETS, W, _dev, _placed_turned, _refused, _rows, _same, _skin_step, _turn, _xy
from test_gpu_mesh_normals import _flat, _sphere
from test_gpu_mesh_refit import _set_qnodes

pytestmark = pytest.mark.gpu

f32 = np.float32
IDENT = np.eye(4, dtype=f32).reshape(-1)
FLAGS = tuple(range(8))
WHITE = np.full((2, 3, 4), 255, np.uint8)


def _device_uvs(b):
    """mesh_uvs() as float32 [V,2], read after everything enqueued."""
    t = b.mesh_uvs()
    b.synchronize()
    return t.cpu().numpy().copy()


def _check_rows(b, f, what):
    order = b.mesh_order(as_torch=False).copy()
    uvs = _device_uvs(b)
    rows = b.debug_read_scene("uv rows").view(f32).reshape(-1, 8)
    want = rt.uv_rows(order, f, uvs)
    assert rows.shape == (_ntris(f), 8) and _same(rows, want), (what, int((rows.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()))
    assert _same(rows, b.mesh_uv_rows())
    return order, rows


def _textured(b, uvs, texels, flags=0):
    """UVs and a texture on a context whose mesh is uploaded (with or without a tree)."""
    b.mesh_uvs_enable()
    b.mesh_set_uvs(uvs)
    if b.mesh_info().rebuilds:
        b.mesh_uvs_refresh()
    b.mesh_texture_upload(texels, flags)


# ---------------------------------------------------------------- 1: the rows replayed on the host behind every kind of update
@pytest.mark.parametrize("qnodes", [None, "0", "2"])
@pytest.mark.parametrize("mesh", [1, 9, 63, 65, 257, 1000, "parts"])
def test_rows_equal_the_host_definition(monkeypatch, mesh, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    parts = mesh == "parts"
    v, f = _mesh(300 if parts else mesh)
    v, f = np.ascontiguousarray(v, f32), np.ascontiguousarray(f, np.uint32).reshape(-1)
    n, nv = _ntris(f), v.shape[0]
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
        assert b.debug_read_scene("uv rows").size == 0              # not enabled: no array
        b.mesh_uvs_enable()                                         # no tree is needed to enable
        assert b.debug_read_scene("uv rows").size == 0              # ... and there is no scene to read before the first rebuild
        got = _device_uvs(b)
        assert got.shape == (nv, 2) and (got.view(np.uint32) == 0).all()
        b.mesh_colors_enable()                                      # the UV gather runs behind the colours' gather
        b.mesh_set_uvs(_random_uvs(nv, 1))
        rebuild(0); first, rows0 = _check_rows(b, f, "first rebuild")
        assert (rows0[:, :6] != 0).any()
        refit(1); _check_rows(b, f, "refit")
        b.mesh_set_uvs(_random_uvs(nv, 2))
        assert _same(b.mesh_uv_rows(), rows0)                       # writing UVs alone leaves the rows as they were
        b.mesh_uvs_refresh()
        _, rows1 = _check_rows(b, f, "set UVs, refresh")
        assert not _same(rows1, rows0)                              # ... the refresh moves them, with no update
        b.mesh_set_uvs(_random_uvs(max(nv // 2, 1), 3), first=nv - max(nv // 2, 1))            # a range that ends at the last vertex
        refit(1); _check_rows(b, f, "refit behind a partial write")
        rebuild(3); order, _ = _check_rows(b, f, "rebuild, reordered")
        if n >= 63:
            assert not np.array_equal(order, first), "the rebuild kept every triangle in its row: the case does not reorder"
        actions = []
        b.synchronize()
        actions.append(update(4, 1e9)); _check_rows(b, f, "update 1")                # no measured baseline yet: a rebuild
        b.synchronize()
        b.mesh_set_positions((v + np.random.default_rng(11).normal(0, 1.5, v.shape)).astype(f32))
        t = b.mesh_uvs()                                            # the caller's own write, on stream()'s stream
        with torch.cuda.stream(torch.cuda.ExternalStream(b.stream(), device=_dev())):
            t[:, :] = torch.from_numpy(_random_uvs(nv, 4)).to(_dev())
        actions.append(update(4, 1e9)); _check_rows(b, f, "update 2")                # far below the threshold: a refit
        b.synchronize()
        actions.append(update(5, 1.0)); _check_rows(b, f, "update 3")                # at the threshold
        assert actions[:2] == ["rebuild", "refit"] and actions[2] in ("rebuild", "refit"), actions
        b.mesh_uvs_enable(False)
        assert b.debug_read_scene("uv rows").size == 0
        b.mesh_uvs_enable()                                         # a tree exists: enabling fills the rows at once, with zeros
        _, rows = _check_rows(b, f, "enable with a tree")
        assert (rows.view(np.uint32) == 0).all()
        b.mesh_set_uvs(_random_uvs(nv, 5))
        b.mesh_uvs_refresh()
        before, _, rows5 = b.mesh_info().allocations, *_check_rows(b, f, "UVs set again")
        b.mesh_uvs_enable()                                         # already enabled: UVs and rows stay, nothing is allocated
        assert b.mesh_info().allocations == before and _same(_check_rows(b, f, "enable while enabled")[1], rows5) and not _same(rows5, rows)


# ---------------------------------------------------------------- 2: the device queries
def _rays(tris):
    """2049 rays aimed at triangles of the rows `tris` from all around, some of them the other way."""
    rng = np.random.default_rng(3)
    k = rng.integers(0, tris.shape[0], 2049)
    target = (tris[k, 0:3] + (tris[k, 4:7] + tris[k, 8:11]) / 3).astype(f32)
    org = (target + rng.normal(0, 1, target.shape) * 2).astype(f32)
    dirs = target - org
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(f32)
    dirs[::7] = -dirs[::7]
    return org, dirs


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_hit_uvs_and_texels_equal_the_host_definition(size):
    v, f, _, _ = _sphere()
    n, nv = _ntris(f), v.shape[0]
    tex = _random_texture(*size, seed=7)
    with rt.Renderer() as b:
        _animated(b)
        _textured(b, _random_uvs(nv, 5), tex)
        _skin_step(b, 2)
        b.mesh_refit(_model("default"))
        order, uvs = b.mesh_order(as_torch=False).copy(), _device_uvs(b)
        u = _uniforms(1, 0, n)
        h = b.pick(u, _xy())                                        # every pixel, misses included
        hit = h.prim >= 0
        assert hit.sum() >= 200 and (~hit).sum() >= 200
        ht = b.pick(u, torch.from_numpy(_xy()).to(_dev()))
        want_uv = rt.hit_uvs(order, f, uvs, h.record)
        got_uv = b.mesh_hit_uvs(h)
        assert _same(got_uv, want_uv) and (got_uv[~hit].view(np.uint32) == 0).all() and (got_uv[hit] != 0).any()
        got_t = b.mesh_hit_uvs(ht)
        torch.cuda.synchronize()
        assert _same(ht.record.cpu().numpy(), h.record) and _same(got_t.cpu().numpy(), want_uv)
        org, dirs = _rays(_rows(b, n))
        rays = [b.trace_rays(org[:m], dirs[:m]) for m in (1, 63, 64, 65, 2049)]
        assert (rays[-1].prim >= 0).sum() > 300 and (rays[-1].prim < 0).sum() > 50
        rays_t = b.trace_rays(torch.from_numpy(org).to(_dev()), torch.from_numpy(dirs).to(_dev()))
        for r in rays:
            assert _same(b.mesh_hit_uvs(r), rt.hit_uvs(order, f, uvs, r.record)), r.record.shape
        stale = h.record.copy()                                     # stale records: prims outside the mesh answer zeros
        stale[:4, 1] = np.array([n, 2 ** 31 - 1, -2, -2 ** 31], np.int32).view(f32)
        assert (b.mesh_hit_uvs(stale)[:4].view(np.uint32) == 0).all() and _same(b.mesh_hit_uvs(stale), rt.hit_uvs(order, f, uvs, stale))
        seen = set()
        for flags in FLAGS:
            b.mesh_texture_upload(tex, flags)
            want = np.where(hit[:, None], rt.sample_texture(tex, flags, want_uv), f32(0)).astype(f32)
            got = b.mesh_hit_texels(h)
            assert _same(got, want), flags
            seen.add(got.tobytes())
            got_t = b.mesh_hit_texels(ht)
            torch.cuda.synchronize()
            assert _same(got_t.cpu().numpy(), want), flags
            for r in rays:
                on = r.prim >= 0
                want_r = np.where(on[:, None], rt.sample_texture(tex, flags, rt.hit_uvs(order, f, uvs, r.record)), f32(0)).astype(f32)
                assert _same(b.mesh_hit_texels(r), want_r), (flags, r.record.shape)
            got_t = b.mesh_hit_texels(rays_t.record)
            torch.cuda.synchronize()
            assert _same(got_t.cpu().numpy(), want_r), flags
            got_s = b.mesh_hit_texels(stale)
            assert (got_s[:4].view(np.uint32) == 0).all() and _same(got_s[4:], want[4:]), flags
        assert len(seen) == (2 if size == (1, 1) else 8)            # every flag combination is a different lookup (1x1: the encoding alone)
        assert b.mesh_hit_uvs(h.record[:0]).shape == (0, 2) and b.mesh_hit_texels(h.record[:0]).shape == (0, 3)


def test_texels_written_on_the_device_between_two_queries():
    """mesh_texture() hands out the texels: a write on stream()'s stream between two queries, with no host wait, is seen by the second alone."""
    v, f, _, _ = _sphere()
    n, nv = _ntris(f), v.shape[0]
    tex0, tex1 = _random_texture(3, 5, 1), _random_texture(3, 5, 2)
    with rt.Renderer() as b:
        _animated(b)
        _textured(b, _random_uvs(nv, 6), tex0, rt.TEX_CLAMP)
        order, uvs = b.mesh_order(as_torch=False).copy(), _device_uvs(b)
        h = b.pick(_uniforms(1, 0, n), torch.from_numpy(_xy()).to(_dev()))
        new = torch.from_numpy(tex1).to(_dev())
        t = b.mesh_texture()
        assert tuple(t.shape) == (5, 3, 4) and t.dtype == torch.uint8 and b.mesh_texture(as_torch=False)[1:] == (60, 3, 5)
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.ExternalStream(b.stream(), device=_dev())):
            first = b.mesh_hit_texels(h)
            t.copy_(new)
            second = b.mesh_hit_texels(h)
        torch.cuda.synchronize()
        rec = h.record.cpu().numpy()
        on = (h.prim.cpu().numpy() >= 0)[:, None]
        uv = rt.hit_uvs(order, f, uvs, rec)
        assert _same(first.cpu().numpy(), np.where(on, rt.sample_texture(tex0, rt.TEX_CLAMP, uv), f32(0)).astype(f32))
        assert _same(second.cpu().numpy(), np.where(on, rt.sample_texture(tex1, rt.TEX_CLAMP, uv), f32(0)).astype(f32))
        assert not _same(first.cpu().numpy(), second.cpu().numpy())


# ---------------------------------------------------------------- 3: the white anchor
@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("colored", [False, True])
@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_white_anchor_frames_are_the_untextured_frames(pipeline, spp, colored, normals):
    """An all-255 texture is the factor 1.0f: with random UVs the textured frame is the untextured frame on all four targets, COLOR0 included, with GI
    and AO on -- every substitution site; and so is the frame after the texture was released."""
    v, f = _flat()
    n, nv = _ntris(f), v.shape[0]
    u = _uniforms(spp, 0, n)

    def run(mode):
        with rt.Renderer(pipeline=pipeline) as b:
            _flat_scene(b, _random_colors(nv, 9) if colored else None)
            if normals:
                b.mesh_normals_enable()
            if mode != "never":
                _textured(b, _random_uvs(nv, 4), WHITE if mode == "white" else _random_texture(3, 5, 8), mode == "white" and rt.TEX_SRGB or 0)
            if mode == "released":
                b.mesh_texture_upload(None)
            if mode == "uvs off":
                b.mesh_uvs_enable(False)
            return _frame(b, u), b.pick(u, _xy())

    off, h = run("never")
    hit = h.prim >= 0
    assert hit.sum() >= 200 and (~hit).sum() >= 200
    assert (off[0].reshape(-1, off[0].shape[-1])[hit][:, :3] != 0).any()
    for mode in ("white", "released", "uvs off"):
        got, _ = run(mode)
        for name, x, y in zip(TARGETS, got, off):
            assert _same(x, y), (mode, name)


# ---------------------------------------------------------------- 4: the product
@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_product(pipeline, spp):
    """A first frame (no history), GI off (its luminance clamp couples channels), AO on.  A 1x1 texture of code (255, 0, 255) leaves R and B of COLOR0
    at the untextured frame's bits and G nowhere above it; a 2x2 checker changes the frame somewhere on the mesh and nowhere off it."""
    v, f = _flat()
    n, nv = _ntris(f), v.shape[0]
    u = _uniforms(spp, 0, n, gi=0)
    uvs = np.ascontiguousarray(v[:, [0, 2]] * f32(0.37), f32)     # the checker repeats across the floor and the ceiling

    def run(texels, flags=0):
        with rt.Renderer(pipeline=pipeline) as b:
            _flat_scene(b, None)
            if texels is not None:
                _textured(b, uvs, texels, flags)
            return _frame(b, u), b.pick(u, _xy())

    off, h = run(None)
    hit = (h.prim >= 0).reshape(H, W)
    magenta, _ = run(np.array([[[255, 0, 255, 77]]], np.uint8))
    assert _same(magenta[0][..., 0], off[0][..., 0]) and _same(magenta[0][..., 2], off[0][..., 2])
    g_on, g_off = magenta[0][..., 1].astype(np.float64), off[0][..., 1].astype(np.float64)
    assert (g_on <= g_off).all() and (g_on[hit] < g_off[hit]).any()
    for name, x, y in list(zip(TARGETS, magenta, off))[1:]:
        assert _same(x, y), name
    checker = np.zeros((2, 2, 4), np.uint8)
    checker[0, 0, :3] = checker[1, 1, :3] = 255
    checker[0, 1, :3] = checker[1, 0, :3] = 40
    got, _ = run(checker, rt.TEX_NEAREST)
    differs = (got[0].view(np.uint16) != off[0].view(np.uint16)).reshape(H, W, -1).any(axis=2)
    assert differs[hit].any() and not differs[~hit].any() and (~differs[hit]).any()      # the dark squares and the white ones
    for name, x, y in list(zip(TARGETS, got, off))[1:]:
        assert _same(x, y), name


# ---------------------------------------------------------------- 5: pipelines and other scenes
@functools.lru_cache(maxsize=None)
def _frame_run(pipeline, spp, textured, dressed):
    """Stages on one context with GI and AO on and motion enabled -> {stage: targets}.  dressed: colours and smooth normals as well."""
    v, f, _, _ = _sphere()
    n, nv = _ntris(f), v.shape[0]
    out = {}
    with rt.Renderer(pipeline=pipeline) as b:
        _animated(b, _random_colors(nv, 6) if dressed else None, normals=dressed, motion=True)
        if textured:
            _textured(b, _random_uvs(nv, 12), _random_texture(3, 5, 13))
        out["rest"] = _frame(b, _uniforms(spp, 0, n))
        _skin_step(b, 2)
        b.mesh_refit(_model("default"))
        out["refit"] = _frame(b, _uniforms(spp, 0, n))
        out["hybrid"] = _frame(b, _uniforms(spp, 0, n, use_bvh=rt.RT_SCENE_HYBRID))
        out["analytic"] = _frame(b, _uniforms(spp, 0, n, use_bvh=False))
        _skin_step(b, 3)
        b.mesh_rebuild(_placed_turned())                            # turned where it stands: the rows are reordered
        out["rebuild"] = _frame(b, _uniforms(spp, 0, n))
    return out


STAGES = ("rest", "refit", "rebuild")


@pytest.mark.parametrize("dressed", [False, True])
@pytest.mark.parametrize("spp", [1, 2])
def test_wavefront_equals_megakernel_and_only_color_changes(spp, dressed):
    wave, mega = _frame_run(PIPELINES[0], spp, True, dressed), _frame_run(PIPELINES[1], spp, True, dressed)
    off = _frame_run(PIPELINES[0], spp, False, dressed)
    for stage in STAGES + ("hybrid", "analytic"):
        for name, x, y in zip(TARGETS, wave[stage], mega[stage]):
            assert _same(x, y), (stage, name)
    for stage in STAGES:
        assert not _same(wave[stage][0], off[stage][0]), stage      # the shading follows the texture ...
        for name, x, y in list(zip(TARGETS, wave[stage], off[stage]))[1:]:
            assert _same(x, y), (stage, name)                       # ... MOTION, GPOS and GNRM do not
    for stage in ("hybrid", "analytic"):                            # the hybrid and the analytic scene are unchanged
        for name, x, y in zip(TARGETS, wave[stage], off[stage]):
            assert _same(x, y), (stage, name)


# ---------------------------------------------------------------- 6: ordering and counters
@pytest.mark.parametrize("spp", [1, 2])
def test_render_frames_equals_single_calls(spp):
    v, f, _, _ = _sphere()
    n, nv = _ntris(f), v.shape[0]
    with rt.Renderer() as b:
        _animated(b, _random_colors(nv, 7))
        _textured(b, _random_uvs(nv, 8), _random_texture(64, 64, 9), rt.TEX_SRGB)
        _skin_step(b, 2)
        b.mesh_refit(_model("default"))
        us = [_uniforms(spp, k, n, moved=False) for k in range(4)]
        rows0 = b.mesh_uv_rows()
        b.reset_accum()
        for u in us:
            b.render_frame(u)
        single = b.read_all()
        b.reset_accum()
        b.render_frames(us)
        batch = b.read_all()
        for name, x, y in zip(TARGETS, batch, single):
            assert _same(x, y), name
        assert _same(b.mesh_uv_rows(), rows0)                       # frames change no mesh state


def test_call_order_holds_across_lanes(monkeypatch):
    """set_uvs, refresh, frame, device texel write, frame, update, frame -- each call on whatever lane stream() has reached, without a host synchronise,
    and behind every frame a pick and both hit queries asked for on the device; everything equals a run that synchronises after every call."""
    _set_qnodes(monkeypatch, "0")                                   # no quantised form: the updates have no host wait of their own
    v, f, _, _ = _sphere()
    n, nv = _ntris(f), v.shape[0]
    xy = torch.from_numpy(_xy()).to(_dev())
    new = torch.from_numpy(_random_texture(3, 5, 22)).to(_dev())
    torch.cuda.synchronize()

    def run(sync):
        with rt.Renderer() as b:
            _animated(b)
            _textured(b, _random_uvs(nv, 30), _random_texture(3, 5, 21))
            b.synchronize()
            wait = (lambda: (b.synchronize(), torch.cuda.synchronize())) if sync else (lambda: None)
            asked, streams = [], set()

            def frame(k):
                u = _uniforms(1, k, n)
                b.render_frame(u); wait()
                streams.add(b.stream())
                h = b.pick(u, xy); wait()
                asked.append((h.record, b.mesh_hit_uvs(h), b.mesh_hit_texels(h))); wait()

            b.mesh_set_uvs(_random_uvs(nv, 31)); wait()
            b.mesh_uvs_refresh(); wait()
            frame(0)
            t = b.mesh_texture()
            with torch.cuda.stream(torch.cuda.ExternalStream(b.stream(), device=_dev())):    # behind frame 0 and its queries, in front of frame 1
                t.copy_(new)
            wait()
            frame(1)
            b.mesh_set_uvs(_random_uvs(nv, 32)); wait()
            _skin_step(b, 4); wait()
            b.mesh_rebuild(_placed_turned()); wait()
            frame(2)
            assert b.mesh_info().hostSyncs == 0
            b.synchronize()
            torch.cuda.synchronize()
            return b.read_all(), b.mesh_uv_rows(), [tuple(x.cpu().numpy().copy() for x in a) for a in asked], streams

    targets_s, rows_s, asked_s, _ = run(True)
    targets_a, rows_a, asked_a, streams = run(False)
    assert len(streams) > 1, "the frames did not move stream(): the case does not cross lanes"
    for name, x, y in zip(TARGETS, targets_a, targets_s):
        assert _same(x, y), name
    assert _same(rows_a, rows_s)
    for k, (a, s) in enumerate(zip(asked_a, asked_s)):
        assert all(_same(x, y) for x, y in zip(a, s)), k
    for k, texels in enumerate((_random_texture(3, 5, 21), new.cpu().numpy(), new.cpu().numpy())):        # the texel write lies between frames 0 and 1
        rec, uv, got = asked_s[k]
        on = (np.ascontiguousarray(rec[:, 1]).view(np.int32) >= 0)[:, None]
        assert on.sum() >= 200 and _same(got, np.where(on, rt.sample_texture(texels, 0, uv), f32(0)).astype(f32)), k
    assert not _same(asked_s[1][1], asked_s[2][1])                                              # the update: other UVs


@pytest.mark.parametrize("qnodes", ["0", "2"])
def test_no_allocation_no_host_wait(monkeypatch, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    v, f, bi, w = _sphere()
    n, nv = _ntris(f), v.shape[0]
    tex = _random_texture(64, 64, 3)
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_skin_upload(bi, w, 2, rest=v)
        before = b.mesh_info()
        b.mesh_uvs_enable()
        mi0 = b.mesh_info()
        assert mi0.allocations == before.allocations + 2           # the vertex UVs and the rows
        assert mi0.scratchBytes == before.scratchBytes + nv * 8 + n * 32 and mi0.hostSyncs == 0
        b.mesh_texture_upload(tex)
        mi1 = b.mesh_info()
        assert mi1.allocations == mi0.allocations + 2 and mi1.scratchBytes == mi0.scratchBytes + 64 * 64 * 4 + 1024      # the texels and the table
        b.mesh_texture_upload(_random_texture(64, 64, 4), rt.TEX_SRGB | rt.TEX_NEAREST)
        assert b.mesh_info().allocations == mi1.allocations        # the same size: the block is reused
        for k in range(20):
            b.mesh_set_uvs(_random_uvs(nv, 40 + k))
            if k % 4 == 1:                                         # (there is a tree from step 0 on)
                b.mesh_uvs_refresh()
            _skin_step(b, k)
            b.mesh_update(rebuild_above=1.0 if k % 3 == 0 else 1.5)
            mi = b.mesh_info()
            assert mi.allocations == mi1.allocations and mi.hostSyncs == (0 if qnodes == "0" else k + 1)      # the quantised form's status read alone
        _check_rows(b, f, "after 20 steps")
        b.mesh_texture_upload(_random_texture(3, 5, 4))            # another size: a new block, the old bytes given back
        mi2 = b.mesh_info()
        assert mi2.allocations == mi1.allocations + 2 and mi2.scratchBytes == mi0.scratchBytes + 60 + 1024
        b.mesh_texture_upload(None)
        b.mesh_uvs_enable(False)                                   # released: the bytes are given back
        assert b.mesh_info().scratchBytes == before.scratchBytes


# ---------------------------------------------------------------- 7: state and refusals
def test_state_and_refusals():
    v, f, _, _ = _sphere()
    nv = v.shape[0]
    rec = np.zeros((4, 4), f32)
    zero = np.zeros((nv, 2), f32)
    tex = _random_texture(3, 5, 1)

    def uv_calls(b):
        return {"mesh_uvs": b.mesh_uvs, "mesh_set_uvs": lambda: b.mesh_set_uvs(zero), "mesh_uvs_refresh": b.mesh_uvs_refresh,
                "mesh_hit_uvs": lambda: b.mesh_hit_uvs(rec), "mesh_hit_uvs (device)": lambda: b.mesh_hit_uvs(torch.from_numpy(rec).to(_dev()))}

    def tex_calls(b):
        return {"mesh_texture": b.mesh_texture, "mesh_hit_texels": lambda: b.mesh_hit_texels(rec),
                "mesh_hit_texels (device)": lambda: b.mesh_hit_texels(torch.from_numpy(rec).to(_dev()))}

    with rt.Renderer() as b:
        assert "no mesh" in _refused(b.mesh_uvs_enable)
        assert "no mesh" in _refused(lambda: b.mesh_texture_upload(tex))
        for name, call in {**uv_calls(b), **tex_calls(b)}.items():
            _refused(call)
        b.mesh_upload(v, f)
        for name, call in {**uv_calls(b), **tex_calls(b)}.items():  # a mesh, nothing enabled, no tree
            _refused(call)
        b.mesh_rebuild()
        for name, call in uv_calls(b).items():                     # a tree, UVs not enabled
            assert "rt_mesh_uvs_enable" in _refused(call), name
        assert "rt_mesh_texture_upload" in _refused(b.mesh_texture)
        assert "rt_mesh_uvs_enable" in _refused(lambda: b.mesh_hit_texels(rec))
        assert b.mesh_uv_rows().size == 0
        b.mesh_upload(v, f)
        b.mesh_uvs_enable()
        b.mesh_uvs()                                               # the array exists as soon as UVs are enabled, and can be written ...
        b.mesh_set_uvs(zero)
        for name, call in list(uv_calls(b).items())[2:]:           # ... the gather and the query need a tree
            assert "rebuild" in _refused(call), name
        b.mesh_rebuild()
        for name, call in uv_calls(b).items():
            call()
        assert "rt_mesh_texture_upload" in _refused(lambda: b.mesh_hit_texels(rec))        # UVs and a tree, no texture
        b.mesh_texture_upload(tex, 7)
        for name, call in tex_calls(b).items():
            call()
        out = np.full((4, 3), 7, f32)                               # no output written on refusal: an unaligned record pointer on the device path
        d_rec, d_out = torch.zeros((5, 4), dtype=torch.float32, device=_dev()), torch.from_numpy(out).to(_dev())
        import ctypes as C
        for entry in ("rt_mesh_hit_uvs", "rt_mesh_hit_texels"):
            rc = getattr(rt.lib(), entry)(b._h, C.c_void_p(d_rec.data_ptr() + 4), 4, C.c_void_p(d_out.data_ptr()))
            assert rc == rt.RT_ERR_INVALID and "16-byte aligned" in (rt.lib().rt_last_error(b._h) or b"").decode() and entry in (rt.lib().rt_last_error(b._h) or b"").decode()
            rc = getattr(rt.lib(), entry)(b._h, None, 4, C.c_void_p(d_out.data_ptr()))
            assert rc == rt.RT_ERR_INVALID and "bad arguments" in (rt.lib().rt_last_error(b._h) or b"").decode()
        torch.cuda.synchronize()
        assert _same(d_out.cpu().numpy(), out)
        ptr, size, w, h = C.c_void_p(5), C.c_size_t(5), C.c_int(5), C.c_int(5)
        b.mesh_texture_upload(None)
        assert rt.lib().rt_mesh_texture(b._h, C.byref(ptr), C.byref(size), C.byref(w), C.byref(h)) == rt.RT_ERR_INVALID
        assert (ptr.value, size.value, w.value, h.value) == (None, 0, 0, 0)                # outputs cleared on refusal
        for bad in (np.nan, np.inf, -np.inf):                      # host UVs that are non-finite
            c = zero.copy()
            c[nv - 1, 1] = bad
            assert "finite" in _refused(lambda: b.mesh_set_uvs(c))
        neg = zero.copy()
        neg[0, 0], neg[1, 1] = -3.25, -0.0                         # negative values are fine
        b.mesh_set_uvs(neg)
        assert "vertices" in _refused(lambda: b.mesh_set_uvs(zero, first=1))               # past the last vertex
        _refused(lambda: b.mesh_set_uvs(zero[:2], first=-1))
        _refused(lambda: b.mesh_set_uvs(np.zeros(3, f32)))         # no multiple of two
        b.mesh_set_uvs(zero[:0], first=nv)                         # nothing, at the end: fine
        for bad_flags in (8, -1, 0x100):
            assert "flag" in _refused(lambda: b.mesh_texture_upload(tex, bad_flags))
        _refused(lambda: b.mesh_texture_upload(tex[:, :, :3]))
        _refused(lambda: b.mesh_texture_upload(tex.astype(np.float32)))
        one = np.zeros(4, np.uint8)
        for w_, h_ in ((0, 1), (1, 0), (-1, 1), (rt.TEX_MAX_SIZE + 1, 1), (1, rt.TEX_MAX_SIZE + 1)):
            assert rt.lib().rt_mesh_texture_upload(b._h, C.c_void_p(one.ctypes.data), w_, h_, 0) == rt.RT_ERR_INVALID and "texels" in (rt.lib().rt_last_error(b._h) or b"").decode()
        assert rt.lib().rt_mesh_texture_upload(b._h, None, 1, 1, 0) == rt.RT_ERR_INVALID
        _refused(lambda: b.mesh_hit_uvs(rec[:, :3]))
        _refused(lambda: b.mesh_hit_texels(rec.astype(np.float64)))
        b.mesh_texture_upload(tex)
        b.mesh_uvs_enable(False)                                   # released on request: the texture alone does not answer
        for name, call in uv_calls(b).items():
            _refused(call)
        assert "rt_mesh_uvs_enable" in _refused(lambda: b.mesh_hit_texels(rec))
        b.mesh_texture()                                           # ... but it is still there
        b.mesh_uvs_enable()
        b.mesh_upload(v, f)                                        # ... with the mesh by mesh_upload ...
        b.mesh_rebuild()
        for name, call in {**uv_calls(b), **tex_calls(b)}.items():
            _refused(call)
        b.mesh_uvs_enable()
        b.mesh_texture_upload(tex)
        b.mesh_upload_parts(v, f, [0, 640, _ntris(f)])             # ... by mesh_upload_parts ...
        b.mesh_rebuild_parts()
        for name, call in {**uv_calls(b), **tex_calls(b)}.items():
            _refused(call)
        b.mesh_uvs_enable()
        b.mesh_texture_upload(tex)
        nodes, tris12 = rt.build_bvh(rt.gather_triangles(v, f, IDENT))
        b.upload_bvh(nodes, tris12)                                # ... and by upload_bvh
        assert "no mesh" in _refused(b.mesh_uvs_enable)
        for name, call in {**uv_calls(b), **tex_calls(b)}.items():
            _refused(call)
        assert b.debug_read_scene(rt.RT_SCENE_ARRAY_UV_ROWS).size == 0 and b.scene_info().nTris == _ntris(f)


# ---------------------------------------------------------------- 8: the command-line host
def test_cli_texture(tmp_path):
    """rt_cli --obj m.obj --texture t.png: the PNG differs from the run without --texture and equals the same steps through the Python harness (the
    mesh read with its vt records, colours at 1, the PNG's rows flipped so that row 0 is v = 0, the default placement)."""
    import subprocess

    import scenes
    cli = scenes.ROOT / "opengl-raytracing_amd" / "rt_cli"
    v, f = rt.meshgen.icosphere(2)
    v = np.asarray(v, np.float64)
    uv = np.stack([np.arctan2(v[:, 2], v[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(v[:, 1], -1, 1)) / np.pi], axis=1)
    obj = tmp_path / "ball.obj"
    with open(obj, "w") as fh:
        fh.writelines(f"v {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n" for p in v)
        fh.writelines(f"vt {t[0]:.9g} {t[1]:.9g}\n" for t in uv)
        fh.writelines("f " + " ".join(f"{i + 1}/{i + 1}" for i in tri) + "\n" for tri in np.asarray(f).reshape(-1, 3))
    png = np.zeros((8, 16, 3), np.uint8)
    png[::2, ::2] = png[1::2, 1::2] = (250, 60, 30)
    png[::2, 1::2] = png[1::2, ::2] = (20, 90, 240)
    png[0] = 255                                                    # the top row differs from the bottom one: the flip matters
    rt.save_png(tmp_path / "t.png", png)
    base = [str(cli), "--obj", str(obj), "--cam", "-2,1.5,1.0,-90,0", "--size", f"{W}x{H}", "--spp", "2", "--frames", "2"]
    outs = {}
    for name, extra in (("plain", []), ("tex", ["--texture", str(tmp_path / "t.png")]), ("srgb", ["--texture", str(tmp_path / "t.png"), "--texture-srgb"])):
        r = subprocess.run(base + extra + ["--out", str(tmp_path / name)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("[TEXTURE]" in r.stdout) == bool(extra)
        outs[name] = rt.load_png(tmp_path / f"{name}.png")
    assert outs["plain"].shape == outs["tex"].shape and not np.array_equal(outs["plain"], outs["tex"]) and not np.array_equal(outs["srgb"], outs["tex"])
    p = rt.default_render_params()
    p.sppPerFrame = 2
    pos, uvs, idx = rt.load_obj_uv(obj)
    rgba = np.concatenate([png[::-1], np.full(png.shape[:2] + (1,), 255, np.uint8)], axis=2)
    with rt.Renderer() as b:
        b.mesh_upload(pos, idx)
        b.mesh_colors_enable()
        b.mesh_set_colors(np.ones((pos.shape[0], 3), f32))
        b.mesh_uvs_enable()
        b.mesh_set_uvs(uvs)
        b.mesh_texture_upload(rgba)
        b.mesh_rebuild(rt.default_bvh_transform())
        b.resize(W, H)
        for _ in range(2):
            b.render_ray(p, scenes.camera("closeup", aspect=W / H), use_bvh=True)
        want = b.present(p)[::-1]                                   # PNG rows are top-down
    assert np.array_equal(outs["tex"], want)
    r = subprocess.run(base[:1] + ["--texture", str(tmp_path / "t.png")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--texture takes one --obj" in r.stderr
