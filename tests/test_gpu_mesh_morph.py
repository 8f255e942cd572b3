"""Morph targets of the dynamic mesh on the device.  Contract: after mesh_morph() the destination -- the positions, or the rest
array the skin reads -- is, bit for bit, what morph_positions (rt_morph_positions, pinned to numpy by tests/test_mesh_morph_host.py) computes from the
base positions, the targets and the weight table as it stood when the call was made; skins, rebuilds, refits, bound raster draws, frames and queries
then read it as they read any other positions, in call order, wherever frames have moved stream() in between.  Every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import opengl_raytracing_amd as rt
import raster_ref as rr
import scenes
from test_gpu_dynamic_mesh import _assert_same_scene, _mesh, _ntris
from test_gpu_mesh_parts import _refitted, _uploaded
from test_gpu_mesh_refit import _set_qnodes
from test_gpu_mesh_skin import IDENT, _dev, _indices, _on_stream, _read, _same, _skinned_mesh
from test_gpu_raster_dynamic import DRAW_MODEL, _same_frame, _view_proj
from test_mesh_morph_host import FP, I32P, N_PATTERNS, TARGETS, U32P, VERTS, broken_targets, morph_targets, morph_weights
from test_mesh_skin_host import bone_mats, rest_positions

pytestmark = pytest.mark.gpu


def _set_weights_in_ranges(b, w):
    """The table from the host in three sub-ranges, the middle one first."""
    n = w.shape[0]
    cuts = sorted({0, n // 3, (2 * n) // 3, n})
    runs = list(zip(cuts[:-1], cuts[1:]))
    for lo, hi in runs[1:2] + runs[:1] + runs[2:]:
        b.mesh_set_morph_weights(w[lo:hi], first=lo)


def _write_weights(b, w, on_device):
    if on_device:
        _on_stream(b, lambda d: b.mesh_morph_weights().copy_(d), w.reshape(-1, 1))      # the table written on the device ...
    else:
        _set_weights_in_ranges(b, w)                                                     # ... or from the host in sub-ranges


@functools.lru_cache(maxsize=None)
def _region_mesh(mesh, nt=40):
    """(positions, indices, target_first, vert_idx, deltas) of one mesh, read only: nt targets, each a region of the mesh -- the vertices within a
    quarter of the extent of one of them, pushed along a direction of the target's own with a smooth falloff.  Regions overlap."""
    v, f = _mesh(mesh)
    v = np.ascontiguousarray(v, np.float32)
    f = np.ascontiguousarray(f, np.uint32).reshape(-1)
    ext = np.float32((v.max(0) - v.min(0)).max())
    rng = np.random.default_rng(40)
    dense = np.zeros((nt, v.shape[0], 3), np.float32)
    for t in range(nt):
        c = v[(t * 257) % v.shape[0]]
        r = np.linalg.norm(v - c, axis=1).astype(np.float32) / (np.float32(0.25) * ext)
        fall = np.where(r < 1, (np.float32(1) - r * r) ** 2, np.float32(0)).astype(np.float32)
        dense[t] = fall[:, None] * (rng.normal(0, 1, 3).astype(np.float32) * np.float32(0.05) * ext)
    tf, vi, d = rt.morph_targets_from_dense(dense)
    for a in (v, f, tf, vi, d):
        a.setflags(write=False)
    return v, f, tf, vi, d


def _info_dict(i):
    return {k: getattr(i, k) for k, _ in rt.RtMorphInfo._fields_}


# ---------------------------------------------------------------- 1: positions
@pytest.mark.parametrize("nv", VERTS + ("bunny",))
def test_positions_equal_the_host_definition(nv):
    if nv == "bunny":
        base0, f, *region = _region_mesh("bunny")
        assert _ntris(f) == 20480
        cases = [(40, 0, tuple(region))]
    else:
        base0, f = rest_positions(nv), _indices(nv)
        cases = [(nt, o, morph_targets(nv, nt, o)) for nt in TARGETS for o in range(N_PATTERNS if nv == 1 else 1)]      # a single vertex meets every weight pattern in turn
    n = base0.shape[0]
    with rt.Renderer() as b:
        b.mesh_upload(base0, f)
        for i, (nt, offset, (tf, vi, d)) in enumerate(cases):
            b.mesh_morph_upload(tf, vi, d, base=base0)
            ptr, nbytes = b.mesh_morph_weights(as_torch=False)
            assert ptr and nbytes == nt * 4 and b.mesh_morph_base(as_torch=False)[1] == n * 12
            assert tuple(b.mesh_morph_weights().shape) == (nt, 1) and tuple(b.mesh_morph_base().shape) == (n, 3)
            assert not _read(b, b.mesh_morph_weights).view(np.uint32).any()                  # all zero after the upload
            assert _same(_read(b, b.mesh_morph_base), base0)
            assert _info_dict(b.mesh_morph_info()) == _info_dict(rt.debug_morph_pack(n, tf, vi, d)["info"])
            b.mesh_set_positions(base0 + np.float32(1.0))
            b.mesh_morph()
            assert _same(_read(b, b.mesh_positions), base0), (nv, nt, "zero weights")        # every entry skipped: the base, -0 included
            for step in range(2):
                w = morph_weights(nt, offset, step)
                _write_weights(b, w, on_device=(i + step) % 2 == 1)
                assert b.mesh_morph() is None
                got = _read(b, b.mesh_positions)
                want = rt.morph_positions(base0, tf, vi, d, w)
                assert _same(got, want), (nv, nt, offset, step, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
                assert _same(_read(b, b.mesh_morph_weights).reshape(-1), w) and _same(_read(b, b.mesh_morph_base), base0)
            if n >= 63 and (np.repeat(w, np.diff(tf)) != 0).any():      # an entry is left unskipped
                assert not _same(got, base0)
        # base=None: a snapshot of the positions as they stand on the stream, here new ones still in flight
        nt, offset, (tf, vi, d) = cases[-1]
        w = morph_weights(nt, 3, 7)
        base1 = (base0 * np.float32(1.25) + np.float32(0.5)).astype(np.float32)
        b.mesh_set_positions(base1)
        b.mesh_morph_upload(tf, vi, d)
        assert _same(_read(b, b.mesh_morph_base), base1)
        b.mesh_set_morph_weights(w)
        b.mesh_morph()
        snap = _read(b, b.mesh_positions)
        assert _same(snap, rt.morph_positions(base1, tf, vi, d, w))
        # with a skin, base=None snapshots the rest array, not the positions
        bi = np.zeros((n, 4), np.uint16)
        sw = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
        b.mesh_skin_upload(bi, sw, 1, rest=base0)
        b.mesh_morph_upload(tf, vi, d)
        assert _same(_read(b, b.mesh_morph_base), base0) and not _same(_read(b, b.mesh_positions), base0)
        b.mesh_set_morph_weights(w)
        b.mesh_morph()                                                                       # to the positions; the rest array stays
        assert _same(_read(b, b.mesh_positions), rt.morph_positions(base0, tf, vi, d, w)) and _same(_read(b, b.mesh_rest_positions), base0)


# ---------------------------------------------------------------- 2: morph, then skin
@pytest.mark.parametrize("mesh", [1000, "bunny"])
def test_morph_to_rest_then_skin(mesh):
    nb = 300
    v, f, bi, sw = _skinned_mesh(mesh, nb)
    _, _, tf, vi, d = _region_mesh(mesh)
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_skin_upload(bi, sw, nb, rest=v)
        b.mesh_morph_upload(tf, vi, d, base=v)
        for k in range(3):
            w, bones = morph_weights(40, k, k), bone_mats(nb, step=k)
            _write_weights(b, w, on_device=k % 2 == 1)
            b.mesh_set_bones(bones)
            b.mesh_morph(to="rest")
            b.mesh_skin()
            morphed = rt.morph_positions(v, tf, vi, d, w)
            assert _same(_read(b, b.mesh_positions), rt.skin_positions(morphed, bi, sw, bones)), (mesh, k)
            assert _same(_read(b, b.mesh_rest_positions), morphed) and not _same(morphed, v)
            assert _same(_read(b, b.mesh_morph_base), v)                                     # the morph's own base is not what it writes


# ---------------------------------------------------------------- 3: rebuild and refit after a morph
@pytest.mark.parametrize("qnodes", [None, "0", "2"])
@pytest.mark.parametrize("mesh", [1000, "bunny"])
def test_rebuild_and_refit_after_a_morph(monkeypatch, mesh, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    v, f, tf, vi, d = _region_mesh(mesh)
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_morph_upload(tf, vi, d, base=v)
        w = morph_weights(40)
        b.mesh_set_morph_weights(w)
        b.mesh_morph()                                             # before the first rebuild: no tree is needed
        b.mesh_rebuild()
        a, ng, tg = _uploaded(rt.gather_triangles(rt.morph_positions(v, tf, vi, d, w), f, IDENT))       # the host route in a fresh context
        with a:
            _assert_same_scene(a, b, (mesh, qnodes, "rebuild"))
        order = b.mesh_order(as_torch=False)
        for k in range(1, 6):
            w = morph_weights(40, k, k)
            _write_weights(b, w, on_device=k % 2 == 0)
            b.mesh_morph()
            b.mesh_refit()
            r, _, _ = _refitted(ng, tg, order, rt.gather_triangles(rt.morph_positions(v, tf, vi, d, w), f, IDENT))
            with r:
                _assert_same_scene(r, b, (mesh, qnodes, "refit", k))
        assert b.mesh_info().rebuilds == 1 and b.mesh_refit_count() == (5, 5)


# ---------------------------------------------------------------- 4: ordering across lanes
def test_call_order_holds_across_lanes(monkeypatch):
    """set_morph_weights, render_frame, morph, render_frame, mesh_refit, trace_rays -- eight steps, each call on whatever lane stream() has reached,
    without a host synchronise; scene, positions and every step's hits equal those of a run that synchronises after every call."""
    _set_qnodes(monkeypatch, "0")                                  # no quantised form: the refit has no host wait of its own
    v, f, tf, vi, d = _region_mesh("bunny")
    W, H = 96, 64
    faces = scenes.tiny_env(8)
    p = rt.default_render_params()
    p.sppPerFrame = 1
    cam = scenes.camera("default", aspect=W / H)
    L = rt.bvh_layout(_ntris(f))
    rng = np.random.default_rng(5)
    t9 = rt.gather_triangles(v, f, IDENT)
    k = rng.integers(0, t9.shape[0], 2048)
    target = (t9[k, 0:3] + (t9[k, 3:6] + t9[k, 6:9]) / 3).astype(np.float32)
    org = (target + rng.normal(0, 1, target.shape) * 3).astype(np.float32)
    dirs = target - org
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    dev = _dev()
    o, dd = torch.from_numpy(org).to(dev), torch.from_numpy(dirs).to(dev)
    torch.cuda.synchronize()

    def run(sync):
        with rt.Renderer() as b:
            b.upload_env(faces)
            b.resize(W, H)
            b.mesh_upload(v, f)
            b.mesh_morph_upload(tf, vi, d, base=v)
            b.mesh_rebuild()
            b.synchronize()
            wait = b.synchronize if sync else (lambda: None)
            hits, streams = [], set()
            for step in range(8):
                u = rt.frame_uniforms(p, cam, W, H, 2 * step, True, L.nNodes, L.nTris)
                b.mesh_set_morph_weights(morph_weights(40, step, step + 1) * np.float32(4.0)); wait()
                b.render_frame(u); wait()
                streams.add(b.stream())
                b.mesh_morph(); wait()
                b.render_frame(u); wait()
                streams.add(b.stream())
                b.mesh_refit(); wait()
                hits.append(b.trace_rays(o, dd)); wait()
            mi = b.mesh_info()
            assert mi.hostSyncs == 0 and mi.rebuilds == 1 and b.mesh_refit_count() == (8, 8)
            b.synchronize()
            scene = {name: b.debug_read_scene(name) for name in rt.SCENE_ARRAYS}
            return scene, b.mesh_positions().cpu().numpy().copy(), [h.record.cpu().numpy().copy() for h in hits], streams

    scene_s, pos_s, hits_s, _ = run(True)
    scene_a, pos_a, hits_a, streams = run(False)
    assert len(streams) > 1, "the frames did not move stream(): the case does not cross lanes"
    assert _same(pos_s, rt.morph_positions(v, tf, vi, d, morph_weights(40, 7, 8) * np.float32(4.0))) and _same(pos_a, pos_s)
    for name in scene_s:
        assert np.array_equal(scene_a[name], scene_s[name]), name
    for step, (x, y) in enumerate(zip(hits_a, hits_s)):
        assert _same(x, y), step
        assert (x.view(np.int32)[:, 1] >= 0).any(), step
    assert not _same(hits_s[0], hits_s[7])                          # the steps do differ


# ---------------------------------------------------------------- 5: raster
def test_bound_raster_draws_read_the_morphed_positions():
    W, H, SLOT = 97, 61, 1
    v, f, tf, vi, d = _region_mesh(1000)
    A, B = morph_weights(40, 0, 1) * np.float32(3.0), morph_weights(40, 2, 5) * np.float32(3.0)
    pa, pb = rt.morph_positions(v, tf, vi, d, A), rt.morph_positions(v, tf, vi, d, B)
    view, proj = _view_proj("outside")
    draws = [rt.raster_draw(SLOT, DRAW_MODEL, (0.9, 0.4, 0.1))]
    p = rt.default_render_params()
    p.sppPerFrame = 1
    cam = scenes.camera("default", aspect=W / H)
    with rt.Renderer() as b:
        b.resize(W, H)
        b.mesh_upload(v, f)
        b.mesh_morph_upload(tf, vi, d)
        b.raster_mesh_dynamic(SLOT)
        frames = {}
        for name, w, pos in (("A", A, pa), ("B", B, pb)):          # a bound draw after a morph == a static slot holding the host-morphed positions
            b.mesh_set_morph_weights(w)
            b.mesh_morph()
            got = b.render_raster(draws, view, proj)
            st = b.raster_stats()
            b.raster_mesh(3, pos, f)
            want = b.render_raster([rt.raster_draw(3, DRAW_MODEL, (0.9, 0.4, 0.1))], view, proj)
            _same_frame(got, want, name)
            s2 = b.raster_stats()
            for key in ("trianglesIn", "trianglesDropped", "trianglesClipped", "trianglesSetUp", "binEntries"):
                assert getattr(st, key) == getattr(s2, key), (name, key)
            frames[name] = got
        assert any((np.asarray(x) != np.asarray(y)).any() for x, y in zip(frames["A"][:3], frames["B"][:3])) and (frames["A"][1] != rr.BACKGROUND).any()
        b.mesh_rebuild()
        b.render_ray(p, cam, use_bvh=True)                         # the first frame runs on the stream stream() starts as: the next one moves it
        for cross_lanes in (False, True):                        # a morph enqueued right after a bound draw does not change that draw
            b.mesh_set_morph_weights(A)
            b.mesh_morph()
            b.synchronize()
            s0 = b.stream()
            b.render_raster_async(draws, view, proj)
            if cross_lanes:
                b.render_ray(p, cam, use_bvh=True)
                assert b.stream() != s0
            b.mesh_set_morph_weights(B)
            b.mesh_morph()
            _same_frame(b.read_raster(), frames["A"], ("in flight", cross_lanes))
            _same_frame(b.render_raster(draws, view, proj), frames["B"], ("after", cross_lanes))


# ---------------------------------------------------------------- 6: counters
@pytest.mark.parametrize("qnodes", ["0", "2"])
def test_no_allocation_no_host_wait(monkeypatch, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    v, f, tf, vi, d = _region_mesh(1000)
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        before = b.mesh_info()
        b.mesh_morph_upload(tf, vi, d, base=v)
        mi0, info = b.mesh_info(), b.mesh_morph_info()
        assert mi0.allocations == before.allocations + 4           # base positions, slice table, records, weight table
        assert info.bytes == info.paddedEntries * 16 + (info.nSlices + 1) * 4 + v.shape[0] * 12 + 40 * 4
        assert mi0.scratchBytes == before.scratchBytes + info.bytes and mi0.hostSyncs == 0
        for k in range(20):
            b.mesh_set_morph_weights(morph_weights(40, k, k))
            b.mesh_morph()
            assert b.mesh_info().hostSyncs == (0 if qnodes == "0" else k)          # the morph itself never waits
            b.mesh_update(rebuild_above=1.5)
            mi = b.mesh_info()
            assert mi.allocations == mi0.allocations and mi.hostSyncs == (0 if qnodes == "0" else k + 1)      # the quantised form's status read alone
        assert _same(_read(b, b.mesh_positions), rt.morph_positions(v, tf, vi, d, morph_weights(40, 19, 19)))
        b.mesh_morph_upload(None, None, None)                      # released: the bytes are given back
        assert b.mesh_info().scratchBytes == before.scratchBytes


# ---------------------------------------------------------------- 7: state and refusals
def test_state_and_refusals():
    nv, nt, nb = 257, 3, 2
    base = rest_positions(nv)
    tf, vi, d = morph_targets(nv, nt)
    w = morph_weights(nt, 2)
    f = _indices(nv)
    bi = np.zeros((nv, 4), np.uint16)
    sw = np.tile(np.array([0.5, 0.5, 0, 0], np.float32), (nv, 1))

    def refused(call, code=rt.RT_ERR_INVALID):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == code
        return str(e.value)

    def morph_calls(b):
        return {"mesh_morph_base": lambda: b.mesh_morph_base(as_torch=False), "mesh_morph_weights": lambda: b.mesh_morph_weights(as_torch=False),
                "mesh_set_morph_weights": lambda: b.mesh_set_morph_weights(w[:1]), "mesh_morph": b.mesh_morph,
                "mesh_morph_rest": lambda: b.mesh_morph(to="rest"), "mesh_morph_info": b.mesh_morph_info}

    L = rt.lib()
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    with rt.Renderer() as b:
        raw = lambda n, t=tf, i=vi, dd=d: L.rt_mesh_morph_upload(b._h, ptr(base, FP), ptr(t, I32P), ptr(i, U32P), ptr(dd, FP), n)
        assert raw(nt) == rt.RT_ERR_INVALID and b"no mesh" in L.rt_last_error(b._h)          # no mesh
        for call in morph_calls(b).values():
            refused(call)
        b.mesh_upload(base, f)
        allocs = b.mesh_info().allocations
        for name, call in morph_calls(b).items():                  # a mesh, no morph
            assert "rt_mesh_morph_upload" in refused(call), name
        for name, (t2, v2, d2, n2) in broken_targets(nv, nt, tf, vi, d).items():
            if n2 == 0:
                continue                                           # nTargets == 0 releases; below
            assert raw(n2, t2, v2, d2) == rt.RT_ERR_INVALID and L.rt_last_error(b._h).startswith(b"rt_mesh_morph_upload: "), name
        assert raw(nt, None) == rt.RT_ERR_INVALID and raw(nt, tf, None) == rt.RT_ERR_INVALID and raw(nt, tf, vi, None) == rt.RT_ERR_INVALID      # a null array
        assert "vertex" in refused(lambda: b.mesh_morph_upload(tf, np.where(vi == vi.max(), nv, vi), d))
        assert "finite" in refused(lambda: b.mesh_morph_upload(tf, vi, np.where(d == d.max(), np.float32(np.inf), d)))
        refused(lambda: b.mesh_morph_upload(tf, vi, d, base=base[:-1]))
        refused(b.mesh_morph)                                      # none of the refused uploads left a morph behind, or allocated
        assert b.mesh_info().allocations == allocs
        b.mesh_morph_upload(tf, vi, d, base=base)
        for first, count in ((nt, 1), (nt - 1, 2), (-1, 1), (0, nt + 1)):                    # a range outside the weight table
            refused(lambda: b.mesh_set_morph_weights(np.ones(count, np.float32), first=first))
        b.mesh_set_morph_weights(w[nt - 1:], first=nt - 1)
        b.mesh_set_morph_weights(w)
        for dst in (2, -1):                                        # an unknown destination
            assert "destination" in refused(lambda: b.mesh_morph(to=dst))
        refused(lambda: b.mesh_morph(to="bones"))
        assert "rt_mesh_skin_upload" in refused(lambda: b.mesh_morph(to="rest"))             # to the rest array without a skin
        b.mesh_morph()
        want = rt.morph_positions(base, tf, vi, d, w)
        assert _same(_read(b, b.mesh_positions), want) and not _same(want, base)
        # a skin upload and a skin release leave the morph alone
        b.mesh_skin_upload(bi, sw, nb, rest=base)
        assert _same(_read(b, b.mesh_morph_weights).reshape(-1), w) and _same(_read(b, b.mesh_morph_base), base)
        b.mesh_morph(to="rest")
        b.mesh_skin()
        assert _same(_read(b, b.mesh_positions), rt.skin_positions(want, bi, sw, np.tile(IDENT, (nb, 1))))
        b.mesh_skin_upload(None, None, 0)
        assert "rt_mesh_skin_upload" in refused(lambda: b.mesh_morph(to="rest"))
        b.mesh_set_positions(base)
        b.mesh_morph()
        assert _same(_read(b, b.mesh_positions), want) and _same(_read(b, b.mesh_morph_weights).reshape(-1), w)
        # a second upload replaces the first: other targets, a weight table of another size, all zero again
        tf2, vi2, d2 = morph_targets(nv, 40, 1)
        w2 = morph_weights(40, 1)
        b.mesh_morph_upload(tf2, vi2, d2, base=base)
        assert b.mesh_morph_info().nTargets == 40 and b.mesh_info().allocations == allocs + 4 + 4 + 4
        assert not _read(b, b.mesh_morph_weights).view(np.uint32).any()
        b.mesh_set_morph_weights(w2)
        b.mesh_morph()
        assert _same(_read(b, b.mesh_positions), rt.morph_positions(base, tf2, vi2, d2, w2))
        b.mesh_morph_upload(tf[:1], vi[:0], d[:0])                 # nTargets == 0 releases the morph, not the mesh
        assert b.mesh_info().nVerts == nv
        for call in morph_calls(b).values():
            refused(call)
        b.mesh_morph_upload(tf, vi, d, base=base)
        b.mesh_upload(base, f)                                     # mesh_upload releases the morph with the mesh
        for call in morph_calls(b).values():
            refused(call)
        b.mesh_morph_upload(tf, vi, d)
        b.mesh_morph()
        nodes, tris12 = rt.build_bvh(rt.gather_triangles(base, f, IDENT))
        b.upload_bvh(nodes, tris12)                                # and so does upload_bvh
        assert raw(nt) == rt.RT_ERR_INVALID and b"no mesh" in L.rt_last_error(b._h)
        for call in morph_calls(b).values():
            refused(call)
        assert b.scene_info().nTris == _ntris(f)
