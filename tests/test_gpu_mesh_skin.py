"""Skinning of the dynamic mesh on the device.  Contract: after mesh_skin() the device positions are, bit for bit, what
skin_positions (rt_skin_positions, pinned to numpy by tests/test_mesh_skin_host.py) computes from the rest positions, the tables and the bone table
as it stood when the call was made; rebuilds, refits, mesh_update, bound raster draws, frames and queries then read those positions as they read any
others, in call order, wherever frames have moved stream() in between.  Every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import opengl_raytracing_amd as rt
import raster_ref as rr
import scenes
from bvh_build_ref import ref_build
from test_gpu_dynamic_mesh import _assert_same_scene, _mesh, _ntris
from test_gpu_mesh_parts import _refitted, _uploaded
from test_gpu_mesh_refit import _set_qnodes
from test_gpu_raster_dynamic import DRAW_MODEL, _same_frame, _view_proj
from test_mesh_skin_host import BONES, N_PATTERNS, VERTS, bone_mats, rest_positions, skin_case, skin_tables

pytestmark = pytest.mark.gpu

IDENT = np.eye(4, dtype=np.float32).reshape(-1)


def _dev():
    return torch.device("cuda", 0)


def _same(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def _indices(nv):
    """Index triples that name every one of nv vertices (a single vertex: one degenerate triangle)."""
    return (np.arange(3 * ((nv + 2) // 3), dtype=np.uint32) % nv).astype(np.uint32)


def _read(b, tensor):
    """A library device array on the host, after everything enqueued so far."""
    b.synchronize()
    return tensor().cpu().numpy().copy()


def _on_stream(b, fn, *host_arrays):
    """fn(*device copies of host_arrays) under torch on the library stream, tied back to torch's own stream."""
    dev = _dev()
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in host_arrays]
    torch.cuda.current_stream(dev).synchronize()
    ext = torch.cuda.ExternalStream(b.stream(), device=dev)
    with torch.cuda.stream(ext):
        fn(*d)
    torch.cuda.current_stream(dev).wait_stream(ext)


def _set_bones_in_ranges(b, bones):
    """The table from the host in three sub-ranges, the middle one first."""
    n = bones.shape[0]
    cuts = sorted({0, n // 3, (2 * n) // 3, n})
    runs = list(zip(cuts[:-1], cuts[1:]))
    for lo, hi in runs[1:2] + runs[:1] + runs[2:]:
        b.mesh_set_bones(bones[lo:hi], first=lo)


# ---------------------------------------------------------------- 1: positions
@pytest.mark.parametrize("nv", VERTS + ("bunny",))
def test_positions_equal_the_host_definition(nv):
    if nv == "bunny":
        v, f = _mesh("bunny")
        rest0 = np.ascontiguousarray(v, np.float32)
        f = np.ascontiguousarray(f, np.uint32).reshape(-1)
        assert _ntris(f) == 20480
    else:
        rest0, f = rest_positions(nv), _indices(nv)
    n = rest0.shape[0]
    with rt.Renderer() as b:
        b.mesh_upload(rest0, f)
        for i, nb in enumerate(BONES):
            for offset in range(N_PATTERNS if n < N_PATTERNS else 1):      # a single vertex meets every weight pattern in turn
                bi, w = skin_tables(n, nb, offset)
                bones = bone_mats(nb, step=i)
                b.mesh_skin_upload(bi, w, nb, rest=rest0)
                ptr, nbytes = b.mesh_bones(as_torch=False)
                assert ptr and ptr % 64 == 0 and nbytes == nb * 64
                assert tuple(b.mesh_bones().shape) == (nb, 16) and tuple(b.mesh_rest_positions().shape) == (n, 3)
                assert _same(_read(b, b.mesh_bones), np.tile(IDENT, (nb, 1)))           # identities after the upload
                assert _same(_read(b, b.mesh_rest_positions), rest0)
                b.mesh_skin()
                assert _same(_read(b, b.mesh_positions), rt.skin_positions(rest0, bi, w, np.tile(IDENT, (nb, 1)))), (nv, nb, "identities")
                if i % 2:
                    _on_stream(b, lambda d: b.mesh_bones().copy_(d), bones)              # the table written on the device ...
                else:
                    _set_bones_in_ranges(b, bones)                                       # ... or from the host in sub-ranges
                assert b.mesh_skin() is None
                got = _read(b, b.mesh_positions)
                want = rt.skin_positions(rest0, bi, w, bones)
                assert _same(got, want), (nv, nb, offset, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
                assert _same(_read(b, b.mesh_bones), bones) and _same(_read(b, b.mesh_rest_positions), rest0)
                if n >= 63:
                    assert not _same(got, rest0)
        # rest=None: a snapshot of the positions as they stand on the stream, here new ones still in flight
        rest1 = (rest0 * np.float32(1.25) + np.float32(0.5)).astype(np.float32)
        b.mesh_set_positions(rest1)
        bi, w = skin_tables(n, 300)
        bones = bone_mats(300, step=7)
        b.mesh_skin_upload(bi, w, 300)
        assert _same(_read(b, b.mesh_rest_positions), rest1)
        b.mesh_set_bones(bones)
        b.mesh_skin()
        snap = _read(b, b.mesh_positions)
        assert _same(snap, rt.skin_positions(rest1, bi, w, bones))
        b.mesh_skin_upload(bi, w, 300, rest=rest1)                                       # against explicit rest positions
        b.mesh_set_bones(bones)
        b.mesh_skin()
        assert _same(_read(b, b.mesh_positions), snap)


# ---------------------------------------------------------------- 2: rebuild and refit after a skin
@functools.lru_cache(maxsize=None)
def _skinned_mesh(mesh, nb=300):
    """(rest, indices, bone_idx, weights) of one mesh, read only."""
    v, f = _mesh(mesh)
    v = np.ascontiguousarray(v, np.float32)
    f = np.ascontiguousarray(f, np.uint32).reshape(-1)
    bi, w = skin_tables(v.shape[0], nb)
    for a in (v, f, bi, w):
        a.setflags(write=False)
    return v, f, bi, w


@pytest.mark.parametrize("qnodes", [None, "0", "2"])
@pytest.mark.parametrize("mesh", [1000, "bunny"])
def test_rebuild_and_refit_after_a_skin(monkeypatch, mesh, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    nb = 300
    v, f, bi, w = _skinned_mesh(mesh, nb)
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_skin_upload(bi, w, nb, rest=v)
        bones = bone_mats(nb)
        b.mesh_set_bones(bones)
        b.mesh_skin()                                              # before the first rebuild: no tree is needed
        b.mesh_rebuild()
        t9 = rt.gather_triangles(rt.skin_positions(v, bi, w, bones), f, IDENT)
        a, ng, tg = _uploaded(t9)
        with a:
            _assert_same_scene(a, b, (mesh, qnodes, "rebuild"))
        order = b.mesh_order(as_torch=False)
        for k in range(1, 6):
            bones = bone_mats(nb, step=k)
            if k % 2:
                b.mesh_set_bones(bones)
            else:
                _on_stream(b, lambda d: b.mesh_bones().copy_(d), bones)
            b.mesh_skin()
            b.mesh_refit()
            r, _, _ = _refitted(ng, tg, order, rt.gather_triangles(rt.skin_positions(v, bi, w, bones), f, IDENT))
            with r:
                _assert_same_scene(r, b, (mesh, qnodes, "refit", k))
        assert b.mesh_info().rebuilds == 1 and b.mesh_refit_count() == (5, 5)


# ---------------------------------------------------------------- 3: mesh_update through a growing bend
BEND_ABOVE = 1.15


@functools.lru_cache(maxsize=None)
def _bend_mesh():
    """The small stand-in with two bones blended along x: bone 0 holds the left end, bone 1 the right one."""
    v, f = rt.meshgen.bunny_standin(3)
    v = np.ascontiguousarray(v, np.float32)
    f = np.ascontiguousarray(f, np.uint32).reshape(-1)
    x = v[:, 0]
    t = np.clip((x - x.min()) / (x.max() - x.min()) * np.float32(2.0) - np.float32(0.5), 0, 1).astype(np.float32)
    w = np.zeros((v.shape[0], 4), np.float32)
    w[:, 0], w[:, 1] = np.float32(1.0) - t, t
    bi = np.zeros((v.shape[0], 4), np.uint16)
    bi[:, 1] = 1
    return v, f, bi, w


def _bend_bones(k):
    """Step k of the bend: bone 1 turned about z by 0.4 rad more than at the step before, folding its end of the mesh over the other."""
    a = 0.4 * k
    M = np.eye(4)
    M[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    return np.stack([IDENT, np.ascontiguousarray(M.T, np.float32).reshape(-1)]).astype(np.float32)


def _bend_replay(steps):
    """rt_mesh_update's rule for a caller who synchronises between steps, on the host definitions -> per step (action, nodes12, tris12)."""
    v, f, bi, w = _bend_mesh()
    out, tree, base, latest = [], None, None, None
    for k in range(steps):
        t9 = rt.gather_triangles(rt.skin_positions(v, bi, w, _bend_bones(k)), f, IDENT)
        if tree is None:
            rebuild = True
        elif base.degenerate or latest.degenerate:
            rebuild = False
        else:
            rebuild = latest.cost > float(np.float32(BEND_ABOVE)) * base.cost
        if rebuild:
            tree = ref_build(t9)
            latest = base = rt.bvh_cost(tree[0])
        else:
            n2, t2 = rt.refit_bvh(tree[0], tree[1], tree[2], t9)
            tree = (n2, t2, tree[2])
            latest = rt.bvh_cost(n2)
        out.append(("rebuild" if rebuild else "refit", tree[0], tree[1]))
    return out


def test_mesh_update_through_a_growing_bend(monkeypatch):
    monkeypatch.delenv("RT_QNODES", raising=False)
    v, f, bi, w = _bend_mesh()
    want = _bend_replay(10)
    actions = [x[0] for x in want]
    assert actions[0] == "rebuild" and "rebuild" in actions[2:] and actions.count("refit") >= 3, actions      # the definitions' own sequence has both
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_skin_upload(bi, w, 2, rest=v)
        for k, (action, nodes, tris) in enumerate(want):
            b.mesh_set_bones(_bend_bones(k))
            b.mesh_skin()
            b.synchronize()
            got = b.mesh_update(rebuild_above=BEND_ABOVE)
            assert got == action, (k, got, actions)
            with rt.Renderer() as a:
                a.upload_bvh(nodes, tris)
                _assert_same_scene(a, b, ("bend", k, action))


# ---------------------------------------------------------------- 4: ordering across lanes
def test_call_order_holds_across_lanes(monkeypatch):
    """set_bones, render_frame, skin, render_frame, mesh_refit, trace_rays -- eight steps, each call on whatever lane stream() has reached, without a
    host synchronise; scene, positions and every step's hits equal those of a run that synchronises after every call."""
    _set_qnodes(monkeypatch, "0")                                  # no quantised form: the refit has no host wait of its own
    nb = 64
    v, f, bi, w = _skinned_mesh("bunny", nb)
    W, H = 96, 64
    faces = scenes.tiny_env(8)
    p = rt.default_render_params()
    p.sppPerFrame = 1
    cam = scenes.camera("default", aspect=W / H)
    L = rt.bvh_layout(_ntris(f))
    rng = np.random.default_rng(5)
    t9 = rt.gather_triangles(rt.skin_positions(v, bi, w, bone_mats(nb)), f, IDENT)
    k = rng.integers(0, t9.shape[0], 2048)
    target = (t9[k, 0:3] + (t9[k, 3:6] + t9[k, 6:9]) / 3).astype(np.float32)
    org = (target + rng.normal(0, 1, target.shape) * 3).astype(np.float32)
    dirs = target - org
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    dev = _dev()
    o, d = torch.from_numpy(org).to(dev), torch.from_numpy(dirs).to(dev)
    torch.cuda.synchronize()

    def run(sync):
        with rt.Renderer() as b:
            b.upload_env(faces)
            b.resize(W, H)
            b.mesh_upload(v, f)
            b.mesh_skin_upload(bi, w, nb, rest=v)
            b.mesh_rebuild()
            b.synchronize()
            wait = b.synchronize if sync else (lambda: None)
            hits, streams = [], set()
            for step in range(8):
                u = rt.frame_uniforms(p, cam, W, H, 2 * step, True, L.nNodes, L.nTris)
                b.mesh_set_bones(bone_mats(nb, step=step + 1)); wait()
                b.render_frame(u); wait()
                streams.add(b.stream())
                b.mesh_skin(); wait()
                b.render_frame(u); wait()
                streams.add(b.stream())
                b.mesh_refit(); wait()
                hits.append(b.trace_rays(o, d)); wait()
            mi = b.mesh_info()
            assert mi.hostSyncs == 0 and mi.rebuilds == 1 and b.mesh_refit_count() == (8, 8)
            b.synchronize()
            scene = {name: b.debug_read_scene(name) for name in rt.SCENE_ARRAYS}
            return scene, b.mesh_positions().cpu().numpy().copy(), [h.record.cpu().numpy().copy() for h in hits], streams

    scene_s, pos_s, hits_s, _ = run(True)
    scene_a, pos_a, hits_a, streams = run(False)
    assert len(streams) > 1, "the frames did not move stream(): the case does not cross lanes"
    assert _same(pos_s, rt.skin_positions(v, bi, w, bone_mats(nb, step=8))) and _same(pos_a, pos_s)
    for name in scene_s:
        assert np.array_equal(scene_a[name], scene_s[name]), name
    for step, (x, y) in enumerate(zip(hits_a, hits_s)):
        assert _same(x, y), step
        assert (x.view(np.int32)[:, 1] >= 0).any(), step
    assert not _same(hits_s[0], hits_s[7])                          # the steps do differ


# ---------------------------------------------------------------- 5: raster
def test_bound_raster_draws_read_the_skinned_positions():
    W, H, SLOT = 97, 61, 1
    v, f = _mesh(1000)
    v = np.ascontiguousarray(v, np.float32)
    bi, w = skin_tables(v.shape[0], 2)
    A, B = bone_mats(2, step=1), bone_mats(2, step=5)
    pa, pb = rt.skin_positions(v, bi, w, A), rt.skin_positions(v, bi, w, B)
    view, proj = _view_proj("outside")
    draws = [rt.raster_draw(SLOT, DRAW_MODEL, (0.9, 0.4, 0.1))]
    p = rt.default_render_params()
    p.sppPerFrame = 1
    cam = scenes.camera("default", aspect=W / H)
    with rt.Renderer() as b:
        b.resize(W, H)
        b.mesh_upload(v, f)
        b.mesh_skin_upload(bi, w, 2)
        b.raster_mesh_dynamic(SLOT)
        frames = {}
        for name, bones, pos in (("A", A, pa), ("B", B, pb)):      # a bound draw after a skin == a static slot holding the host-skinned positions
            b.mesh_set_bones(bones)
            b.mesh_skin()
            got = b.render_raster(draws, view, proj)
            st = b.raster_stats()
            b.raster_mesh(3, pos, f)
            want = b.render_raster([rt.raster_draw(3, DRAW_MODEL, (0.9, 0.4, 0.1))], view, proj)
            _same_frame(got, want, name)
            s2 = b.raster_stats()
            for key in ("trianglesIn", "trianglesDropped", "trianglesClipped", "trianglesSetUp", "binEntries"):
                assert getattr(st, key) == getattr(s2, key), (name, key)
            frames[name] = got
        assert (frames["A"][1] != frames["B"][1]).any() and (frames["A"][1] != rr.BACKGROUND).any()
        b.mesh_rebuild()
        b.render_ray(p, cam, use_bvh=True)                         # the first frame runs on the stream stream() starts as: the next one moves it
        for cross_lanes in (False, True):                        # a skin enqueued right after a bound draw does not change that draw
            b.mesh_set_bones(A)
            b.mesh_skin()
            b.synchronize()
            s0 = b.stream()
            b.render_raster_async(draws, view, proj)
            if cross_lanes:
                b.render_ray(p, cam, use_bvh=True)
                assert b.stream() != s0
            b.mesh_set_bones(B)
            b.mesh_skin()
            _same_frame(b.read_raster(), frames["A"], ("in flight", cross_lanes))
            _same_frame(b.render_raster(draws, view, proj), frames["B"], ("after", cross_lanes))


# ---------------------------------------------------------------- 6: counters
@pytest.mark.parametrize("qnodes", ["0", "2"])
def test_no_allocation_no_host_wait(monkeypatch, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    nb = 300
    v, f, bi, w = _skinned_mesh(1000, nb)
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        before = b.mesh_info()
        b.mesh_skin_upload(bi, w, nb, rest=v)
        mi0 = b.mesh_info()
        assert mi0.allocations == before.allocations + 4           # rest positions, indices, weights, bone table
        assert mi0.scratchBytes == before.scratchBytes + v.shape[0] * (12 + 8 + 16) + nb * 64 and mi0.hostSyncs == 0
        for k in range(20):
            b.mesh_set_bones(bone_mats(nb, step=k))
            b.mesh_skin()
            assert b.mesh_info().hostSyncs == (0 if qnodes == "0" else k)          # the skin itself never waits
            b.mesh_update(rebuild_above=1.5)
            mi = b.mesh_info()
            assert mi.allocations == mi0.allocations and mi.hostSyncs == (0 if qnodes == "0" else k + 1)      # the quantised form's status read alone
        assert _same(_read(b, b.mesh_positions), rt.skin_positions(v, bi, w, bone_mats(nb, step=19)))
        b.mesh_skin_upload(None, None, 0)                          # released: the bytes are given back
        assert b.mesh_info().scratchBytes == before.scratchBytes


# ---------------------------------------------------------------- 7: state and refusals
def test_state_and_refusals():
    nv, nb = 257, 300
    rest, bi, w, bones = skin_case(nv, nb)
    f = _indices(nv)

    def refused(call, code=rt.RT_ERR_INVALID):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == code
        return str(e.value)

    def skin_calls(b):
        return {"mesh_bones": lambda: b.mesh_bones(as_torch=False), "mesh_set_bones": lambda: b.mesh_set_bones(bones[:1]),
                "mesh_rest_positions": lambda: b.mesh_rest_positions(as_torch=False), "mesh_skin": b.mesh_skin}

    L = rt.lib()
    fp, u16 = C.POINTER(C.c_float), C.POINTER(C.c_uint16)
    with rt.Renderer() as b:
        raw = lambda n, i=bi, ww=w: L.rt_mesh_skin_upload(b._h, rest.ctypes.data_as(fp), None if i is None else i.ctypes.data_as(u16),
                                                          None if ww is None else ww.ctypes.data_as(fp), n)
        assert raw(nb) == rt.RT_ERR_INVALID and b"no mesh" in L.rt_last_error(b._h)        # no mesh
        for call in skin_calls(b).values():
            refused(call)
        b.mesh_upload(rest, f)
        allocs = b.mesh_info().allocations
        for name, call in skin_calls(b).items():                   # a mesh, no skin
            assert "rt_mesh_skin_upload" in refused(call), name
        bad = bi.copy(); bad[200, 2] = nb
        w0 = w.copy(); w0[200, 2] = 0.0
        assert "bone" in refused(lambda: b.mesh_skin_upload(bad, w0, nb, rest=rest))       # a bad index under a zero weight
        for x in (np.nan, np.inf):
            wn = w.copy(); wn[3, 1] = x
            assert "finite" in refused(lambda: b.mesh_skin_upload(bi, wn, nb, rest=rest))
        assert raw(-1) == rt.RT_ERR_INVALID and raw(rt.RT_MAX_MESH_BONES + 1) == rt.RT_ERR_INVALID      # nBones out of range
        assert raw(nb, None) == rt.RT_ERR_INVALID and raw(nb, bi, None) == rt.RT_ERR_INVALID            # a null table
        refused(b.mesh_skin)                                       # none of the refused uploads left a skin behind, or allocated
        assert b.mesh_info().allocations == allocs
        b.mesh_skin_upload(bi, w, nb, rest=rest)
        for first, count in ((nb, 1), (nb - 1, 2), (-1, 1), (0, nb + 1)):                  # a range outside the bone table
            refused(lambda: b.mesh_set_bones(bone_mats(count), first=first))
        b.mesh_set_bones(bones[nb - 1:], first=nb - 1)
        b.mesh_set_bones(bones)
        b.mesh_skin()
        want = rt.skin_positions(rest, bi, w, bones)
        assert _same(_read(b, b.mesh_positions), want)
        other = (rest + np.float32(2.0)).astype(np.float32)
        b.mesh_set_positions(other)                                # legal after a skin upload ...
        assert _same(_read(b, b.mesh_positions), other)
        b.mesh_skin()                                              # ... and the next skin overwrites it
        assert _same(_read(b, b.mesh_positions), want)
        morph = (rest * np.float32(0.5)).astype(np.float32)        # the rest array written on the stream: what a morph target does
        _on_stream(b, lambda d: b.mesh_rest_positions().copy_(d), morph)
        b.mesh_skin()
        assert _same(_read(b, b.mesh_positions), rt.skin_positions(morph, bi, w, bones))
        b.mesh_skin_upload(None, None, 0)                          # nBones == 0 releases the skin, not the mesh
        assert b.mesh_info().nVerts == nv
        for call in skin_calls(b).values():
            refused(call)
        b.mesh_skin_upload(bi, w, nb, rest=rest)
        b.mesh_upload(rest, f)                                     # mesh_upload releases the skin with the mesh
        for call in skin_calls(b).values():
            refused(call)
        b.mesh_skin_upload(bi, w, nb)
        b.mesh_skin()
        nodes, tris12 = rt.build_bvh(rt.gather_triangles(rest, f, IDENT))
        b.upload_bvh(nodes, tris12)                                # and so does upload_bvh
        assert raw(nb) == rt.RT_ERR_INVALID and b"no mesh" in L.rt_last_error(b._h)
        for call in skin_calls(b).values():
            refused(call)
        assert b.scene_info().nTris == _ntris(f)
