"""Parts of the dynamic mesh: a mesh is a list of parts, each with its own model matrix on the device.  Contracts, all bit for bit:
after mesh_rebuild_parts() the context's scene is what gather_triangles_parts -> build_bvh_gpu -> upload_bvh installs in a fresh context (route A);
after mesh_refit_parts() it is what upload_bvh installs from refit_bvh(route A's arrays of the last rebuild, mesh_order's order,
gather_triangles_parts(...)); mesh_hit_parts maps a hit's prim to (part, triangle of the part) as searchsorted(part_first, order[prim]) does."""
import ctypes as C
import functools

import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scenes
from bvh_build_ref import ref_build
from test_gpu_dynamic_mesh import _assert_same_scene, _have_torch, _mesh, _ntris, _step_model
from test_gpu_mesh_refit import COORDS, _displace, _set_qnodes, _sinus
from test_mesh_parts_host import part_models, split, splits_for

pytestmark = pytest.mark.gpu

CASES = [(n, s) for n in (1, 9, 17, 100, 1000) for s in splits_for(n)] + [("bunny", "equal40")]
QNODES = [None, "2", "0"]


def _part_first(mesh, name, n):
    return np.linspace(0, n, 41).astype(np.int32) if name == "equal40" else split(name, n)


@functools.lru_cache(maxsize=None)
def _case(mesh, name):
    """(positions, indices, part_first, models, route A's nine-float array, ref_build's (nodes12, tris12, order) of it): computed once, read only."""
    v, f = _mesh(mesh)
    v = np.ascontiguousarray(v, np.float32)
    pf = _part_first(mesh, name, _ntris(f))
    models = part_models(pf.size - 1)
    t9 = rt.gather_triangles_parts(v, f, pf, models)
    out = (v, f, pf, models, t9, ref_build(t9))
    for a in (v, f, pf, models, t9) + tuple(out[5]):
        a.setflags(write=False)
    return out


def _uploaded(t9):
    """Route A: a fresh context with build_bvh_gpu's arrays of t9 uploaded -> (renderer, nodes12, tris12)."""
    r = rt.Renderer()
    ng, tg = r.build_bvh_gpu(t9)
    r.upload_bvh(ng, tg)
    return r, ng, tg


def _refitted(ng, tg, order, t9):
    n2, t2 = rt.refit_bvh(ng, tg, order, t9)
    r = rt.Renderer()
    r.upload_bvh(n2, t2)
    return r, n2, t2


def _write_matrices(b, sel, new):
    """Matrices new[k] into entries sel[k] of the table: on the device through mesh_part_matrices() on the library stream when torch is present, else
    mesh_set_part_matrices with sub-ranges."""
    new = np.ascontiguousarray(new, np.float32).reshape(-1, 16)
    if _have_torch():
        import torch
        dev = torch.device("cuda", 0)
        d = torch.from_numpy(new).to(dev)
        ix = torch.from_numpy(np.asarray(sel, np.int64)).to(dev)
        torch.cuda.current_stream(dev).synchronize()
        ext = torch.cuda.ExternalStream(b.stream(), device=dev)
        with torch.cuda.stream(ext):
            b.mesh_part_matrices().index_copy_(0, ix, d)
        torch.cuda.current_stream(dev).wait_stream(ext)      # `d` and `ix` stay tied to torch's own stream
    else:
        runs = np.split(np.arange(len(sel)), np.flatnonzero(np.diff(sel) != 1) + 1)
        for run in runs:
            b.mesh_set_part_matrices(new[run], first=int(sel[run[0]]))


def _same(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def _want_parts(pf, order, prim):
    """The host formula: (-1, -1) for a prim outside [0, nTris), else the part whose range holds order[prim] and the offset in it."""
    prim = np.asarray(prim).astype(np.int64)
    ok = (prim >= 0) & (prim < order.size)
    t = order[np.where(ok, prim, 0)].astype(np.int64)
    part = np.searchsorted(pf, t, "right") - 1
    return np.where(ok, part, -1).astype(np.int32), np.where(ok, t - pf[part], -1).astype(np.int32)


# ---------------------------------------------------------------- 1: array identity, rebuild
@pytest.mark.parametrize("qnodes", QNODES)
@pytest.mark.parametrize("mesh,name", CASES)
def test_array_identity_rebuild(monkeypatch, mesh, name, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    v, f, pf, models, t9, (rn, rt12, rorder) = _case(mesh, name)
    with rt.Renderer() as b:
        b.mesh_upload_parts(v, f, pf)
        assert np.array_equal(b.mesh_parts(), pf)
        b.mesh_set_part_matrices(models)
        assert b.mesh_rebuild_parts() is None
        a, ng, tg = _uploaded(t9)
        with a:
            info = _assert_same_scene(a, b, (mesh, name, qnodes))
            if qnodes == "2" and _ntris(f) > 8:
                assert a.debug_read_scene("qnodes4").size > 0 or info.flags & rt.RT_SCENE_QNODES_REJECTED
            if qnodes == "0":
                assert a.debug_read_scene("qnodes4").size == 0
        assert np.array_equal(b.mesh_order(as_torch=False), rorder)
        assert b.mesh_info().rebuilds == 1
        if (mesh, name) == (100, "uneven"):       # the numpy definition's own arrays in a fresh context
            with rt.Renderer() as r:
                r.upload_bvh(rn, rt12)
                _assert_same_scene(r, b, (mesh, name, qnodes, "ref_build"))


# ---------------------------------------------------------------- 2: array identity, refit
@pytest.mark.parametrize("qnodes", QNODES)
@pytest.mark.parametrize("mesh,name", CASES)
def test_array_identity_refit(monkeypatch, mesh, name, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    v, f, pf, models, t9, (_, _, order) = _case(mesh, name)
    k = pf.size - 1
    with rt.Renderer() as b:
        b.mesh_upload_parts(v, f, pf)
        b.mesh_set_part_matrices(models)
        b.mesh_rebuild_parts()
        a, ng, tg = _uploaded(t9)
        with a:
            assert b.mesh_refit_parts() is None                  # (a) nothing moved: the rebuild's own arrays
            _assert_same_scene(a, b, (mesh, name, qnodes, "a"))
        assert np.array_equal(b.mesh_order(as_torch=False), order)

        def check(step, want9):
            r, _, _ = _refitted(ng, tg, order, want9)
            with r:
                _assert_same_scene(r, b, (mesh, name, qnodes, step))

        sel = np.arange(1, k, 2) if k > 1 else np.arange(1)      # (b) new matrices for every second part, written on the device
        cur = models.copy()
        cur[sel] = part_models(k, shift=k + 3)[sel]
        _write_matrices(b, sel, cur[sel])
        b.mesh_refit_parts()
        check("b", rt.gather_triangles_parts(v, f, pf, cur))
        pos = _displace(b, v, _sinus(v))                         # (c) the positions deformed as well
        b.mesh_refit_parts()
        check("c", rt.gather_triangles_parts(pos, f, pf, cur))
        M = _step_model(2)                                       # (d) one matrix for everything on the same mesh, then the parts again
        b.mesh_refit(M)
        check("d single", rt.gather_triangles(pos, f, M))
        b.mesh_refit_parts()
        check("d parts", rt.gather_triangles_parts(pos, f, pf, cur))
        assert b.mesh_info().rebuilds == 1 and b.mesh_refit_count() == (5, 5)
        assert np.array_equal(b.mesh_order(as_torch=False), order)


# ---------------------------------------------------------------- 3: parts that share vertices and coincide
@pytest.mark.parametrize("twins", ["identical", "distinct"])
def test_coinciding_parts(twins):
    v, f1 = _mesh(100)
    v = np.ascontiguousarray(v, np.float32)
    f = np.concatenate([f1, f1])                                  # two parts index the same triangles
    pf = np.array([0, 100, 200], np.int32)
    models = part_models(4)[[3, 3]] if twins == "identical" else part_models(4)[[3, 1]]
    t9 = rt.gather_triangles_parts(v, f, pf, models)
    if twins == "identical":
        assert np.array_equal(t9[:100].view(np.uint32), t9[100:].view(np.uint32))      # every triangle ties with its twin
    _, _, rorder = ref_build(t9)
    a, ng, tg = _uploaded(t9)
    with a, rt.Renderer() as b:
        b.mesh_upload_parts(v, f, pf)
        b.mesh_set_part_matrices(models)
        b.mesh_rebuild_parts()
        _assert_same_scene(a, b, twins)
        order = b.mesh_order(as_torch=False)
        assert np.array_equal(order, rorder)
        b.mesh_refit_parts()
        _assert_same_scene(a, b, (twins, "refit"))
        if twins == "identical":
            rng = np.random.default_rng(3)
            k = rng.integers(0, 200, 256)
            target = (t9[k, 0:3] + (t9[k, 3:6] + t9[k, 6:9]) / 3).astype(np.float32)   # centroids: every ray meets a pair of twins
            org = (target + rng.normal(0, 1, (256, 3)) * 3).astype(np.float32)
            dirs = target - org
            dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
            ha, hb = a.trace_rays(org, dirs), b.trace_rays(org, dirs)
            assert _same(ha.t, hb.t) and _same(ha.prim, hb.prim)
            assert (np.asarray(hb.prim) >= 0).sum() > 200
            parts, tris = b.mesh_hit_parts(hb)
            wp, wt = _want_parts(pf, order, hb.prim)
            assert np.array_equal(parts, wp) and np.array_equal(tris, wt)
            assert (parts >= 0).sum() > 200


# ---------------------------------------------------------------- 4: mesh_upload is one part
def test_mesh_upload_is_one_part():
    v, f = _mesh(100)
    v = np.ascontiguousarray(v, np.float32)
    ident = np.eye(4, dtype=np.float32).reshape(-1)
    M = _step_model(3)
    with rt.Renderer() as b, rt.Renderer() as s:
        b.mesh_upload(v, f)
        s.mesh_upload(v, f)
        assert np.array_equal(b.mesh_parts(), [0, 100])
        ptr, nbytes = b.mesh_part_matrices(as_torch=False)
        assert ptr and nbytes == 64
        if _have_torch():
            tab = b.mesh_part_matrices()
            b.synchronize()
            assert tuple(tab.shape) == (1, 16) and np.array_equal(tab.cpu().numpy().reshape(-1).view(np.uint32), ident.view(np.uint32))
        b.mesh_rebuild_parts()
        s.mesh_rebuild(ident)
        _assert_same_scene(s, b, "identity")
        b.mesh_set_part_matrices([M])
        b.mesh_rebuild_parts()
        s.mesh_rebuild(M)
        _assert_same_scene(s, b, "M")
        b.mesh_refit_parts()
        _assert_same_scene(s, b, "M refit")
        assert np.array_equal(b.mesh_order(as_torch=False), s.mesh_order(as_torch=False))


# ---------------------------------------------------------------- 5: hit -> part
def _three_bunnies():
    """One small bunny stand-in in the position pool, indexed by three parts (shared vertices) that their matrices translate apart."""
    v, f1 = rt.meshgen.bunny_standin(2)
    v = np.ascontiguousarray(v, np.float32)
    n1 = _ntris(f1)
    f = np.concatenate([f1, f1, f1])
    pf = np.array([0, n1, 2 * n1, 3 * n1], np.int32)
    models = np.stack([np.asarray(rt.default_bvh_transform(), np.float32).reshape(-1).copy() for _ in range(3)])
    models[0, 12] -= 1.5
    models[2, 12] += 1.5
    return v, f, pf, models


def test_hit_to_part():
    v, f, pf, models = _three_bunnies()
    n = _ntris(f)
    t9 = rt.gather_triangles_parts(v, f, pf, models)
    W, H = 32, 24
    p = rt.default_render_params()
    cam = scenes.camera("default", aspect=W / H)
    rng = np.random.default_rng(8)
    k = rng.integers(0, n, 1024)
    target = (t9[k, 0:3] + (t9[k, 3:6] + t9[k, 6:9]) / 3).astype(np.float32)
    org = (target + rng.normal(0, 1, (1024, 3)) * 4).astype(np.float32)
    dirs = target - org
    dirs[768:] = rng.normal(0, 1, (256, 3))                       # a quarter of the rays go anywhere: misses among them
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)
    L = rt.bvh_layout(n)
    with rt.Renderer() as b:
        b.resize(W, H)
        b.mesh_upload_parts(v, f, pf)
        b.mesh_set_part_matrices(models)
        b.mesh_rebuild_parts()
        order = b.mesh_order(as_torch=False)
        rows = b.debug_read_scene("tris").view(np.float32).reshape(-1, 12)[:n, COORDS]
        u1 = rt.frame_uniforms(p, cam, W, H, 0, 1, L.nNodes, L.nTris, env_loaded=False)
        uh = rt.frame_uniforms(p, cam, W, H, 0, rt.RT_SCENE_HYBRID, L.nNodes, L.nTris, env_loaded=False)
        batches = {"trace_rays": b.trace_rays(org, dirs), "pick": b.pick(u1, xy), "hybrid": b.trace_scene_rays(uh, org, dirs)}
        own = np.stack([rt.gather_triangles(v, f.reshape(-1, 3)[pf[q]:pf[q + 1]].reshape(-1), models[q]) for q in range(3)])      # [part, tri, 9]
        for what, h in batches.items():
            prim = np.asarray(h.prim)
            parts, tris = b.mesh_hit_parts(h)
            assert parts.dtype == np.int32 and tris.dtype == np.int32 and parts.shape == tris.shape == prim.shape
            wp, wt = _want_parts(pf, order, prim)
            assert np.array_equal(parts, wp) and np.array_equal(tris, wt), what
            assert ((parts == -1) == (prim < 0)).all() and ((tris == -1) == (prim < 0)).all(), what
            hit = prim >= 0
            assert hit.any(), what
            # the part's own gather row for (part, tri) is row prim of the device triangle array
            assert np.array_equal(own[parts[hit], tris[hit]].view(np.uint32), rows[prim[hit]].view(np.uint32)), what
            if _have_torch():
                import torch
                rec = torch.from_numpy(np.ascontiguousarray(h.record)).to(torch.device("cuda", 0))
                tp, tt = b.mesh_hit_parts(rec)
                assert tp.dtype == torch.int32 and tp.is_cuda and np.array_equal(tp.cpu().numpy(), wp) and np.array_equal(tt.cpu().numpy(), wt), what
        prim = np.asarray(batches["trace_rays"].prim)
        assert (prim < 0).any() and set(np.unique(b.mesh_hit_parts(batches["trace_rays"])[0])) == {-1, 0, 1, 2}
        assert (np.asarray(batches["hybrid"].object)[np.asarray(batches["hybrid"].prim) < 0] >= 0).any()      # analytic hits are present
        # records the test forges: one past the last row, and a negative value that is not -1
        rec = np.ascontiguousarray(batches["trace_rays"].record).copy()
        good = int(np.flatnonzero(prim >= 0)[0])
        rec.view(np.int32)[good, 1] = n
        rec.view(np.int32)[good + 1, 1] = -7
        rec.view(np.int32)[good + 2, 1] = n - 1
        parts, tris = b.mesh_hit_parts(rec)
        wp, wt = _want_parts(pf, order, rec.view(np.int32)[:, 1])
        assert (parts[good], tris[good]) == (-1, -1) and (parts[good + 1], tris[good + 1]) == (-1, -1) and parts[good + 2] >= 0
        assert np.array_equal(parts, wp) and np.array_equal(tris, wt)
        assert rt.lib().rt_mesh_hit_parts_host(b._h, C.c_void_p(rec.ctypes.data), 4, None, None) == rt.RT_ERR_INVALID      # both outputs null
        only = np.zeros(rec.shape[0], np.int32)
        assert rt.lib().rt_mesh_hit_parts_host(b._h, C.c_void_p(rec.ctypes.data), rec.shape[0], None, C.c_void_p(only.ctypes.data)) == rt.RT_OK
        assert np.array_equal(only, wt)                                                                                    # one output alone


# ---------------------------------------------------------------- 6: frames
@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel"])
def test_frames_on_a_scene_of_parts(pipeline):
    pl = rt.RT_PIPELINE_AUTO if pipeline == "wavefront" else rt.RT_PIPELINE_MEGAKERNEL
    v, f, pf, models = _three_bunnies()
    t9 = rt.gather_triangles_parts(v, f, pf, models)
    W, H = 120, 80
    faces = scenes.tiny_env(8)
    p = rt.default_render_params()
    p.sppPerFrame = 2
    cam = scenes.camera("default", aspect=W / H)
    with rt.Renderer(pipeline=pl) as a, rt.Renderer(pipeline=pl) as b:
        ng, tg = a.build_bvh_gpu(t9)
        a.upload_bvh(ng, tg)
        b.mesh_upload_parts(v, f, pf)
        b.mesh_set_part_matrices(models)
        b.mesh_rebuild_parts()
        for r in (a, b):
            r.upload_env(faces)
            r.resize(W, H)
        u = rt.frame_uniforms(p, cam, W, H, 0, True, ng.shape[0], tg.shape[0])
        a.render_frame(u)
        b.render_frame(u)
        for x, y, name in zip(a.read_all(), b.read_all(), ("color", "motion", "gpos", "gnrm")):
            assert np.array_equal(x, y), name
        assert np.asarray(b.read_target(2)).any()                 # the parts are in view


# ---------------------------------------------------------------- 7: ordering and accounting
@pytest.mark.parametrize("qnodes", ["0", "2"])
def test_ordering_and_accounting(monkeypatch, qnodes):
    """rebuild_parts, queries, set_part_matrices, refit_parts, queries, a frame -- enqueued back to back; every batch of answers is that of the scene
    that was current when it was enqueued.  With torch the queries take the zero-copy path (no host wait anywhere); without it they synchronise."""
    _set_qnodes(monkeypatch, qnodes)
    v, f, pf, m0 = _three_bunnies()
    m1 = m0.copy()
    m1[1] = _step_model(1)
    m1[2, 13] += 0.4
    W, H = 96, 64
    faces = scenes.tiny_env(8)
    p = rt.default_render_params()
    p.sppPerFrame = 1
    cam = scenes.camera("default", aspect=W / H)
    rng = np.random.default_rng(2)
    centre = np.array([-2.0, 1.5, 0.0], np.float32)
    org = (centre + rng.normal(0, 1, (2048, 3)) * 3).astype(np.float32)
    dirs = centre - org + rng.normal(0, 0.8, org.shape).astype(np.float32)
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    tmax = np.full(org.shape[0], 4.0, np.float32)
    use_torch = _have_torch()
    L = rt.bvh_layout(_ntris(f))
    u = rt.frame_uniforms(p, cam, W, H, 0, True, L.nNodes, L.nTris)

    def queries(r):
        if use_torch:
            import torch
            dev = torch.device("cuda", 0)
            o, d, t = (torch.from_numpy(x).to(dev) for x in (org, dirs, tmax))
            h = r.trace_rays(o, d)
            return h, r.trace_rays(o, d, tmax=t, any_hit=True), (r.mesh_hit_parts(h) if r.mesh_info().nTris else None)
        h = r.trace_rays(org, dirs)
        return h, r.trace_rays(org, dirs, tmax=tmax, any_hit=True), (r.mesh_hit_parts(h) if r.mesh_info().nTris else None)

    def host(q):
        h, occ, hp = q
        c = (lambda x: x.cpu().numpy()) if use_torch else np.asarray
        return c(h.record), c(occ), None if hp is None else (c(hp[0]), c(hp[1]))

    with rt.Renderer() as b:
        b.upload_env(faces)
        b.resize(W, H)
        b.mesh_upload_parts(v, f, pf)
        allocs = b.mesh_info().allocations
        b.mesh_set_part_matrices(m0)
        if use_torch:
            import torch
            torch.zeros(1, device="cuda")         # torch's context and allocator exist before the sequence starts
            torch.cuda.synchronize()
        b.mesh_rebuild_parts()
        q1 = queries(b)
        b.mesh_set_part_matrices(m1[1:], first=1)
        b.mesh_refit_parts()
        q2 = queries(b)
        b.render_frame(u)
        mi = b.mesh_info()
        assert mi.allocations == allocs and mi.rebuilds == 1 and b.mesh_refit_count() == (1, 1)
        assert mi.hostSyncs == (0 if qnodes == "0" else 2)        # RT_QNODES=2: the status-word read of each update, none otherwise
        got = (host(q1), host(q2), b.read_all())
        order = b.mesh_order(as_torch=False)
    a, ng, tg = _uploaded(rt.gather_triangles_parts(v, f, pf, m0))
    with a:
        want1 = host(queries(a))
    r, _, _ = _refitted(ng, tg, order, rt.gather_triangles_parts(v, f, pf, m1))
    with r:
        r.upload_env(faces)
        r.resize(W, H)
        want2 = host(queries(r))
        r.render_frame(u)
        frame = r.read_all()
    for i, (g, w) in enumerate(((got[0], want1), (got[1], want2))):
        assert _same(g[0], w[0]) and _same(g[1], w[1]), i
        wp, wt = _want_parts(pf, order, g[0].view(np.int32)[:, 1])
        assert np.array_equal(g[2][0], wp) and np.array_equal(g[2][1], wt), i
        assert (wp >= 0).sum() > 100
    assert not _same(got[0][0], got[1][0])                        # the two scenes do differ
    for x, y, name in zip(got[2], frame, ("color", "motion", "gpos", "gnrm")):
        assert np.array_equal(x, y), name


# ---------------------------------------------------------------- 8: refusals
def test_refusals(monkeypatch):
    v, f = _mesh(100)
    v = np.ascontiguousarray(v, np.float32)
    pf = split("uneven", 100)
    k = pf.size - 1
    hits = np.zeros((4, 4), np.float32)

    def new_calls(b):
        return {"mesh_parts": b.mesh_parts, "mesh_part_matrices": lambda: b.mesh_part_matrices(as_torch=False),
                "mesh_set_part_matrices": lambda: b.mesh_set_part_matrices(part_models(1)), "mesh_rebuild_parts": b.mesh_rebuild_parts,
                "mesh_refit_parts": b.mesh_refit_parts, "mesh_hit_parts": lambda: b.mesh_hit_parts(hits)}

    def refused(call, code=rt.RT_ERR_INVALID):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == code
        return str(e.value)

    with rt.Renderer() as b:
        for name, call in new_calls(b).items():                  # no mesh
            refused(call)
        for bad in (np.r_[1, pf[1:]], np.r_[pf[:-1], 99], np.r_[pf[:3], 9, 8, pf[5:]], pf[:1]):      # first, last, decreasing, no part
            refused(lambda: b.mesh_upload_parts(v, f, np.asarray(bad, np.int32)))
            assert "rt_mesh_upload_parts" in str(rt.lib().rt_last_error(b._h))
        big = np.zeros(rt.RT_MAX_MESH_PARTS + 2, np.int32); big[-1] = 100
        refused(lambda: b.mesh_upload_parts(v, f, big))
        idx = f.copy(); idx[22] = v.shape[0]
        refused(lambda: b.mesh_upload_parts(v, idx, pf))
        refused(lambda: b.mesh_upload_parts(v, f[:-1], pf))
        assert rt.lib().rt_mesh_upload_parts(b._h, v.ctypes.data_as(rt._FP), v.shape[0], f.ctypes.data_as(rt._U32P), f.size, None, k) == rt.RT_ERR_INVALID
        monkeypatch.setenv("RT_FUSED", "1")
        assert "RT_FUSED" in refused(lambda: b.mesh_upload_parts(v, f, pf), rt.RT_ERR_UNSUPPORTED)
        monkeypatch.delenv("RT_FUSED")
        assert b.mesh_info().nTris == 0
        b.mesh_upload_parts(v, f, pf)
        assert b.mesh_info().nTris == 100 and np.array_equal(b.mesh_parts(), pf)
        assert "rt_mesh_rebuild" in refused(b.mesh_refit_parts)  # a mesh, no tree yet
        assert "rt_mesh_rebuild" in refused(lambda: b.mesh_hit_parts(hits))
        for first, count in ((k, 1), (k - 1, 2), (-1, 1), (0, k + 1)):
            refused(lambda: b.mesh_set_part_matrices(part_models(count), first=first))      # a range past the table
        b.mesh_set_part_matrices(part_models(1), first=k - 1)
        b.mesh_set_part_matrices(part_models(k))
        b.mesh_rebuild_parts()
        b.mesh_refit_parts()
        parts, tris = b.mesh_hit_parts(hits)                      # prim = 0 in every record: row 0
        assert (parts >= 0).all() and (tris >= 0).all()
        nodes, tris12 = rt.build_bvh(rt.gather_triangles(*_mesh(17), _step_model(0)))
        b.upload_bvh(nodes, tris12)                               # an upload releases the mesh
        for name, call in new_calls(b).items():
            refused(call)
        assert b.scene_info().nTris == 17
