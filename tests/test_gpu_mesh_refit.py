"""The device refit.  Contract: after mesh_refit(M) the context's scene is, byte for byte in every device array and in RtSceneInfo,
what upload_bvh installs in a fresh context from refit_bvh(nodes12, tris12, order, gather_triangles(positions, indices, M)), where nodes12 / tris12
are route A's arrays of the last rebuild (build_bvh_gpu) and order is mesh_order's -- and everything downstream gives that context's answers."""
import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scenes
from test_gpu_dynamic_mesh import TRANSFORMS, _assert_same_scene, _have_torch, _mesh, _model, _ntris, _route_a, _step_model

pytestmark = pytest.mark.gpu

COORDS = [0, 1, 2, 4, 5, 6, 8, 9, 10]


def _set_qnodes(monkeypatch, qnodes):
    if qnodes is None:
        monkeypatch.delenv("RT_QNODES", raising=False)
    else:
        monkeypatch.setenv("RT_QNODES", qnodes)


def _sinus(pos, k=0):
    """A displacement of 3 % of the mesh's extent, smooth in the position: what an animation step does."""
    ext = np.float32((pos.max(0) - pos.min(0)).max())
    return (np.float32(0.03) * ext * np.sin(np.float32(3.0) * pos / ext + np.float32(0.7 + k))).astype(np.float32)


def _scatter(pos, seed=4):
    """Every vertex thrown somewhere within three extents: the tree's boxes overlap almost completely."""
    ext = np.float32((pos.max(0) - pos.min(0)).max())
    return (np.random.default_rng(seed).uniform(-3, 3, pos.shape) * ext).astype(np.float32)


def _displace(b, pos, delta):
    """pos + delta in fp32, on the device through mesh_positions() on the library stream (torch) or from the host; -> the host's copy of the sum."""
    new = (pos + delta).astype(np.float32)
    if _have_torch():
        import torch
        dev = torch.device("cuda", 0)
        d = torch.from_numpy(delta).to(dev)
        torch.cuda.current_stream(dev).synchronize()
        ext = torch.cuda.ExternalStream(b.stream(), device=dev)
        with torch.cuda.stream(ext):
            b.mesh_positions().add_(d)
        torch.cuda.current_stream(dev).wait_stream(ext)      # `d` stays tied to torch's own stream
    else:
        b.mesh_set_positions(new)
    return new


def _refitted(ng, tg, order, pos, f, M):
    """The contract's right-hand side: a fresh context with rt_refit_bvh's arrays uploaded -> (renderer, nodes12, tris12)."""
    n2, t2 = rt.refit_bvh(ng, tg, order, rt.gather_triangles(pos, f, M))
    r = rt.Renderer()
    r.upload_bvh(n2, t2)
    return r, n2, t2


def _ident():
    return TRANSFORMS["identity"]


# ---------------------------------------------------------------- 0: one million triangles, the quantised form in use
def test_million_triangles(monkeypatch):
    monkeypatch.delenv("RT_QNODES", raising=False)
    v, f = rt.meshgen.million_triangle_scene()
    v = np.ascontiguousarray(v, np.float32)
    M = rt.default_bvh_transform()
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_rebuild(M)
        a, ng, tg = _route_a(v, f, M)
        a.close()
        assert b.mesh_info().hostSyncs == 1
        order = b.mesh_order(as_torch=False)
        pos = _displace(b, v, _sinus(v))
        b.mesh_refit(M)
        assert b.mesh_info().hostSyncs == 2
        r, _, _ = _refitted(ng, tg, order, pos, f, M)
        with r:
            info = _assert_same_scene(r, b, "1M refit")
            assert r.debug_read_scene("qnodes4").size > 0 and info.flags == 0      # the quantised form is in use
        b.mesh_refit(_ident())
        assert b.mesh_info().hostSyncs == 3 and b.mesh_info().rebuilds == 1 and b.mesh_refit_count() == (2, 2)
        r, _, _ = _refitted(ng, tg, order, pos, f, _ident())
        with r:
            _assert_same_scene(r, b, "1M second refit")


# ---------------------------------------------------------------- 1: array identity
@pytest.mark.parametrize("qnodes", [None, "2", "0"])
@pytest.mark.parametrize("mesh", [1, 8, 9, 17, 100, 1000, 20480, "bunny", "bunny6"])
def test_array_identity(monkeypatch, mesh, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    v, f = _mesh(mesh)
    v = np.ascontiguousarray(v, np.float32)
    M0, M1 = _model("rot-scale"), _model("default")
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_rebuild(M0)
        a, ng, tg = _route_a(v, f, M0)
        order = b.mesh_order(as_torch=False)
        with a:
            b.mesh_refit(M0)                                     # (a) nothing moved: the rebuild's own arrays
            info = _assert_same_scene(a, b, (mesh, qnodes, "a"))
            if qnodes == "2" and _ntris(f) > 8:
                assert a.debug_read_scene("qnodes4").size > 0 or info.flags & rt.RT_SCENE_QNODES_REJECTED
            if qnodes == "0":
                assert a.debug_read_scene("qnodes4").size == 0
        steps = [("b", None, M1),                                # (b) another transform
                 ("c", _sinus, M1),                              # (c) a deformation written on the device
                 ("d", lambda p: _sinus(p, 1), None),            # (d) a second refit on top of (c); NULL matrix: the identity
                 ("e", _scatter, M0)]                            # (e) a badly degraded tree is still exact
        pos = v
        for name, deform, M in steps:
            if deform is not None:
                pos = _displace(b, pos, deform(pos))
            assert b.mesh_refit(M) is None
            r, _, _ = _refitted(ng, tg, order, pos, f, _ident() if M is None else M)
            with r:
                _assert_same_scene(r, b, (mesh, qnodes, name))
        assert b.mesh_info().rebuilds == 1 and b.mesh_refit_count() == (5, 5)
        assert np.array_equal(b.mesh_order(as_torch=False), order)      # a refit does not change the order


# ---------------------------------------------------------------- 2: the order
@pytest.mark.parametrize("mesh", [1, 9, 1000, "bunny"])
def test_mesh_order(mesh):
    v, f = _mesh(mesh)
    v = np.ascontiguousarray(v, np.float32)
    n = _ntris(f)
    M = _model("rot-scale")
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_rebuild(M)
        order = b.mesh_order(as_torch=False)
        assert order.dtype == np.int32 and order.shape == (n,) and np.array_equal(np.sort(order), np.arange(n))
        rows = b.debug_read_scene("tris").view(np.float32).reshape(-1, 12)[:n]
        assert np.array_equal(rows[:, COORDS].view(np.uint32), rt.gather_triangles(v, f, M)[order].view(np.uint32))
        if _have_torch():
            dev_order = b.mesh_order()
            b.synchronize()
            assert str(dev_order.dtype) == "torch.int32" and np.array_equal(dev_order.cpu().numpy(), order)
        pos = _displace(b, v, _sinus(v))
        b.mesh_refit(None)
        assert np.array_equal(b.mesh_order(as_torch=False), order)
        rows = b.debug_read_scene("tris").view(np.float32).reshape(-1, 12)[:n]
        assert np.array_equal(rows[:, COORDS].view(np.uint32), rt.gather_triangles(pos, f, _ident())[order].view(np.uint32))
        b.mesh_rebuild(None)                                     # a rebuild over moved triangles: a new order, valid again
        order2 = b.mesh_order(as_torch=False)
        assert np.array_equal(np.sort(order2), np.arange(n))
        rows = b.debug_read_scene("tris").view(np.float32).reshape(-1, 12)[:n]
        assert np.array_equal(rows[:, COORDS].view(np.uint32), rt.gather_triangles(pos, f, _ident())[order2].view(np.uint32))


def test_pick_maps_back_to_the_index_buffer():
    """A full-frame pick on the bench mesh after a refit: every mesh hit's prim goes through order to an input triangle whose (v0, e1, e2) and the
    returned barycentrics reproduce the returned point.

    Bound.  The kernel returns p = ro + rd t, and t, u, v are Moeller-Trumbore quotients N / det with det = e1 . (rd x e2), each N a dot product of a
    cross product: about eight roundings, so |dN| <= 8 eps |factors|.  With tv = ro - v0 and S = |e1| |e2| / |det| that gives
    |dt| <= 8 eps |tv| S, |du| |e1| <= 8 eps |tv| S, |dv| |e2| <= 8 eps |tv| S, and evaluating the two sides adds at most
    4 eps (|ro| + t + |v0| + |e1| + |e2|).  The test allows twice the first-order sum: second-order terms and the rounding of det itself."""
    v, f = rt.meshgen.bunny_standin(6)
    v = np.ascontiguousarray(v, np.float32)
    M = rt.default_bvh_transform()
    W, H = 192, 128
    p = rt.default_render_params()
    cam = scenes.camera("closeup", aspect=W / H)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)
    L = rt.bvh_layout(_ntris(f))
    with rt.Renderer() as b:
        b.resize(W, H)
        b.mesh_upload(v, f)
        b.mesh_rebuild(M)
        pos = _displace(b, v, _sinus(v))
        b.mesh_refit(M)
        order = b.mesh_order(as_torch=False)
        u = rt.frame_uniforms(p, cam, W, H, 0, 1, L.nNodes, L.nTris, env_loaded=False)
        h = b.pick(u, xy)
    t9 = rt.gather_triangles(pos, f, M).astype(np.float64)
    hit = np.asarray(h.object) == rt.RT_OBJECT_MESH
    assert hit.sum() > 2000
    prim = np.asarray(h.prim)[hit]
    assert (prim >= 0).all() and (prim < L.nTris).all()
    tri = t9[order[prim]]
    v0, e1, e2 = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    uv = np.asarray(h.uv)[hit].astype(np.float64)
    t = np.asarray(h.t)[hit].astype(np.float64)
    point = np.asarray(h.point)[hit].astype(np.float64)
    assert (uv >= 0).all() and (uv.sum(1) <= 1 + 1e-6).all()
    want = v0 + uv[:, :1] * e1 + uv[:, 1:] * e2
    ro = np.array(list(cam.pos), np.float64)
    rd = (point - ro) / np.linalg.norm(point - ro, axis=1, keepdims=True)
    nrm = lambda x: np.linalg.norm(x, axis=1)
    det = np.abs(np.einsum("ij,ij->i", e1, np.cross(rd, e2)))
    S = nrm(e1) * nrm(e2) / det
    eps = 2.0 ** -24
    bound = 2 * eps * (24 * nrm(ro - v0) * S + 4 * (np.linalg.norm(ro) + t + nrm(v0) + nrm(e1) + nrm(e2)))
    err = nrm(want - point)
    worst = int(np.argmax(err / bound))
    print(f"pick: {hit.sum()} mesh hits, worst error {err[worst]:.3e} against its bound {bound[worst]:.3e}")
    assert (err <= bound).all(), (err[worst], bound[worst])
    # the same prims through a wrong map do not: the check has teeth
    wrong = t9[prim]
    assert nrm(wrong[:, 0:3] + uv[:, :1] * wrong[:, 3:6] + uv[:, 1:] * wrong[:, 6:9] - point).max() > 1e-3


# ---------------------------------------------------------------- 3: frames
def _refit_pair(pipeline):
    """(refitted mesh context, fresh context with rt_refit_bvh's arrays, those arrays): bunny 5, rebuilt, deformed, refitted under another transform."""
    v, f = rt.meshgen.bunny_standin(5)
    v = np.ascontiguousarray(v, np.float32)
    M = rt.default_bvh_transform()
    b = rt.Renderer(pipeline=pipeline)
    b.mesh_upload(v, f)
    b.mesh_rebuild(_model("rot-scale"))
    a, ng, tg = _route_a(v, f, _model("rot-scale"))
    a.close()
    order = b.mesh_order(as_torch=False)
    pos = _displace(b, v, _sinus(v))
    b.mesh_refit(M)
    n2, t2 = rt.refit_bvh(ng, tg, order, rt.gather_triangles(pos, f, M))
    r = rt.Renderer(pipeline=pipeline)
    r.upload_bvh(n2, t2)
    return b, r, n2, t2


@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel"])
def test_frames_after_a_refit(orc, pipeline):
    pl = rt.RT_PIPELINE_AUTO if pipeline == "wavefront" else rt.RT_PIPELINE_MEGAKERNEL
    W, H = 120, 80
    faces = scenes.tiny_env(8)
    p = rt.default_render_params()
    p.sppPerFrame = 2
    cam = scenes.camera("closeup", aspect=W / H)
    b, r, n2, t2 = _refit_pair(pl)
    with b, r:
        for x in (r, b):
            x.upload_env(faces)
            x.resize(W, H)
        for frame in range(3):
            u = rt.frame_uniforms(p, cam, W, H, frame, True, n2.shape[0], t2.shape[0])
            r.render_frame(u)
            b.render_frame(u)
            gr, gb = r.read_all(), b.read_all()
            for x, y, name in zip(gr, gb, ("color", "motion", "gpos", "gnrm")):
                assert np.array_equal(x, y), (frame, name)
            if frame == 0:
                want, _ = orc.render(u, n2, t2, faces, None)
                for g, w_, name in zip(gb, want, ("color", "motion", "gpos", "gnrm")):
                    st = orc.compare(g, w_)
                    assert st["bit_diff"] == 0 and st["rmse"] < 1e-4, ("oracle", name, st)


def test_hybrid_frame_after_a_refit(orc):
    W, H = 120, 80
    faces = scenes.tiny_env(8)
    p = rt.default_render_params()
    p.sppPerFrame = 2
    cam = scenes.camera("default", aspect=W / H)
    b, r, n2, t2 = _refit_pair(rt.RT_PIPELINE_AUTO)
    with b, r:
        for x in (r, b):
            x.upload_env(faces)
            x.resize(W, H)
        u = rt.frame_uniforms(p, cam, W, H, 0, rt.RT_SCENE_HYBRID, n2.shape[0], t2.shape[0])
        r.render_frame(u)
        b.render_frame(u)
        gb = b.read_all()
        for x, y, name in zip(r.read_all(), gb, ("color", "motion", "gpos", "gnrm")):
            assert np.array_equal(x, y), name
        want, _ = orc.render(u, n2, t2, faces, None)
        for g, w_, name in zip(gb, want, ("color", "motion", "gpos", "gnrm")):
            st = orc.compare(g, w_)
            assert st["bit_diff"] == 0 and st["rmse"] < 1e-4, ("oracle", name, st)


# ---------------------------------------------------------------- 4: queries and picking
def test_queries_after_a_refit():
    W, H = 64, 48
    p = rt.default_render_params()
    cam = scenes.camera("default", aspect=W / H)
    rng = np.random.default_rng(9)
    org = (rng.normal(0, 1, (3000, 3)) * 2.5 + [0, 1.5, 0]).astype(np.float32)
    tmax = np.full(org.shape[0], 5.0, np.float32)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)
    same = lambda x, y: np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    b, r, n2, t2 = _refit_pair(rt.RT_PIPELINE_AUTO)
    centre = ((n2[0, 0:3] + n2[0, 4:7]) * 0.5).astype(np.float32)
    dirs = centre - org + rng.normal(0, 0.3, org.shape).astype(np.float32)      # towards the mesh, most of them through it
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    with b, r:
        hr, hb = (x.trace_rays(org, dirs, normals=True) for x in (r, b))
        assert same(hr.record, hb.record) and same(hr.normal, hb.normal)
        assert (np.asarray(hb.prim) >= 0).sum() > 100
        assert same(r.trace_rays(org, dirs, tmax=tmax, any_hit=True), b.trace_rays(org, dirs, tmax=tmax, any_hit=True))
        for mode in (1, rt.RT_SCENE_HYBRID):
            u = rt.frame_uniforms(p, cam, W, H, 0, mode, n2.shape[0], t2.shape[0], env_loaded=False)
            hr, hb = (x.trace_scene_rays(u, org, dirs, normals=True, points=True) for x in (r, b))
            for name in ("record", "object", "normal", "point"):
                assert same(getattr(hr, name), getattr(hb, name)), (mode, name)
            assert same(r.trace_scene_rays(u, org, dirs, tmax=tmax, any_hit=True), b.trace_scene_rays(u, org, dirs, tmax=tmax, any_hit=True)), mode
            pr, pb = r.pick(u, xy), b.pick(u, xy)
            for name in ("record", "object", "normal", "point"):
                assert same(getattr(pr, name), getattr(pb, name)), (mode, "pick", name)
            assert (np.asarray(pb.object) == rt.RT_OBJECT_MESH).any()


# ---------------------------------------------------------------- 5: an animation on one context
REBUILD_AT = (0, 4)


@pytest.mark.parametrize("qnodes", [None, "2"])
def test_animation(monkeypatch, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    v, f = rt.meshgen.bunny_standin(4)
    pos = np.ascontiguousarray(v, np.float32)
    with rt.Renderer() as b:
        b.mesh_upload(pos, f)
        allocs = b.mesh_info().allocations
        refits = since = 0
        for k in range(6):
            if k:
                pos = _displace(b, pos, _sinus(pos, k))
            M = _step_model(k)
            if k in REBUILD_AT:
                b.mesh_rebuild(M)
                a, ng, tg = _route_a(pos, f, M)
                order = b.mesh_order(as_torch=False)
                since = 0
                want = a
            else:
                b.mesh_refit(M)
                refits, since = refits + 1, since + 1
                want, _, _ = _refitted(ng, tg, order, pos, f, M)
            with want:
                _assert_same_scene(want, b, ("step", k, qnodes))
            mi = b.mesh_info()
            assert mi.allocations == allocs                                   # nothing allocated after mesh_upload
            assert mi.rebuilds == sum(1 for r in REBUILD_AT if r <= k)        # rebuilds only
            assert b.mesh_refit_count() == (refits, since)
            assert mi.hostSyncs == (0 if qnodes is None else k + 1)           # RT_QNODES=2: one wait per rebuild or refit, none otherwise


def test_ordering_without_host_waits():
    """Frames, refits, a rebuild and queries enqueued back to back give the bytes of the same sequence with a host wait after every call."""
    v, f = rt.meshgen.bunny_standin(4)
    v = np.ascontiguousarray(v, np.float32)
    W, H = 96, 64
    faces = scenes.tiny_env(8)
    p = rt.default_render_params()
    p.sppPerFrame = 1
    cam = scenes.camera("default", aspect=W / H)
    rng = np.random.default_rng(2)
    org = (rng.normal(0, 1, (4096, 3)) * 3).astype(np.float32)
    dirs = -org + rng.normal(0, 0.3, org.shape).astype(np.float32)
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    tmax = np.full(org.shape[0], 4.0, np.float32)
    L = rt.bvh_layout(_ntris(f))
    use_torch = _have_torch()
    deltas = [_sinus(v, k) for k in range(3)]

    def run(wait):
        if use_torch:
            import torch
            dev = torch.device("cuda", 0)
            o, d, t = (torch.from_numpy(x).to(dev) for x in (org, dirs, tmax))
            dl = [torch.from_numpy(x).to(dev) for x in deltas]
            torch.cuda.synchronize()
        out = []
        with rt.Renderer() as b:
            sync = b.synchronize if wait else (lambda: None)

            def frames(first):
                b.render_frames([rt.frame_uniforms(p, cam, W, H, first + k, True, L.nNodes, L.nTris) for k in range(4)])
                sync()

            def move(k):
                if use_torch:
                    ext = torch.cuda.ExternalStream(b.stream(), device=dev)
                    with torch.cuda.stream(ext):
                        b.mesh_positions().add_(dl[k])
                    torch.cuda.current_stream(dev).wait_stream(ext)
                else:
                    b.mesh_set_positions((v + sum(deltas[:k + 1])).astype(np.float32))
                sync()

            def queries():
                q = (b.trace_rays(o, d, normals=True), b.trace_rays(o, d, tmax=t, any_hit=True)) if use_torch else \
                    (b.trace_rays(org, dirs, normals=True), b.trace_rays(org, dirs, tmax=tmax, any_hit=True))
                sync()
                out.append(q)

            b.upload_env(faces)
            b.resize(W, H)
            b.mesh_upload(v, f)
            b.mesh_rebuild(_step_model(0)); sync()
            frames(0)
            move(0); b.mesh_refit(_step_model(1)); sync()
            queries()
            frames(4)
            move(1); b.mesh_refit(_step_model(2)); sync()
            queries()
            b.mesh_rebuild(_step_model(3)); sync()
            move(2); b.mesh_refit(_step_model(3)); sync()
            queries()
            frames(8)
            assert b.mesh_info().hostSyncs == 0 and b.mesh_refit_count() == (3, 1)
            res = []
            for h, occ in out:
                res += [h.record.cpu().numpy(), h.normal.cpu().numpy(), occ.cpu().numpy()] if use_torch else [np.asarray(h.record), np.asarray(h.normal), np.asarray(occ)]
            return res + b.read_all()

    got, want = run(False), run(True)
    assert len(got) == len(want) == 13
    for i, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), i
    assert not np.array_equal(got[0], got[3]) and not np.array_equal(got[3], got[6])      # the three scenes do differ


# ---------------------------------------------------------------- 6: refusals
def test_refusals():
    v, f = _mesh(100)
    M = _model("rot-scale")
    with rt.Renderer() as b:
        for call in (lambda: b.mesh_refit(M), lambda: b.mesh_order(as_torch=False)):
            with pytest.raises(rt.RtError) as e:
                call()                                           # no mesh
            assert e.value.code == rt.RT_ERR_INVALID
        b.mesh_upload(v, f)
        for call in (lambda: b.mesh_refit(M), lambda: b.mesh_order(as_torch=False), lambda: b.mesh_order(as_torch=_have_torch())):
            with pytest.raises(rt.RtError) as e:
                call()                                           # a mesh, no tree yet
            assert e.value.code == rt.RT_ERR_INVALID and "rt_mesh_rebuild" in str(e.value)
        assert b.mesh_refit_count() == (0, 0)
        b.mesh_rebuild(M)
        b.mesh_refit(M)
        assert b.mesh_refit_count() == (1, 1)
        with pytest.raises(rt.RtError) as e:
            b.mesh_refit(np.zeros(9, np.float32))
        assert e.value.code == rt.RT_ERR_INVALID
        v2, f2 = _mesh(1000)
        b.mesh_upload(v2, f2)                                    # a new mesh forgets the tree and the counters
        assert b.mesh_refit_count() == (0, 0)
        with pytest.raises(rt.RtError) as e:
            b.mesh_refit(M)
        assert e.value.code == rt.RT_ERR_INVALID
        b.mesh_rebuild(M)
        b.mesh_refit(M)
        nodes, tris = rt.build_bvh(rt.gather_triangles(*_mesh(17), M))
        b.upload_bvh(nodes, tris)                                # an upload releases the mesh
        for call in (lambda: b.mesh_refit(M), lambda: b.mesh_order(as_torch=False)):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == rt.RT_ERR_INVALID
        assert b.scene_info().nTris == 17
