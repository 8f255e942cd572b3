"""The dynamic mesh: after mesh_rebuild(M) the context's scene is, byte for byte in every device array, what
gather_triangles(positions, indices, M) -> build_bvh_gpu -> upload_bvh installs (route A), and everything downstream -- frames in both pipelines,
the hybrid extension, ray and scene queries, picking -- gives route A's answers.  Route B is mesh_upload + mesh_rebuild."""
import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scenes

pytestmark = pytest.mark.gpu

ARRAYS = tuple(rt.SCENE_ARRAYS)


def _rot_scale():
    """A rotation about a skew axis times a non-uniform scale and a translation, column-major."""
    a = np.array([0.3, -0.8, 0.52]); a /= np.linalg.norm(a)
    th = 0.7
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    M = np.eye(4)
    M[:3, :3] = R @ np.diag([1.7, 0.45, 1.1])
    M[:3, 3] = [0.25, -0.6, 1.3]
    return np.ascontiguousarray(M.T, dtype=np.float32).reshape(-1)


TRANSFORMS = {"identity": np.eye(4, dtype=np.float32).reshape(-1), "default": None, "rot-scale": _rot_scale()}


def _model(name):
    return rt.default_bvh_transform() if TRANSFORMS[name] is None else TRANSFORMS[name]


def _soup(n):
    """n random triangles as an indexed mesh with shared vertices."""
    rng = np.random.default_rng(n)
    nv = max(3, n // 2 + 3)
    v = rng.normal(0, 1, (nv, 3)).astype(np.float32)
    f = rng.integers(0, nv, (n, 3)).astype(np.uint32)
    return v, f.reshape(-1)


def _mesh(name):
    """Triangle soups by count; the bunny stand-in (symmetric centroids, so median ties occur) at subdivision 5 (20 480 triangles) and at the bench
    mesh's subdivision 6 (81 920)."""
    if name == "bunny":
        return rt.meshgen.bunny_standin(5)
    if name == "bunny6":
        return rt.meshgen.bunny_standin(6)
    return _soup(name)


def _route_a(v, f, M):
    t9 = rt.gather_triangles(v, f, M)
    r = rt.Renderer()
    ng, tg = r.build_bvh_gpu(t9)
    r.upload_bvh(ng, tg)
    return r, ng, tg


def _assert_same_scene(a, b, what):
    ia, ib = a.scene_info(), b.scene_info()
    assert bytes(ia) == bytes(ib), (what, ia.to_dict(), ib.to_dict())
    for name in ARRAYS:
        x, y = a.debug_read_scene(name), b.debug_read_scene(name)
        assert x.size == y.size, (what, name, x.size, y.size)
        if not np.array_equal(x, y):
            bad = np.flatnonzero(x != y)
            raise AssertionError(f"{what}: array {name} differs in {bad.size} of {x.size} bytes, first at byte {bad[0]}")
    return ia


def _ntris(f):
    return np.asarray(f).size // 3


def _check_layout(info, n):
    L = rt.bvh_layout(n)
    got = (info.nNodes, info.nTris, info.nInner, info.treeDepth, info.nWide4, info.nPairs, info.bytesNodes2, info.bytesPairs, info.bytesTris)
    assert got == (L.nNodes, L.nTris, L.nInner, L.treeDepth, L.nWide4, L.nPairs, L.bytesNodes2, L.bytesPairs, L.bytesTris)
    if not info.flags & rt.RT_SCENE_QNODES_REJECTED:
        assert info.bytesNodes4 == L.bytesNodes4


# ---------------------------------------------------------------- 0: one million triangles, the quantised form chosen by the tree-size rule
def test_million_triangles(monkeypatch):
    monkeypatch.delenv("RT_QNODES", raising=False)
    v, f = rt.meshgen.million_triangle_scene()
    M = rt.default_bvh_transform()
    a, _, _ = _route_a(v, f, M)
    with a, rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_rebuild(M)
        info = _assert_same_scene(a, b, "1M")
        assert a.debug_read_scene("qnodes4").size > 0 and info.flags == 0      # the quantised form is in use
        _check_layout(info, _ntris(f))
        assert b.mesh_info().hostSyncs == 1


# ---------------------------------------------------------------- 1: array identity
@pytest.mark.parametrize("qnodes", [None, "2", "0"])
@pytest.mark.parametrize("mesh", [1, 8, 9, 17, 100, 1000, 20480, "bunny", "bunny6"])
def test_array_identity(monkeypatch, mesh, qnodes):
    if qnodes is None:
        monkeypatch.delenv("RT_QNODES", raising=False)
    else:
        monkeypatch.setenv("RT_QNODES", qnodes)
    v, f = _mesh(mesh)
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        for name in TRANSFORMS:
            M = _model(name)
            b.mesh_rebuild(M)
            a, _, _ = _route_a(v, f, M)
            with a:
                info = _assert_same_scene(a, b, (mesh, name, qnodes))
                if qnodes == "2" and _ntris(f) > 8:
                    assert a.debug_read_scene("qnodes4").size > 0 or info.flags & rt.RT_SCENE_QNODES_REJECTED
                if qnodes == "0":
                    assert a.debug_read_scene("qnodes4").size == 0
            _check_layout(info, _ntris(f))
        assert b.mesh_rebuild(None) is None                                     # NULL matrix: the identity
        a, _, _ = _route_a(v, f, TRANSFORMS["identity"])
        with a:
            _assert_same_scene(a, b, (mesh, "null", qnodes))


# ---------------------------------------------------------------- 2: frames
@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel"])
def test_frames_after_a_rebuild(orc, pipeline):
    pl = rt.RT_PIPELINE_AUTO if pipeline == "wavefront" else rt.RT_PIPELINE_MEGAKERNEL
    v, f = rt.meshgen.bunny_standin(5)
    M = rt.default_bvh_transform()
    t9 = rt.gather_triangles(v, f, M)
    W, H = 120, 80
    faces = scenes.tiny_env(8)
    p = rt.default_render_params()
    p.sppPerFrame = 2
    cam = scenes.camera("closeup", aspect=W / H)
    with rt.Renderer(pipeline=pl) as a, rt.Renderer(pipeline=pl) as b:
        ng, tg = a.build_bvh_gpu(t9)
        a.upload_bvh(ng, tg)
        b.mesh_upload(v, f)
        b.mesh_rebuild(M)
        prev = None
        for r in (a, b):
            r.upload_env(faces)
            r.resize(W, H)
        for frame in range(3):
            u = rt.frame_uniforms(p, cam, W, H, frame, True, ng.shape[0], tg.shape[0])
            a.render_frame(u)
            b.render_frame(u)
            ga, gb = a.read_all(), b.read_all()
            for x, y, name in zip(ga, gb, ("color", "motion", "gpos", "gnrm")):
                assert np.array_equal(x, y), (frame, name)
            if frame == 0:
                want, _ = orc.render(u, ng, tg, faces, prev)
                for g, w_, name in zip(gb, want, ("color", "motion", "gpos", "gnrm")):
                    assert np.array_equal(g, w_), ("oracle", name)


# ---------------------------------------------------------------- 3: an animation on one context
def _have_torch():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def _step_model(k):
    M = np.eye(4)
    c, s = np.cos(0.37 * k), np.sin(0.37 * k)
    M[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([1.0 + 0.1 * k, 1.0, 1.0 - 0.05 * k])
    M[:3, 3] = [0.1 * k, 0.6, -0.2 * k]
    return np.ascontiguousarray(M.T, dtype=np.float32).reshape(-1)


@pytest.mark.parametrize("qnodes", [None, "2"])
def test_animation(monkeypatch, qnodes):
    if qnodes is None:
        monkeypatch.delenv("RT_QNODES", raising=False)
    else:
        monkeypatch.setenv("RT_QNODES", qnodes)
    v, f = rt.meshgen.bunny_standin(4)
    rng = np.random.default_rng(5)
    pos = v.astype(np.float32).copy()
    use_torch = _have_torch()
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        allocs = None
        for k in range(6):
            if k >= 3:      # displace the positions on the device; the same fp32 addition on the host for route A
                delta = (rng.normal(0, 0.02, pos.shape)).astype(np.float32)
                pos = pos + delta
                if use_torch:
                    import torch
                    dev = torch.device("cuda", 0)
                    d = torch.from_numpy(delta).to(dev)
                    torch.cuda.current_stream(dev).synchronize()
                    ext = torch.cuda.ExternalStream(b.stream(), device=dev)
                    with torch.cuda.stream(ext):
                        b.mesh_positions().add_(d)
                    # `d` stays tied to torch's own stream, never to the library's, which dies with the context before the tensor may
                    torch.cuda.current_stream(dev).wait_stream(ext)
                else:
                    b.mesh_set_positions(pos)
            M = _step_model(k)
            b.mesh_rebuild(M)
            mi = b.mesh_info()
            if k == 0:
                allocs = mi.allocations
            assert mi.allocations == allocs and mi.rebuilds == k + 1
            assert mi.hostSyncs == (0 if qnodes is None else k + 1)       # RT_QNODES=2: the one allowed wait per rebuild, none otherwise
            a, _, _ = _route_a(pos, f, M)
            with a:
                _assert_same_scene(a, b, ("step", k, qnodes))


# ---------------------------------------------------------------- 4: ordering without host waits
def test_ordering_without_host_waits():
    """Frames, a rebuild, queries, another rebuild, queries, frames -- enqueued back to back; every batch sees the scene that was current when it was
    enqueued.  With torch the queries take the zero-copy path (no host wait anywhere); without it they go through host arrays, which synchronise."""
    v, f = rt.meshgen.bunny_standin(4)
    Ms = [_step_model(0), _step_model(2), _step_model(5)]
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
    use_torch = _have_torch()

    def queries(r):
        if use_torch:
            import torch
            dev = torch.device("cuda", 0)
            T = lambda x: torch.from_numpy(x).to(dev, non_blocking=False)
            o, d, t = T(org), T(dirs), T(tmax)
            return r.trace_rays(o, d, normals=True), r.trace_rays(o, d, tmax=t, any_hit=True)
        return r.trace_rays(org, dirs, normals=True), r.trace_rays(org, dirs, tmax=tmax, any_hit=True)

    def host(q):
        h, occ = q
        if use_torch:
            return h.record.cpu().numpy(), h.normal.cpu().numpy(), occ.cpu().numpy()
        return np.asarray(h.record), np.asarray(h.normal), np.asarray(occ)

    def frames(r, first, n_nodes, n_tris):
        r.render_frames([rt.frame_uniforms(p, cam, W, H, first + k, True, n_nodes, n_tris) for k in range(8)])

    L = rt.bvh_layout(_ntris(f))
    with rt.Renderer() as b:
        b.upload_env(faces)
        b.resize(W, H)
        b.mesh_upload(v, f)
        if use_torch:
            import torch
            torch.zeros(1, device="cuda")         # torch's context and allocator exist before the sequence starts
            torch.cuda.synchronize()
        b.mesh_rebuild(Ms[0])
        frames(b, 0, L.nNodes, L.nTris)
        b.mesh_rebuild(Ms[1])
        q1 = queries(b)
        b.mesh_rebuild(Ms[2])
        q2 = queries(b)
        frames(b, 8, L.nNodes, L.nTris)
        assert b.mesh_info().hostSyncs == 0
        got = (host(q1), host(q2), b.read_all())
    a, ng, tg = _route_a(v, f, Ms[0])
    with a:
        a.upload_env(faces)
        a.resize(W, H)
        frames(a, 0, ng.shape[0], tg.shape[0])
        want = []
        for M in Ms[1:]:
            t9 = rt.gather_triangles(v, f, M)
            ng, tg = a.build_bvh_gpu(t9)
            a.upload_bvh(ng, tg)                     # like a rebuild, an upload keeps the accumulation
            want.append(host(queries(a)))
        frames(a, 8, ng.shape[0], tg.shape[0])
        want.append(a.read_all())
    for i in range(2):
        for x, y, name in zip(got[i], want[i], ("hits", "normals", "occluded")):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (i, name)
    assert not np.array_equal(got[0][0], got[1][0])      # the two scenes do differ
    for x, y, name in zip(got[2], want[2], ("color", "motion", "gpos", "gnrm")):
        assert np.array_equal(x, y), name


# ---------------------------------------------------------------- 5: scene queries and picking
def test_scene_queries_and_picking_after_a_rebuild():
    v, f = rt.meshgen.bunny_standin(4)
    M = rt.default_bvh_transform()
    W, H = 64, 48
    p = rt.default_render_params()
    cam = scenes.camera("default", aspect=W / H)
    rng = np.random.default_rng(9)
    org = (rng.normal(0, 1, (3000, 3)) * 2.5 + [0, 1.5, 0]).astype(np.float32)
    dirs = rng.normal(0, 1, org.shape)
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    tmax = np.full(org.shape[0], 5.0, np.float32)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)
    a, ng, tg = _route_a(v, f, M)
    with a, rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_rebuild(M)
        for mode in (1, rt.RT_SCENE_HYBRID):
            u = rt.frame_uniforms(p, cam, W, H, 0, mode, ng.shape[0], tg.shape[0], env_loaded=False)
            ha, hb = (r.trace_scene_rays(u, org, dirs, normals=True, points=True) for r in (a, b))
            for name in ("record", "object", "normal", "point"):
                assert np.array_equal(np.asarray(getattr(ha, name)).view(np.uint8), np.asarray(getattr(hb, name)).view(np.uint8)), (mode, name)
            assert np.array_equal(a.trace_scene_rays(u, org, dirs, tmax=tmax, any_hit=True), b.trace_scene_rays(u, org, dirs, tmax=tmax, any_hit=True)), mode
            pa, pb = a.pick(u, xy), b.pick(u, xy)
            for name in ("record", "object", "normal", "point"):
                assert np.array_equal(np.asarray(getattr(pa, name)).view(np.uint8), np.asarray(getattr(pb, name)).view(np.uint8)), (mode, "pick", name)
            assert (np.asarray(pa.object) == rt.RT_OBJECT_MESH).any()


# ---------------------------------------------------------------- 6: refusals and hand-over
def test_refusals_and_hand_over(monkeypatch):
    v, f = _soup(100)
    M = _rot_scale()
    with rt.Renderer() as b:
        with pytest.raises(rt.RtError) as e:
            b.mesh_rebuild(M)
        assert e.value.code == rt.RT_ERR_INVALID and "rt_mesh_upload" in str(e.value)
        bad = f.copy()
        bad[22] = v.shape[0]
        with pytest.raises(rt.RtError) as e:
            b.mesh_upload(v, bad)
        assert e.value.code == rt.RT_ERR_INVALID
        with pytest.raises(rt.RtError) as e:
            b.mesh_upload(v, f[:-1])
        assert e.value.code == rt.RT_ERR_INVALID
        for var, val in (("RT_FUSED", "1"), ("RT_IMPLICIT", "1"), ("RT_ANYHIT_TREE", "sah")):
            monkeypatch.setenv(var, val)
            with pytest.raises(rt.RtError) as e:
                b.mesh_upload(v, f)
            assert e.value.code == rt.RT_ERR_UNSUPPORTED and var in str(e.value)
            monkeypatch.delenv(var)
        assert b.mesh_info().nTris == 0
        # upload_bvh after mesh_upload takes the scene over and releases the mesh
        b.mesh_upload(v, f)
        b.mesh_rebuild(M)
        assert b.mesh_info().nTris == 100 and b.scene_info().nTris == 100
        nodes, tris = rt.build_bvh(rt.gather_triangles(*_soup(17), M))
        b.upload_bvh(nodes, tris)
        assert b.scene_info().nTris == 17 and b.mesh_info().nTris == 0
        with pytest.raises(rt.RtError) as e:
            b.mesh_rebuild(M)
        assert e.value.code == rt.RT_ERR_INVALID
        # a mesh of another triangle count replaces the mesh
        for n in (1000, 9):
            v2, f2 = _soup(n)
            b.mesh_upload(v2, f2)
            assert b.scene_info().nNodes == 0            # no scene until the rebuild
            b.mesh_rebuild(M)
            a, _, _ = _route_a(v2, f2, M)
            with a:
                _assert_same_scene(a, b, ("replaced", n))
        b.mesh_upload(v2, None)                          # nIdx == 0 releases the mesh and its scene
        assert b.mesh_info().nTris == 0 and b.scene_info().nNodes == 0
