"""Multi-hit queries on the GPU (rt_trace_rays_multi, rt_pick_pixels_multi): every answer against rt.multi_hits -- the host
definition, itself pinned to the oracle's primitives in test_multi_hit_host.py -- on the same arrays, bit for bit: ray counts about the wave and
block sizes, every K about the buffer's bounds, numpy and torch, ray layouts, every node form and pipeline, the dynamic mesh after a rebuild, a refit
and a rebuild of parts (and the mesh_hit_* queries over the flattened records), pixel picking, stream ordering with torch, isolation from the
frame state, no allocation after the first query, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import analytic_ref as ar
import mesh_fixtures as mf
import multi_hit_ref as ref
import opengl_raytracing_amd as rt
import scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
bits = ref.bits
NS = (1, 63, 64, 65, 2049)
KS = (0, 1, 2, 4, 8, 32)
OPTION_VARS = ("RT_COOP", "RT_FUSED", "RT_IMPLICIT", "RT_NEAR_FIRST", "RT_QNODES", "RT_QNODES_SPARSE_BOXES", "RT_ANYHIT_TREE", "RT_LEAFB",
               "RT_LEAFB_CLOSEST", "RT_QUAD_REFILL", "RT_REFILL_MIN", "RT_GUIDED", "RT_CHUNK", "RT_MIN_SEARCH", "RT_REVERSE", "RT_DENSE_TAKE",
               "RT_TRACE_STATS", "RT_TRACE_TIMING", "RT_DEBUG_SKIP_TRAVERSAL")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in OPTION_VARS:
        monkeypatch.delenv(v, raising=False)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _to(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _case(name):
    """(nodes12, tris12, origins, dirs, tmax) with at least 2 049 rays."""
    if name == "one_leaf":
        return ref.one_leaf_rays(300)
    if name == "bunny":
        return ref.bunny_rays(2, 300)
    nodes, tris = ref.layer_stack()
    o, d = ref.layer_rays()
    tm = np.random.default_rng(8).uniform(-0.5, 9.0, o.shape[0]).astype(f32)   # limits between the layers, some slots empty
    return nodes, tris, o, d, tm


def _same(got, want, what):
    gh, gc = (got.hits.cpu().numpy(), got.count.cpu().numpy()) if not isinstance(got.hits, np.ndarray) else (got.hits, got.count)
    assert gh.shape == want.hits.shape and gc.shape == want.count.shape, what
    assert np.array_equal(gc, want.count), (what, np.flatnonzero(gc != want.count)[:8])
    bad = np.flatnonzero((bits(gh) != bits(want.hits)).reshape(gh.shape[0], -1).any(1))
    assert bad.size == 0, (what, bad[:8], gh[bad[:1]], want.hits[bad[:1]])


# ---------------------------------------------------------------- 1: against the definition

@pytest.mark.parametrize("mesh", ["one_leaf", "bunny", "layers"])
def test_answers_equal_the_definition(mesh):
    nodes, tris, o, d, tm = _case(mesh)
    assert o.shape[0] >= NS[-1]
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        for n in NS:
            pick = np.arange(n) * (o.shape[0] // n)            # across all the kinds of rays
            on, dn, tn = o[pick], d[pick], tm[pick]
            for K in KS:
                for t in (None, tn):
                    want = rt.multi_hits(nodes, tris, on, dn, t, max_hits=K)
                    _same(ren.trace_rays_multi(on, dn, t, max_hits=K), want, (mesh, n, K, t is not None, "numpy"))
                    if n in (65, 2049):
                        _same(ren.trace_rays_multi(_to(on), _to(dn), _to(t), max_hits=K), want, (mesh, n, K, t is not None, "torch"))
        full = rt.multi_hits(nodes, tris, o, d, max_hits=32)
        _same(ren.trace_rays_multi(o, d, max_hits=32), full, (mesh, "all"))
    if mesh == "layers":
        assert o.shape[0] == 3000 and set(np.unique(full.count)) == {18, 36}
    if mesh == "bunny":
        assert full.count.max() >= 5 and (full.count == 0).sum() > 100


def test_layouts_give_identical_bytes():
    nodes, tris, o, d, tm = _case("bunny")
    N = o.shape[0]
    o4 = np.zeros((N, 4), f32); o4[:, :3] = o; o4[:, 3] = 7.0
    d4 = np.zeros((N, 4), f32); d4[:, :3] = d; d4[:, 3] = np.nan
    i8 = np.full((N, 8), 9.0, f32); i8[:, 0:3] = o; i8[:, 4:7] = d
    want = rt.multi_hits(nodes, tris, o, d, tm, max_hits=4)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        t8, tt = _to(i8), _to(tm)
        for name, (oo, dd, t) in {"numpy3": (o, d, tm), "numpy4": (o4, d4, tm), "numpy8": (i8[:, 0:4], i8[:, 4:8], tm), "torch3": (_to(o), _to(d), tt),
                                  "torch4": (_to(o4), _to(d4), tt), "torch8": (t8[:, 0:3], t8[:, 4:7], tt)}.items():
            _same(ren.trace_rays_multi(oo, dd, t, max_hits=4), want, name)


OPTIONS = {"default": {}, "exact": {"RT_QNODES": "0"}, "qnodes2": {"RT_QNODES": "2"}, "fused": {"RT_FUSED": "1"}, "implicit": {"RT_IMPLICIT": "1"}}
PIPELINES = {"megakernel": rt.RT_PIPELINE_MEGAKERNEL, "wavefront": rt.RT_PIPELINE_WAVEFRONT}


@pytest.mark.parametrize("pipeline", list(PIPELINES))
@pytest.mark.parametrize("option", list(OPTIONS))
def test_every_node_form_gives_identical_bytes(monkeypatch, option, pipeline):
    """The query reads the two-child records and the triangle rows alone: what else the upload builds does not matter."""
    for k, v in OPTIONS[option].items():
        monkeypatch.setenv(k, v)
    nodes, tris, o, d, tm = _case("bunny")
    with rt.Renderer(pipeline=PIPELINES[pipeline]) as ren:
        ren.upload_bvh(nodes, tris)
        _same(ren.trace_rays_multi(o, d, tm, max_hits=4), rt.multi_hits(nodes, tris, o, d, tm, max_hits=4), (option, pipeline))
        _same(ren.trace_rays_multi(o, d, max_hits=2), rt.multi_hits(nodes, tris, o, d, max_hits=2), (option, pipeline))


# ---------------------------------------------------------------- 2: the dynamic mesh

def _want_parts(pf, order, prim):
    """The host formula of rt_mesh_hit_parts: (-1, -1) for a prim outside [0, nTris), else the part whose range holds order[prim] and the offset in it."""
    prim = np.asarray(prim).astype(np.int64)
    ok = (prim >= 0) & (prim < order.size)
    t = order[np.where(ok, prim, 0)].astype(np.int64)
    part = np.searchsorted(pf, t, "right") - 1
    return np.where(ok, part, -1).astype(np.int32), np.where(ok, t - pf[part], -1).astype(np.int32)


def _check_mesh_state(ren, host, f, pf, colors, what):
    o, d, tm = scenes.adversarial_rays(host.nodes, host.tris, n=100, seed=21)
    lo, hi = host.nodes[0, 0:3], host.nodes[0, 4:7]
    away = np.tile(np.array([1, 0, 0], f32), (64, 1))          # ... and rays that leave from beside the mesh: misses for sure
    o = np.concatenate([o, (hi + (hi - lo) * f32(0.5) + np.arange(64, dtype=f32)[:, None] * f32(0.01)).astype(f32)])
    d, tm = np.concatenate([d, away]), np.concatenate([tm, np.full(64, 5, f32)])
    for K, t in ((1, None), (32, tm), (4, None)):
        want = rt.multi_hits(host.nodes, host.tris, o, d, t, max_hits=K)
        got = ren.trace_rays_multi(o, d, t, max_hits=K)
        _same(got, want, (what, K))
        _same(ren.trace_rays_multi(_to(o), _to(d), _to(t), max_hits=K), want, (what, K, "torch"))
    assert (want.count > 1).sum() > 20 and (want.count == 0).sum() >= 64
    rec = got.hits.reshape(-1, 4)                              # K = 4: the flattened records, miss slots included
    prim = rec.view(np.int32)[:, 1]
    assert (prim < 0).sum() > 100 and (prim >= 0).sum() > 100
    parts, offs = ren.mesh_hit_parts(rec)
    wp, wo = _want_parts(np.asarray(pf, np.int64), host.order, prim)
    assert np.array_equal(parts, wp) and np.array_equal(offs, wo), what
    cols = ren.mesh_hit_colors(rec)
    assert mf.same(cols, rt.hit_colors(host.tris, host.order, f, colors, rec)), what
    assert (cols[prim < 0].view(np.uint32) == 0).all() and (parts[prim < 0] == -1).all()


def test_dynamic_mesh_rebuild_refit_and_parts():
    v, f, _, _ = mf.sphere()
    n, nv = f.size // 3, v.shape[0]
    colors = mf.random_colors(nv, 5)
    with rt.Renderer() as ren:
        ren.mesh_upload(v, f)
        ren.mesh_colors_enable()
        ren.mesh_set_colors(colors)
        ren.mesh_rebuild(mf.turn(0))
        host = mf.HostMesh(f).rebuild(rt.gather_triangles(v, f, mf.turn(0)))
        _check_mesh_state(ren, host, f, [0, n], colors, "rebuild")
        ren.mesh_refit(mf.turn(1))                       # the same tree under a turned matrix: boxes overlap, rows stay
        host.refit(rt.gather_triangles(v, f, mf.turn(1)))
        _check_mesh_state(ren, host, f, [0, n], colors, "refit")
    v, f = mf.parts_mesh()
    nv = v.shape[0]
    colors = mf.random_colors(nv, 6)
    with rt.Renderer() as ren:
        ren.mesh_upload_parts(v, f, mf.PART_FIRST)
        ren.mesh_colors_enable()
        ren.mesh_set_colors(colors)
        ren.mesh_set_part_matrices(mf.part_models(1))
        ren.mesh_rebuild_parts()
        host = mf.HostMesh(f).rebuild(rt.gather_triangles_parts(v, f, mf.PART_FIRST, mf.part_models(1)))
        _check_mesh_state(ren, host, f, mf.PART_FIRST, colors, "parts")


# ---------------------------------------------------------------- 3: pixel picking

def test_pick_multi_on_every_pixel_of_a_jittered_frame():
    nodes, tris = scenes.bunny_bvh(3)
    W, H = 64, 48
    p = rt.default_render_params()
    p.enableJitter = 1
    u = rt.frame_uniforms(p, scenes.camera("closeup", aspect=W / H), W, H, 3, True, nodes.shape[0], tris.shape[0])
    assert u.frameIndex == 3 and u.enableJitter == 1 and (u.jitter[0] != 0 or u.jitter[1] != 0)
    y, x = np.mgrid[0:H, 0:W]
    xy = np.stack([x.ravel(), y.ravel()], 1).astype(np.int32)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        one = ren.pick(u, xy)
        got = ren.pick_multi(u, xy, max_hits=4)
        got_t = ren.pick_multi(u, _to(xy), max_hits=4)
        ro, rd = ar.pixel_rays(u, xy)                      # the rays rebuilt from the uniforms
        rays = ren.trace_rays_multi(ro, rd, max_hits=4, eps=u.eps, inf=u.inf)
        counts = ren.pick_multi(u, xy, max_hits=0)
        single = ren.pick_multi(u, xy[1234:1235], max_hits=32)      # one pixel: one block
        none = rt.RtUniforms.from_buffer_copy(u)
        none.nodeCount = 0                                 # the frame's scene has no mesh
        empty = ren.pick_multi(none, xy, max_hits=2)
    hit = one.prim >= 0
    assert 200 < hit.sum() < W * H - 200
    assert np.array_equal(got.count > 0, hit)
    assert (ref.key(got.t[hit, 0]) <= ref.key(one.t[hit])).all()
    want = rt.multi_hits(nodes, tris, ro, rd, max_hits=4, eps=u.eps, inf=u.inf)
    _same(rays, want, "rays rebuilt from the uniforms")
    _same(got, want, "pick_multi")
    _same(got_t, want, "pick_multi torch")
    assert np.array_equal(counts.count, want.count) and counts.hits.shape == (W * H, 0, 4)
    assert (want.count >= 2).sum() > 100                  # the closed mesh: a way in and a way out
    _same(single, rt.multi_hits(nodes, tris, ro[1234:1235], rd[1234:1235], max_hits=32, eps=u.eps, inf=u.inf), "one pixel")
    assert not empty.count.any() and (empty.prim == -1).all() and (empty.t == f32(u.inf)).all()


# ---------------------------------------------------------------- 4: stream ordering with torch

def test_rays_written_by_torch_just_before_the_call_are_the_ones_traced():
    import torch
    nodes, tris, org, dirs, tm = _case("bunny")
    dev = _dev()
    want = rt.multi_hits(nodes, tris, org, dirs, max_hits=4)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        o = torch.zeros((org.shape[0], 3), device=dev)
        d = torch.zeros((org.shape[0], 3), device=dev)
        d[:, 1] = 1.0                                             # placeholder rays: straight up from the origin
        torch.cuda.synchronize()
        src_o, src_d = torch.from_numpy(org).to(dev), torch.from_numpy(dirs).to(dev)
        x = torch.randn(4096, 4096, device=dev)
        for _ in range(8):                                        # keep torch's stream busy, so that the writes below land late
            x = x @ x
            x = x / x.norm()
        o.copy_(src_o + 0.0 * x[0, 0])
        d.copy_(src_d + 0.0 * x[0, 1])
        got = ren.trace_rays_multi(o, d, max_hits=4)
        hits, count = got.hits.clone().cpu().numpy(), got.count.clone().cpu().numpy()      # read by torch on its own stream, no synchronise
    _same(rt.MultiHits(hits, count), want, "late rays")


def test_two_calls_on_two_torch_streams_without_a_host_wait():
    import torch
    nodes, tris, o, d, tm = _case("layers")
    bn, bt, bo, bd, btm = _case("bunny")
    want_a = rt.multi_hits(nodes, tris, o, d, tm, max_hits=32)
    want_b = rt.multi_hits(nodes, tris, bo, bd, max_hits=2)     # (the bunny's rays against the layer stack: another ray count, another K)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        ta, tb = (_to(o), _to(d), _to(tm)), (_to(bo), _to(bd))
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
        with torch.cuda.stream(s1):
            a = ren.trace_rays_multi(*ta, max_hits=32)
        with torch.cuda.stream(s2):
            b = ren.trace_rays_multi(*tb, max_hits=2)
        with torch.cuda.stream(s1):
            a2 = ren.trace_rays_multi(*ta, max_hits=32)
        torch.cuda.synchronize()
        _same(a, want_a, "stream 1"); _same(b, want_b, "stream 2"); _same(a2, want_a, "stream 1 again")


# ---------------------------------------------------------------- 5: isolation from frames, no allocation

@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
def test_queries_do_not_touch_frame_state(pipeline):
    """Three BVH frames with multi-hit queries (host and device path, rays and pixels) enqueued between them against the same three frames without:
    COLOR0 of every frame, the frame index, RtCounters (the megakernel's counting build), the traced-ray tallies and rt_debug_builds are identical."""
    nodes, tris = scenes.bunny_bvh(3)
    _, _, org, dirs, tmax = ref.bunny_rays(3, 300)
    W, H = 160, 96
    cam = scenes.camera("closeup", aspect=W / H)
    p = rt.default_render_params()
    mega = pipeline == "megakernel"
    xy = np.stack([np.arange(64) % W, np.arange(64) % H], 1).astype(np.int32)

    def run(with_queries):
        out = []
        with rt.Renderer(pipeline=PIPELINES[pipeline], count_work=mega) as ren:
            ren.upload_bvh(nodes, tris)
            ren.resize(W, H)
            for frame in range(3):
                u = rt.frame_uniforms(p, cam, W, H, frame, True, nodes.shape[0], tris.shape[0])
                if with_queries:
                    ren.trace_rays_multi(org, dirs, max_hits=4)
                    ren.pick_multi(u, xy, max_hits=2)
                ren.render_frame(u)
                if with_queries:                               # device path, enqueued behind the frame on rt_stream()'s stream
                    ren.trace_rays_multi(_to(org), _to(dirs), _to(tmax), max_hits=32)
                    ren.pick_multi(u, _to(xy), max_hits=0)
                out.append(ren.read_target(rt.RT_TARGET_COLOR).tobytes())
            out.append(ren.frame_index)
            out.append(ren.debug_builds(reset=False))
            if mega:
                c = ren.counters()
                assert c.raysClosest > 0 and c.raysShadow > 0
                out.append(bytes(c))
            tr = ren.traced_rays()
            assert mega or tr.primary > 0
            out.append({n: getattr(tr, n) for n, _ in tr._fields_})
        return out

    got, want = run(True), run(False)
    # (gatherLoadsShadow depends on the any-hit walks' dynamic scheduling and differs between two runs of the same frames: test_gpu_ray_query.py)
    gs, ws = got[-1].pop("gatherLoadsShadow"), want[-1].pop("gatherLoadsShadow")
    assert abs(gs - ws) <= 1e-3 * max(ws, 1), (gs, ws)
    assert got == want


def test_no_allocation_after_the_first_query():
    import torch
    nodes, tris, o, d, tm = _case("bunny")
    L = rt.lib()
    N = o.shape[0]
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        to, td, ttm = _to(o), _to(d), _to(tm)
        hits = torch.empty((N, 32, 4), dtype=torch.float32, device=_dev())
        count = torch.empty(N, dtype=torch.int32, device=_dev())
        xy = _to(np.zeros((N, 2), np.int32))
        u = rt.frame_uniforms(rt.default_render_params(), scenes.camera("closeup"), 64, 64, 0, True, nodes.shape[0], tris.shape[0])
        torch.cuda.synchronize()
        P = lambda t: C.c_void_p(t.data_ptr())

        def both(k):
            K = KS[::-1][k % len(KS)]
            rc = L.rt_trace_rays_multi(ren._h, P(to), 3, P(td), 3, P(ttm) if k & 1 else None, 1e-4, 1e30, N, K, P(hits), P(count))
            assert rc == rt.RT_OK, L.rt_last_error(ren._h)
            assert L.rt_pick_pixels_multi(ren._h, C.byref(u), P(xy), N, K, P(hits), P(count)) == rt.RT_OK, L.rt_last_error(ren._h)

        both(0)                                                    # the context's first queries (the largest K): the scratch, the kernels' code
        ren.synchronize()
        before = ren.memory_info()
        for k in range(20):
            both(k)
        ren.synchronize()
        after = ren.memory_info()
        assert bytes(after) == bytes(before), ({n: (getattr(before, n), getattr(after, n)) for n, _ in before._fields_})


# ---------------------------------------------------------------- 6: refusals

def test_every_refusal_leaves_the_outputs_unwritten():
    import torch
    L = rt.lib()
    nodes, tris, o, d, tm = ref.one_leaf_rays()
    o, d, tm = o[:8].copy(), d[:8].copy(), np.abs(tm[:8])
    N = 8
    hits, counts = np.full((N, 4, 4), f32(-7.5), f32), np.full(N, -77, np.int32)
    dh, dc = _to(hits), _to(counts)
    do, dd, dtm = _to(o), _to(d), _to(tm)
    xy = np.zeros((N, 2), np.int32)
    dxy = _to(xy)
    torch.cuda.synchronize()
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
    off = lambda a, k: C.c_void_p(P(a).value + k)
    u = rt.frame_uniforms(rt.default_render_params(), scenes.camera("closeup"), 64, 64, 0, True, nodes.shape[0], tris.shape[0])

    with rt.Renderer() as ren:
        h = ren._h
        err = lambda: L.rt_last_error(h).decode()

        def rays(host, o_=0, os_=3, d_=0, ds=3, t=None, n=N, K=4, hits_=0, counts_=0):
            A = (o, d, hits, counts) if host else (do, dd, dh, dc)
            fn = L.rt_trace_rays_multi_host if host else L.rt_trace_rays_multi
            pick = lambda x, a: P(a) if isinstance(x, int) and x == 0 else x
            return fn(h, pick(o_, A[0]), os_, pick(d_, A[1]), ds, t, 1e-4, 1e30, n, K, pick(hits_, A[2]), pick(counts_, A[3]))

        def pixels(host, u_=u, xy_=0, n=N, K=4, hits_=0, counts_=0):
            A = (xy, hits, counts) if host else (dxy, dh, dc)
            fn = L.rt_pick_pixels_multi_host if host else L.rt_pick_pixels_multi
            pick = lambda x, a: P(a) if isinstance(x, int) and x == 0 else x
            return fn(h, None if u_ is None else C.byref(u_), pick(xy_, A[0]), n, K, pick(hits_, A[1]), pick(counts_, A[2]))

        for host in (True, False):
            assert rays(host) == rt.RT_ERR_STATE and "no BVH uploaded" in err()
            assert pixels(host) == rt.RT_ERR_STATE and "uploaded 0 / 0" in err()
        ren.upload_bvh(nodes, tris)
        for host in (True, False):
            for K in (-1, rt.RT_MULTI_HIT_MAX + 1):
                assert rays(host, K=K) == rt.RT_ERR_INVALID and "RT_MULTI_HIT_MAX = 32" in err()
                assert pixels(host, K=K) == rt.RT_ERR_INVALID and "RT_MULTI_HIT_MAX = 32" in err()
            assert rays(host, n=-1) == rt.RT_ERR_INVALID and "n = -1" in err()
            assert pixels(host, n=-1) == rt.RT_ERR_INVALID and "n = -1" in err()
            assert rays(host, os_=2) == rt.RT_ERR_INVALID and "strides 2 / 3" in err()
            assert rays(host, ds=2) == rt.RT_ERR_INVALID and "strides 3 / 2" in err()
            assert rays(host, o_=None) == rt.RT_ERR_INVALID and "null ray arrays" in err()
            assert rays(host, d_=None) == rt.RT_ERR_INVALID and "null ray arrays" in err()
            assert rays(host, hits_=None) == rt.RT_ERR_INVALID and "needs hits" in err()
            assert rays(host, K=0, counts_=None) == rt.RT_ERR_INVALID and "needs counts" in err()
            assert pixels(host, hits_=None) == rt.RT_ERR_INVALID and "needs hits" in err()
            assert pixels(host, K=0, counts_=None) == rt.RT_ERR_INVALID and "needs counts" in err()
            assert rays(host, n=1 << 27, K=32) == rt.RT_ERR_INVALID and "INT32_MAX" in err()
            assert pixels(host, n=1 << 27, K=32) == rt.RT_ERR_INVALID and "INT32_MAX" in err()
            assert rays(host, n=1 << 30, K=1, os_=8) == rt.RT_ERR_INVALID and "2^32 floats" in err()
            assert pixels(host, u_=None) == rt.RT_ERR_INVALID and "null uniforms" in err()
            assert pixels(host, xy_=None) == rt.RT_ERR_INVALID and "null pixel array" in err()
            for mode in (0, rt.RT_SCENE_HYBRID):
                bad = rt.RtUniforms.from_buffer_copy(u)
                bad.useBVH = mode
                assert pixels(host, u_=bad) == rt.RT_ERR_INVALID and "BVH scene only" in err()
            bad = rt.RtUniforms.from_buffer_copy(u)
            bad.triCount = tris.shape[0] + 1
            assert pixels(host, u_=bad) == rt.RT_ERR_STATE and "uniforms name" in err()
            assert rays(host, n=0, o_=None, d_=None, hits_=None, counts_=None) == rt.RT_OK          # n == 0: a no-op
            assert pixels(host, n=0, xy_=None, hits_=None, counts_=None) == rt.RT_OK
        # the device entries: alignment
        assert rays(False, hits_=off(dh, 4)) == rt.RT_ERR_INVALID and "16-byte aligned" in err()
        assert rays(False, o_=off(do, 2)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert rays(False, counts_=off(dc, 1)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert rays(False, t=off(dtm, 3)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert pixels(False, hits_=off(dh, 8)) == rt.RT_ERR_INVALID and "16-byte aligned" in err()
        assert pixels(False, xy_=off(dxy, 2)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        ren.synchronize()
        assert (hits == f32(-7.5)).all() and (counts == -77).all()
        assert (dh.cpu().numpy() == f32(-7.5)).all() and (dc.cpu().numpy() == -77).all()
        # Python: refused before any call into the library
        for call in (lambda: ren.trace_rays_multi(o, d, max_hits=33), lambda: ren.pick_multi(u, xy, max_hits=-1), lambda: ren.trace_rays_multi(o[:, :2], d),
                     lambda: ren.trace_rays_multi(o, d[:3]), lambda: ren.trace_rays_multi(o.astype(np.float64), d), lambda: ren.trace_rays_multi(do, d),
                     lambda: ren.trace_rays_multi(torch.from_numpy(o), torch.from_numpy(d)), lambda: ren.pick_multi(u, xy.astype(np.int64)),
                     lambda: ren.trace_rays_multi(o, d, tm[:3])):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == rt.RT_ERR_INVALID
        # ... and a good call still works afterwards
        _same(ren.trace_rays_multi(o, d, tm, max_hits=4), rt.multi_hits(nodes, tris, o, d, tm, max_hits=4), "after the refusals")
        assert len(ren.trace_rays_multi(o[:0], d[:0])) == 0 and len(ren.pick_multi(u, xy[:0])) == 0
