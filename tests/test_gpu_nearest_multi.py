"""Proximity queries on the GPU (rt_query_nearest_multi): every answer against rt.nearest_points_multi -- the host definition, itself
pinned to its numpy restatement in test_nearest_multi_host.py -- on the same arrays, bit for bit: point counts about the wave and block sizes times
K = 0 .. 32 with and without counts, numpy and torch, point layouts, both visit orders, every node form (in fresh child processes), the dynamic mesh
after a rebuild, a refit and a rebuild of parts (and the mesh_hit_* queries over the flattened records), stream ordering with torch, isolation from
the frame state, no allocation after the first query, the refusals, and the cull as conditions on the boxes visited."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_fixtures as mf
import nearest_multi_ref as mref
import nearest_ref as ref
import opengl_raytracing_amd as rt
import scenes
from query_gpu import PIPELINES, _clean_env, dev as _dev, np_of as _np, to as _to  # noqa: F401  (_clean_env: autouse)

pytestmark = pytest.mark.gpu

f32 = np.float32
bits = ref.bits
NS = (1, 63, 64, 65, 257, 2049)
KS = (0, 1, 2, 4, 8, 32)


def _same(got, want, what, pick=None):
    """got (numpy or torch) against the rows `pick` of the host answer: hits, points and -- where got has it -- count, bit for bit."""
    pick = slice(None) if pick is None else pick
    gh, gp, gc = _np(got.hits), _np(got.points), _np(got.count)
    wh, wp, wc = want.hits[pick], want.points[pick], want.count[pick]
    assert gh.shape == wh.shape and gp.shape == wp.shape, (what, gh.shape, wh.shape)
    bad = np.flatnonzero((bits(gh) != bits(wh)).any((1, 2)))
    assert bad.size == 0, (what, bad[:8], gh[bad[:2]], wh[bad[:2]])
    bad = np.flatnonzero((bits(gp) != bits(wp)).any((1, 2)))
    assert bad.size == 0, (what, bad[:8], gp[bad[:2]], wp[bad[:2]])
    if gc is not None:
        bad = np.flatnonzero(gc != wc)
        assert bad.size == 0, (what, bad[:8], gc[bad[:8]], wc[bad[:8]])


@functools.lru_cache(maxsize=None)
def _want(mesh, K, limited):
    """The host definition on all of case(mesh) at limit(mesh) or without a limit.  The answer of a point depends on that point alone, so the
    answer of a subset is the subset of the answers.  Computed once; leave it unchanged."""
    nodes, tris, pts, _ = ref.case(mesh)
    return rt.nearest_points_multi(nodes, tris, pts, K, mref.limit(mesh) if limited else None)


# ---------------------------------------------------------------- 1: against the definition, in both visit orders

@pytest.mark.parametrize("order", ["near_first", "far_first"])
@pytest.mark.parametrize("mesh", mref.MESHES)
def test_answers_equal_the_definition(monkeypatch, mesh, order):
    if order == "far_first":
        monkeypatch.setenv("RT_NEAREST_FAR_FIRST", "1")
    nodes, tris, pts, _ = ref.case(mesh)
    md = mref.limit(mesh)
    assert pts.shape[0] >= NS[-1]
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        for n in NS:
            pick = np.arange(n) * (pts.shape[0] // n)               # across all the kinds of points
            pn, mn = np.ascontiguousarray(pts[pick]), np.ascontiguousarray(md[pick])
            tp, tm = (_to(pn), _to(mn)) if n in (65, 2049) else (None, None)
            for K in KS:
                for limited, m, t in ((False, None, None), (True, mn, tm)):
                    want = _want(mesh, K, limited)
                    for counts in ((True,) if K == 0 else (True, False)):
                        what = (mesh, order, n, K, limited, counts)
                        _same(ren.nearest_points_multi(pn, K, m, counts=counts), want, what + ("numpy",), pick)
                        if tp is not None:
                            _same(ren.nearest_points_multi(tp, K, t, counts=counts, visits=True), want, what + ("torch",), pick)
        for limited in (False, True):
            m = md if limited else None
            got = ren.nearest_points_multi(pts, 4, m, visits=True)
            _same(got, _want(mesh, 4, limited), (mesh, order, "all", limited))
            empty = ~np.isfinite(pts).all(1) if m is None else (~np.isfinite(pts).all(1) | (m < 0))
            assert (got.visits[empty] == 0).all() and (got.visits[~empty] >= 1).all() and got.visits.max() <= 2 * nodes.shape[0]
            assert (got.count[empty] == 0).all() and (got.prim[empty] == -1).all()


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("mesh", mref.MESHES)
def test_the_two_consistency_rules_on_the_device(mesh, limited):
    """1: with K = 1 the records and points are Renderer.nearest_points' bit for bit.  2: count > 0 exactly where it answers."""
    nodes, tris, pts, case_md = ref.case(mesh)
    md = case_md if limited else None                              # (nearest_ref's own random limits)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        one = ren.nearest_points(pts, md)
        for counts in (True, False):
            got = ren.nearest_points_multi(pts, 1, md, counts=counts)
            assert np.array_equal(bits(got.hits[:, 0]), bits(one.hits)) and np.array_equal(bits(got.points[:, 0]), bits(one.points)), counts
        got = ren.nearest_points_multi(pts, 0, md)
        assert got.hits.shape == (pts.shape[0], 0, 4) and np.array_equal(got.count > 0, one.prim >= 0)


def test_layouts_give_identical_bytes():
    nodes, tris, pts, _ = ref.case("bunny")
    md = mref.limit("bunny")
    N = pts.shape[0]
    p4 = np.zeros((N, 4), f32); p4[:, :3] = pts; p4[:, 3] = np.nan
    i8 = np.full((N, 8), 9.0, f32); i8[:, 2:5] = pts
    want = _want("bunny", 4, True)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        t8, tm = _to(i8), _to(md)
        for name, (pp, m) in {"numpy3": (pts, md), "numpy4": (p4, md), "numpy8": (i8[:, 2:5], md), "torch3": (_to(pts), tm), "torch4": (_to(p4), tm),
                              "torch8": (t8[:, 2:5], tm)}.items():
            _same(ren.nearest_points_multi(pp, 4, m), want, name)


def _digest(*answers):
    return hashlib.sha256(b"".join(a.hits.tobytes() + a.points.tobytes() + a.count.tobytes() for a in answers)).hexdigest()


_CHILD = r'''
import hashlib, sys, numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import opengl_raytracing_amd as rt, nearest_ref as ref, nearest_multi_ref as mref
nodes, tris, pts, _ = ref.case("bunny")
with rt.Renderer() as ren:
    ren.upload_bvh(nodes, tris)
    answers = (ren.nearest_points_multi(pts, 4), ren.nearest_points_multi(pts, 8, mref.limit("bunny")))
print("NEAREST_MULTI", hashlib.sha256(b"".join(a.hits.tobytes() + a.points.tobytes() + a.count.tobytes() for a in answers)).hexdigest())
'''


@pytest.mark.parametrize("option", ["RT_QNODES=2", "RT_FUSED=1", "RT_IMPLICIT=1"])
def test_every_node_form_gives_identical_bytes(option):
    """The query reads the two-child records and the triangle rows alone: what else the upload builds does not matter.  The options are read from
    the environment of the process, so each runs in a fresh child."""
    want = _digest(_want("bunny", 4, False), _want("bunny", 8, True))
    name, value = option.split("=")
    out = subprocess.run([sys.executable, "-c", _CHILD], cwd=str(scenes.ROOT), env=dict(os.environ, **{name: value}), capture_output=True, text=True, timeout=120)
    assert f"NEAREST_MULTI {want}" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---------------------------------------------------------------- 2: the dynamic mesh

def _want_parts(pf, order, prim):
    """The host formula of rt_mesh_hit_parts: (-1, -1) for a prim outside [0, nTris), else the part whose range holds order[prim] and the offset in it."""
    prim = np.asarray(prim).astype(np.int64)
    ok = (prim >= 0) & (prim < order.size)
    t = order[np.where(ok, prim, 0)].astype(np.int64)
    part = np.searchsorted(pf, t, "right") - 1
    return np.where(ok, part, -1).astype(np.int32), np.where(ok, t - pf[part], -1).astype(np.int32)


def _mesh_points(host, seed):
    """Points about a mesh: vertices of its rows, points near the surface, in the root box and far outside, and one limit for all (some slots empty)."""
    rng = np.random.default_rng(seed)
    t = host.tris
    lo, hi = host.nodes[0, 0:3], host.nodes[0, 4:7]
    ext = float((hi - lo).max())
    k = rng.integers(0, t.shape[0], 300)
    w = rng.dirichlet((1, 1, 1), 300)
    on = t[k, 0:3] + t[k, 4:7] * w[:, 1:2] + t[k, 8:11] * w[:, 2:3]
    pts = np.concatenate([t[::7, 0:3], (on + rng.normal(size=(300, 3)) * 0.03 * ext), rng.uniform(lo, hi, (150, 3)),
                          (lo + hi) * 0.5 + rng.normal(size=(64, 3)) * 20 * ext]).astype(f32)
    md = np.full(pts.shape[0], f32(0.08 * ext), f32)
    md[::97] = -1
    return pts, md


def _check_mesh_state(ren, host, f, pf, colors, what):
    pts, md = _mesh_points(host, 21)
    K = 4
    for m in (None, md):
        want = rt.nearest_points_multi(host.nodes, host.tris, pts, K, m)
        got = ren.nearest_points_multi(pts, K, m)
        _same(got, want, (what, m is not None))
        _same(ren.nearest_points_multi(_to(pts), K, _to(m), counts=False), want, (what, m is not None, "torch, culling"))
    rec = got.hits.reshape(-1, 4)                              # with the limit: full, partly filled and empty points, flattened
    prim = got.prim.reshape(-1)
    assert (got.count == 0).sum() > 50 and ((got.count > 0) & (got.count < K)).sum() > 0 and (got.count > K).sum() > 100
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


# ---------------------------------------------------------------- 3: stream ordering with torch

def test_points_written_by_torch_just_before_the_call_are_the_ones_queried():
    import torch
    nodes, tris, pts, _ = ref.case("bunny")
    dev = _dev()
    want = _want("bunny", 4, False)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        p = torch.zeros((pts.shape[0], 3), device=dev)              # placeholder points: the origin
        torch.cuda.synchronize()
        src = _to(pts)
        x = torch.randn(4096, 4096, device=dev)
        for _ in range(8):                                          # keep torch's stream busy, so that the write below lands late
            x = x @ x
            x = x / x.norm()
        p.copy_(src)                                                # (enqueued behind the products)
        got = ren.nearest_points_multi(p, 4)
        hits, closest, count = (a.clone().cpu().numpy() for a in (got.hits, got.points, got.count))      # read by torch on its own stream, no synchronise
    _same(rt.NearestMulti(hits, closest, count), want, "late points")


def test_two_calls_on_two_torch_streams_without_a_host_wait():
    import torch
    nodes, tris, pts, _ = ref.case("layers")
    md = mref.limit("layers")
    _, _, bp, _ = ref.case("bunny")                                # (the bunny's points against the layer stack: another count)
    want_a, want_b = _want("layers", 8, True), rt.nearest_points_multi(nodes, tris, bp, 2)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        ta, tb = (_to(pts), 8, _to(md)), (_to(bp), 2)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
        with torch.cuda.stream(s1):
            a = ren.nearest_points_multi(*ta)
        with torch.cuda.stream(s2):
            b = ren.nearest_points_multi(*tb)
        with torch.cuda.stream(s1):
            a2 = ren.nearest_points_multi(*ta)
        torch.cuda.synchronize()
        _same(a, want_a, "stream 1"); _same(b, want_b, "stream 2"); _same(a2, want_a, "stream 1 again")


# ---------------------------------------------------------------- 4: isolation from frames, no allocation

@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
def test_queries_do_not_touch_frame_state(pipeline):
    """Three BVH frames with proximity queries (host and device path) enqueued between them against the same three frames without: COLOR0 of
    every frame, the frame index, RtCounters (the megakernel's counting build), the traced-ray tallies and rt_debug_builds are identical."""
    nodes, tris = scenes.bunny_bvh(3)
    rng = np.random.default_rng(3)
    pts = rng.uniform(nodes[0, 0:3] - 0.5, nodes[0, 4:7] + 0.5, (700, 3)).astype(f32)
    md = rng.uniform(0, 1, 700).astype(f32)
    W, H = 160, 96
    cam = scenes.camera("closeup", aspect=W / H)
    p = rt.default_render_params()
    mega = pipeline == "megakernel"

    def run(with_queries):
        out = []
        with rt.Renderer(pipeline=PIPELINES[pipeline], count_work=mega) as ren:
            ren.upload_bvh(nodes, tris)
            ren.resize(W, H)
            for frame in range(3):
                u = rt.frame_uniforms(p, cam, W, H, frame, True, nodes.shape[0], tris.shape[0])
                if with_queries:
                    ren.nearest_points_multi(pts, 4, counts=False, visits=True)
                ren.render_frame(u)
                if with_queries:                               # device path, enqueued behind the frame on rt_stream()'s stream
                    ren.nearest_points_multi(_to(pts), 8, _to(md))
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
    nodes, tris, pts, _ = ref.case("bunny")
    md = mref.limit("bunny")
    L = rt.lib()
    N, K = pts.shape[0], 32
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        tp, tm = _to(pts), _to(md)
        hits = torch.empty((N, K, 4), dtype=torch.float32, device=_dev())
        closest = torch.empty((N, K, 3), dtype=torch.float32, device=_dev())
        counts = torch.empty(N, dtype=torch.int32, device=_dev())
        visits = torch.empty(N, dtype=torch.int32, device=_dev())
        torch.cuda.synchronize()
        P = lambda t: C.c_void_p(t.data_ptr())

        def call(k):
            maxHits = (0, 1, 4, 32)[k % 4]
            rc = L.rt_query_nearest_multi(ren._h, P(tp), 3, P(tm) if k & 1 else None, N, maxHits, P(hits), P(counts) if (k & 8 or maxHits == 0) else None,
                                          P(closest) if k & 2 else None, P(visits) if k & 4 else None)
            assert rc == rt.RT_OK, L.rt_last_error(ren._h)

        for k in (15, 7, 14, 6):                                   # the context's first queries: the scratch, the code of both builds of the walk
            call(k)
        ren.synchronize()
        before = ren.memory_info()
        for k in range(20):
            call(k)
        ren.synchronize()
        after = ren.memory_info()
        assert bytes(after) == bytes(before), ({n: (getattr(before, n), getattr(after, n)) for n, _ in before._fields_})


# ---------------------------------------------------------------- 5: refusals

def test_every_refusal_leaves_the_outputs_unwritten():
    import torch
    L = rt.lib()
    nodes, tris, pts, md = ref.case("one_leaf")
    N, K = 8, 4
    pts, md = np.array(pts[1:1 + N]), np.abs(md[1:1 + N])          # (copies: the shared fixtures are read-only)
    hits, closest = np.full((N, K, 4), f32(-7.5), f32), np.full((N, K, 3), f32(-7.5), f32)
    counts, visits = np.full(N, -77, np.int32), np.full(N, -77, np.int32)
    dh, dc, dn, dv = _to(hits), _to(closest), _to(counts), _to(visits)
    dp, dm = _to(pts), _to(md)
    torch.cuda.synchronize()
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
    off = lambda a, k: C.c_void_p(P(a).value + k)

    with rt.Renderer() as ren:
        h = ren._h
        err = lambda: L.rt_last_error(h).decode()

        def call(host, p_=0, stride=3, m=None, n=N, k=K, hits_=0, counts_=0, closest_=0, visits_=0):
            A = (pts, hits, counts, closest, visits) if host else (dp, dh, dn, dc, dv)
            fn = L.rt_query_nearest_multi_host if host else L.rt_query_nearest_multi
            pick = lambda x, a: P(a) if isinstance(x, int) and x == 0 else x
            return fn(h, pick(p_, A[0]), stride, m, n, k, pick(hits_, A[1]), pick(counts_, A[2]), pick(closest_, A[3]), pick(visits_, A[4]))

        for host in (True, False):
            assert call(host) == rt.RT_ERR_STATE and "no BVH uploaded" in err()
        ren.upload_bvh(nodes, tris)
        for host in (True, False):
            assert call(host, k=-1) == rt.RT_ERR_INVALID and "maxHits = -1" in err()
            assert call(host, k=33) == rt.RT_ERR_INVALID and "RT_NEAREST_MULTI_MAX" in err()
            assert call(host, k=0, counts_=None) == rt.RT_ERR_INVALID and "needs counts" in err()
            assert call(host, n=(1 << 31) // K + 1) == rt.RT_ERR_INVALID and "INT32_MAX" in err()
            assert call(host, n=-1) == rt.RT_ERR_INVALID and "n = -1" in err()
            assert call(host, stride=2) == rt.RT_ERR_INVALID and "stride 2" in err()
            assert call(host, p_=None) == rt.RT_ERR_INVALID and "null point array" in err()
            assert call(host, hits_=None) == rt.RT_ERR_INVALID and "needs hits" in err()
            assert call(host, n=1 << 28, stride=32, k=1) == rt.RT_ERR_INVALID and "2^32 floats" in err()
            assert call(host, n=0, p_=None, hits_=None, counts_=None, closest_=None, visits_=None) == rt.RT_OK          # n == 0: a no-op
        # the device entry: alignment
        assert call(False, hits_=off(dh, 4)) == rt.RT_ERR_INVALID and "16-byte aligned" in err()
        assert call(False, p_=off(dp, 2)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, m=off(dm, 3)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, counts_=off(dn, 1)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, closest_=off(dc, 1)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, visits_=off(dv, 2)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        ren.synchronize()
        assert (hits == f32(-7.5)).all() and (closest == f32(-7.5)).all() and (counts == -77).all() and (visits == -77).all()
        assert (dh.cpu().numpy() == f32(-7.5)).all() and (dc.cpu().numpy() == f32(-7.5)).all() and (dn.cpu().numpy() == -77).all() and (dv.cpu().numpy() == -77).all()
        # K = 0 with counts writes the counts alone, on both paths
        for host in (True, False):
            assert call(host, k=0, hits_=None, closest_=None, visits_=None, m=P(md) if host else P(dm)) == rt.RT_OK
        ren.synchronize()
        want0 = rt.nearest_points_multi(nodes, tris, pts, 0, md).count
        assert np.array_equal(counts, want0) and np.array_equal(dn.cpu().numpy(), want0) and (dh.cpu().numpy() == f32(-7.5)).all() and (hits == f32(-7.5)).all()
        # Python: refused before any call into the library
        for bad in (lambda: ren.nearest_points_multi(pts[:, :2], 2), lambda: ren.nearest_points_multi(pts.astype(np.float64), 2),
                    lambda: ren.nearest_points_multi(dp, 2, md), lambda: ren.nearest_points_multi(torch.from_numpy(pts), 2),
                    lambda: ren.nearest_points_multi(pts, 2, md[:3]), lambda: ren.nearest_points_multi(dp, 2, dm[:3]),
                    lambda: ren.nearest_points_multi(pts, 33), lambda: ren.nearest_points_multi(pts, -1), lambda: ren.nearest_points_multi(pts, 0, counts=False)):
            with pytest.raises(rt.RtError) as e:
                bad()
            assert e.value.code == rt.RT_ERR_INVALID
        # ... and a good call still works afterwards
        _same(ren.nearest_points_multi(pts, K, md, visits=True), rt.nearest_points_multi(nodes, tris, pts, K, md), "after the refusals")
        assert len(ren.nearest_points_multi(pts[:0], 2)) == 0 and len(ren.nearest_points_multi(dp[:0], 2)) == 0


# ---------------------------------------------------------------- 6: the cull, as conditions on the boxes visited

@pytest.mark.parametrize("order", ["near_first", "far_first"])
def test_one_record_without_counts_is_the_nearest_point_walk(monkeypatch, order):
    """K = 1 without counts culls against its best as rt_query_nearest does: the same boxes, element for element, in either order."""
    if order == "far_first":
        monkeypatch.setenv("RT_NEAREST_FAR_FIRST", "1")
    for mesh in ("bunny", "layers", "two_clusters"):
        nodes, tris, pts, md = ref.case(mesh)
        with rt.Renderer() as ren:
            ren.upload_bvh(nodes, tris)
            for m in (None, md):
                one = ren.nearest_points(pts, m, visits=True)
                got = ren.nearest_points_multi(pts, 1, m, counts=False, visits=True)
                got_t = ren.nearest_points_multi(_to(pts), 1, _to(m), counts=False, visits=True)
                assert np.array_equal(got.visits, one.visits) and np.array_equal(_np(got_t.visits), one.visits), (mesh, order, m is not None)
                assert np.array_equal(bits(got.hits[:, 0]), bits(one.hits))


def test_the_walk_culls_against_the_limit_and_against_its_kth_best():
    """The two-cluster mesh.  With counts, a point 1 000 units away with max_dist = 1 is done after the root box.  For every point, culling against
    the K-th best (no counts) never evaluates more boxes than culling against the limit alone (counts): its bound is never the larger one, and the
    walk with the smaller bound visits a subset of the nodes in the same order.  The answers are the same bytes."""
    nodes, tris, pts, _ = ref.case("two_clusters")
    md = mref.limit("two_clusters")
    far = np.array([[1000.0, 0.5, 1.0], [2.0, -1000.0, 1.0]], f32)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        away = ren.nearest_points_multi(far, 4, np.ones(2, f32), visits=True)
        away0 = ren.nearest_points_multi(_to(far), 0, _to(np.ones(2, f32)), visits=True)
        unbounded = ren.nearest_points_multi(far, 4, visits=True)
        assert (away.visits == 1).all() and (away.count == 0).all() and (away.prim == -1).all()
        assert (_np(away0.visits) == 1).all() and (_np(away0.count) == 0).all()
        assert (unbounded.count == tris.shape[0]).all() and (unbounded.visits == nodes.shape[0]).all()      # no limit, counts: every box
        less = 0
        for name in ("two_clusters", "bunny"):
            nodes, tris, pts, _ = ref.case(name)
            ren.upload_bvh(nodes, tris)
            for m in (None, mref.limit(name)):
                for K in (1, 4, 32):
                    with_counts = ren.nearest_points_multi(pts, K, m, counts=True, visits=True)
                    without = ren.nearest_points_multi(pts, K, m, counts=False, visits=True)
                    assert (without.visits <= with_counts.visits).all(), (name, K, m is not None)
                    assert np.array_equal(bits(without.hits), bits(with_counts.hits)) and np.array_equal(bits(without.points), bits(with_counts.points))
                    less += int((without.visits < with_counts.visits).sum())
        assert less > 0                                            # ... and the K-th best does cull
