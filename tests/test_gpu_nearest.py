"""Nearest-point queries on the GPU (rt_query_nearest): every answer against rt.nearest_points -- the host definition, itself pinned to
its numpy restatement in test_nearest_host.py -- on the same arrays, bit for bit: point counts about the wave and block sizes, numpy and torch, point
layouts, both visit orders, every node form (in fresh child processes), the dynamic mesh after a rebuild, a refit and a rebuild of parts (and the
mesh_hit_* queries over the records), stream ordering with torch, isolation from the frame state, no allocation after the first query, the
refusals, and the cull as a condition on the boxes visited."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_fixtures as mf
import nearest_ref as ref
import opengl_raytracing_amd as rt
import scenes
from query_gpu import PIPELINES, _clean_env, dev as _dev, np_of as _np, to as _to  # noqa: F401  (_clean_env: autouse)

pytestmark = pytest.mark.gpu

f32 = np.float32
bits = ref.bits
NS = (1, 63, 64, 65, 257, 2049)


def _same(got, want, what):
    gh, gp = _np(got.hits), _np(got.points)
    assert gh.shape == want.hits.shape and gp.shape == want.points.shape, what
    bad = np.flatnonzero((bits(gh) != bits(want.hits)).any(1))
    assert bad.size == 0, (what, bad[:8], gh[bad[:2]], want.hits[bad[:2]])
    bad = np.flatnonzero((bits(gp) != bits(want.points)).any(1))
    assert bad.size == 0, (what, bad[:8], gp[bad[:2]], want.points[bad[:2]])


# ---------------------------------------------------------------- 1: against the definition, in both visit orders

@pytest.mark.parametrize("order", ["near_first", "far_first"])
@pytest.mark.parametrize("mesh", ref.MESHES)
def test_answers_equal_the_definition(monkeypatch, mesh, order):
    if order == "far_first":
        monkeypatch.setenv("RT_NEAREST_FAR_FIRST", "1")
    nodes, tris, pts, md = ref.case(mesh)
    assert pts.shape[0] >= NS[-1]
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        for n in NS:
            pick = np.arange(n) * (pts.shape[0] // n)               # across all the kinds of points
            pn, mn = np.ascontiguousarray(pts[pick]), np.ascontiguousarray(md[pick])
            for m in (None, mn):
                want = rt.nearest_points(nodes, tris, pn, m)
                _same(ren.nearest_points(pn, m), want, (mesh, order, n, m is not None, "numpy"))
                if n in (65, 2049):
                    _same(ren.nearest_points(_to(pn), _to(m), visits=True), want, (mesh, order, n, m is not None, "torch"))
        for m in (None, md):
            full = rt.nearest_points(nodes, tris, pts, m)
            got = ren.nearest_points(pts, m, visits=True)
            _same(got, full, (mesh, order, "all", m is not None))
            empty = ~np.isfinite(pts).all(1) if m is None else (~np.isfinite(pts).all(1) | (m < 0))
            assert (got.visits[empty] == 0).all() and (got.visits[~empty] >= 1).all() and got.visits.max() <= 2 * nodes.shape[0]
            assert (got.prim[empty] == -1).all()


def test_the_two_orders_visit_differently_and_answer_alike(monkeypatch):
    """The switch does change the walk: the farther child first finds a farther first candidate and culls less, so over 3 799 points it evaluates
    more boxes in total -- and the bytes of the answer are the same."""
    nodes, tris, pts, md = ref.case("bunny")
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        near = ren.nearest_points(pts, visits=True)
        monkeypatch.setenv("RT_NEAREST_FAR_FIRST", "1")
        far = ren.nearest_points(pts, visits=True)
        far_t = ren.nearest_points(_to(pts), visits=True)
    assert np.array_equal(bits(near.hits), bits(far.hits)) and np.array_equal(bits(near.points), bits(far.points))
    assert np.array_equal(far.visits, _np(far_t.visits))
    assert int(near.visits.sum()) < int(far.visits.sum())


def test_layouts_give_identical_bytes():
    nodes, tris, pts, md = ref.case("bunny")
    N = pts.shape[0]
    p4 = np.zeros((N, 4), f32); p4[:, :3] = pts; p4[:, 3] = np.nan
    i8 = np.full((N, 8), 9.0, f32); i8[:, 2:5] = pts
    want = rt.nearest_points(nodes, tris, pts, md)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        t8, tm = _to(i8), _to(md)
        for name, (pp, m) in {"numpy3": (pts, md), "numpy4": (p4, md), "numpy8": (i8[:, 2:5], md), "torch3": (_to(pts), tm), "torch4": (_to(p4), tm),
                              "torch8": (t8[:, 2:5], tm)}.items():
            _same(ren.nearest_points(pp, m), want, name)


_CHILD = r'''
import hashlib, sys, numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import opengl_raytracing_amd as rt, nearest_ref as ref
nodes, tris, pts, md = ref.case("bunny")
with rt.Renderer() as ren:
    ren.upload_bvh(nodes, tris)
    a, b = ren.nearest_points(pts), ren.nearest_points(pts, md)
print("NEAREST", hashlib.sha256(a.hits.tobytes() + a.points.tobytes() + b.hits.tobytes() + b.points.tobytes()).hexdigest())
'''


@pytest.mark.parametrize("option", ["RT_QNODES=2", "RT_FUSED=1", "RT_IMPLICIT=1"])
def test_every_node_form_gives_identical_bytes(option):
    """The query reads the two-child records and the triangle rows alone: what else the upload builds does not matter.  The options are read from
    the environment of the process, so each runs in a fresh child."""
    nodes, tris, pts, md = ref.case("bunny")
    a, b = rt.nearest_points(nodes, tris, pts), rt.nearest_points(nodes, tris, pts, md)
    want = hashlib.sha256(a.hits.tobytes() + a.points.tobytes() + b.hits.tobytes() + b.points.tobytes()).hexdigest()
    name, value = option.split("=")
    out = subprocess.run([sys.executable, "-c", _CHILD], cwd=str(scenes.ROOT), env=dict(os.environ, **{name: value}), capture_output=True, text=True, timeout=120)
    assert f"NEAREST {want}" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---------------------------------------------------------------- 2: the dynamic mesh

def _want_parts(pf, order, prim):
    """The host formula of rt_mesh_hit_parts: (-1, -1) for a prim outside [0, nTris), else the part whose range holds order[prim] and the offset in it."""
    prim = np.asarray(prim).astype(np.int64)
    ok = (prim >= 0) & (prim < order.size)
    t = order[np.where(ok, prim, 0)].astype(np.int64)
    part = np.searchsorted(pf, t, "right") - 1
    return np.where(ok, part, -1).astype(np.int32), np.where(ok, t - pf[part], -1).astype(np.int32)


def _mesh_points(host, seed):
    """Points about a mesh: vertices of its rows, points near the surface, in the root box and far outside, and a limit for each (some slots empty)."""
    rng = np.random.default_rng(seed)
    t = host.tris
    lo, hi = host.nodes[0, 0:3], host.nodes[0, 4:7]
    ext = float((hi - lo).max())
    k = rng.integers(0, t.shape[0], 300)
    w = rng.dirichlet((1, 1, 1), 300)
    on = t[k, 0:3] + t[k, 4:7] * w[:, 1:2] + t[k, 8:11] * w[:, 2:3]
    pts = np.concatenate([t[::7, 0:3], (on + rng.normal(size=(300, 3)) * 0.03 * ext), rng.uniform(lo, hi, (150, 3)),
                          (lo + hi) * 0.5 + rng.normal(size=(64, 3)) * 20 * ext]).astype(f32)
    md = rng.uniform(0, 0.3 * ext, pts.shape[0]).astype(f32)
    md[::97] = -1
    return pts, md


def _check_mesh_state(ren, host, f, pf, colors, what):
    pts, md = _mesh_points(host, 21)
    for m in (None, md):
        want = rt.nearest_points(host.nodes, host.tris, pts, m)
        got = ren.nearest_points(pts, m)
        _same(got, want, (what, m is not None))
        _same(ren.nearest_points(_to(pts), _to(m)), want, (what, m is not None, "torch"))
    rec = got.hits                                             # with the limits: answers and misses
    prim = got.prim
    assert (prim < 0).sum() > 50 and (prim >= 0).sum() > 100
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
    nodes, tris, pts, md = ref.case("bunny")
    dev = _dev()
    want = rt.nearest_points(nodes, tris, pts)
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
        got = ren.nearest_points(p)
        hits, closest = got.hits.clone().cpu().numpy(), got.points.clone().cpu().numpy()      # read by torch on its own stream, no synchronise
    _same(rt.NearestPoints(hits, closest), want, "late points")


def test_two_calls_on_two_torch_streams_without_a_host_wait():
    import torch
    nodes, tris, pts, md = ref.case("layers")
    _, _, bp, bm = ref.case("bunny")                               # (the bunny's points against the layer stack: another count)
    want_a, want_b = rt.nearest_points(nodes, tris, pts, md), rt.nearest_points(nodes, tris, bp)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        ta, tb = (_to(pts), _to(md)), (_to(bp),)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
        with torch.cuda.stream(s1):
            a = ren.nearest_points(*ta)
        with torch.cuda.stream(s2):
            b = ren.nearest_points(*tb)
        with torch.cuda.stream(s1):
            a2 = ren.nearest_points(*ta)
        torch.cuda.synchronize()
        _same(a, want_a, "stream 1"); _same(b, want_b, "stream 2"); _same(a2, want_a, "stream 1 again")


# ---------------------------------------------------------------- 4: isolation from frames, no allocation

@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
def test_queries_do_not_touch_frame_state(pipeline):
    """Three BVH frames with nearest-point queries (host and device path) enqueued between them against the same three frames without: COLOR0 of
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
                    ren.nearest_points(pts, visits=True)
                ren.render_frame(u)
                if with_queries:                               # device path, enqueued behind the frame on rt_stream()'s stream
                    ren.nearest_points(_to(pts), _to(md))
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
    nodes, tris, pts, md = ref.case("bunny")
    L = rt.lib()
    N = pts.shape[0]
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        tp, tm = _to(pts), _to(md)
        hits = torch.empty((N, 4), dtype=torch.float32, device=_dev())
        closest = torch.empty((N, 3), dtype=torch.float32, device=_dev())
        visits = torch.empty(N, dtype=torch.int32, device=_dev())
        torch.cuda.synchronize()
        P = lambda t: C.c_void_p(t.data_ptr())

        def call(k):
            rc = L.rt_query_nearest(ren._h, P(tp), 3, P(tm) if k & 1 else None, N, P(hits), P(closest) if k & 2 else None, P(visits) if k & 4 else None)
            assert rc == rt.RT_OK, L.rt_last_error(ren._h)

        call(7)                                                    # the context's first query: the scratch, the kernels' code
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
    N = 8
    pts, md = np.array(pts[1:1 + N]), np.abs(md[1:1 + N])          # (copies: the shared fixtures are read-only)
    hits, closest, visits = np.full((N, 4), f32(-7.5), f32), np.full((N, 3), f32(-7.5), f32), np.full(N, -77, np.int32)
    dh, dc, dv = _to(hits), _to(closest), _to(visits)
    dp, dm = _to(pts), _to(md)
    torch.cuda.synchronize()
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
    off = lambda a, k: C.c_void_p(P(a).value + k)

    with rt.Renderer() as ren:
        h = ren._h
        err = lambda: L.rt_last_error(h).decode()

        def call(host, p_=0, stride=3, m=None, n=N, hits_=0, closest_=0, visits_=0):
            A = (pts, hits, closest, visits) if host else (dp, dh, dc, dv)
            fn = L.rt_query_nearest_host if host else L.rt_query_nearest
            pick = lambda x, a: P(a) if isinstance(x, int) and x == 0 else x
            return fn(h, pick(p_, A[0]), stride, m, n, pick(hits_, A[1]), pick(closest_, A[2]), pick(visits_, A[3]))

        for host in (True, False):
            assert call(host) == rt.RT_ERR_STATE and "no BVH uploaded" in err()
        ren.upload_bvh(nodes, tris)
        for host in (True, False):
            assert call(host, n=-1) == rt.RT_ERR_INVALID and "n = -1" in err()
            assert call(host, stride=2) == rt.RT_ERR_INVALID and "stride 2" in err()
            assert call(host, p_=None) == rt.RT_ERR_INVALID and "null point array" in err()
            assert call(host, hits_=None) == rt.RT_ERR_INVALID and "needs hits" in err()
            assert call(host, n=1 << 30, stride=8) == rt.RT_ERR_INVALID and "2^32 floats" in err()
            assert call(host, n=0, p_=None, hits_=None, closest_=None, visits_=None) == rt.RT_OK          # n == 0: a no-op
        # the device entry: alignment
        assert call(False, hits_=off(dh, 4)) == rt.RT_ERR_INVALID and "16-byte aligned" in err()
        assert call(False, p_=off(dp, 2)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, m=off(dm, 3)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, closest_=off(dc, 1)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, visits_=off(dv, 2)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        ren.synchronize()
        assert (hits == f32(-7.5)).all() and (closest == f32(-7.5)).all() and (visits == -77).all()
        assert (dh.cpu().numpy() == f32(-7.5)).all() and (dc.cpu().numpy() == f32(-7.5)).all() and (dv.cpu().numpy() == -77).all()
        # Python: refused before any call into the library
        for bad in (lambda: ren.nearest_points(pts[:, :2]), lambda: ren.nearest_points(pts.astype(np.float64)), lambda: ren.nearest_points(dp, md),
                    lambda: ren.nearest_points(torch.from_numpy(pts)), lambda: ren.nearest_points(pts, md[:3]), lambda: ren.nearest_points(dp, dm[:3])):
            with pytest.raises(rt.RtError) as e:
                bad()
            assert e.value.code == rt.RT_ERR_INVALID
        # ... and a good call still works afterwards
        _same(ren.nearest_points(pts, md, visits=True), rt.nearest_points(nodes, tris, pts, md), "after the refusals")
        assert len(ren.nearest_points(pts[:0])) == 0 and len(ren.nearest_points(dp[:0])) == 0


# ---------------------------------------------------------------- 6: the cull, as a condition

def test_the_walk_culls_against_its_best():
    """The two-cluster mesh, near child first.  A point within 1 unit of cluster A tests the root, its two children and the child boxes inside A's
    subtree; B's subtree waits on the stack with lbEff ~ 95^2 and is dropped at the pop without a box test: visits <= (nNodes - 1) / 2 + 2.  A walk
    that did not cull would test every box of B as well.  A point 1 000 units away with max_dist = 1 is done after the root box."""
    nodes, tris, pts, md = ref.case("two_clusters")
    free = rt.nearest_points(nodes, tris, pts)
    near_a = (free.prim >= 0) & (free.dist2 <= 1.0) & (pts[:, 0] < 50)
    assert near_a.sum() > 500
    p = np.ascontiguousarray(pts[near_a])
    far = np.array([[1000.0, 0.5, 1.0], [2.0, -1000.0, 1.0]], f32)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        got = ren.nearest_points(p, visits=True)
        got_t = ren.nearest_points(_to(p), visits=True)
        away = ren.nearest_points(far, np.ones(2, f32), visits=True)
        unbounded = ren.nearest_points(far, visits=True)
    _same(got, rt.nearest_points(nodes, tris, p), "near cluster A")
    bound = (nodes.shape[0] - 1) // 2 + 2
    assert got.visits.max() <= bound, (int(got.visits.max()), bound)
    assert np.array_equal(got.visits, _np(got_t.visits))
    assert (away.visits == 1).all() and (away.prim == -1).all()
    assert (unbounded.prim >= 0).all() and (unbounded.visits > 1).all()
