"""Triangle queries on the GPU (rt_query_tris): every answer against rt.tri_overlaps -- the host definition, itself pinned to its numpy
restatement in test_tri_query_host.py -- on the same arrays, bit for bit and with no query left out: query counts about the wave and block sizes,
the counts alone, the exact two-pass lists and fixed capacities, numpy and torch, query layouts, `visits` against the reference walk element for
element and against the box query on the boxes of the queries' points, the entries no list reaches left as they were, every node form (in fresh child
processes), the dynamic mesh after a rebuild, a refit and a rebuild of parts (with mesh_hit_parts over .hits(), self queries from the device's
current rows, and every list ascending on the device builders' trees), stream ordering with torch, isolation from the frame state, no allocation
after the first query, and the refusals."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_fixtures as mf
import opengl_raytracing_amd as rt
import scenes
import tri_query_ref as ref

pytestmark = pytest.mark.gpu

f32 = np.float32
NS = (1, 63, 64, 65, 257, 2049)
CAPS = (0, 1, 8)
SENTINEL = -77
OPTION_VARS = ("RT_COOP", "RT_FUSED", "RT_IMPLICIT", "RT_NEAR_FIRST", "RT_QNODES", "RT_QNODES_SPARSE_BOXES", "RT_ANYHIT_TREE", "RT_LEAFB",
               "RT_LEAFB_CLOSEST", "RT_QUAD_REFILL", "RT_REFILL_MIN", "RT_GUIDED", "RT_CHUNK", "RT_MIN_SEARCH", "RT_REVERSE", "RT_DENSE_TAKE",
               "RT_TRACE_STATS", "RT_TRACE_TIMING", "RT_DEBUG_SKIP_TRAVERSAL", "RT_NEAREST_FAR_FIRST")
PIPELINES = {"megakernel": rt.RT_PIPELINE_MEGAKERNEL, "wavefront": rt.RT_PIPELINE_WAVEFRONT}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in OPTION_VARS:
        monkeypatch.delenv(v, raising=False)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _to(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, copy=True, order="C")).to(_dev())      # (the shared fixtures are read-only)


def _np(a):
    return a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()


def _lists(ans):
    """The list of every query of a TriOverlaps with exact slots."""
    prims, off = _np(ans.prims), _np(ans.offsets)
    return [prims[off[i]:off[i + 1]] for i in range(len(ans))]


def _expect(lists, offsets, sentinel):
    """What a call leaves of a prims array pre-filled with `sentinel`: slot i holds the first min(capacity, count) rows of lists[i]."""
    out = np.full(int(offsets[-1]), sentinel, np.int32)
    for i, rows in enumerate(lists):
        k = min(int(offsets[i + 1] - offsets[i]), rows.size)
        out[int(offsets[i]):int(offsets[i]) + k] = rows[:k]
    return out


def _same(got, lists, count, what, cap=None):
    """got (numpy or torch) against the host answer's lists and counts: count, offsets and prims, element for element."""
    gc, go, gp = _np(got.count), _np(got.offsets), _np(got.prims)
    n = len(lists)
    assert gc.dtype == np.int32 and go.dtype == np.int32 and gp.dtype == np.int32, what
    bad = np.flatnonzero(gc != count)
    assert bad.size == 0, (what, bad[:8], gc[bad[:8]], count[bad[:8]])
    want_off = np.concatenate([[0], np.cumsum(count)]) if cap is None else np.arange(n + 1) * cap
    assert np.array_equal(go, want_off), what
    want = _expect(lists, want_off, -1)
    assert gp.shape == want.shape, (what, gp.shape, want.shape)
    bad = np.flatnonzero(gp != want)
    assert bad.size == 0, (what, bad[:8], gp[bad[:8]], want[bad[:8]])


@functools.lru_cache(maxsize=None)
def _want(mesh):
    """(lists, count) of the host definition on all of case(mesh).  The answer of a query depends on that query alone, so the answer of a subset is
    the subset of the answers.  Computed once; leave it unchanged."""
    nodes, tris, qtris = ref.case(mesh)
    ans = rt.tri_overlaps(nodes, tris, qtris)
    return _lists(ans), ans.count


# ---------------------------------------------------------------- 1: against the definition

@pytest.mark.parametrize("mesh", ref.MESHES)
def test_answers_equal_the_definition(mesh):
    nodes, tris, qtris = ref.case(mesh)
    lists, count = _want(mesh)
    visits = ref.walk(mesh).visits
    assert qtris.shape[0] >= NS[-1]
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        for n in NS:
            pick = np.arange(n) * (qtris.shape[0] // n)               # across all the kinds of queries
            bn = np.ascontiguousarray(qtris[pick])
            ln, cn = [lists[i] for i in pick], count[pick]
            for arr, kind in ((bn, "numpy"),) + (((_to(bn), "torch"),) if n in (65, 2049) else ()):
                got = ren.tri_overlaps(arr, visits=True)
                _same(got, ln, cn, (mesh, n, kind, "exact"))
                assert np.array_equal(_np(got.visits), visits[pick]), (mesh, n, kind)
                assert np.array_equal(_np(got.pairs()), np.array([(i, t) for i, rows in enumerate(ln) for t in rows], np.int32).reshape(-1, 2))
                for cap in CAPS:
                    _same(ren.tri_overlaps(arr, cap=cap), ln, cn, (mesh, n, kind, cap), cap)
        got = ren.tri_overlaps(qtris, cap=8, visits=True)
        _same(got, lists, count, (mesh, "all"), 8)
        live = ref.live(qtris)
        assert np.array_equal(got.visits, visits) and (got.visits[~live] == 0).all() and (got.count[~live] == 0).all()
        assert got.visits.max() <= 2 * nodes.shape[0] and all((np.diff(r) > 0).all() for r in lists)
        # the walk is the box query's for [qlo, qhi]: the same visits from the box kernel on the same context, numpy and torch
        box = ref.aabb(qtris)
        box[~live] = np.nan                                            # (fmin / fmax pass over a NaN: the empty slots are marked again)
        assert np.array_equal(ren.box_overlaps(box, cap=0, visits=True).visits, got.visits)
        assert np.array_equal(_np(ren.box_overlaps(_to(box), cap=0, visits=True).visits), _np(ren.tri_overlaps(_to(qtris), cap=0, visits=True).visits))


def test_layouts_give_identical_bytes():
    nodes, tris, qtris = ref.case("bunny")
    lists, count = _want("bunny")
    N = qtris.shape[0]
    b7 = np.full((N, 12), np.nan, f32); b7[:, :9] = qtris
    i12 = np.full((N, 14), 9.0, f32); i12[:, 3:12] = qtris
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        t12 = _to(i12)
        for name, bb in {"numpy9": qtris, "numpy12": b7, "numpy view": i12[:, 3:12], "numpy 3x3": qtris.reshape(N, 3, 3), "torch9": _to(qtris), "torch12": _to(b7),
                         "torch view": t12[:, 3:12], "torch 3x3": _to(qtris).reshape(N, 3, 3)}.items():
            _same(ren.tri_overlaps(bb), lists, count, name)
            _same(ren.tri_overlaps(bb, cap=8), lists, count, name, 8)


def test_entries_no_list_reaches_are_left_as_they_were():
    """The C entries on arrays pre-filled with a sentinel, device and host path: the counts alone; lists alone in exact slots with a guard word behind;
    slots one short; fixed capacities; slots of negative length or with a negative start."""
    import torch
    L = rt.lib()
    nodes, tris, qtris = ref.case("bunny")
    lists, count = _want("bunny")
    N = qtris.shape[0]
    qtris = np.array(qtris)
    exact = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    short = np.concatenate([[0], np.cumsum(np.maximum(count - 1, 0))]).astype(np.int32)
    odd = np.array([3, 1, 1, -5, 2, 2], np.int32)
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        db = _to(qtris)
        for host in (True, False):
            fn = L.rt_query_tris_host if host else L.rt_query_tris
            put = (lambda a: None if a is None else np.array(a)) if host else _to
            get = _np

            def run(n, offsets, cap, room, with_counts, with_visits=False):
                prims = None if room is None else put(np.full(room, SENTINEL, np.int32))
                counts = put(np.full(n, SENTINEL, np.int32)) if with_counts else None
                vis = put(np.full(n, SENTINEL, np.int32)) if with_visits else None
                o = put(offsets)
                torch.cuda.synchronize()
                assert fn(ren._h, P(qtris if host else db), 9, n, P(o), cap, P(prims), P(counts), P(vis)) == rt.RT_OK, L.rt_last_error(ren._h)
                ren.synchronize()
                return get(prims), get(counts), get(vis)

            _, c, v = run(N, None, 0, None, True, True)                                     # the counts alone
            assert np.array_equal(c, count) and np.array_equal(v, ref.walk("bunny").visits), host
            p, c, _ = run(N, exact, 0, exact[-1] + 1, False)                                 # lists alone, a guard word behind the last slot
            assert c is None and np.array_equal(p[:-1], _expect(lists, exact, SENTINEL)) and p[-1] == SENTINEL, host
            p, c, _ = run(N, short, 0, short[-1], True)                                      # slots one short
            assert np.array_equal(p, _expect(lists, short, SENTINEL)) and np.array_equal(c, count), host
            for cap in (1, 8):
                off = np.arange(N + 1) * cap
                p, c, _ = run(N, None, cap, N * cap, cap == 8)
                want = _expect(lists, off, SENTINEL)
                assert np.array_equal(p, want) and (want == SENTINEL).any() and (c is None or np.array_equal(c, count)), (host, cap)
            if not host:                                                                     # (the host twin refuses offsets that descend)
                p, c, _ = run(5, odd, 0, 8, True)
                assert (p == SENTINEL).all() and np.array_equal(c, count[:5])


def _digest(lists, count):
    return hashlib.sha256(np.concatenate(lists).astype(np.int32).tobytes() + count.tobytes()).hexdigest()


_CHILD = r'''
import hashlib, sys, numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import opengl_raytracing_amd as rt, tri_query_ref as ref
nodes, tris, qtris = ref.case("bunny")
with rt.Renderer() as ren:
    ren.upload_bvh(nodes, tris)
    got = ren.tri_overlaps(qtris)
print("TRI_QUERY", hashlib.sha256(got.prims.tobytes() + got.count.tobytes()).hexdigest())
'''


@pytest.mark.parametrize("option", ["RT_QNODES=2", "RT_FUSED=1", "RT_IMPLICIT=1"])
def test_every_node_form_gives_identical_bytes(option):
    """The query reads the two-child records and the triangle rows alone: what else the upload builds does not matter.  The options are read from
    the environment of the process, so each runs in a fresh child."""
    want = _digest(*_want("bunny"))
    name, value = option.split("=")
    out = subprocess.run([sys.executable, "-c", _CHILD], cwd=str(scenes.ROOT), env=dict(os.environ, **{name: value}), capture_output=True, text=True, timeout=120)
    assert f"TRI_QUERY {want}" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---------------------------------------------------------------- 2: the dynamic mesh

def _want_parts(pf, order, prim):
    """The host formula of rt_mesh_hit_parts: (-1, -1) for a prim outside [0, nTris), else the part whose range holds order[prim] and the offset in it."""
    prim = np.asarray(prim).astype(np.int64)
    ok = (prim >= 0) & (prim < order.size)
    t = order[np.where(ok, prim, 0)].astype(np.int64)
    part = np.searchsorted(pf, t, "right") - 1
    return np.where(ok, part, -1).astype(np.int32), np.where(ok, t - pf[part], -1).astype(np.int32)


def _mesh_tris(host, seed):
    """Query triangles about a mesh: on its surface with edges 2^-k of the root extent, points at vertices, one that cuts the whole mesh, far away,
    empty slots."""
    rng = np.random.default_rng(seed)
    t = host.tris
    lo, hi = host.nodes[0, 0:3].astype(np.float64), host.nodes[0, 4:7].astype(np.float64)
    ext = hi - lo
    mid = (lo + hi) * 0.5
    k = rng.integers(0, t.shape[0], 400)
    w = rng.dirichlet((1, 1, 1), 400)
    on = t[k, 0:3] + t[k, 4:7] * w[:, 1:2] + t[k, 8:11] * w[:, 2:3]
    edge = ext * 2.0 ** -rng.integers(1, 9, (400, 1))
    far = mid + rng.normal(size=(40, 3)) * 20 * ext
    cut = np.concatenate([mid + ext * (-4, -4, 0.01), mid + ext * (4, -4, 0.02), mid + ext * (0, 6, -0.03)])
    q = np.concatenate([np.concatenate([on + rng.normal(size=(400, 3)) * edge for _ in range(3)], 1), np.tile(t[::9, 0:3], (1, 3)), cut[None],
                        np.concatenate([far + rng.normal(size=(40, 3)) * 0.1 * ext for _ in range(3)], 1)]).astype(f32)
    q[::97, 4] = np.nan
    q[1] = cut.astype(f32)                                          # (wherever the empty slots fell, the cutting triangle is there)
    return q


def _check_mesh_state(ren, host, pf, what):
    qtris = _mesh_tris(host, 23)
    want = rt.tri_overlaps(host.nodes, host.tris, qtris)
    lists = _lists(want)
    got = ren.tri_overlaps(qtris)
    _same(got, lists, want.count, (what, "numpy"))
    _same(ren.tri_overlaps(_to(qtris)), lists, want.count, (what, "torch"))
    got8 = ren.tri_overlaps(_to(qtris), cap=8)
    _same(got8, lists, want.count, (what, "torch, cap 8"), 8)
    assert (want.count == 0).sum() > 20 and ((want.count > 0) & (want.count < 8)).sum() > 20 and (want.count > 8).sum() > 20
    assert all((np.diff(r) > 0).all() for r in lists), what                 # ascending on the device builders' trees too
    for ans in (got, got8):                                                 # .hits() feeds mesh_hit_parts as it stands (prim -1: no part)
        rec = ans.hits()
        prim = _np(ans.prims)
        assert tuple(rec.shape) == (prim.size, 4)
        parts, offs = ren.mesh_hit_parts(rec)
        wp, wo = _want_parts(np.asarray(pf, np.int64), host.order, prim)
        assert np.array_equal(_np(parts), wp) and np.array_equal(_np(offs), wo), what
    assert (wp[prim < 0] == -1).all() and (prim < 0).any()
    # self queries: the device's current rows as query triangles, by the definition's adds, each list its own row
    rows = ren.debug_read_scene("tris").view(f32).reshape(-1, 12)[:host.tris.shape[0]]
    assert np.array_equal(rows, host.tris), what
    own = rt.rows_as_tris(rows)
    mine = ren.tri_overlaps(_to(own))
    _same(mine, _lists(rt.tri_overlaps(host.nodes, host.tris, own)), rt.tri_overlaps(host.nodes, host.tris, own).count, (what, "self"))
    pairs = _np(mine.pairs())
    assert np.isin(np.arange(own.shape[0]) * (1 << 32) + np.arange(own.shape[0]), pairs[:, 0].astype(np.int64) * (1 << 32) + pairs[:, 1]).all(), what
    assert np.array_equal(_np(rt.rows_as_tris(_to(rows))), own)


def test_dynamic_mesh_rebuild_refit_and_parts():
    v, f, _, _ = mf.sphere()
    n = f.size // 3
    with rt.Renderer() as ren:
        ren.mesh_upload(v, f)
        ren.mesh_rebuild(mf.turn(0))
        host = mf.HostMesh(f).rebuild(rt.gather_triangles(v, f, mf.turn(0)))
        _check_mesh_state(ren, host, [0, n], "rebuild")
        ren.mesh_refit(mf.turn(1))                       # the same tree under a turned matrix: qtris overlap, rows stay
        host.refit(rt.gather_triangles(v, f, mf.turn(1)))
        _check_mesh_state(ren, host, [0, n], "refit")
    v, f = mf.parts_mesh()
    with rt.Renderer() as ren:
        ren.mesh_upload_parts(v, f, mf.PART_FIRST)
        ren.mesh_set_part_matrices(mf.part_models(1))
        ren.mesh_rebuild_parts()
        host = mf.HostMesh(f).rebuild(rt.gather_triangles_parts(v, f, mf.PART_FIRST, mf.part_models(1)))
        _check_mesh_state(ren, host, mf.PART_FIRST, "parts")


# ---------------------------------------------------------------- 3: stream ordering with torch

def test_queries_written_by_torch_just_before_the_call_are_the_ones_queried():
    import torch
    nodes, tris, qtris = ref.case("bunny")
    lists, count = _want("bunny")
    dev = _dev()
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        b = torch.full((qtris.shape[0], 9), float("nan"), device=dev)  # placeholder queries: empty slots
        torch.cuda.synchronize()
        src = _to(qtris)
        x = torch.randn(4096, 4096, device=dev)
        for _ in range(8):                                          # keep torch's stream busy, so that the write below lands late
            x = x @ x
            x = x / x.norm()
        b.copy_(src)                                                # (enqueued behind the products)
        got = ren.tri_overlaps(b, cap=8)
        c, o, p = (a.clone().cpu().numpy() for a in (got.count, got.offsets, got.prims))          # read by torch on its own stream, no synchronise
        exact = ren.tri_overlaps(b)
    _same(rt.TriOverlaps(c, o, p), lists, count, "late queries", 8)
    _same(exact, lists, count, "late queries, exact")


def test_two_calls_on_two_torch_streams_without_a_host_wait():
    import torch
    nodes, tris, qtris = ref.case("layers")
    lists, count = _want("layers")
    _, _, bb = ref.case("bunny")                                   # (the bunny's queries against the layer stack: another count)
    other = rt.tri_overlaps(nodes, tris, bb)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        ta, tb = _to(qtris), _to(bb)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
        with torch.cuda.stream(s1):
            a = ren.tri_overlaps(ta, cap=8)
        with torch.cuda.stream(s2):
            b = ren.tri_overlaps(tb, cap=3)
        with torch.cuda.stream(s1):
            a2 = ren.tri_overlaps(ta, cap=8)
        torch.cuda.synchronize()
        _same(a, lists, count, "stream 1", 8); _same(b, _lists(other), other.count, "stream 2", 3); _same(a2, lists, count, "stream 1 again", 8)


# ---------------------------------------------------------------- 4: isolation from frames, no allocation

@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
def test_queries_do_not_touch_frame_state(pipeline):
    """Three BVH frames with triangle queries (host and device path) enqueued between them against the same three frames without: COLOR0 of every frame,
    the frame index, RtCounters (the megakernel's counting build), the traced-ray tallies and rt_debug_builds are identical."""
    nodes, tris = scenes.bunny_bvh(3)
    rng = np.random.default_rng(3)
    ctr = rng.uniform(nodes[0, 0:3] - 0.5, nodes[0, 4:7] + 0.5, (700, 3))
    qtris = np.concatenate([ctr + rng.uniform(-0.5, 0.5, (700, 3)) for _ in range(3)], 1).astype(f32)
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
                    ren.tri_overlaps(qtris, visits=True)
                ren.render_frame(u)
                if with_queries:                               # device path, enqueued behind the frame on rt_stream()'s stream
                    ren.tri_overlaps(_to(qtris), cap=8)
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
    nodes, tris, qtris = ref.case("bunny")
    _, count = _want("bunny")
    L = rt.lib()
    N, cap = qtris.shape[0], 8
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        tb = _to(qtris)
        off = _to(np.concatenate([[0], np.cumsum(count)]).astype(np.int32))
        prims = torch.empty(max(N * cap, int(count.sum())), dtype=torch.int32, device=_dev())
        counts = torch.empty(N, dtype=torch.int32, device=_dev())
        visits = torch.empty(N, dtype=torch.int32, device=_dev())
        torch.cuda.synchronize()
        P = lambda t: C.c_void_p(t.data_ptr())

        def call(k):
            form = k % 3                                           # the counts alone, fixed capacity, exact slots
            rc = L.rt_query_tris(ren._h, P(tb), 9, N, P(off) if form == 2 else None, cap, P(prims) if form else None,
                                  P(counts) if (form == 0 or k & 4) else None, P(visits) if k & 8 else None)
            assert rc == rt.RT_OK, L.rt_last_error(ren._h)

        for k in (0, 1, 2):                                        # the context's first queries: the scratch, the code of both builds of the walk
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
    nodes, tris, qtris = ref.case("one_leaf")
    N, cap = 8, 4
    qtris = np.array(qtris[1:1 + N])                               # (a copy: the shared fixtures are read-only)
    prims, counts, visits = np.full(N * cap, SENTINEL, np.int32), np.full(N, SENTINEL, np.int32), np.full(N, SENTINEL, np.int32)
    offsets = (np.arange(N + 1) * cap).astype(np.int32)
    db, dp, dn, dv, do = _to(qtris), _to(prims), _to(counts), _to(visits), _to(offsets)
    torch.cuda.synchronize()
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
    off = lambda a, k: C.c_void_p(P(a).value + k)

    with rt.Renderer() as ren:
        h = ren._h
        err = lambda: L.rt_last_error(h).decode()

        def call(host, b_=0, stride=9, n=N, offsets_=None, cap_=cap, prims_=0, counts_=0, visits_=0):
            A = (qtris, prims, counts, visits) if host else (db, dp, dn, dv)
            fn = L.rt_query_tris_host if host else L.rt_query_tris
            pick = lambda x, a: P(a) if isinstance(x, int) and x == 0 else x
            return fn(h, pick(b_, A[0]), stride, n, offsets_, cap_, pick(prims_, A[1]), pick(counts_, A[2]), pick(visits_, A[3]))

        for host in (True, False):
            assert call(host) == rt.RT_ERR_STATE and "no BVH uploaded" in err()
        ren.upload_bvh(nodes, tris)
        for host in (True, False):
            assert call(host, n=-1) == rt.RT_ERR_INVALID and "n = -1" in err()
            assert call(host, stride=8) == rt.RT_ERR_INVALID and "stride 8" in err()
            assert call(host, b_=None) == rt.RT_ERR_INVALID and "null triangle array" in err()
            assert call(host, prims_=None, counts_=None) == rt.RT_ERR_INVALID and "prims or counts" in err()
            assert call(host, cap_=-1) == rt.RT_ERR_INVALID and "cap = -1" in err()
            assert call(host, n=(1 << 31) // cap + 1) == rt.RT_ERR_INVALID and "INT32_MAX" in err()
            assert call(host, n=1 << 28, stride=32, prims_=None) == rt.RT_ERR_INVALID and "2^32 floats" in err()
            assert call(host, n=0, b_=None, prims_=None, counts_=None, visits_=None) == rt.RT_OK          # n == 0: a no-op
        # the host twin inspects its offsets; the device entry cannot
        assert call(True, offsets_=P(np.array([0, 4, 2, 8, 12, 16, 20, 24, 28], np.int32))) == rt.RT_ERR_INVALID and "descend" in err()
        assert call(True, offsets_=P(np.array([-4, 0, 4, 8, 12, 16, 20, 24, 28], np.int32))) == rt.RT_ERR_INVALID and "offsets[0]" in err()
        # the device entry: alignment
        assert call(False, b_=off(db, 2)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, offsets_=off(do, 1)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, prims_=off(dp, 3)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, counts_=off(dn, 1)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, visits_=off(dv, 2)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        ren.synchronize()
        assert (prims == SENTINEL).all() and (counts == SENTINEL).all() and (visits == SENTINEL).all()
        assert (dp.cpu().numpy() == SENTINEL).all() and (dn.cpu().numpy() == SENTINEL).all() and (dv.cpu().numpy() == SENTINEL).all()
        # Python: refused before any call into the library
        for bad in (lambda: ren.tri_overlaps(qtris[:, :8]), lambda: ren.tri_overlaps(qtris.astype(np.float64)), lambda: ren.tri_overlaps(torch.from_numpy(qtris)),
                    lambda: ren.tri_overlaps(db.double()), lambda: ren.tri_overlaps(qtris, cap=-1), lambda: ren.tri_overlaps(db.t()), lambda: ren.tri_overlaps(db.reshape(N, 3, 3).transpose(1, 2)), lambda: ren.tri_overlaps(list(qtris))):
            with pytest.raises(rt.RtError) as e:
                bad()
            assert e.value.code == rt.RT_ERR_INVALID
        # ... and a good call still works afterwards, on both paths and with the offsets
        want = rt.tri_overlaps(nodes, tris, qtris)
        _same(ren.tri_overlaps(qtris, visits=True), _lists(want), want.count, "after the refusals")
        for host in (True, False):
            assert call(host, offsets_=P(offsets) if host else P(do), cap_=0) == rt.RT_OK, err()
        ren.synchronize()
        filled = _expect(_lists(want), offsets, SENTINEL)
        assert np.array_equal(prims, filled) and np.array_equal(dp.cpu().numpy(), filled) and np.array_equal(counts, want.count) and np.array_equal(dn.cpu().numpy(), want.count)
        assert len(ren.tri_overlaps(qtris[:0])) == 0 and len(ren.tri_overlaps(db[:0])) == 0 and len(ren.tri_overlaps(db[:0], cap=4)) == 0
