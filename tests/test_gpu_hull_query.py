"""Hull queries on the GPU (rt_query_hulls, rt_pick_rects): every answer against rt.hull_overlaps -- the host definition, itself pinned to
its numpy restatement in test_hull_query_host.py -- on the same arrays, bit for bit and with no query left out: query counts about the wave and block
sizes, the counts alone, the exact two-pass lists and fixed capacities, numpy and torch, query layouts, `visits` against the reference walk element
for element, the entries no list reaches left as they were, every node form (in fresh child processes), the dynamic mesh after a rebuild, a refit and
a rebuild of parts (with mesh_hit_parts over .hits() and the oriented box of a part), marquee picking against rt.rect_frusta, Renderer.pick and
Renderer.pick_multi, stream ordering with torch, isolation from the frame state, no allocation after the first query, and the refusals."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import hull_query_ref as ref
import mesh_fixtures as mf
import opengl_raytracing_amd as rt
import scenes

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
    """The list of every query of a HullOverlaps with exact slots."""
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


def _bits(a):
    return np.ascontiguousarray(_np(a), f32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _want(mesh):
    """(lists, count) of the host definition on all of case(mesh).  The answer of a query depends on that query alone, so the answer of a subset is
    the subset of the answers.  Computed once; leave it unchanged."""
    nodes, tris, hulls = ref.case(mesh)
    ans = rt.hull_overlaps(nodes, tris, hulls)
    return _lists(ans), ans.count


# ---------------------------------------------------------------- 1: against the definition

@pytest.mark.parametrize("mesh", ref.MESHES)
def test_answers_equal_the_definition(mesh):
    nodes, tris, hulls = ref.case(mesh)
    lists, count = _want(mesh)
    visits = ref.walk(mesh).visits
    assert hulls.shape[0] >= NS[-1]
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        for n in NS:
            pick = np.arange(n) * (hulls.shape[0] // n)               # across all the kinds of queries
            bn = np.ascontiguousarray(hulls[pick])
            ln, cn = [lists[i] for i in pick], count[pick]
            for arr, kind in ((bn, "numpy"),) + (((_to(bn), "torch"),) if n in (65, 2049) else ()):
                got = ren.hull_overlaps(arr, visits=True)
                assert isinstance(got, rt.HullOverlaps) and got.corners is None
                _same(got, ln, cn, (mesh, n, kind, "exact"))
                assert np.array_equal(_np(got.visits), visits[pick]), (mesh, n, kind)
                assert np.array_equal(_np(got.pairs()), np.array([(i, t) for i, rows in enumerate(ln) for t in rows], np.int32).reshape(-1, 2))
                for cap in CAPS:
                    _same(ren.hull_overlaps(arr, cap=cap), ln, cn, (mesh, n, kind, cap), cap)
        got = ren.hull_overlaps(hulls, cap=8, visits=True)
        _same(got, lists, count, (mesh, "all"), 8)
        live = ref.live(hulls)
        assert np.array_equal(got.visits, visits) and (got.visits[~live] == 0).all() and (got.count[~live] == 0).all()
        assert got.visits.max() <= 2 * nodes.shape[0] and all((np.diff(r) > 0).all() for r in lists)
        # the six normals only ever spare visits: never more than the box kernel's on [lo, hi], on the same context
        box = ref.aabb(hulls)
        box[~live] = np.nan                                            # (fmin / fmax pass over a NaN: the empty slots are marked again)
        plain = ren.box_overlaps(box, cap=0, visits=True).visits
        assert (got.visits <= plain).all() and np.array_equal(plain, ref.box_visits(nodes, hulls))


def test_layouts_give_identical_bytes():
    nodes, tris, hulls = ref.case("bunny")
    lists, count = _want("bunny")
    N = hulls.shape[0]
    b32 = np.full((N, 32), np.nan, f32); b32[:, :24] = hulls
    i30 = np.full((N, 30), 9.0, f32); i30[:, 3:27] = hulls
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        t30 = _to(i30)
        for name, bb in {"numpy24": hulls, "numpy32": b32, "numpy view": i30[:, 3:27], "numpy 8x3": hulls.reshape(N, 8, 3), "torch24": _to(hulls), "torch32": _to(b32),
                         "torch view": t30[:, 3:27], "torch 8x3": _to(hulls).reshape(N, 8, 3)}.items():
            _same(ren.hull_overlaps(bb), lists, count, name)
            _same(ren.hull_overlaps(bb, cap=8), lists, count, name, 8)


def test_entries_no_list_reaches_are_left_as_they_were():
    """The C entries on arrays pre-filled with a sentinel, device and host path: the counts alone; lists alone in exact slots with a guard word behind;
    slots one short; fixed capacities; slots of negative length or with a negative start."""
    import torch
    L = rt.lib()
    nodes, tris, hulls = ref.case("bunny")
    lists, count = _want("bunny")
    N = hulls.shape[0]
    hulls = np.array(hulls)
    exact = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    short = np.concatenate([[0], np.cumsum(np.maximum(count - 1, 0))]).astype(np.int32)
    odd = np.array([3, 1, 1, -5, 2, 2], np.int32)
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        db = _to(hulls)
        for host in (True, False):
            fn = L.rt_query_hulls_host if host else L.rt_query_hulls
            put = (lambda a: None if a is None else np.array(a)) if host else _to
            get = _np

            def run(n, offsets, cap, room, with_counts, with_visits=False):
                prims = None if room is None else put(np.full(room, SENTINEL, np.int32))
                counts = put(np.full(n, SENTINEL, np.int32)) if with_counts else None
                vis = put(np.full(n, SENTINEL, np.int32)) if with_visits else None
                o = put(offsets)
                torch.cuda.synchronize()
                assert fn(ren._h, P(hulls if host else db), 24, n, P(o), cap, P(prims), P(counts), P(vis)) == rt.RT_OK, L.rt_last_error(ren._h)
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
import opengl_raytracing_amd as rt, hull_query_ref as ref
nodes, tris, hulls = ref.case("bunny")
with rt.Renderer() as ren:
    ren.upload_bvh(nodes, tris)
    got = ren.hull_overlaps(hulls)
print("HULL_QUERY", hashlib.sha256(got.prims.tobytes() + got.count.tobytes()).hexdigest())
'''


@pytest.mark.parametrize("option", ["RT_QNODES=2", "RT_FUSED=1", "RT_IMPLICIT=1"])
def test_every_node_form_gives_identical_bytes(option):
    """The query reads the two-child records and the triangle rows alone: what else the upload builds does not matter.  The options are read from
    the environment of the process, so each runs in a fresh child."""
    want = _digest(*_want("bunny"))
    name, value = option.split("=")
    out = subprocess.run([sys.executable, "-c", _CHILD], cwd=str(scenes.ROOT), env=dict(os.environ, **{name: value}), capture_output=True, text=True, timeout=120)
    assert f"HULL_QUERY {want}" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---------------------------------------------------------------- 2: the dynamic mesh

def _want_parts(pf, order, prim):
    """The host formula of rt_mesh_hit_parts: (-1, -1) for a prim outside [0, nTris), else the part whose range holds order[prim] and the offset in it."""
    prim = np.asarray(prim).astype(np.int64)
    ok = (prim >= 0) & (prim < order.size)
    t = order[np.where(ok, prim, 0)].astype(np.int64)
    part = np.searchsorted(pf, t, "right") - 1
    return np.where(ok, part, -1).astype(np.int32), np.where(ok, t - pf[part], -1).astype(np.int32)


def _mesh_hulls(host, seed):
    """Hulls about a mesh: sheared boxes on its surface with edges 2^-k of the root extent, generic hexahedra, points at vertices, a slab that cuts the
    whole mesh, far away, empty slots."""
    rng = np.random.default_rng(seed)
    t = host.tris
    lo, hi = host.nodes[0, 0:3].astype(np.float64), host.nodes[0, 4:7].astype(np.float64)
    ext = hi - lo
    mid = (lo + hi) * 0.5
    k = rng.integers(0, t.shape[0], 400)
    w = rng.dirichlet((1, 1, 1), 400)
    on = (t[k, 0:3] + t[k, 4:7] * w[:, 1:2] + t[k, 8:11] * w[:, 2:3]).astype(np.float64)
    half = ext * 2.0 ** -rng.integers(1, 9, (400, 1)) * rng.uniform(0.3, 1.0, (400, 3))
    Ms = np.stack([ref._matrix(rng, i % 3, on[i]) for i in range(400)]).astype(f32)
    boxes = rt.box_corners(np.concatenate([-half, half], 1).astype(f32), Ms)
    generic = ref.generic_hexahedra(rng, on[:200], float(ext.max()) * 2.0 ** -rng.uniform(1, 8, 200)).astype(f32)
    far = ref.generic_hexahedra(rng, mid + rng.normal(size=(40, 3)) * 20 * ext, np.full(40, 0.1 * float(ext.max()))).astype(f32)
    cut = rt.box_corners(np.concatenate([mid - ext * (4, 4, 0.01), mid + ext * (4, 4, 0.02)])[None].astype(f32), ref._matrix(rng, 2, np.zeros(3)).astype(f32))
    q = np.concatenate([boxes, generic, np.tile(t[::9, 0:3], (1, 8)), cut, far]).astype(f32)
    q[::97, 4] = np.nan
    q[1] = cut[0]                                                   # (wherever the empty slots fell, the cutting slab is there)
    return q


def _check_mesh_state(ren, host, pf, what):
    hulls = _mesh_hulls(host, 23)
    want = rt.hull_overlaps(host.nodes, host.tris, hulls)
    lists = _lists(want)
    got = ren.hull_overlaps(hulls)
    _same(got, lists, want.count, (what, "numpy"))
    _same(ren.hull_overlaps(_to(hulls)), lists, want.count, (what, "torch"))
    got8 = ren.hull_overlaps(_to(hulls), cap=8)
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


def test_dynamic_mesh_rebuild_refit_and_parts():
    v, f, _, _ = mf.sphere()
    n = f.size // 3
    with rt.Renderer() as ren:
        ren.mesh_upload(v, f)
        ren.mesh_rebuild(mf.turn(0))
        host = mf.HostMesh(f).rebuild(rt.gather_triangles(v, f, mf.turn(0)))
        _check_mesh_state(ren, host, [0, n], "rebuild")
        ren.mesh_refit(mf.turn(1))                       # the same tree under a turned matrix: the hulls overlap other rows, the rows stay
        host.refit(rt.gather_triangles(v, f, mf.turn(1)))
        _check_mesh_state(ren, host, [0, n], "refit")
    v, f = mf.parts_mesh()
    models = mf.part_models(1)
    with rt.Renderer() as ren:
        ren.mesh_upload_parts(v, f, mf.PART_FIRST)
        ren.mesh_set_part_matrices(models)
        ren.mesh_rebuild_parts()
        host = mf.HostMesh(f).rebuild(rt.gather_triangles_parts(v, f, mf.PART_FIRST, models))
        _check_mesh_state(ren, host, mf.PART_FIRST, "parts")
        # The trigger volume that moves with a part: the part's object-space box, grown by a thousandth of its extent so that no vertex lies on a
        # face, under the part's own matrix.  It lists every row of its part -- it encloses them --, and rows of those parts alone whose world boxes
        # its own box reaches
        pf = np.asarray(mf.PART_FIRST, np.int64)
        fi = np.asarray(f, np.int64).reshape(-1, 3)
        obj = []
        for p in range(pf.size - 1):
            pts = np.asarray(v, f32).reshape(-1, 3)[fi[pf[p]:pf[p + 1]].reshape(-1)]
            grow = f32(1e-3) * (pts.max(0) - pts.min(0))
            obj.append(np.concatenate([pts.min(0) - grow, pts.max(0) + grow]))
        hulls = rt.box_corners(np.array(obj, f32), np.asarray(models, f32).reshape(-1, 16))
        got = ren.hull_overlaps(_to(hulls))
        want = rt.hull_overlaps(host.nodes, host.tris, hulls)
        _same(got, _lists(want), want.count, "part boxes")
        part_of_row = np.searchsorted(pf, host.order.astype(np.int64), "right") - 1
        a, b, c = ref.row_points(host.tris)
        rlo, rhi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        box = ref.aabb(hulls)
        for p, rows in enumerate(_lists(want)):
            assert set(np.flatnonzero(part_of_row == p)) <= set(rows), p
            for other in set(part_of_row[rows]):
                mine = part_of_row == other
                assert (rlo[mine].min(0) <= box[p, 3:6]).all() and (box[p, 0:3] <= rhi[mine].max(0)).all(), (p, other)


# ---------------------------------------------------------------- 3: marquee picking

def _frame(nodes, tris, W, H, jitter):
    """The uniforms of a W x H BVH frame whose camera is hull_query_ref.view's."""
    u = rt.frame_uniforms(rt.default_render_params(), scenes.camera("closeup", aspect=W / H), W, H, 0, True, nodes.shape[0], tris.shape[0])
    cam = ref.view("bunny", W, H, jitter)
    for name in ("camPos", "camRight", "camUp", "camFwd"):
        for k in range(3):
            getattr(u, name)[k] = getattr(cam, name)[k]
    u.tanHalfFov, u.aspect = cam.tanHalfFov, cam.aspect
    u.enableJitter, u.jitter[0], u.jitter[1] = cam.enableJitter, cam.jitter[0], cam.jitter[1]
    return u


@pytest.mark.parametrize("jitter", [None, (0.31, -0.22)])
def test_pick_rects_against_rect_frusta_pick_and_pick_multi(jitter):
    nodes, tris = ref.mesh("bunny")
    assert tris.shape[0] == 320
    W, H = 48, 36
    u = _frame(nodes, tris, W, H, jitter)
    rects = np.array([[0, 0, W, H], [2 * W, 0, 3 * W, H], [10, 8, 30, 25], [20.25, 14.5, 27.75, 19], [23, 17, 24, 18], [0, 0, 12, 36], [30, 20, 47.5, 35.5],
                      [-5, -5, 20, 12], [24, 0, 24, 36], [np.nan, 0, 4, 4], [9, 9, 8, 10]], f32)
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H), indexing="xy"), -1).reshape(-1, 2).astype(np.int32)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        for t_near in (0.0, 0.25):
            want_corners = rt.rect_frusta(u, nodes[0, 0:3], nodes[0, 4:7], rects, t_near)
            want = rt.hull_overlaps(nodes, tris, want_corners)
            for arr, kind in ((rects, "numpy"), (_to(rects), "torch")):
                got = ren.pick_rects(u, arr, t_near=t_near, visits=True)
                assert isinstance(got, rt.HullOverlaps) and np.array_equal(_bits(got.corners), _bits(want_corners)), (kind, t_near)
                _same(got, _lists(want), want.count, ("pick_rects", kind, t_near))
                assert np.array_equal(_np(got.visits), ref.Walk(nodes, tris.shape[0], want_corners).visits)
                _same(ren.pick_rects(u, arr, t_near=t_near, cap=8), _lists(want), want.count, ("pick_rects", kind, t_near, 8), 8)
                _same(ren.hull_overlaps(got.corners), _lists(want), want.count, ("hull_overlaps on the corners", kind))
        wide = np.full((rects.shape[0], 6), np.nan, f32); wide[:, :4] = rects
        far = 2.0 * float((nodes[0, 4:7] - nodes[0, 0:3]).max())
        got = ren.pick_rects(u, _to(wide)[:, :4], t_near=0.1, t_far=far)           # strided rows, a far depth of the caller's
        assert np.array_equal(_bits(got.corners), _bits(rt.rect_frusta(u, nodes[0, 0:3], nodes[0, 4:7], rects, 0.1, far)))
        # what the pixels show, and what lies behind them
        got = ren.pick_rects(u, rects)
        lists = _lists(got)
        first = ren.pick(u, xy).prim
        deep = ren.pick_multi(u, xy, max_hits=32)
        assert (first >= 0).sum() > 150 and (deep.count > 1).sum() > 100 and deep.count.max() <= 32
        cx, cy = xy[:, 0] + 0.5, xy[:, 1] + 0.5
        for i, r in enumerate(rects):
            inside = (r[0] < cx) & (cx < r[2]) & (r[1] < cy) & (cy < r[3])
            shown = set(first[inside & (first >= 0)]) | set(deep.prim[inside][deep.prim[inside] >= 0])
            assert shown <= set(lists[i]), (i, sorted(shown - set(lists[i])))
        assert set(first[first >= 0]) | set(deep.prim[deep.prim >= 0]) <= set(lists[0]) and len(lists[0]) > 100
        assert [len(lists[i]) for i in (1, 9, 10)] == [0, 0, 0] and 0 < len(lists[4]) < len(lists[3]) < len(lists[2]) < len(lists[0])


# ---------------------------------------------------------------- 4: stream ordering with torch

def test_queries_written_by_torch_just_before_the_call_are_the_ones_queried():
    import torch
    nodes, tris, hulls = ref.case("bunny")
    lists, count = _want("bunny")
    dev = _dev()
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        b = torch.full((hulls.shape[0], 24), float("nan"), device=dev)  # placeholder queries: empty slots
        torch.cuda.synchronize()
        src = _to(hulls)
        x = torch.randn(4096, 4096, device=dev)
        for _ in range(8):                                          # keep torch's stream busy, so that the write below lands late
            x = x @ x
            x = x / x.norm()
        b.copy_(src)                                                # (enqueued behind the products)
        got = ren.hull_overlaps(b, cap=8)
        c, o, p = (a.clone().cpu().numpy() for a in (got.count, got.offsets, got.prims))          # read by torch on its own stream, no synchronise
        exact = ren.hull_overlaps(b)
    _same(rt.HullOverlaps(c, o, p), lists, count, "late queries", 8)
    _same(exact, lists, count, "late queries, exact")


def test_two_calls_on_two_torch_streams_without_a_host_wait():
    import torch
    nodes, tris, hulls = ref.case("layers")
    lists, count = _want("layers")
    _, _, bb = ref.case("bunny")                                   # (the bunny's queries against the layer stack: another count)
    other = rt.hull_overlaps(nodes, tris, bb)
    u = _frame(nodes, tris, 48, 36, None)
    rects = np.array([[0, 0, 48, 36], [10, 10, 20, 20]], f32)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        ta, tb, tr = _to(hulls), _to(bb), _to(rects)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(_dev()), torch.cuda.Stream(_dev())
        with torch.cuda.stream(s1):
            a = ren.hull_overlaps(ta, cap=8)
        with torch.cuda.stream(s2):
            b = ren.hull_overlaps(tb, cap=3)
            r = ren.pick_rects(u, tr, cap=8)
        with torch.cuda.stream(s1):
            a2 = ren.hull_overlaps(ta, cap=8)
        torch.cuda.synchronize()
        _same(a, lists, count, "stream 1", 8); _same(b, _lists(other), other.count, "stream 2", 3); _same(a2, lists, count, "stream 1 again", 8)
        wr = rt.hull_overlaps(nodes, tris, rt.rect_frusta(u, nodes[0, 0:3], nodes[0, 4:7], rects))
        _same(r, _lists(wr), wr.count, "rects on stream 2", 8)


# ---------------------------------------------------------------- 5: isolation from frames, no allocation

@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
def test_queries_do_not_touch_frame_state(pipeline):
    """Three BVH frames with hull queries and rect picks (host and device path) enqueued between them against the same three frames without: COLOR0 of
    every frame, the frame index, RtCounters (the megakernel's counting build), the traced-ray tallies and rt_debug_builds are identical."""
    nodes, tris = scenes.bunny_bvh(3)
    rng = np.random.default_rng(3)
    ctr = rng.uniform(nodes[0, 0:3] - 0.5, nodes[0, 4:7] + 0.5, (700, 3))
    hulls = ref.generic_hexahedra(rng, ctr, rng.uniform(0.1, 0.6, 700)).astype(f32)
    W, H = 160, 96
    rects = np.array([[0, 0, W, H], [40, 30, 90, 70]], f32)
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
                    ren.hull_overlaps(hulls, visits=True)
                    ren.pick_rects(u, rects, cap=8)
                ren.render_frame(u)
                if with_queries:                               # device path, enqueued behind the frame on rt_stream()'s stream
                    ren.hull_overlaps(_to(hulls), cap=8)
                    ren.pick_rects(u, _to(rects), cap=8)
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
    nodes, tris, hulls = ref.case("bunny")
    _, count = _want("bunny")
    L = rt.lib()
    N, cap = hulls.shape[0], 8
    u = _frame(nodes, tris, 48, 36, None)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        tb = _to(hulls)
        off = _to(np.concatenate([[0], np.cumsum(count)]).astype(np.int32))
        prims = torch.empty(max(N * cap, int(count.sum())), dtype=torch.int32, device=_dev())
        counts = torch.empty(N, dtype=torch.int32, device=_dev())
        visits = torch.empty(N, dtype=torch.int32, device=_dev())
        rects = _to(np.tile(np.array([[3, 4, 20, 30]], f32), (64, 1)))
        corners = torch.empty((64, 24), dtype=torch.float32, device=_dev())
        torch.cuda.synchronize()
        P = lambda t: C.c_void_p(t.data_ptr())

        def call(k):
            form = k % 3                                           # the counts alone, fixed capacity, exact slots
            rc = L.rt_query_hulls(ren._h, P(tb), 24, N, P(off) if form == 2 else None, cap, P(prims) if form else None,
                                   P(counts) if (form == 0 or k & 4) else None, P(visits) if k & 8 else None)
            assert rc == rt.RT_OK, L.rt_last_error(ren._h)
            rc = L.rt_pick_rects(ren._h, C.byref(u), P(rects), 4, 64, 0.0, -1.0, P(corners), None, cap, P(prims) if form else None, P(counts), None)
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


# ---------------------------------------------------------------- 6: refusals

def test_every_refusal_leaves_the_outputs_unwritten():
    import torch
    L = rt.lib()
    nodes, tris, hulls = ref.case("one_leaf")
    N, cap = 8, 4
    hulls = np.array(hulls[1:1 + N])                               # (a copy: the shared fixtures are read-only)
    prims, counts, visits = np.full(N * cap, SENTINEL, np.int32), np.full(N, SENTINEL, np.int32), np.full(N, SENTINEL, np.int32)
    offsets = (np.arange(N + 1) * cap).astype(np.int32)
    rects = np.tile(np.array([[3, 4, 20, 30]], f32), (N, 1))
    corners = np.full((N, 24), SENTINEL, f32)
    db, dp, dn, dv, do, dr, dc = _to(hulls), _to(prims), _to(counts), _to(visits), _to(offsets), _to(rects), _to(corners)
    torch.cuda.synchronize()
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
    off = lambda a, k: C.c_void_p(P(a).value + k)
    u = _frame(nodes, tris, 48, 36, None)

    with rt.Renderer() as ren:
        h = ren._h
        err = lambda: L.rt_last_error(h).decode()

        def call(host, b_=0, stride=24, n=N, offsets_=None, cap_=cap, prims_=0, counts_=0, visits_=0):
            A = (hulls, prims, counts, visits) if host else (db, dp, dn, dv)
            fn = L.rt_query_hulls_host if host else L.rt_query_hulls
            pick = lambda x, a: P(a) if isinstance(x, int) and x == 0 else x
            return fn(h, pick(b_, A[0]), stride, n, offsets_, cap_, pick(prims_, A[1]), pick(counts_, A[2]), pick(visits_, A[3]))

        def rect_call(host, u_=0, r_=0, stride=4, n=N, t_near=0.0, t_far=-1.0, corners_=0, cap_=cap, prims_=0, counts_=0):
            A = (rects, corners, prims, counts, visits) if host else (dr, dc, dp, dn, dv)
            fn = L.rt_pick_rects_host if host else L.rt_pick_rects
            pick = lambda x, a: P(a) if isinstance(x, int) and x == 0 else x
            return fn(h, C.byref(u) if isinstance(u_, int) else u_, pick(r_, A[0]), stride, n, t_near, t_far, pick(corners_, A[1]), None, cap_, pick(prims_, A[2]),
                      pick(counts_, A[3]), P(A[4]))

        for host in (True, False):
            assert call(host) == rt.RT_ERR_STATE and "no BVH uploaded" in err()
            assert rect_call(host) == rt.RT_ERR_STATE and "no BVH uploaded" in err()
        ren.upload_bvh(nodes, tris)
        bad_res = _frame(nodes, tris, 48, 36, None)
        bad_res.resolution[0] = 0.0
        for host in (True, False):
            assert call(host, n=-1) == rt.RT_ERR_INVALID and "n = -1" in err()
            assert call(host, stride=23) == rt.RT_ERR_INVALID and "stride 23" in err()
            assert call(host, b_=None) == rt.RT_ERR_INVALID and "null hull array" in err()
            assert call(host, prims_=None, counts_=None) == rt.RT_ERR_INVALID and "prims or counts" in err()
            assert call(host, cap_=-1) == rt.RT_ERR_INVALID and "cap = -1" in err()
            assert call(host, n=(1 << 31) // cap + 1) == rt.RT_ERR_INVALID and "INT32_MAX" in err()
            assert call(host, n=1 << 28, stride=32, prims_=None) == rt.RT_ERR_INVALID and "2^32 floats" in err()
            assert call(host, n=0, b_=None, prims_=None, counts_=None, visits_=None) == rt.RT_OK          # n == 0: a no-op
            assert rect_call(host, u_=None) == rt.RT_ERR_INVALID and "null uniforms" in err()
            assert rect_call(host, u_=C.byref(bad_res)) == rt.RT_ERR_INVALID and "resolution" in err()
            assert rect_call(host, stride=3) == rt.RT_ERR_INVALID and "stride 3" in err()
            assert rect_call(host, t_near=-1.0) == rt.RT_ERR_INVALID and "tNear" in err()
            assert rect_call(host, t_near=float("nan")) == rt.RT_ERR_INVALID
            assert rect_call(host, t_far=float("nan")) == rt.RT_ERR_INVALID
            assert rect_call(host, r_=None) == rt.RT_ERR_INVALID and "null rect or corner array" in err()
            assert rect_call(host, corners_=None) == rt.RT_ERR_INVALID and "null rect or corner array" in err()
            assert rect_call(host, n=-1) == rt.RT_ERR_INVALID and "n = -1" in err()
            assert rect_call(host, prims_=None, counts_=None) == rt.RT_ERR_INVALID and "prims or counts" in err()
            assert rect_call(host, cap_=-1) == rt.RT_ERR_INVALID and "cap = -1" in err()
        # the host twin inspects its offsets; the device entry cannot
        assert call(True, offsets_=P(np.array([0, 4, 2, 8, 12, 16, 20, 24, 28], np.int32))) == rt.RT_ERR_INVALID and "descend" in err()
        assert call(True, offsets_=P(np.array([-4, 0, 4, 8, 12, 16, 20, 24, 28], np.int32))) == rt.RT_ERR_INVALID and "offsets[0]" in err()
        # the device entry: alignment
        assert call(False, b_=off(db, 2)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, offsets_=off(do, 1)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, prims_=off(dp, 3)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, counts_=off(dn, 1)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert call(False, visits_=off(dv, 2)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert rect_call(False, r_=off(dr, 2)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        assert rect_call(False, corners_=off(dc, 1)) == rt.RT_ERR_INVALID and "4-byte aligned" in err()
        ren.synchronize()
        assert (prims == SENTINEL).all() and (counts == SENTINEL).all() and (visits == SENTINEL).all() and (corners == SENTINEL).all()
        assert (dp.cpu().numpy() == SENTINEL).all() and (dn.cpu().numpy() == SENTINEL).all() and (dv.cpu().numpy() == SENTINEL).all()
        assert (dc.cpu().numpy() == SENTINEL).all()
        # Python: refused before any call into the library
        for bad in (lambda: ren.hull_overlaps(hulls[:, :23]), lambda: ren.hull_overlaps(hulls.astype(np.float64)), lambda: ren.hull_overlaps(torch.from_numpy(hulls)),
                    lambda: ren.hull_overlaps(db.double()), lambda: ren.hull_overlaps(hulls, cap=-1), lambda: ren.hull_overlaps(db.t()),
                    lambda: ren.hull_overlaps(db.reshape(N, 8, 3).transpose(1, 2)), lambda: ren.hull_overlaps(list(hulls)), lambda: ren.pick_rects(u, rects[:, :3]),
                    lambda: ren.pick_rects(u, rects.astype(np.float64)), lambda: ren.pick_rects(u, torch.from_numpy(rects)), lambda: ren.pick_rects(u, dr.t()),
                    lambda: ren.pick_rects(u, rects, cap=-1), lambda: ren.pick_rects(u, rects, t_near=-1.0), lambda: ren.pick_rects(None, rects),
                    lambda: ren.pick_rects(None, dr)):
            with pytest.raises(rt.RtError) as e:
                bad()
            assert e.value.code == rt.RT_ERR_INVALID
        # ... and a good call still works afterwards, on both paths and with the offsets
        want = rt.hull_overlaps(nodes, tris, hulls)
        _same(ren.hull_overlaps(hulls, visits=True), _lists(want), want.count, "after the refusals")
        for host in (True, False):
            assert call(host, offsets_=P(offsets) if host else P(do), cap_=0) == rt.RT_OK, err()
        ren.synchronize()
        filled = _expect(_lists(want), offsets, SENTINEL)
        assert np.array_equal(prims, filled) and np.array_equal(dp.cpu().numpy(), filled) and np.array_equal(counts, want.count) and np.array_equal(dn.cpu().numpy(), want.count)
        assert len(ren.hull_overlaps(hulls[:0])) == 0 and len(ren.hull_overlaps(db[:0])) == 0 and len(ren.hull_overlaps(db[:0], cap=4)) == 0
        assert len(ren.pick_rects(u, rects[:0])) == 0 and len(ren.pick_rects(u, dr[:0], cap=4)) == 0
