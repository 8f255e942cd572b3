"""The tests that the three overlap queries share (25: one walk, three shapes), as bodies over a Shape: what differs between
boxes, triangles and hulls is a field of the record -- the reference module, the floats per query, the entry names, the query sets -- or a small
callable on it.  tests/test_{box,tri,hull}_query_host.py and tests/test_gpu_{box,tri,hull}_query.py keep every test, with its name, parametrisation
and docstring, and call the body with BOX, TRI or HULL; what exists for one shape only stays in that file.

A body holds no branch on which shape it runs for.  Where one file's test checked more than the others', the check is a hook on the shape that the
body calls -- `each_answer`, `after_answers`, `mesh_state_extra`, `after_parts`, `on_stream2`, `with_frames`, `more_calls`, `host_extra` -- and does
nothing for the shapes that had none."""
import ctypes as C
import dataclasses
import functools
import hashlib
import os
import subprocess
import sys
import types
import typing

import numpy as np
import pytest

import box_query_ref
import hull_query_ref
import mesh_fixtures as mf
import opengl_raytracing_amd as rt
import scenes
import tri_query_ref
from query_gpu import PIPELINES, dev, np_of, to

f32 = np.float32
NS = (1, 63, 64, 65, 257, 2049)
CAPS = (0, 1, 8)
HOST_CAPS = (0, 1, 3, 8)
SENTINEL = -77


def _nothing(*args):
    return None


@dataclasses.dataclass(frozen=True, eq=False)
class Shape:
    ref: types.ModuleType                      # the numpy definition and the query sets
    floats: int                                # per query
    strides: tuple                             # of the strided host test
    padded: int                                # floats per row of the padded layout, the query first
    inner: int                                 # floats per row of the layout that holds the query from float 3 on
    points: typing.Optional[int]               # the queries may come as [N, points, 3]; None: as [N, floats] alone
    name: str                                  # rt.<name> (host definition) and Renderer.<name>
    raw: str                                   # the host definition's C entry
    query: str                                 # the context's C entry; <query>_host is its host-memory twin
    tag: str                                   # what the child process of the node-form test prints before its digest
    result: type                               # what both Python entries return
    noun: str                                  # as the refusal of a null query array names it
    first: int                                 # the first of the four queries of the host refusal test
    visits: typing.Callable                    # mesh -> the reference walk's visits on ref.case(mesh)
    pairs: typing.Callable                     # answer -> its [P,2] (query, row) pairs
    mesh_queries: typing.Callable              # (HostMesh, seed) -> queries about a dynamic mesh
    frame_queries: typing.Callable             # (rng, centres [700,3]) -> the queries enqueued between frames
    swapped_queries: typing.Callable           # () -> the three queries of the hand-made tree
    each_answer: typing.Callable = _nothing    # (got): on every answer of test_answers_equal_the_definition
    after_answers: typing.Callable = _nothing  # (ren, nodes, queries, live, got): at its end, got = all queries with cap 8 and visits
    mesh_state_extra: typing.Callable = _nothing   # (ren, host, want, what): at the end of every mesh state
    after_parts: typing.Callable = _nothing    # (ren, host, v, f, models): after the parts' state
    on_stream2: typing.Callable = lambda ren, nodes, tris: (_nothing, _nothing)   # -> (enqueue on stream 2, check after the synchronise)
    with_frames: typing.Callable = _nothing    # (ren, u, W, H, put): further queries beside each of the shape's between frames
    more_calls: typing.Callable = lambda ren, nodes, tris: _nothing   # -> call(form, cap, prims, counts) beside each query of the allocation test
    host_extra: typing.Callable = _nothing     # (got, tris): on the exact host answer

    def host(self, *args, **kw):
        return getattr(rt, self.name)(*args, **kw)

    def device(self, ren, *args, **kw):
        return getattr(ren, self.name)(*args, **kw)


# ================================================================ the GPU side

def _lists(ans):
    """The list of every query of an answer with exact slots."""
    prims, off = np_of(ans.prims), np_of(ans.offsets)
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
    gc, go, gp = np_of(got.count), np_of(got.offsets), np_of(got.prims)
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
def _want(shape, mesh):
    """(lists, count) of the host definition on all of case(mesh).  The answer of a query depends on that query alone, so the answer of a subset is
    the subset of the answers.  Computed once; leave it unchanged."""
    nodes, tris, q = shape.ref.case(mesh)
    ans = shape.host(nodes, tris, q)
    return _lists(ans), ans.count


def _pairs_of(lists):
    return np.array([(i, t) for i, rows in enumerate(lists) for t in rows], np.int32).reshape(-1, 2)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


# ---------------------------------------------------------------- 1: against the definition

def answers_equal_the_definition(shape, mesh):
    nodes, tris, q = shape.ref.case(mesh)
    lists, count = _want(shape, mesh)
    visits = shape.visits(mesh)
    assert q.shape[0] >= NS[-1]
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        for n in NS:
            pick = np.arange(n) * (q.shape[0] // n)                   # across all the kinds of queries
            bn = np.ascontiguousarray(q[pick])
            ln, cn = [lists[i] for i in pick], count[pick]
            for arr, kind in ((bn, "numpy"),) + (((to(bn), "torch"),) if n in (65, 2049) else ()):
                got = shape.device(ren, arr, visits=True)
                shape.each_answer(got)
                _same(got, ln, cn, (mesh, n, kind, "exact"))
                assert np.array_equal(np_of(got.visits), visits[pick]), (mesh, n, kind)
                assert np.array_equal(np_of(shape.pairs(got)), _pairs_of(ln))
                for cap in CAPS:
                    _same(shape.device(ren, arr, cap=cap), ln, cn, (mesh, n, kind, cap), cap)
        got = shape.device(ren, q, cap=8, visits=True)
        _same(got, lists, count, (mesh, "all"), 8)
        live = shape.ref.live(q)
        assert np.array_equal(got.visits, visits) and (got.visits[~live] == 0).all() and (got.count[~live] == 0).all()
        assert got.visits.max() <= 2 * nodes.shape[0] and all((np.diff(r) > 0).all() for r in lists)
        shape.after_answers(ren, nodes, q, live, got)


def layouts_give_identical_bytes(shape):
    nodes, tris, q = shape.ref.case("bunny")
    lists, count = _want(shape, "bunny")
    N, k = q.shape[0], shape.floats
    padded = np.full((N, shape.padded), np.nan, f32); padded[:, :k] = q
    within = np.full((N, shape.inner), 9.0, f32); within[:, 3:3 + k] = q
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        tw = to(within)
        layouts = {"numpy": q, "numpy padded": padded, "numpy view": within[:, 3:3 + k], "torch": to(q), "torch padded": to(padded), "torch view": tw[:, 3:3 + k]}
        if shape.points:
            layouts.update({"numpy points": q.reshape(N, shape.points, 3), "torch points": to(q).reshape(N, shape.points, 3)})
        for name, bb in layouts.items():
            _same(shape.device(ren, bb), lists, count, name)
            _same(shape.device(ren, bb, cap=8), lists, count, name, 8)


def entries_no_list_reaches_are_left_as_they_were(shape):
    import torch
    L = rt.lib()
    nodes, tris, q = shape.ref.case("bunny")
    lists, count = _want(shape, "bunny")
    N = q.shape[0]
    q = np.array(q)
    exact = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    short = np.concatenate([[0], np.cumsum(np.maximum(count - 1, 0))]).astype(np.int32)
    odd = np.array([3, 1, 1, -5, 2, 2], np.int32)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        db = to(q)
        for host in (True, False):
            fn = getattr(L, shape.query + "_host" if host else shape.query)
            put = (lambda a: None if a is None else np.array(a)) if host else to

            def run(n, offsets, cap, room, with_counts, with_visits=False):
                prims = None if room is None else put(np.full(room, SENTINEL, np.int32))
                counts = put(np.full(n, SENTINEL, np.int32)) if with_counts else None
                vis = put(np.full(n, SENTINEL, np.int32)) if with_visits else None
                o = put(offsets)
                torch.cuda.synchronize()
                assert fn(ren._h, _ptr(q if host else db), shape.floats, n, _ptr(o), cap, _ptr(prims), _ptr(counts), _ptr(vis)) == rt.RT_OK, L.rt_last_error(ren._h)
                ren.synchronize()
                return np_of(prims), np_of(counts), np_of(vis)

            _, c, v = run(N, None, 0, None, True, True)                                     # the counts alone
            assert np.array_equal(c, count) and np.array_equal(v, shape.visits("bunny")), host
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
import opengl_raytracing_amd as rt, {ref} as ref
nodes, tris, q = ref.case("bunny")
with rt.Renderer() as ren:
    ren.upload_bvh(nodes, tris)
    got = ren.{name}(q)
print("{tag}", hashlib.sha256(got.prims.tobytes() + got.count.tobytes()).hexdigest())
'''


def every_node_form_gives_identical_bytes(shape, option):
    want = _digest(*_want(shape, "bunny"))
    name, value = option.split("=")
    child = _CHILD.format(ref=shape.ref.__name__, name=shape.name, tag=shape.tag)
    out = subprocess.run([sys.executable, "-c", child], cwd=str(scenes.ROOT), env=dict(os.environ, **{name: value}), capture_output=True, text=True, timeout=120)
    assert f"{shape.tag} {want}" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---------------------------------------------------------------- 2: the dynamic mesh

def _want_parts(pf, order, prim):
    """The host formula of rt_mesh_hit_parts: (-1, -1) for a prim outside [0, nTris), else the part whose range holds order[prim] and the offset in it."""
    prim = np.asarray(prim).astype(np.int64)
    ok = (prim >= 0) & (prim < order.size)
    t = order[np.where(ok, prim, 0)].astype(np.int64)
    part = np.searchsorted(pf, t, "right") - 1
    return np.where(ok, part, -1).astype(np.int32), np.where(ok, t - pf[part], -1).astype(np.int32)


def _check_mesh_state(shape, ren, host, pf, what):
    q = shape.mesh_queries(host, 23)
    want = shape.host(host.nodes, host.tris, q)
    lists = _lists(want)
    got = shape.device(ren, q)
    _same(got, lists, want.count, (what, "numpy"))
    _same(shape.device(ren, to(q)), lists, want.count, (what, "torch"))
    got8 = shape.device(ren, to(q), cap=8)
    _same(got8, lists, want.count, (what, "torch, cap 8"), 8)
    assert (want.count == 0).sum() > 20 and ((want.count > 0) & (want.count < 8)).sum() > 20 and (want.count > 8).sum() > 20
    assert all((np.diff(r) > 0).all() for r in lists), what                 # ascending on the device builders' trees too
    for ans in (got, got8):                                                 # .hits() feeds mesh_hit_parts as it stands (prim -1: no part)
        rec = ans.hits()
        prim = np_of(ans.prims)
        assert tuple(rec.shape) == (prim.size, 4)
        parts, offs = ren.mesh_hit_parts(rec)
        wp, wo = _want_parts(np.asarray(pf, np.int64), host.order, prim)
        assert np.array_equal(np_of(parts), wp) and np.array_equal(np_of(offs), wo), what
    assert (wp[prim < 0] == -1).all() and (prim < 0).any()
    shape.mesh_state_extra(ren, host, want, what)


def dynamic_mesh_rebuild_refit_and_parts(shape):
    v, f, _, _ = mf.sphere()
    n = f.size // 3
    with rt.Renderer() as ren:
        ren.mesh_upload(v, f)
        ren.mesh_rebuild(mf.turn(0))
        host = mf.HostMesh(f).rebuild(rt.gather_triangles(v, f, mf.turn(0)))
        _check_mesh_state(shape, ren, host, [0, n], "rebuild")
        ren.mesh_refit(mf.turn(1))                       # the same tree under a turned matrix: the queries overlap other rows, the rows stay
        host.refit(rt.gather_triangles(v, f, mf.turn(1)))
        _check_mesh_state(shape, ren, host, [0, n], "refit")
    v, f = mf.parts_mesh()
    models = mf.part_models(1)
    with rt.Renderer() as ren:
        ren.mesh_upload_parts(v, f, mf.PART_FIRST)
        ren.mesh_set_part_matrices(models)
        ren.mesh_rebuild_parts()
        host = mf.HostMesh(f).rebuild(rt.gather_triangles_parts(v, f, mf.PART_FIRST, models))
        _check_mesh_state(shape, ren, host, mf.PART_FIRST, "parts")
        shape.after_parts(ren, host, v, f, models)


# ---------------------------------------------------------------- 3: stream ordering with torch

def written_by_torch_just_before_the_call_are_the_ones_queried(shape):
    import torch
    nodes, tris, q = shape.ref.case("bunny")
    lists, count = _want(shape, "bunny")
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        b = torch.full((q.shape[0], shape.floats), float("nan"), device=dev())  # placeholder queries: empty slots
        torch.cuda.synchronize()
        src = to(q)
        x = torch.randn(4096, 4096, device=dev())
        for _ in range(8):                                          # keep torch's stream busy, so that the write below lands late
            x = x @ x
            x = x / x.norm()
        b.copy_(src)                                                # (enqueued behind the products)
        got = shape.device(ren, b, cap=8)
        c, o, p = (a.clone().cpu().numpy() for a in (got.count, got.offsets, got.prims))          # read by torch on its own stream, no synchronise
        exact = shape.device(ren, b)
    _same(shape.result(c, o, p), lists, count, "late queries", 8)
    _same(exact, lists, count, "late queries, exact")


def two_calls_on_two_torch_streams_without_a_host_wait(shape):
    import torch
    nodes, tris, q = shape.ref.case("layers")
    lists, count = _want(shape, "layers")
    _, _, bb = shape.ref.case("bunny")                             # (the bunny's queries against the layer stack: another count)
    other = shape.host(nodes, tris, bb)
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        ta, tb = to(q), to(bb)
        enqueue, check = shape.on_stream2(ren, nodes, tris)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(dev()), torch.cuda.Stream(dev())
        with torch.cuda.stream(s1):
            a = shape.device(ren, ta, cap=8)
        with torch.cuda.stream(s2):
            b = shape.device(ren, tb, cap=3)
            enqueue()
        with torch.cuda.stream(s1):
            a2 = shape.device(ren, ta, cap=8)
        torch.cuda.synchronize()
        _same(a, lists, count, "stream 1", 8); _same(b, _lists(other), other.count, "stream 2", 3); _same(a2, lists, count, "stream 1 again", 8)
        check()


# ---------------------------------------------------------------- 4: isolation from frames, no allocation

def queries_do_not_touch_frame_state(shape, pipeline):
    nodes, tris = scenes.bunny_bvh(3)
    rng = np.random.default_rng(3)
    ctr = rng.uniform(nodes[0, 0:3] - 0.5, nodes[0, 4:7] + 0.5, (700, 3))
    q = shape.frame_queries(rng, ctr)
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
                    shape.device(ren, q, visits=True)
                    shape.with_frames(ren, u, W, H, np.asarray)
                ren.render_frame(u)
                if with_queries:                               # device path, enqueued behind the frame on rt_stream()'s stream
                    shape.device(ren, to(q), cap=8)
                    shape.with_frames(ren, u, W, H, to)
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


def no_allocation_after_the_first_query(shape):
    import torch
    nodes, tris, q = shape.ref.case("bunny")
    _, count = _want(shape, "bunny")
    L = rt.lib()
    fn = getattr(L, shape.query)
    N, cap = q.shape[0], 8
    with rt.Renderer() as ren:
        ren.upload_bvh(nodes, tris)
        tb = to(q)
        off = to(np.concatenate([[0], np.cumsum(count)]).astype(np.int32))
        prims = torch.empty(max(N * cap, int(count.sum())), dtype=torch.int32, device=dev())
        counts = torch.empty(N, dtype=torch.int32, device=dev())
        visits = torch.empty(N, dtype=torch.int32, device=dev())
        more = shape.more_calls(ren, nodes, tris)
        torch.cuda.synchronize()

        def call(k):
            form = k % 3                                           # the counts alone, fixed capacity, exact slots
            rc = fn(ren._h, _ptr(tb), shape.floats, N, _ptr(off) if form == 2 else None, cap, _ptr(prims) if form else None,
                    _ptr(counts) if (form == 0 or k & 4) else None, _ptr(visits) if k & 8 else None)
            assert rc == rt.RT_OK, L.rt_last_error(ren._h)
            more(form, cap, prims, counts)

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

def every_refusal_leaves_the_outputs_unwritten(shape):
    import torch
    L = rt.lib()
    nodes, tris, q = shape.ref.case("one_leaf")
    N, cap, k = 8, 4, shape.floats
    q = np.array(q[1:1 + N])                                       # (a copy: the shared fixtures are read-only)
    prims, counts, visits = np.full(N * cap, SENTINEL, np.int32), np.full(N, SENTINEL, np.int32), np.full(N, SENTINEL, np.int32)
    offsets = (np.arange(N + 1) * cap).astype(np.int32)
    db, dp, dn, dv, do = to(q), to(prims), to(counts), to(visits), to(offsets)
    torch.cuda.synchronize()
    off = lambda a, by: C.c_void_p(_ptr(a).value + by)

    with rt.Renderer() as ren:
        h = ren._h
        err = lambda: L.rt_last_error(h).decode()

        def call(host, b_=0, stride=k, n=N, offsets_=None, cap_=cap, prims_=0, counts_=0, visits_=0):
            A = (q, prims, counts, visits) if host else (db, dp, dn, dv)
            fn = getattr(L, shape.query + "_host" if host else shape.query)
            pick = lambda x, a: _ptr(a) if isinstance(x, int) and x == 0 else x
            return fn(h, pick(b_, A[0]), stride, n, offsets_, cap_, pick(prims_, A[1]), pick(counts_, A[2]), pick(visits_, A[3]))

        for host in (True, False):
            assert call(host) == rt.RT_ERR_STATE and "no BVH uploaded" in err()
        ren.upload_bvh(nodes, tris)
        for host in (True, False):
            assert call(host, n=-1) == rt.RT_ERR_INVALID and "n = -1" in err()
            assert call(host, stride=k - 1) == rt.RT_ERR_INVALID and f"stride {k - 1}" in err()
            assert call(host, b_=None) == rt.RT_ERR_INVALID and f"null {shape.noun} array" in err()
            assert call(host, prims_=None, counts_=None) == rt.RT_ERR_INVALID and "prims or counts" in err()
            assert call(host, cap_=-1) == rt.RT_ERR_INVALID and "cap = -1" in err()
            assert call(host, n=(1 << 31) // cap + 1) == rt.RT_ERR_INVALID and "INT32_MAX" in err()
            assert call(host, n=1 << 28, stride=32, prims_=None) == rt.RT_ERR_INVALID and "2^32 floats" in err()
            assert call(host, n=0, b_=None, prims_=None, counts_=None, visits_=None) == rt.RT_OK          # n == 0: a no-op
        # the host twin inspects its offsets; the device entry cannot
        assert call(True, offsets_=_ptr(np.array([0, 4, 2, 8, 12, 16, 20, 24, 28], np.int32))) == rt.RT_ERR_INVALID and "descend" in err()
        assert call(True, offsets_=_ptr(np.array([-4, 0, 4, 8, 12, 16, 20, 24, 28], np.int32))) == rt.RT_ERR_INVALID and "offsets[0]" in err()
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
        ask = lambda *a, **kw: shape.device(ren, *a, **kw)
        refused = [lambda: ask(q[:, :k - 1]), lambda: ask(q.astype(np.float64)), lambda: ask(torch.from_numpy(q)), lambda: ask(db.double()),
                   lambda: ask(q, cap=-1), lambda: ask(db.t()), lambda: ask(list(q))]
        if shape.points:
            refused.append(lambda: ask(db.reshape(N, shape.points, 3).transpose(1, 2)))
        for bad in refused:
            with pytest.raises(rt.RtError) as e:
                bad()
            assert e.value.code == rt.RT_ERR_INVALID
        # ... and a good call still works afterwards, on both paths and with the offsets
        want = shape.host(nodes, tris, q)
        _same(ask(q, visits=True), _lists(want), want.count, "after the refusals")
        for host in (True, False):
            assert call(host, offsets_=_ptr(offsets) if host else _ptr(do), cap_=0) == rt.RT_OK, err()
        ren.synchronize()
        filled = _expect(_lists(want), offsets, SENTINEL)
        assert np.array_equal(prims, filled) and np.array_equal(dp.cpu().numpy(), filled) and np.array_equal(counts, want.count) and np.array_equal(dn.cpu().numpy(), want.count)
        assert len(ask(q[:0])) == 0 and len(ask(db[:0])) == 0 and len(ask(db[:0], cap=4)) == 0


# ================================================================ the host side

def _raw(shape, nodes, tris, queries, stride, n, offsets, cap, prims, counts):
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    return getattr(rt.lib(), shape.raw)(p(nodes), nodes.shape[0], p(tris), tris.shape[0], p(queries), stride, n, p(offsets), cap, p(prims), p(counts))


def _lists_of(got):
    return [got.prims[got.offsets[i]:got.offsets[i] + min(got.count[i], got.offsets[i + 1] - got.offsets[i])] for i in range(len(got))]


def counts_and_lists_equal_the_numpy_definition(shape, mesh):
    nodes, tris, q = shape.ref.case(mesh)
    want = shape.ref.reference(mesh)
    assert q.shape[0] >= 2049
    got = shape.host(nodes, tris, q)
    bad = np.flatnonzero(got.count != want.count)
    assert bad.size == 0, (mesh, bad[:8], got.count[bad[:8]], want.count[bad[:8]], q[bad[:2]])
    assert isinstance(got, shape.result) and np.array_equal(got.offsets, want.offsets()) and got.prims.dtype == np.int32
    assert np.array_equal(got.prims, want.filled(want.offsets())), mesh
    pairs = shape.pairs(got)
    assert pairs.dtype == np.int32 and np.array_equal(pairs, want.pairs())
    shape.host_extra(got, tris)
    for cap in HOST_CAPS:
        got = shape.host(nodes, tris, q, cap=cap)
        assert np.array_equal(got.count, want.count) and np.array_equal(got.offsets, np.arange(q.shape[0] + 1) * cap)
        assert np.array_equal(got.prims, want.filled(cap=cap, sentinel=-1)), (mesh, cap)
        kept = shape.pairs(got)                                        # the written entries alone: the first min(cap, count) of every list
        assert np.array_equal(kept, np.array([(i, t) for i, rows in enumerate(want.lists) for t in rows[:cap]], np.int32).reshape(-1, 2))
    hits = shape.host(nodes, tris, q[:65], cap=3).hits()
    assert hits.shape == (195, 4) and np.array_equal(hits.view(np.int32)[:, 1], want.filled(cap=3, sentinel=-1)[:195])
    assert (hits[:, 0] == 0).all() and (hits[:, 2:4] == f32(1) / f32(3)).all()


def strided_counts_alone_lists_alone_and_sentinels(shape, stride):
    nodes, tris, q = shape.ref.case("bunny")
    want = shape.ref.reference("bunny")
    N, k = q.shape[0], shape.floats
    wide = np.full((N, stride), np.nan, f32)
    wide[:, :k] = q
    flat = np.ascontiguousarray(wide.reshape(-1)[:(N - 1) * stride + k])          # exactly as long as a call may read
    views = [np.lib.stride_tricks.as_strided(flat, (N, k), (4 * stride, 4))]
    if shape.points:                                                              # [N, points, 3]
        views.append(np.lib.stride_tricks.as_strided(flat, (N, shape.points, 3), (4 * stride, 12, 4)))
    for view in views:
        got = shape.host(nodes, tris, view)
        assert np.array_equal(got.count, want.count) and np.array_equal(got.prims, want.filled(want.offsets()))
    # counts alone
    counts = np.full(N, SENTINEL, np.int32)
    assert _raw(shape, nodes, tris, flat, stride, N, None, 0, None, counts) == rt.RT_OK and np.array_equal(counts, want.count)
    # lists alone: exact slots with a guard word behind the last, slots one short, and fixed capacities
    off = want.offsets()
    prims = np.full(off[-1] + 1, SENTINEL, np.int32)
    assert _raw(shape, nodes, tris, flat, stride, N, off, 0, prims, None) == rt.RT_OK
    assert np.array_equal(prims[:-1], want.filled(off)) and prims[-1] == SENTINEL
    short = np.concatenate([[0], np.cumsum(np.maximum(want.count - 1, 0))]).astype(np.int32)
    prims = np.full(short[-1], SENTINEL, np.int32)
    counts[:] = SENTINEL
    assert _raw(shape, nodes, tris, flat, stride, N, short, 0, prims, counts) == rt.RT_OK
    assert np.array_equal(prims, want.filled(short)) and np.array_equal(counts, want.count)
    for cap in HOST_CAPS:
        prims = np.full(N * cap, SENTINEL, np.int32)
        assert _raw(shape, nodes, tris, flat, stride, N, None, cap, prims if cap else np.zeros(1, np.int32), None) == rt.RT_OK
        filled = want.filled(cap=cap, sentinel=SENTINEL)
        assert np.array_equal(prims, filled), cap
        if cap:
            assert (filled == SENTINEL).any() and ((prims == SENTINEL) == (np.arange(N * cap) % cap >= np.repeat(want.count, cap))).all()
    # a slot of negative length, and one with a negative start, hold nothing
    odd = np.array([3, 1, 1, -5, 2, 2], np.int32)
    prims = np.full(8, SENTINEL, np.int32)
    counts = np.full(5, SENTINEL, np.int32)
    assert _raw(shape, nodes, tris, flat, stride, 5, odd, 0, prims, counts) == rt.RT_OK
    assert np.array_equal(counts, want.count[:5]) and (prims == SENTINEL).all()


def every_refusal_writes_nothing(shape):
    nodes, tris, q = shape.ref.case("layers")
    k = shape.floats
    q = np.array(q[shape.first:shape.first + 4])
    prims, counts = np.full(32, SENTINEL, np.int32), np.full(4, SENTINEL, np.int32)
    off = np.array([0, 8, 16, 24, 32], np.int32)
    ok = dict(nodes=nodes, tris=tris, queries=q, stride=k, n=4, offsets=off, cap=0, prims=prims, counts=counts)
    call = lambda **kw: _raw(shape, **dict(ok, **kw))
    assert call(n=-1) == rt.RT_ERR_INVALID
    assert call(stride=k - 1) == rt.RT_ERR_INVALID
    assert call(queries=None) == rt.RT_ERR_INVALID
    assert call(prims=None, counts=None) == rt.RT_ERR_INVALID
    assert call(offsets=None, cap=-1) == rt.RT_ERR_INVALID
    assert call(offsets=None, cap=(1 << 31) // 4 + 1) == rt.RT_ERR_INVALID                   # n * cap beyond INT32_MAX
    for link in (-1.0, 1e9, np.nan, float(nodes.shape[0]), 0.0):                             # nodes that are no tree over the rows
        bad = nodes.copy()
        bad[0, 3] = link
        assert call(nodes=bad) == rt.RT_ERR_INVALID, link
    bad = nodes.copy()
    leaf = [j for j in range(nodes.shape[0]) if nodes[j, 9] > 0][0]
    bad[leaf, 8] = 2e9
    assert call(nodes=bad) == rt.RT_ERR_INVALID
    assert (prims == SENTINEL).all() and (counts == SENTINEL).all()
    assert _raw(shape, nodes, tris, None, k, 0, None, 0, None, None) == rt.RT_OK              # n == 0: a no-op
    assert call() == rt.RT_OK and (counts != SENTINEL).all()
    ask = lambda *a, **kw: shape.host(nodes, tris, *a, **kw)
    refused = [lambda: ask(q[:, :k - 1]), lambda: ask(q.astype(np.float64)), lambda: ask(q, cap=-1), lambda: ask(list(q))]
    if shape.points:
        refused += [lambda: ask(q.reshape(4, shape.points, 3).transpose(0, 2, 1)), lambda: ask(q.reshape(2, 2, k))]
    for bad_call in refused:
        with pytest.raises(rt.RtError) as e:
            bad_call()
        assert e.value.code == rt.RT_ERR_INVALID
    empty = ask(q[:0])
    assert len(empty) == 0 and empty.prims.size == 0 and np.array_equal(empty.offsets, [0]) and shape.pairs(empty).shape == (0, 2)


def the_path_mask_removes_nothing_and_every_list_ascends(shape, mesh):
    want = shape.ref.reference(mesh)
    assert not (want.sat.accept & ~want.walk.path).any()
    assert np.array_equal(want.walk.order, np.arange(want.walk.order.size))
    assert all((np.diff(rows) > 0).all() for rows in want.lists)


def a_tree_with_swapped_children_lists_in_walk_order(shape):
    t9 = np.array([[x, 0, 0, 0.5, 0, 0, 0, 0.5, 0.25] for x in (0.0, 1.0, 2.0, 3.0)], f32)
    tris = np.zeros((4, 12), f32)
    tris[:, 0:3], tris[:, 4:7], tris[:, 8:11] = t9[:, 0:3], t9[:, 3:6], t9[:, 6:9]

    def box(rows):
        v = np.concatenate([tris[rows, 0:3], tris[rows, 0:3] + tris[rows, 4:7], tris[rows, 0:3] + tris[rows, 8:11]])
        return v.min(0), v.max(0)

    nodes = np.zeros((3, 12), f32)
    for k, rows in enumerate(([0, 1, 2, 3], [0, 1], [2, 3])):
        nodes[k, 0:3], nodes[k, 4:7] = box(rows)
    nodes[0, 3], nodes[0, 7] = 1, 2
    nodes[1, 8], nodes[1, 9] = 0, 2
    nodes[2, 8], nodes[2, 9] = 2, 2
    q = shape.swapped_queries()
    got = shape.host(nodes, tris, q)
    want = shape.ref.Answer(nodes, tris, q)
    assert [list(r) for r in _lists_of(got)] == [[2, 3, 0, 1], [2, 1], []] and [list(r) for r in want.lists] == [[2, 3, 0, 1], [2, 1], []]
    assert list(want.visits) == [3, 3, 3]
    assert np.array_equal(shape.pairs(got), [[0, 2], [0, 3], [0, 0], [0, 1], [1, 2], [1, 1]])
    nodes[0, 3], nodes[0, 7] = 2, 1
    got = shape.host(nodes, tris, q)
    assert [list(r) for r in _lists_of(got)] == [[0, 1, 2, 3], [1, 2], []]
    assert [list(r) for r in shape.ref.Answer(nodes, tris, q).lists] == [[0, 1, 2, 3], [1, 2], []]
    # condition (a) is part of the definition: shrink the right child's box off its rows, and the walk no longer reaches rows 2 and 3
    nodes[2, 0] = 10.0
    got = shape.host(nodes, tris, q)
    assert [list(r) for r in _lists_of(got)] == [[0, 1], [1], []]
    assert [list(r) for r in shape.ref.Answer(nodes, tris, q).lists] == [[0, 1], [1], []]


# ================================================================ the three shapes

def _about(host, rng):
    """What the dynamic-mesh query makers start from: the root box, and 400 points on the surface."""
    t = host.tris
    lo, hi = host.nodes[0, 0:3].astype(np.float64), host.nodes[0, 4:7].astype(np.float64)
    k = rng.integers(0, t.shape[0], 400)
    w = rng.dirichlet((1, 1, 1), 400)
    return lo, hi, t[k, 0:3] + t[k, 4:7] * w[:, 1:2] + t[k, 8:11] * w[:, 2:3]


def _mesh_boxes(host, seed):
    """Boxes about a mesh: on its surface with half-extents 2^-k of the root extent, degenerate at vertices, the root box, far away, empty slots."""
    rng = np.random.default_rng(seed)
    t = host.tris
    lo, hi, on = _about(host, rng)
    ext = hi - lo
    half = ext * 2.0 ** -rng.integers(1, 9, (400, 3))
    far = (lo + hi) * 0.5 + rng.normal(size=(40, 3)) * 20 * ext
    boxes = np.concatenate([np.concatenate([on - half, on + half], 1), np.concatenate([t[::9, 0:3], t[::9, 0:3]], 1),
                            np.concatenate([lo, hi])[None], np.concatenate([far - 0.1 * ext, far + 0.1 * ext], 1)]).astype(f32)
    boxes[::97, 0] = np.nan
    boxes[1] = np.concatenate([lo, hi]).astype(f32)                # (wherever the empty slots fell, the root box is there)
    return boxes


def _mesh_tris(host, seed):
    """Query triangles about a mesh: on its surface with edges 2^-k of the root extent, points at vertices, one that cuts the whole mesh, far away,
    empty slots."""
    rng = np.random.default_rng(seed)
    t = host.tris
    lo, hi, on = _about(host, rng)
    ext = hi - lo
    mid = (lo + hi) * 0.5
    edge = ext * 2.0 ** -rng.integers(1, 9, (400, 1))
    far = mid + rng.normal(size=(40, 3)) * 20 * ext
    cut = np.concatenate([mid + ext * (-4, -4, 0.01), mid + ext * (4, -4, 0.02), mid + ext * (0, 6, -0.03)])
    q = np.concatenate([np.concatenate([on + rng.normal(size=(400, 3)) * edge for _ in range(3)], 1), np.tile(t[::9, 0:3], (1, 3)), cut[None],
                        np.concatenate([far + rng.normal(size=(40, 3)) * 0.1 * ext for _ in range(3)], 1)]).astype(f32)
    q[::97, 4] = np.nan
    q[1] = cut.astype(f32)                                          # (wherever the empty slots fell, the cutting triangle is there)
    return q


def _mesh_hulls(host, seed):
    """Hulls about a mesh: sheared boxes on its surface with edges 2^-k of the root extent, generic hexahedra, points at vertices, a slab that cuts the
    whole mesh, far away, empty slots."""
    ref = hull_query_ref
    rng = np.random.default_rng(seed)
    t = host.tris
    lo, hi, on = _about(host, rng)
    on = on.astype(np.float64)
    ext = hi - lo
    mid = (lo + hi) * 0.5
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


def _frame_boxes(rng, ctr):
    half = rng.uniform(0.01, 0.5, (700, 3))
    return np.concatenate([ctr - half, ctr + half], 1).astype(f32)


def _swapped_hulls():
    """A slab about the plane y = 0.1 over all four rows; a thin box turned 20 degrees about z that crosses rows 1 and 2; a point inside the right
    child's box."""
    co, si = np.cos(np.radians(20.0)), np.sin(np.radians(20.0))
    turn = np.array([co, si, 0, 0, -si, co, 0, 0, 0, 0, 1, 0, 1.75, 0.2, 0.1, 1], f32)       # column-major: 20 degrees about z, to (1.75, 0.2, 0.1)
    return np.concatenate([rt.box_corners(np.array([[-1, 0.05, -1, 5, 0.15, 1]], f32)),
                           rt.box_corners(np.array([[-0.9, -0.05, -0.5, 0.9, 0.05, 0.5]], f32), turn), np.tile(np.array([[2.6, 0.3, 0]], f32), (1, 8))])


# ---------------------------------------------------------------- what one shape's tests check beyond the others'

def _box_lists_everything(ren, host, want, what):
    assert want.count.max() == host.tris.shape[0]                   # the root box


def _tri_walk_is_the_box_querys(ren, nodes, q, live, got):
    """The walk is the box query's for [qlo, qhi]: the same visits from the box kernel on the same context, numpy and torch."""
    box = tri_query_ref.aabb(q)
    box[~live] = np.nan                                            # (fmin / fmax pass over a NaN: the empty slots are marked again)
    assert np.array_equal(ren.box_overlaps(box, cap=0, visits=True).visits, got.visits)
    assert np.array_equal(np_of(ren.box_overlaps(to(box), cap=0, visits=True).visits), np_of(ren.tri_overlaps(to(q), cap=0, visits=True).visits))


def _tri_self_queries(ren, host, want, what):
    """Self queries: the device's current rows as query triangles, by the definition's adds, each list its own row."""
    rows = ren.debug_read_scene("tris").view(f32).reshape(-1, 12)[:host.tris.shape[0]]
    assert np.array_equal(rows, host.tris), what
    own = rt.rows_as_tris(rows)
    mine = ren.tri_overlaps(to(own))
    _same(mine, _lists(rt.tri_overlaps(host.nodes, host.tris, own)), rt.tri_overlaps(host.nodes, host.tris, own).count, (what, "self"))
    pairs = np_of(mine.pairs())
    assert np.isin(np.arange(own.shape[0]) * (1 << 32) + np.arange(own.shape[0]), pairs[:, 0].astype(np.int64) * (1 << 32) + pairs[:, 1]).all(), what
    assert np.array_equal(np_of(rt.rows_as_tris(to(rows))), own)


def _tri_rows_as_tris(got, tris):
    assert np.array_equal(rt.rows_as_tris(tris), tri_query_ref.rows_as_tris(tris)) and rt.rows_as_tris(tris).dtype == f32


def _hull_answer(got):
    assert isinstance(got, rt.HullOverlaps) and got.corners is None


def _hull_host_answer(got, tris):
    assert isinstance(got, rt.TriOverlaps) and got.corners is None


def _hull_normals_only_spare_visits(ren, nodes, q, live, got):
    """The six normals only ever spare visits: never more than the box kernel's on [lo, hi], on the same context."""
    box = hull_query_ref.aabb(q)
    box[~live] = np.nan                                            # (fmin / fmax pass over a NaN: the empty slots are marked again)
    plain = ren.box_overlaps(box, cap=0, visits=True).visits
    assert (got.visits <= plain).all() and np.array_equal(plain, hull_query_ref.box_visits(nodes, q))


def _hull_part_boxes(ren, host, v, f, models):
    """The trigger volume that moves with a part: the part's object-space box, grown by a thousandth of its extent so that no vertex lies on a face,
    under the part's own matrix.  It lists every row of its part -- it encloses them --, and rows of those parts alone whose world boxes its own box
    reaches."""
    pf = np.asarray(mf.PART_FIRST, np.int64)
    fi = np.asarray(f, np.int64).reshape(-1, 3)
    obj = []
    for p in range(pf.size - 1):
        pts = np.asarray(v, f32).reshape(-1, 3)[fi[pf[p]:pf[p + 1]].reshape(-1)]
        grow = f32(1e-3) * (pts.max(0) - pts.min(0))
        obj.append(np.concatenate([pts.min(0) - grow, pts.max(0) + grow]))
    hulls = rt.box_corners(np.array(obj, f32), np.asarray(models, f32).reshape(-1, 16))
    got = ren.hull_overlaps(to(hulls))
    want = rt.hull_overlaps(host.nodes, host.tris, hulls)
    _same(got, _lists(want), want.count, "part boxes")
    part_of_row = np.searchsorted(pf, host.order.astype(np.int64), "right") - 1
    a, b, c = hull_query_ref.row_points(host.tris)
    rlo, rhi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    box = hull_query_ref.aabb(hulls)
    for p, rows in enumerate(_lists(want)):
        assert set(np.flatnonzero(part_of_row == p)) <= set(rows), p
        for other in set(part_of_row[rows]):
            mine = part_of_row == other
            assert (rlo[mine].min(0) <= box[p, 3:6]).all() and (box[p, 0:3] <= rhi[mine].max(0)).all(), (p, other)


def frame(nodes, tris, W, H, jitter):
    """The uniforms of a W x H BVH frame whose camera is hull_query_ref.view's."""
    u = rt.frame_uniforms(rt.default_render_params(), scenes.camera("closeup", aspect=W / H), W, H, 0, True, nodes.shape[0], tris.shape[0])
    cam = hull_query_ref.view("bunny", W, H, jitter)
    for name in ("camPos", "camRight", "camUp", "camFwd"):
        for k in range(3):
            getattr(u, name)[k] = getattr(cam, name)[k]
    u.tanHalfFov, u.aspect = cam.tanHalfFov, cam.aspect
    u.enableJitter, u.jitter[0], u.jitter[1] = cam.enableJitter, cam.jitter[0], cam.jitter[1]
    return u


def _hull_rects_on_stream2(ren, nodes, tris):
    """A rect pick behind the hull query on stream 2."""
    u = frame(nodes, tris, 48, 36, None)
    rects = np.array([[0, 0, 48, 36], [10, 10, 20, 20]], f32)
    tr = to(rects)
    got = []

    def check():
        wr = rt.hull_overlaps(nodes, tris, rt.rect_frusta(u, nodes[0, 0:3], nodes[0, 4:7], rects))
        _same(got[0], _lists(wr), wr.count, "rects on stream 2", 8)

    return lambda: got.append(ren.pick_rects(u, tr, cap=8)), check


def _hull_rects_with_frames(ren, u, W, H, put):
    ren.pick_rects(u, put(np.array([[0, 0, W, H], [40, 30, 90, 70]], f32)), cap=8)


def _hull_rect_calls(ren, nodes, tris):
    """A rect pick of 64 rects beside every hull query."""
    import torch
    L = rt.lib()
    u = frame(nodes, tris, 48, 36, None)
    rects = to(np.tile(np.array([[3, 4, 20, 30]], f32), (64, 1)))
    corners = torch.empty((64, 24), dtype=torch.float32, device=dev())

    def call(form, cap, prims, counts):
        rc = L.rt_pick_rects(ren._h, C.byref(u), _ptr(rects), 4, 64, 0.0, -1.0, _ptr(corners), None, cap, _ptr(prims) if form else None, _ptr(counts), None)
        assert rc == rt.RT_OK, L.rt_last_error(ren._h)

    return call


BOX = Shape(ref=box_query_ref, floats=6, strides=(6, 7, 12), padded=7, inner=12, points=None, name="box_overlaps", raw="rt_box_overlaps", query="rt_query_boxes",
            tag="BOX_QUERY", result=rt.BoxOverlaps, noun="box", first=0, visits=lambda mesh: box_query_ref.reference(mesh).visits,
            pairs=lambda got: rt.TriOverlaps(got.count, got.offsets, got.prims).pairs(), mesh_queries=_mesh_boxes, frame_queries=_frame_boxes,
            swapped_queries=lambda: np.array([[-1, -1, -1, 5, 1, 1], [0.9, -1, -1, 2.2, 1, 1], [2.6, 0, 0, 2.6, 0, 0]], f32),
            mesh_state_extra=_box_lists_everything)
TRI = Shape(ref=tri_query_ref, floats=9, strides=(9, 10, 12), padded=12, inner=14, points=3, name="tri_overlaps", raw="rt_tri_overlaps", query="rt_query_tris",
            tag="TRI_QUERY", result=rt.TriOverlaps, noun="triangle", first=0, visits=lambda mesh: tri_query_ref.walk(mesh).visits, pairs=lambda got: got.pairs(),
            mesh_queries=_mesh_tris, frame_queries=lambda rng, ctr: np.concatenate([ctr + rng.uniform(-0.5, 0.5, (700, 3)) for _ in range(3)], 1).astype(f32),
            swapped_queries=lambda: np.array([[-1, 0.1, -1, 5, 0.1, -1, 2, 0.1, 5], [0.9, 0.1, -1, 2.6, 0.1, -1, 1.75, 0.1, 3], [2.6, 0, 0, 2.6, 0, 0, 2.6, 0, 0]], f32),
            after_answers=_tri_walk_is_the_box_querys, mesh_state_extra=_tri_self_queries, host_extra=_tri_rows_as_tris)
HULL = Shape(ref=hull_query_ref, floats=24, strides=(24, 25, 32), padded=32, inner=30, points=8, name="hull_overlaps", raw="rt_hull_overlaps", query="rt_query_hulls",
             tag="HULL_QUERY", result=rt.HullOverlaps, noun="hull", first=1, visits=lambda mesh: hull_query_ref.walk(mesh).visits, pairs=lambda got: got.pairs(),
             mesh_queries=_mesh_hulls, frame_queries=lambda rng, ctr: hull_query_ref.generic_hexahedra(rng, ctr, rng.uniform(0.1, 0.6, 700)).astype(f32),
             swapped_queries=_swapped_hulls, each_answer=_hull_answer, after_answers=_hull_normals_only_spare_visits, after_parts=_hull_part_boxes,
             on_stream2=_hull_rects_on_stream2, with_frames=_hull_rects_with_frames, more_calls=_hull_rect_calls, host_extra=_hull_host_answer)
