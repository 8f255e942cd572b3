"""Tree quality on the device.  mesh_measure + mesh_quality give rt_bvh_cost of the host route's nodes bit for bit -- after a rebuild,
after a refit, after a refit of parts; mesh_update refits or rebuilds by the rule of the header, replayed here on the numpy definitions; none of it
waits, allocates, or changes what frames and queries compute."""
import ctypes as C
import functools

import numpy as np
import pytest

import bvh_build_ref as B
import bvh_cost_ref as K
import opengl_raytracing_amd as rt
import scenes

pytestmark = pytest.mark.gpu

IDENT = np.eye(4, dtype=np.float32).reshape(-1)
# one node; under one wave of nodes; a ragged last block; 20 480 triangles (5119 nodes) across many blocks; and the number edges of the corpus
MESHES = ("count_1", "count_8", "count_9", "count_257", "lattice", "floor_grid", "identical", "point", "signed_zero", "denormal", "huge", "mixed_scale",
          "degenerate", "bunny5")
FIELDS = K.FIELDS


@functools.lru_cache(maxsize=1)
def _corpus():
    c = B.corpus()
    c["bunny5"] = rt.meshgen.bunny_standin(5)
    return c


@functools.lru_cache(maxsize=None)
def _host_route(name):
    """(positions, indices, ref_build's (nodes12, tris12, order) of the library's gather under the identity): computed once, read only."""
    v, f = _corpus()[name]
    v = np.ascontiguousarray(v, np.float32)
    f = np.ascontiguousarray(f, np.uint32)
    built = B.ref_build(rt.gather_triangles(v, f, IDENT))
    for a in (v, f) + tuple(built):
        a.setflags(write=False)
    return v, f, built


def _same_record(got, want, what):
    """got: RtBvhCost from the device; want: RtBvhCost from rt_bvh_cost.  Integers equal, doubles equal in their bits."""
    for k in FIELDS:
        g, w = getattr(got, k), getattr(want, k)
        same = K.bits(g) == K.bits(w) if isinstance(w, float) else g == w
        assert same, f"{what}: {k} = {g!r} on the device, rt_bvh_cost says {w!r}"


def _scattered(v, seed=3):
    """Every vertex somewhere else: the tree of the rebuild is a poor one for these positions."""
    span = max(float(np.abs(v).max()), 1e-30)
    return (v + np.random.default_rng(seed).uniform(-0.5, 0.5, v.shape) * span).astype(np.float32)


def _grid_parts():
    v, f = K.grid(32)
    f, first = K.interleave_parts(f, 4)
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.uint32), first


# ---------------------------------------------------------------- 1: the device against the definition
@pytest.mark.parametrize("name", MESHES)
def test_device_equals_rt_bvh_cost(monkeypatch, name):
    monkeypatch.delenv("RT_QNODES", raising=False)
    v, f, (nodes, tris, order) = _host_route(name)
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_rebuild(IDENT)
        b.mesh_measure()
        q = b.mesh_quality(wait=True)
        want = rt.bvh_cost(nodes)
        K.assert_same(want, K.ref_cost(nodes), f"{name}: rt_bvh_cost")           # the host is the definition's (the CPU suite says so at length)
        _same_record(q.cost, want, f"{name} rebuilt")
        assert (q.update, q.refitsSinceRebuild, q.skipped) == (1, 0, 0)
        assert q.cost.degenerate == (1 if name == "point" else 0)
        base = b.mesh_quality("baseline", wait=False)
        assert bytes(base) == bytes(q)
        # the same tree over scattered vertices
        moved = _scattered(v)
        b.mesh_set_positions(moved)
        b.mesh_refit(IDENT)
        b.mesh_measure()
        q2 = b.mesh_quality(wait=True)
        with np.errstate(all="ignore"):
            n2, _ = rt.refit_bvh(nodes, tris, order, rt.gather_triangles(moved, f, IDENT))
        _same_record(q2.cost, rt.bvh_cost(n2), f"{name} refitted")
        assert (q2.update, q2.refitsSinceRebuild, q2.skipped) == (2, 1, 0)
        assert bytes(b.mesh_quality("baseline", wait=False)) == bytes(base)      # the baseline stays the rebuild's
        assert b.mesh_info().hostSyncs == 0


def test_device_equals_rt_bvh_cost_after_a_refit_of_parts():
    v, f, first = _grid_parts()
    with rt.Renderer() as b:
        b.mesh_upload_parts(v, f, first)
        b.mesh_rebuild_parts()
        b.mesh_measure()
        rest = rt.gather_triangles_parts(v, f, first, K.translations(4, 0.0))
        assert np.array_equal(rest, K.gather_parts(v, f, first, K.translations(4, 0.0)))
        nodes, tris, order = B.ref_build(rest)
        q0 = b.mesh_quality(wait=True)
        _same_record(q0.cost, rt.bvh_cost(nodes), "grid rebuilt")
        ratios = []
        for step in (0.5, 2.0):
            m = K.translations(4, step)
            b.mesh_set_part_matrices(m)
            b.mesh_refit_parts()
            b.mesh_measure()
            n2, _ = rt.refit_bvh(nodes, tris, order, rt.gather_triangles_parts(v, f, first, m))
            q = b.mesh_quality(wait=True)
            _same_record(q.cost, rt.bvh_cost(n2), f"grid refitted, parts {step} apart")
            ratios.append(q.cost.cost / q0.cost.cost)
        assert ratios[0] > 5 and ratios[1] > ratios[0]                            # what the policy is for
        assert b.mesh_quality("baseline", wait=False).update == 1


# ---------------------------------------------------------------- 2: the policy
def _replay(v, f, first, steps, rebuild_above):
    """The rule of rt_mesh_update for a caller who synchronises before every step, on the numpy definitions alone -> per step (action, nodes12, tris12)."""
    out, tree, base, latest = [], None, None, None
    for m in steps:
        t9 = K.gather_parts(v, f, first, m)
        if tree is None or base is None:
            rebuild = True
        elif base["degenerate"] or latest["degenerate"]:
            rebuild = False
        else:
            rebuild = latest["cost"] > float(np.float32(rebuild_above)) * base["cost"]
        if rebuild:
            tree = B.ref_build(t9)
            latest = base = K.ref_cost(tree[0])
        else:
            n2, t2 = B.ref_refit(t9, tree[2], tree[0], tree[1])
            tree = (n2, t2, tree[2])
            latest = K.ref_cost(n2)
        out.append(("rebuild" if rebuild else "refit", tree[0], tree[1]))
    return out


def _assert_scene_is(b, nodes, tris, what):
    with rt.Renderer() as a:
        a.upload_bvh(nodes, tris)
        assert bytes(a.scene_info()) == bytes(b.scene_info()), what
        for name in rt.SCENE_ARRAYS:
            assert np.array_equal(a.debug_read_scene(name), b.debug_read_scene(name)), (what, name)


def test_policy_follows_the_rule(monkeypatch):
    monkeypatch.delenv("RT_QNODES", raising=False)
    v, f, first = _grid_parts()
    steps = [K.translations(4, 0.0)] + [K.translations(4, 0.5)] * 3
    want = _replay(v, f, first, steps, 2.0)
    assert [w[0] for w in want] == ["rebuild", "refit", "rebuild", "refit"]      # what the definitions imply; the device is held to `want`, not to this
    with rt.Renderer() as b:
        b.mesh_upload_parts(v, f, first)
        allocs = b.mesh_info().allocations
        rebuilds = refits = 0
        for k, (m, (action, nodes, tris)) in enumerate(zip(steps, want)):
            b.mesh_set_part_matrices(m)
            b.synchronize()
            got = b.mesh_update(parts=True, rebuild_above=2.0)
            assert got == action, (k, got, action)
            rebuilds += action == "rebuild"
            refits += action == "refit"
            _assert_scene_is(b, nodes, tris, ("step", k, action))
            mi = b.mesh_info()
            assert (mi.rebuilds, b.mesh_refit_count()[0]) == (rebuilds, refits)
            assert mi.allocations == allocs and mi.hostSyncs == 0
            q = b.mesh_quality(wait=True)                                         # every step measured its own tree
            _same_record(q.cost, rt.bvh_cost(nodes), ("step", k))
            assert q.update == k + 1 and q.refitsSinceRebuild == b.mesh_refit_count()[1]


def test_policy_single_matrix_and_a_tree_nobody_measured(monkeypatch):
    monkeypatch.delenv("RT_QNODES", raising=False)
    v, f, _ = _host_route("count_257")
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_rebuild(IDENT)                                    # the plain call: no measurement, so no baseline
        b.synchronize()
        assert b.mesh_update(rebuild_above=1.5) == "rebuild"     # rule 2
        b.synchronize()
        assert b.mesh_update(IDENT, rebuild_above=1.5) == "refit"
        b.synchronize()
        assert b.mesh_update(IDENT.reshape(4, 4), rebuild_above=1.0) == "refit"          # equal costs: not above
        assert (b.mesh_info().rebuilds, b.mesh_refit_count()) == (2, (2, 2))
        b.mesh_set_positions(_scattered(v))
        b.synchronize()
        assert b.mesh_update(rebuild_above=1.0) == "refit"       # the decision rests on the tree of the step before
        b.synchronize()
        q, base = b.mesh_quality(wait=False), b.mesh_quality("baseline", wait=False)
        assert q.cost.cost > base.cost.cost and q.refitsSinceRebuild == 3
        assert b.mesh_update(rebuild_above=1.0) == "rebuild"
        b.synchronize()
        assert b.mesh_quality("baseline", wait=False).update == b.mesh_quality(wait=False).update == 6
    v, f, _ = _host_route("point")                               # a degenerate record never asks for a rebuild
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        actions = []
        for _ in range(3):
            actions.append(b.mesh_update(rebuild_above=1.0))
            b.synchronize()
        assert actions == ["rebuild", "refit", "refit"] and b.mesh_quality(wait=False).cost.degenerate == 1


# ---------------------------------------------------------------- 3: no wait, no allocation
def test_no_wait_no_allocation(monkeypatch):
    monkeypatch.delenv("RT_QNODES", raising=False)
    v, f, (nodes, _, _) = _host_route("bunny5")
    want = rt.bvh_cost(nodes)
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        mi0 = b.mesh_info()
        b.mesh_rebuild(IDENT)
        b.mesh_measure()
        try:                                                     # straight behind the enqueue: not yet, or the right record -- never a wrong one
            q = b.mesh_quality(wait=False)
        except rt.RtError as e:
            assert e.code == rt.RT_ERR_STATE
        else:
            _same_record(q.cost, want, "polled")
            assert (q.update, q.refitsSinceRebuild) == (1, 0)
        _same_record(b.mesh_quality(wait=True).cost, want, "waited")
        # more measures than result slots, back to back: each behind a refit of its own, so that every measurement has its own serial
        calls, skipped_at = 3 * rt.RT_MESH_QUALITY_SLOTS, []
        seen = 0
        for k in range(calls):
            b.mesh_refit(IDENT)
            b.mesh_measure()
            now = b.mesh_quality(wait=False).skipped             # a record arrived above, so this cannot be RT_ERR_STATE
            if now != seen:
                skipped_at.append(k)
            assert now - seen in (0, 1)
            seen = now
        enqueued = [k for k in range(calls) if k not in skipped_at]
        b.synchronize()
        q = b.mesh_quality(wait=False)                           # drained: the newest enqueued measurement has arrived
        assert enqueued and q.update == 2 + enqueued[-1] and q.refitsSinceRebuild == 1 + enqueued[-1]
        assert q.skipped + len(enqueued) == calls and q.skipped == len(skipped_at)
        _same_record(q.cost, want, "after the burst")           # nothing moved: the rebuild's boxes, measured while other measurements were in flight
        b.mesh_update(rebuild_above=2.0)
        mi = b.mesh_info()
        assert mi.allocations == mi0.allocations and mi.hostSyncs == 0 and mi.scratchBytes == mi0.scratchBytes


# ---------------------------------------------------------------- 4: isolation
def test_frames_and_queries_do_not_see_measurements(monkeypatch):
    monkeypatch.delenv("RT_QNODES", raising=False)
    v, f = rt.meshgen.bunny_standin(4)
    M = rt.default_bvh_transform()
    W, H = 96, 64
    faces = scenes.tiny_env(8)
    p = rt.default_render_params()
    p.sppPerFrame = 1
    cam = scenes.camera("closeup", aspect=W / H)
    rng = np.random.default_rng(2)
    org = (rng.normal(0, 1, (2048, 3)) * 3).astype(np.float32)
    dirs = -org + rng.normal(0, 0.3, org.shape).astype(np.float32)
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)

    def run(measure):
        with rt.Renderer() as b:
            b.mesh_upload(v, f)
            b.mesh_rebuild(M)
            b.upload_env(faces)
            b.resize(W, H)
            info = b.scene_info()
            out = []
            for frame in range(2):
                if measure:
                    b.mesh_measure()
                b.render_frame(rt.frame_uniforms(p, cam, W, H, frame, True, info.nNodes, info.nTris))
                if measure:
                    b.mesh_measure()
                out += [np.array(x) for x in b.read_all()]
                b.mesh_refit(M)
            if measure:
                b.mesh_measure()
            hits = b.trace_rays(org, dirs, normals=True)
            if measure:
                assert b.mesh_quality(wait=True).update == 3
            return out + [np.array(hits.record), np.array(hits.normal)]

    for x, y in zip(run(False), run(True)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_refusals():
    v, f, _ = _host_route("count_9")
    L = rt.lib()
    with rt.Renderer() as b:
        q, action = rt.RtMeshQuality(), C.c_int(7)

        def update(mode, m, above):
            return L.rt_mesh_update(b._h, mode, None if m is None else m.ctypes.data_as(C.POINTER(C.c_float)), C.c_float(above), C.byref(action))

        # no mesh
        assert L.rt_mesh_measure(b._h) == rt.RT_ERR_INVALID
        assert L.rt_mesh_quality(b._h, rt.RT_MESH_QUALITY_LATEST, 0, C.byref(q)) == rt.RT_ERR_INVALID
        assert update(rt.RT_MESH_UPDATE_SINGLE, None, 2.0) == rt.RT_ERR_INVALID and action.value == 7
        b.mesh_upload(v, f)
        # no tree
        assert L.rt_mesh_measure(b._h) == rt.RT_ERR_INVALID
        assert L.rt_mesh_quality(b._h, rt.RT_MESH_QUALITY_LATEST, 1, C.byref(q)) == rt.RT_ERR_STATE       # nothing enqueued: nothing to wait for
        assert L.rt_mesh_quality(b._h, rt.RT_MESH_QUALITY_BASELINE, 0, C.byref(q)) == rt.RT_ERR_STATE
        assert L.rt_mesh_quality(b._h, 2, 0, C.byref(q)) == rt.RT_ERR_INVALID
        assert L.rt_mesh_quality(b._h, rt.RT_MESH_QUALITY_LATEST, 0, None) == rt.RT_ERR_INVALID
        # bad arguments of the policy: nothing is updated
        for above in (float("nan"), 0.999, 0.0, -3.0, float("-inf")):
            assert update(rt.RT_MESH_UPDATE_SINGLE, None, above) == rt.RT_ERR_INVALID
        assert update(rt.RT_MESH_UPDATE_PARTS, IDENT.copy(), 2.0) == rt.RT_ERR_INVALID
        assert update(2, None, 2.0) == rt.RT_ERR_INVALID
        assert b.mesh_info().rebuilds == 0 and action.value == 7
        with pytest.raises(TypeError):
            b.mesh_update()                                      # rebuild_above has no default
        with pytest.raises(TypeError):
            b.mesh_update(None, False, 2.0)                      # and is a keyword
        with pytest.raises(rt.RtError):
            b.mesh_quality("newest")
        assert update(rt.RT_MESH_UPDATE_SINGLE, None, float("inf")) == rt.RT_OK and action.value == rt.RT_MESH_DID_REBUILD
        assert L.rt_mesh_update(b._h, rt.RT_MESH_UPDATE_PARTS, None, C.c_float(1.0), None) == rt.RT_OK      # action may be NULL
        assert b.mesh_quality(wait=True).update == 2
        # rt_upload_bvh releases the mesh
        nodes, tris = rt.build_bvh(rt.gather_triangles(v, f, IDENT))
        b.upload_bvh(nodes, tris)
        assert L.rt_mesh_measure(b._h) == rt.RT_ERR_INVALID
        assert L.rt_mesh_quality(b._h, rt.RT_MESH_QUALITY_LATEST, 1, C.byref(q)) == rt.RT_ERR_INVALID
        assert update(rt.RT_MESH_UPDATE_SINGLE, None, 2.0) == rt.RT_ERR_INVALID
        assert b"rt_upload_bvh releases the mesh" in L.rt_last_error(b._h)
