"""The device BVH builders against their definition (tests/bvh_build_ref.py, proved on the CPU by tests/test_bvh_build_ref.py) on the meshes where a
builder goes wrong: centroid ties at medians, equal extents, signed zeros, denormal and huge coordinates, degenerate triangles, and every count
around the leaf threshold and a ragged last level.  Every comparison is bit for bit; there is no tolerance in this file.

  1. build_bvh_gpu(t9) == ref_build(t9): nodes12 and tris12 as uint32 -- rows inside leaves and the sign of zero box coordinates included.
  2. mesh_upload + mesh_rebuild(M): mesh_order() == the reference's order, the device triangle array == its tris12, and all seven scene arrays and
     RtSceneInfo == those of a fresh context given upload_bvh(reference arrays), under RT_QNODES unset, "2" and "0".
  3. mesh_refit == ref_refit from the reference's arrays: nothing moved (the rebuild's bytes), a deformation, vertices moved onto +-0.
  4. The winner of exact-t ties end to end: closest-hit and any-hit ray queries and frames on the rebuilt scene against the oracle on the reference's
     arrays, on ray sets of which hundreds have two or more triangles at the bit-equal closest t."""
import functools

import numpy as np
import pytest

import bvh_build_ref as ref
import opengl_raytracing_amd as rt
import scenes
from test_gpu_dynamic_mesh import TRANSFORMS, _assert_same_scene, _model

pytestmark = pytest.mark.gpu

f32 = np.float32
NEGZERO = np.where(np.eye(4, dtype=f32) == 0, f32(-0.0), f32(1.0)).astype(f32).reshape(-1)      # the identity with -0 for every 0: keeps some -0 coordinates -0
SMALL = tuple(n for n in ref.corpus(None) if not n.startswith("count_")) + ("bunny5", "bunny6")      # the bunnies tie under "default" only (test_bvh_build_ref.py)
COUNT_NAMES = tuple(f"count_{n}" for n in ref.COUNTS)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@functools.lru_cache(maxsize=1)
def _corpus():
    return ref.corpus(rt.meshgen)


def _matrix(tname):
    return NEGZERO if tname == "negzero" else _model(tname)


def _t9(name, tname, positions=None):
    """The triangles the builders see.  "raw": the mesh's own coordinates (numpy, so -0 stays -0); else the library's gather under that transform."""
    v, f = _corpus()[name]
    v = v if positions is None else positions
    return ref.gather(v, f) if tname == "raw" else rt.gather_triangles(v, f, _matrix(tname))


@functools.lru_cache(maxsize=16)
def _reference(name, tname):
    t9 = _t9(name, tname)
    return (t9,) + ref.ref_build(t9)


def _diff(what, got, want):
    """Where two float arrays differ -- which array, how many rows, the first differing row and column with both versions of it -- or None."""
    g, w = bits(got), bits(want)
    if g.shape != w.shape:
        return f"{what}: shape {g.shape} != {w.shape}"
    bad = np.argwhere(g != w)
    if bad.size == 0:
        return None
    r, c = bad[0]
    return f"{what}: {bad.shape[0]} words differ in {np.unique(bad[:, 0]).size} rows; first row {r} column {c}: got {got[r].tolist()} want {want[r].tolist()}"


def _check_build(r, name, tname):
    t9, nodes, tris, _ = _reference(name, tname)
    ng, tg = r.build_bvh_gpu(t9)
    return [f"{name}/{tname}: {d}" for d in (_diff("nodes12", ng, nodes), _diff("tris12", tg, tris)) if d]


# ---------------------------------------------------------------- 1: build_bvh_gpu == ref_build
@pytest.mark.parametrize("name", SMALL)
def test_build_equals_the_definition(name):
    with rt.Renderer() as r:
        bad = [b for tname in ("raw",) + tuple(TRANSFORMS) for b in _check_build(r, name, tname)]
    assert not bad, "\n".join(bad)


def test_build_equals_the_definition_at_every_count():
    bad = []
    with rt.Renderer() as r:
        for name in COUNT_NAMES:
            for tname in ("raw",) + tuple(TRANSFORMS):
                bad += _check_build(r, name, tname)
    assert not bad, f"{len(bad)} differences\n" + "\n".join(bad[:20])


# ---------------------------------------------------------------- 2: mesh_rebuild installs the definition's scene
def _set_qnodes(monkeypatch, qnodes):
    if qnodes is None:
        monkeypatch.delenv("RT_QNODES", raising=False)
    else:
        monkeypatch.setenv("RT_QNODES", qnodes)


def _rows(b, n):
    return b.debug_read_scene("tris").view(f32).reshape(-1, 12)[:n]


def _assert_scene_is(b, nodes, tris, order, what):
    """Context b's scene against the reference's arrays: the order, the triangle rows, and every scene array and RtSceneInfo of a fresh context given
    upload_bvh(nodes, tris) -- a rejected quantised form (RT_SCENE_QNODES_REJECTED in flags) must be rejected alike."""
    n = tris.shape[0]
    got = b.mesh_order(as_torch=False)
    assert np.array_equal(got, order), (what, "order", int((got != order).sum()), np.flatnonzero(got != order)[:8])
    d = _diff("device tris", _rows(b, n), tris)
    assert d is None, (what, d)
    with rt.Renderer() as a:
        a.upload_bvh(nodes, tris)
        return _assert_same_scene(a, b, what)


def _rebuild_case(b, name, tname, qnodes):
    _, nodes, tris, order = _reference(name, tname)
    b.mesh_rebuild(_matrix(tname))
    info = _assert_scene_is(b, nodes, tris, order, (name, tname, qnodes))
    if qnodes == "0":
        assert b.debug_read_scene("qnodes4").size == 0
    if qnodes == "2" and tris.shape[0] > 8:
        assert b.debug_read_scene("qnodes4").size > 0 or info.flags & rt.RT_SCENE_QNODES_REJECTED
    return info


@pytest.mark.parametrize("qnodes", [None, "2", "0"])
@pytest.mark.parametrize("name", SMALL)
def test_rebuild_installs_the_definition(monkeypatch, name, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    v, f = _corpus()[name]
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        for tname in tuple(TRANSFORMS) + ("negzero",):
            _rebuild_case(b, name, tname, qnodes)


@pytest.mark.parametrize("qnodes", [None, "2", "0"])
def test_rebuild_installs_the_definition_at_every_count(monkeypatch, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    with rt.Renderer() as b:
        for name in COUNT_NAMES:
            b.mesh_upload(*_corpus()[name])
            for tname in ("default", "rot-scale"):
                _rebuild_case(b, name, tname, qnodes)


# ---------------------------------------------------------------- 3: mesh_refit == ref_refit
def _wave(pos, k=0):
    """A smooth displacement of 3 % of the mesh's extent (fp32)."""
    with np.errstate(all="ignore"):
        ext = f32((pos.max(0) - pos.min(0)).max())
        ext = ext if ext > 0 else f32(1.0)
        return (pos + (f32(0.03) * ext * np.sin(f32(3.0) * pos / ext + f32(0.7 + k))).astype(f32)).astype(f32)


def _onto_zero(pos, seed=5):
    """A third of all coordinates moved onto exact zero, -0 and +0 mixed."""
    rng = np.random.default_rng(seed)
    out = np.array(pos, f32)
    hit = rng.random(out.shape) < 1.0 / 3.0
    out[hit] = np.where(rng.random(int(hit.sum())) < 0.5, f32(-0.0), f32(0.0))
    return out


def _refit_case(b, name, tname0, steps, qnodes):
    v, f = _corpus()[name]
    v = np.ascontiguousarray(v, f32)
    _, nodes, tris, order = _reference(name, tname0)
    b.mesh_upload(v, f)
    b.mesh_rebuild(_matrix(tname0))
    b.mesh_refit(_matrix(tname0))                            # nothing moved: the rebuild's bytes, which are the reference's
    _assert_scene_is(b, nodes, tris, order, (name, qnodes, "unmoved"))
    pos = v
    for label, deform, tname in steps:
        pos = deform(pos)
        b.mesh_set_positions(pos)
        b.mesh_refit(_matrix(tname))
        n2, t2 = ref.ref_refit(_t9(name, tname, pos), order, nodes, tris)
        _assert_scene_is(b, n2, t2, order, (name, qnodes, label))
        if label == "zeros" and name in MINUS_ZERO_ROWS:
            assert (bits(t2) == 0x80000000).any(), (name, "no -0 reached the rows")
        if label == "zeros" and name in MINUS_ZERO_BOXES:
            assert (bits(n2[:, [0, 1, 2, 4, 5, 6]]) == 0x80000000).any(), (name, "no -0 reached a box")


MINUS_ZERO_ROWS = ("lattice", "floor_grid", "dup8", "signed_zero", "denormal", "huge", "degenerate", "bunny5", "bunny6")
MINUS_ZERO_BOXES = ("signed_zero", "floor_grid")
STEPS = (("wave", _wave, "default"), ("zeros", _onto_zero, "negzero"), ("wave2", lambda p: _wave(p, 1), "rot-scale"))


@pytest.mark.parametrize("qnodes", [None, "2"])
@pytest.mark.parametrize("name", SMALL)
def test_refit_equals_the_definition(monkeypatch, name, qnodes):
    _set_qnodes(monkeypatch, qnodes)
    with rt.Renderer() as b:
        _refit_case(b, name, "rot-scale", STEPS, qnodes)
        if name == "signed_zero":                            # the suspected case: a rebuild and a refit of the same unmoved -0 / +0 plane
            _refit_case(b, name, "negzero", STEPS[:1], qnodes)


def test_refit_equals_the_definition_at_every_count(monkeypatch):
    _set_qnodes(monkeypatch, None)
    with rt.Renderer() as b:
        for name in COUNT_NAMES:
            _refit_case(b, name, "default", STEPS[:2], None)


# ---------------------------------------------------------------- 1-3 at one million triangles
def test_million_triangles(monkeypatch):
    """The build under the three TRANSFORMS, like every other mesh.  What is cut at this size, for the file's running time: the "raw" build (the scene
    has no -0 coordinate, so it is the identity build again), the rebuild under RT_QNODES "2" and "0" (unset already chooses the quantised form at
    this tree size, asserted below; the form's absence is size-independent and covered by every smaller mesh) and the rebuild under the other
    transforms (tests/test_gpu_dynamic_mesh.py rebuilds this scene under the identity against build_bvh_gpu, which is pinned here)."""
    _set_qnodes(monkeypatch, None)
    name = "million"
    v, f = _corpus()[name]
    v = np.ascontiguousarray(v, f32)
    with rt.Renderer() as b:
        bad = [d for tname in TRANSFORMS for d in _check_build(b, name, tname)]
        assert not bad, "\n".join(bad)
        t9, nodes, tris, order = _reference(name, "default")
        b.mesh_upload(v, f)
        b.mesh_rebuild(_matrix("default"))
        info = _assert_scene_is(b, nodes, tris, order, (name, "rebuild"))
        assert b.debug_read_scene("qnodes4").size > 0 and info.flags == 0      # the quantised form is in use
        b.mesh_refit(_matrix("default"))
        _assert_scene_is(b, nodes, tris, order, (name, "unmoved"))
        pos = _onto_zero(_wave(v), 6)
        b.mesh_set_positions(pos)
        b.mesh_refit(NEGZERO)
        n2, t2 = ref.ref_refit(_t9(name, "negzero", pos), order, nodes, tris)
        _assert_scene_is(b, n2, t2, order, (name, "deformed"))


# ---------------------------------------------------------------- 4: the winner of exact-t ties, end to end
TIE_MESHES = ("dup8", "floor_grid", "lattice")


def _unit(d):
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def _tie_rays(name, nodes, tris, seed=21):
    """scenes.adversarial_rays plus rays built to meet several triangles at one t: axis-parallel rays through mesh vertices and through the midpoints
    of edges, starting an exact small distance away (every product of the intersection is then exact for the integer meshes); for the floor these are
    vertical rays that cross it on grid lines."""
    rng = np.random.default_rng(seed)
    org, dirs, tmax = scenes.adversarial_rays(nodes, tris, n=300)
    O, D, T = [org], [dirs], [tmax]
    n = tris.shape[0]
    k = rng.integers(0, n, 1800)
    v0, e1, e2 = tris[k, 0:3], tris[k, 4:7], tris[k, 8:11]
    corner = np.where((rng.random(k.size) < 0.5)[:, None], v0, (v0 + e1).astype(f32)).astype(f32)
    mid = (v0 + f32(0.5) * e2).astype(f32)
    target = np.where((np.arange(k.size) % 3 == 0)[:, None], mid, corner).astype(f32)      # two vertex rays to one edge ray
    axis = rng.integers(0, 3, k.size)
    if name == "floor_grid":
        axis[:] = 1                                          # a ray in the floor's plane meets nothing
    side = np.where(rng.random(k.size) < 0.5, -1.0, 1.0).astype(f32)
    step = (f32(2.0) ** rng.integers(-8, 2, k.size)).astype(f32)      # powers of two: exact offsets, and short enough that little lies in between
    d = np.zeros((k.size, 3), f32)
    d[np.arange(k.size), axis] = -side
    o = target.copy()
    o[np.arange(k.size), axis] += side * step
    O.append(o.astype(f32)); D.append(d); T.append((step * f32(rng.choice([0.5, 1.0, 2.0], k.size))).astype(f32))   # any-hit: short of, at, and past the tie
    # slanted rays at the same targets: the tie survives only where the arithmetic happens to agree
    o2 = (target + rng.normal(0, 1, target.shape) * 2.0).astype(f32)
    O.append(o2); D.append(_unit(target - o2)); T.append(np.full(k.size, 4.0, f32))
    return np.concatenate(O).astype(f32), np.concatenate(D).astype(f32), np.concatenate(T).astype(f32)


def _oracle_answers(orc, u, nodes, tris, org, dirs, tmax):
    """Per ray the oracle's (prim, t, occluded) and the number of triangles at the bit-equal closest t, counted with the oracle's own triHit over the
    triangles that share a corner position with the winner (in these meshes, triangles meet where they share a vertex or are copies)."""
    N = org.shape[0]
    prim = np.zeros(N, np.int32); t = np.zeros(N, f32); occ = np.zeros(N, bool); ties = np.zeros(N, np.int32)
    corners = np.stack([tris[:, 0:3], (tris[:, 0:3] + tris[:, 4:7]).astype(f32), (tris[:, 0:3] + tris[:, 8:11]).astype(f32)], 1)   # [n, 3, 3]
    keys = bits(corners + f32(0.0)).reshape(-1, 3, 3)                                      # + 0: -0 and +0 are one position
    where = {}
    for row, cs in enumerate(keys.tolist()):
        for c in cs:
            where.setdefault(tuple(c), []).append(row)
    for i in range(N):
        prim[i], t[i] = orc.trace_bvh_prim(u, nodes, tris, org[i], dirs[i])
        occ[i] = orc.trace_bvh_shadow(u, nodes, tris, org[i], dirs[i], float(tmax[i]))
        if prim[i] >= 0:
            cand = sorted({r for c in keys[prim[i]].tolist() for r in where[tuple(c)]})
            for r in cand:
                h = orc.tri_hit(u, org[i], dirs[i], tris[r], u.inf)
                ties[i] += bool(h[0]) and bits(h[1:2])[0] == bits(t[i:i + 1])[0]
    return prim, t, occ, ties


@pytest.mark.parametrize("name", TIE_MESHES)
def test_exact_t_ties_ray_by_ray(orc, monkeypatch, name):
    _set_qnodes(monkeypatch, None)
    v, f = _corpus()[name]
    _, nodes, tris, order = _reference(name, "identity")
    u = rt.frame_uniforms(rt.default_render_params(), rt.default_camera(), 64, 64, 0, True, nodes.shape[0], tris.shape[0])
    org, dirs, tmax = _tie_rays(name, nodes, tris)
    prim, t, occ, ties = _oracle_answers(orc, u, nodes, tris, org, dirs, tmax)
    hit = prim >= 0
    print(f"{name}: {org.shape[0]} rays, {int(hit.sum())} hits, {int(occ.sum())} occluded, {int((ties >= 2).sum())} rays with two or more triangles at the closest t")
    assert (ties >= 2).sum() >= 300, (name, int((ties >= 2).sum()))
    assert (ties[hit] >= 1).all()                            # the winner itself is among the candidates
    with rt.Renderer() as b:
        b.mesh_upload(v, f)
        b.mesh_rebuild(_matrix("identity"))
        dev_order = b.mesh_order(as_torch=False)
        res = b.trace_rays(org, dirs, eps=u.eps, inf=u.inf)
        any_hit = np.asarray(b.trace_rays(org, dirs, tmax, any_hit=True, eps=u.eps, inf=u.inf))
    got_prim, got_t = np.asarray(res.prim), np.asarray(res.t)
    bad = np.flatnonzero(got_prim != prim)
    assert bad.size == 0, (name, "prim", bad.size, [(int(i), int(got_prim[i]), int(prim[i]), int(ties[i])) for i in bad[:8]])
    bad = np.flatnonzero(bits(got_t) != bits(np.where(hit, t, f32(u.inf))))
    assert bad.size == 0, (name, "t", bad.size, bad[:8])
    assert np.array_equal(dev_order[got_prim[hit]], order[prim[hit]])
    bad = np.flatnonzero((any_hit != 0) != occ)
    assert bad.size == 0, (name, "any-hit", bad.size, bad[:8])
    assert 50 < occ.sum() < org.shape[0] - 50


@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel"])
@pytest.mark.parametrize("name", TIE_MESHES)
def test_frames_on_the_tie_meshes(orc, monkeypatch, name, pipeline):
    _set_qnodes(monkeypatch, None)
    pl = rt.RT_PIPELINE_AUTO if pipeline == "wavefront" else rt.RT_PIPELINE_MEGAKERNEL
    v, f = _corpus()[name]
    _, nodes, tris, _ = _reference(name, "default")
    W, H = 64, 48
    faces = scenes.tiny_env(8)
    p = rt.default_render_params()
    p.sppPerFrame = 2
    cam = scenes.camera("closeup", aspect=W / H)
    with rt.Renderer(pipeline=pl) as b:
        b.mesh_upload(v, f)
        b.mesh_rebuild(_matrix("default"))
        b.upload_env(faces)
        b.resize(W, H)
        prev = None
        for frame in range(2):
            u = rt.frame_uniforms(p, cam, W, H, frame, True, nodes.shape[0], tris.shape[0])
            b.render_frame(u)
            want, cnt = orc.render(u, nodes, tris, faces, prev)
            for g, w_, what in zip(b.read_all(), want, ("color", "motion", "gpos", "gnrm")):
                assert np.array_equal(g, w_), (name, pipeline, frame, what, int((g != w_).sum()))
            prev = want[0]
        assert cnt.hitPixels > 0, (name, "the camera does not see the mesh")
