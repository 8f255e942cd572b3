"""tests/bvh_build_ref.py proved before it judges the device (tests/test_gpu_bvh_corpus.py): where the host builder is defined -- tie-free input --
the numpy definition equals it bit for bit; on every corpus mesh it yields a valid tree that rt_refit_bvh reproduces unchanged; and the tie-heavy
meshes really tie."""
import functools
from pathlib import Path

import numpy as np
import pytest

import bvh_build_ref as ref
import opengl_raytracing_amd as rt

GOLDEN = Path(__file__).resolve().parent / "golden"
CORPUS_NAMES = tuple(ref.corpus(None)) + ("bunny5", "bunny6", "million")
# The icosphere-based bunny stand-ins have no tied median in their own coordinates: their symmetric centroids become bit-equal only once the default
# transform has rounded them.  They are tie cases under that transform alone -- the one every frame and the bench use; their "raw" and "identity"
# cases in tests/test_gpu_bvh_corpus.py pin a tie-free tree.
TIES_UNDER_DEFAULT_ONLY = ("bunny5", "bunny6")


@functools.lru_cache(maxsize=1)
def _corpus():
    return ref.corpus(rt.meshgen)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _leaf_sets_equal(nodes, ta, tb):
    first, count = nodes[:, 8].astype(int), nodes[:, 9].astype(int)
    for i in np.flatnonzero(count > 0):
        sl = slice(first[i], first[i] + count[i])
        assert sorted(map(tuple, bits(ta[sl]).tolist())) == sorted(map(tuple, bits(tb[sl]).tolist())), i


def _tie_free_inputs():
    for n in (1, 8, 9, 17, 100, 1000, 20480):               # the soups of test_gpu_bvh_build.py
        rng = np.random.default_rng(n)
        t9 = rng.normal(0, 1, (n, 9)).astype(np.float32)
        t9[:, 3:] *= 0.1
        yield f"soup{n}", t9
    yield "fixture320", np.load(GOLDEN / "bvh_build_320.npz")["tris9"]
    rng = np.random.default_rng(9)                          # test_host_parity.py's cases, drawn as it draws them
    yield "random300", rng.normal(size=(300, 9)).astype(np.float32)
    rng = np.random.default_rng(9)
    yield "n9", rng.normal(size=(9, 9)).astype(np.float32)
    rng = np.random.default_rng(9)
    yield "n1", rng.normal(size=(1, 9)).astype(np.float32)


def test_reference_equals_the_host_builder_on_tie_free_input():
    for name, t9 in _tie_free_inputs():
        stats = {}
        nr, tr, order = ref.ref_build(t9, stats)
        assert stats["tied_medians"] == 0, name
        nh, th, oh = rt.build_bvh_order(t9)
        assert nr.shape == nh.shape and np.array_equal(bits(nr), bits(nh)), name           # numbering, links, first, count, boxes
        _leaf_sets_equal(nh, tr, th)
        assert np.array_equal(np.sort(order), np.sort(oh))
    d = np.load(GOLDEN / "bvh_build_320.npz")                                              # the oracle's own build, as committed
    nr, tr, _ = ref.ref_build(d["tris9"])
    assert np.array_equal(bits(nr), bits(d["nodes12"]))
    _leaf_sets_equal(d["nodes12"], tr, d["tris12"])


def _deformed(v, seed=3):
    """Every vertex moved by up to 5 % of the mesh's extent (fp32), some of them onto exact +-0."""
    rng = np.random.default_rng(seed)
    v = np.ascontiguousarray(v, np.float32)
    with np.errstate(all="ignore"):
        ext = np.float32((v.max(0) - v.min(0)).max())
        out = (v + (rng.uniform(-0.05, 0.05, v.shape) * ext).astype(np.float32)).astype(np.float32)
    hit = rng.random(v.shape) < 0.1
    out[hit] = np.where(rng.random(int(hit.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    return out


@pytest.mark.parametrize("name", CORPUS_NAMES)
def test_corpus_mesh(name):
    v, f = _corpus()[name]
    t9 = ref.gather(v, f)
    stats = {}
    nodes, tris, order = ref.ref_build(t9, stats)
    n = t9.shape[0]
    L = rt.bvh_layout(n)
    assert nodes.shape == (L.nNodes, 12) and tris.shape == (n, 12) and order.dtype == np.int32
    ref.check_tree(nodes, tris, order, t9)                   # a valid tree; order a permutation; rows = tris9[order]
    # the host builder's skeleton: numbering, links, first and count depend on the count alone
    nh, _ = rt.build_bvh(t9)
    assert np.array_equal(bits(nodes[:, [3, 7, 8, 9]]), bits(nh[:, [3, 7, 8, 9]]))
    # nothing moved: rt_refit_bvh returns the reference's arrays unchanged, -0 and denormals included
    n2, t2 = rt.refit_bvh(nodes, tris, order, t9)
    assert np.array_equal(bits(n2), bits(nodes)) and np.array_equal(bits(t2), bits(tris))
    # a deformation: the numpy refit equals rt_refit_bvh
    d9 = ref.gather(_deformed(v), f)
    n3, t3 = rt.refit_bvh(nodes, tris, order, d9)
    r3, s3 = ref.ref_refit(d9, order, nodes, tris)
    assert np.array_equal(bits(n3), bits(r3)) and np.array_equal(bits(t3), bits(s3))
    assert not np.array_equal(bits(n3), bits(nodes))
    # the ties: in the mesh's own coordinates, and under the default transform every other test of the builders gathers with
    under_default = {}
    nd, td, od = ref.ref_build(rt.gather_triangles(v, f), under_default)
    ref.check_tree(nd, td, od, rt.gather_triangles(v, f))
    print(f"{name}: {n} triangles, {L.nInner} inner nodes, tied medians {stats['tied_medians']} (default transform: {under_default['tied_medians']})")
    if name in TIES_UNDER_DEFAULT_ONLY:
        assert stats["tied_medians"] == 0 and under_default["tied_medians"] >= 1, name
    elif name in ref.TIE_HEAVY:
        assert stats["tied_medians"] >= 1 and under_default["tied_medians"] >= 1, name
    if name == "lattice":
        assert n == 5000 and stats["tied_medians"] >= 100


def test_corpus_hits_what_it_is_built_for():
    c = _corpus()
    box = lambda name: ref.ref_build(ref.gather(*c[name]))[0][0]
    ext = lambda b: (b[4:7] - b[0:3])
    e = ext(box("cube_xyz")); assert e[0] == e[1] == e[2] > 0
    e = ext(box("cube_xy")); assert e[0] == e[1] > e[2]
    e = ext(box("cube_xz")); assert e[0] == e[2] > e[1]
    e = ext(box("cube_yz")); assert e[1] == e[2] > e[0]
    assert (ext(box("point")) == 0).all()
    assert ext(box("floor_grid"))[1] == 0
    b = box("signed_zero")                                   # the plane's box: -0 below, +0 above
    assert bits(b[1]) == 0x80000000 and bits(b[5]) == 0
    t9 = ref.gather(*c["signed_zero"])
    assert (bits(t9) == 0x80000000).sum() > 100 and (bits(t9) == 0).sum() > 100
    e = ext(box("denormal")); assert (e > 0).all() and (e < np.float32(1.2e-38)).all()
    assert np.abs(box("huge")[[0, 1, 2, 4, 5, 6]]).min() > 8e29
    nodes = ref.ref_build(ref.gather(*c["mixed_scale"]))[0]
    e = (nodes[:, 4:7] - nodes[:, 0:3]).max(1)
    assert (e[e > 0] < 1e-29).any() and e.max() > 900
    t9 = ref.gather(*c["degenerate"])
    area = np.linalg.norm(np.cross(t9[:, 3:6].astype(np.float64), t9[:, 6:9].astype(np.float64)), axis=1)
    assert 100 < (area == 0).sum() < 300
    assert (np.abs(t9[:, 3:9]).max(1) == 0).sum() >= 50      # repeated-vertex triangles: both edges zero
    assert set(ref.COUNTS) >= set(range(1, 41)) | {15, 16, 17, 127, 128, 129, 4095, 4096, 4097, 32767, 32769}


def test_a_wrong_definition_differs(monkeypatch):
    """The corpus can tell a subtly wrong builder from the right one: a sort that is not stable (here: equal keys in reverse order, so the outcome
    does not depend on the numpy at hand) or `>=` in the axis rule changes boxes and rows on the lattice; on identical triangles, where boxes and rows
    cannot differ, the wrong sort still shows in the order."""
    c = _corpus()

    def wrong(name, attr, fn):
        with monkeypatch.context() as m:
            m.setattr(ref, attr, fn)
            return ref.ref_build(ref.gather(*c[name]))

    ge = lambda ex, ey, ez: np.where(ex >= ey, np.where(ex >= ez, 0, 2), np.where(ey >= ez, 1, 2))
    ties_reversed = lambda key: np.lexsort((-np.arange(key.size), key))
    good = ref.ref_build(ref.gather(*c["lattice"]))
    for bad in (wrong("lattice", "level_sort", ties_reversed), wrong("lattice", "split_axis", ge)):
        assert (bits(good[0]) != bits(bad[0])).any(1).sum() > 100 and (bits(good[1]) != bits(bad[1])).any(1).sum() > 1000
    assert not np.array_equal(bits(ref.ref_build(ref.gather(*c["cube_xyz"]))[0]), bits(wrong("cube_xyz", "split_axis", ge)[0]))
    good, bad = ref.ref_build(ref.gather(*c["identical"])), wrong("identical", "level_sort", ties_reversed)
    assert np.array_equal(bits(good[0]), bits(bad[0])) and np.array_equal(bits(good[1]), bits(bad[1]))
    assert np.array_equal(good[2][-7:], np.arange(7)) and np.array_equal(good[2][:8], np.arange(992, 1000))      # nothing moves: input order, leaf by leaf
    assert not np.array_equal(good[2], bad[2])
