"""The build choice of the traversal launches (csrc/rt_trace_build.cpp) without a GPU: rt.trace_build_cases over the WHOLE domain against
tests/trace_build_ref.py -- launch_trace's selection before the choice left the HIP header, transcribed from that commit -- and against
tests/golden/trace_build_parent.json, what that commit's own launch_trace chose for the environments the GPU option tests set.  Every build chosen is one
the library holds (rt.trace_builds_kept), so launch_trace's "no such kernel" path is unreachable; the precedence rules that tests/test_gpu_options.py quotes
in RAY_CASES' comments each hold over the whole domain.
"""
import functools
import itertools
import json
from pathlib import Path

import numpy as np

import opengl_raytracing_amd as rt
import trace_build_cases
import trace_build_ref as ref

GOLDEN = json.loads((Path(__file__).parent / "golden" / "trace_build_parent.json").read_text())
BIT = {n: v for n, v in rt.RT_BUILD_BITS.items() if n not in ("k_trace", "PACKETS")}

# the whole domain: hit kind, stats, then the tune, the five record forms, the exact any-hit stack size, the depth
AXES = (("any", (0, 1)), ("stats", (0, 1)), ("timing", (0, 1)), ("coop", (0, 1)), ("nearFirst", (0, 1)), ("qnodes", (-1, 0, 1, 2)), ("fused", (0, 1)), ("impl", (0, 1)),
        ("leafb", (2, 4)), ("leafbClosest", (2, 4)), ("q4", (0, 1)), ("wF", (0, 1)), ("iN2", (0, 1)), ("iN4", (0, 1)), ("iQ4", (0, 1)), ("anyStack", (0, 12)),
        ("depth", (1, 18)))


@functools.lru_cache(maxsize=None)
def _product():
    """(cases, builds): every combination of AXES as RtTraceCase records, and the library's answer to each -- one host call."""
    case, _ = rt._trace_build_types()
    grids = np.meshgrid(*[np.array(v, np.int32) for _, v in AXES], indexing="ij")
    cases = np.zeros(grids[0].size, case)
    for (name, _), g in zip(AXES, grids):
        cases[name] = g.reshape(-1)
    builds = rt.trace_build_cases(cases)
    for a in (cases, builds):
        a.setflags(write=False)
    return cases, builds


def test_whole_domain_equals_the_transcription_field_for_field():
    cases, builds = _product()
    assert cases.shape[0] == int(np.prod([len(v) for _, v in AXES])) == 262144
    names = [n for n, _ in AXES]
    combos = np.array(list(itertools.product(*[v for _, v in AXES])), np.int32)
    for j, n in enumerate(names):          # the order of np.meshgrid(indexing="ij"), flattened, is itertools.product's
        assert np.array_equal(cases[n], combos[:, j]), n
    got = zip(builds["opt"].tolist(), builds["nodes"].tolist(), builds["implPairs"].tolist(), builds["implLeafBoxes"].tolist(), builds["stack"].tolist(),
              builds["ldsBytes"].tolist())
    for combo, g in zip(combos.tolist(), got):
        c = dict(zip(names, combo))
        want = ref.launch_trace(bool(c["any"]), bool(c["stats"]), c["depth"], c["anyStack"], bool(c["q4"]), bool(c["wF"]), bool(c["iN2"]), bool(c["iN4"]), bool(c["iQ4"]),
                                c["timing"], c["coop"], c["nearFirst"], c["qnodes"], c["fused"], c["impl"], c["leafb"], c["leafbClosest"])
        assert g == tuple(int(x) for x in want), (c, g, want)


def test_every_build_chosen_is_kept_and_every_kept_build_is_chosen():
    """launch_trace dispatches over the kept lists alone: a choice outside them would launch nothing.  The lists hold nothing that is never chosen."""
    cases, builds = _product()
    for any_ in (0, 1):
        kept = rt.trace_builds_kept(any_)
        assert len(set(kept)) == len(kept)
        chosen = set(np.unique(builds["opt"][cases["any"] == any_]).tolist())
        assert chosen == set(kept), (any_, sorted(chosen), sorted(kept))
    assert len(rt.trace_builds_kept(False)) == 10 and len(rt.trace_builds_kept(True)) == 11     # the parent's instantiations per ray source and hit kind


def test_golden_cases_equal_the_parents_launch_trace():
    listed = trace_build_cases.cases()
    assert {c[0] for c in listed} == set(GOLDEN) and len(GOLDEN) >= 36
    for name, env, any_, stats, depth, any_stack, forms, want_bits in listed:
        g = GOLDEN[name]
        assert (g["env"], g["any"], g["stats"], g["depth"], g["anyStack"], tuple(g["forms"])) == (env, any_, stats, depth, any_stack, forms), name
        assert trace_build_cases.with_env(env, rt.trace_options) == g["tune"] == ref.tune_from_env(env), name
        # with no options given rt.trace_build reads the environment, as the launch does
        b = trace_build_cases.with_env(env, lambda: rt.trace_build(any_, depth=depth, stats=stats, any_stack=any_stack, forms=forms))
        e = g["expect"]
        assert (b.opt, b.nodes, b.implPairs, b.implLeafBoxes, b.stack, b.ldsBytes) == (e["opt"], e["nodes"], e["implPairs"], e["implLeafBoxes"], e["stack"], e["ldsBytes"]), name
        assert b == rt.trace_build(any_, depth=depth, stats=stats, any_stack=any_stack, forms=forms, **g["tune"]), name
        # ... and the parent chose what tests/test_gpu_options.py expects of the device under this environment
        assert b.bits == frozenset(want_bits), (name, b.bits, want_bits)


# ---- the precedence rules quoted in RAY_CASES' comments, each over the whole domain

def _has(builds, bit):
    return (builds["opt"] & BIT[bit]) != 0


def _nodes(builds, name):
    return builds["nodes"] == rt.TRACE_NODES.index(name)


def test_fused_yields_to_coop():
    cases, builds = _product()
    coop = (cases["any"] == 0) & (cases["coop"] != 0)
    assert coop.any() and not _has(builds, "FUSE")[coop].any() and not _nodes(builds, "wF")[coop].any()
    plain = coop & (cases["stats"] == 0)
    assert _has(builds, "COOP")[plain].all()


def test_implicit_closest_hit_records_yield_to_coop_and_to_fused():
    cases, builds = _product()
    closest = cases["any"] == 0
    coop = closest & (cases["coop"] != 0)
    assert not _has(builds, "IMPL")[coop].any() and not _nodes(builds, "iN2")[coop].any()
    fused = closest & _nodes(builds, "wF")
    assert fused.any() and not _has(builds, "IMPL")[fused].any() and not builds["implPairs"][fused].any()


def test_quantised_wins_over_leafb4():
    cases, builds = _product()
    qn = (cases["any"] == 1) & (_has(builds, "QN1") | _has(builds, "QN2"))
    assert (qn & (cases["leafb"] == 4)).any() and not _has(builds, "LEAFB4")[qn].any()
    # ... and only the any-hit launch is quantised: the closest-hit launch of the same tune keeps its own leaf groups
    closest = (cases["any"] == 0) & (cases["stats"] == 0) & (cases["coop"] == 0) & (cases["fused"] == 0) & (cases["impl"] == 0)
    assert (_has(builds, "LEAFB4")[closest] == (cases["leafbClosest"][closest] == 4)).all()
    assert not (_has(builds, "QN1") | _has(builds, "QN2"))[cases["any"] == 0].any()


def test_near_first_walks_the_exact_nodes():
    cases, builds = _product()
    near = (cases["any"] == 1) & (cases["nearFirst"] != 0)
    assert _nodes(builds, "w4")[near].all() and not (_has(builds, "QN1") | _has(builds, "QN2") | _has(builds, "IMPL"))[near].any()
    assert _has(builds, "NEAR")[near & (cases["stats"] == 0)].all()
    assert not _has(builds, "NEAR")[cases["any"] == 0].any()


def test_implicit_any_hit_needs_leafb_below_4_an_exact_stack_and_not_qnodes_1():
    cases, builds = _product()
    impl = (cases["any"] == 1) & _has(builds, "IMPL")
    assert impl.any()
    assert (cases["leafb"][impl] < 4).all() and (cases["anyStack"][impl] > 0).all() and (cases["iN4"][impl] == 1).all() and (cases["impl"][impl] != 0).all()
    assert not _has(builds, "QN1")[impl].any()
    quantised = impl & _has(builds, "QN2")
    assert quantised.any() and (cases["qnodes"][quantised] != 1).all() and _nodes(builds, "iQ4")[quantised].all()
    assert _nodes(builds, "iN4")[impl & ~quantised].all() and builds["implPairs"][impl].all() and builds["implLeafBoxes"][impl].all()
    # RT_QNODES=1 with the quantised nodes built: the seven-wave quantised build, not the implicit one
    q1 = (cases["any"] == 1) & (cases["stats"] == 0) & (cases["nearFirst"] == 0) & (cases["qnodes"] == 1) & (cases["q4"] == 1)
    assert _has(builds, "QN1")[q1].all() and not _has(builds, "IMPL")[q1].any()


def test_timing_ignores_everything_except_implicit():
    cases, builds = _product()
    timing = (cases["stats"] == 1) & (cases["timing"] != 0)
    assert _has(builds, "TIMING")[timing].all() and not _has(builds, "TIMING")[~timing].any()
    assert set(np.unique(builds["opt"][timing]).tolist()) == {BIT["TIMING"], BIT["TIMING"] | BIT["IMPL"]}
    # without sums to add to, RT_TRACE_TIMING changes nothing (rt_debug_trace, the ray queries)
    cases_off = cases[(cases["stats"] == 0) & (cases["timing"] != 0)].copy()
    with_timing = rt.trace_build_cases(cases_off)
    cases_off["timing"] = 0
    assert np.array_equal(with_timing, rt.trace_build_cases(cases_off))


def test_stack_and_lds_bytes():
    """Closest-hit: one 8-byte entry per binary level; any-hit: the exact size of the upload, else three 4-byte entries per two levels; four at least.
    k_trace_packets launches with the any-hit figures."""
    cases, builds = _product()
    a = cases["any"] == 1
    want = np.where(a, np.where(cases["anyStack"] > 0, cases["anyStack"], 3 * ((cases["depth"] + 1) // 2)), cases["depth"])
    assert np.array_equal(builds["stack"], np.maximum(4, want))
    assert np.array_equal(builds["ldsBytes"], 256 * builds["stack"].astype(np.uint64) * np.where(a, 4, 8).astype(np.uint64))
