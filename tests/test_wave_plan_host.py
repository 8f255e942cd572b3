"""The ray-queue planner (csrc/rt_wave_plan.cpp) without a GPU: rt.wave_plan against tests/wave_plan_ref.py -- the arithmetic of
rt_wave_render before the planner existed, transcribed from that commit -- and against tests/golden/wave_plan_parent.json, what that commit allocated on
the device.  Pure arithmetic: every scalar, every arena total, and the layout of every arena.
"""
import json
from pathlib import Path

import pytest

import opengl_raytracing_amd as rt
import wave_plan_cases
import wave_plan_ref as ref

GOLDEN = json.loads((Path(__file__).parent / "golden" / "wave_plan_parent.json").read_text())
BATCH8 = 16_588_800        # pixel slots of eight 1080p frames


def _either_side_of_comfort(spp, ao):
    """Two slot counts (tiles x 256), one tile apart, on either side of the 4 GiB rule -- found with the transcription."""
    lo, hi = 1, 1 << 20        # tiles
    assert not ref.plan(lo * 256, spp, ao)["deferred"] and ref.plan(hi * 256, spp, ao)["deferred"]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ref.plan(mid * 256, spp, ao)["deferred"] else (mid, hi)
    return lo * 256, hi * 256


BELOW, ABOVE = _either_side_of_comfort(4, 4)

# (id, slots, spp, AO rays (0: off), options as rt.wave_plan takes them, hits, share)
CASES = [
    ("one_tile_no_ao", 256, 1, 0, {}, None, 0.0),
    ("4096_spp2_ao3", 4096, 2, 3, {}, None, 0.0),
    ("160x96_1mb", 15360, 2, 3, {"budget_mb": 1}, None, 0.0),
    ("160x96_1mb_hits", 15360, 2, 3, {"budget_mb": 1}, 7234, 0.0),
    ("160x96_1mb_no_hits", 15360, 2, 3, {"budget_mb": 1}, 0, 0.0),
    ("160x96_1mb_from_slots", 15360, 2, 3, {"budget_mb": 1, "chunksFromSlots": 1}, 7234, 0.0),
    ("160x96_1mb_bin_gi", 15360, 2, 3, {"budget_mb": 1, "binGi": 1}, None, 0.0),
    ("160x96_1mb_bin_gi_hits", 15360, 2, 3, {"budget_mb": 1, "binGi": 1}, 7234, 0.0),
    ("spp3_q2_cap_64", 4096, 3, 3, {"q2_cap": 64}, None, 0.0),
    ("spp3_q2_cap_clamped", 4096, 3, 3, {"q2_cap": 10**9}, None, 0.0),
    ("batch8_default", BATCH8, 4, 4, {}, None, 0.0),
    ("batch8_default_7.4m", BATCH8, 4, 4, {}, 7_400_000, 0.0),
    ("batch8_6144mb", BATCH8, 4, 4, {"budget_mb": 6144}, None, 0.0),
    ("batch8_6144mb_1_hit", BATCH8, 4, 4, {"budget_mb": 6144}, 1, 0.0),
    ("batch8_6144mb_7.4m", BATCH8, 4, 4, {"budget_mb": 6144}, 7_400_000, 0.0),
    ("batch8_6144mb_20m", BATCH8, 4, 4, {"budget_mb": 6144}, 20_000_000, 0.0),
    ("below_comfort", BELOW, 4, 4, {}, BELOW // 2, 0.01),
    ("above_comfort", ABOVE, 4, 4, {}, ABOVE // 2, 0.01),
    ("q2_share_0", BATCH8, 4, 4, {}, 7_400_000, 0.0),
    ("q2_share_0.01", BATCH8, 4, 4, {}, 7_400_000, 0.01),
    ("q2_share_0.05", BATCH8, 4, 4, {}, 7_400_000, 0.05),
    ("q2_share_floor", BATCH8, 4, 4, {}, 7_400_000, 1e-9),
    ("q2_predict_off", BATCH8, 4, 4, {"q2Predict": 0}, 7_400_000, 0.01),
    ("q2_share_cap", BATCH8, 4, 4, {"q2_cap": 64}, 7_400_000, 0.01),
    ("q2_share_0.01_6144mb_20m", BATCH8, 4, 4, {"budget_mb": 6144}, 20_000_000, 0.01),
]
REF_NAMES = {"budget_mb": "budget_bytes", "binGi": "bin_gi", "chunksFromSlots": "chunks_from_slots", "q2Predict": "q2_predict", "q2_cap": "q2_cap"}


def _ref(slots, spp, ao, options, hits, share):
    kw = {REF_NAMES[k]: v for k, v in options.items()}
    if "budget_bytes" in kw:
        kw["budget_bytes"] <<= 20
    return ref.plan(slots, spp, ao, hits=hits, share=share, **{k: (bool(v) if k != "budget_bytes" and k != "q2_cap" else v) for k, v in kw.items()})


def _plan(slots, spp, ao, options, hits, share):
    return rt.wave_plan(slots, spp, ao, hits=hits, share=share, **(options or {"probeMode": -1}))   # (an explicit default: never the environment)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_equals_the_parents_arithmetic(case):
    _, slots, spp, ao, options, hits, share = case
    want, got = _ref(slots, spp, ao, options, hits, share), _plan(slots, spp, ao, options, hits, share)
    assert not want["tooLarge"]
    for name in ("S1", "S2", "L1", "perHit", "chBudget", "deferred", "nChunks", "ch", "room", "q2Entries"):
        assert getattr(got, name) == want[name], name
    assert (got.slots, got.spp, got.ao) == (slots, spp, ao)
    assert got.frame.bytes == got.frame.allocBytes == want["frameBytes"]
    assert (got.rays.bytes, got.rays.allocBytes) == (want["raysBytes"], want["raysAllocBytes"])
    assert (got.results.bytes, got.results.allocBytes) == (want["resultsBytes"], want["resultsAllocBytes"])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_arrays_in_order_aligned_disjoint_and_inside(case):
    _, slots, spp, ao, options, hits, share = case
    got = _plan(slots, spp, ao, options, hits, share)
    bin_gi = bool(options.get("binGi"))
    for arena, order, align in ((got.frame, ref.FRAME_ORDER, 16), (got.rays, ref.RAYS_ORDER, 256),
                                (got.results, ref.RESULTS_ORDER_BIN_GI if bin_gi else ref.RESULTS_ORDER, 256)):
        handed = [a for a in arena.arrays if a[1] is not None]
        assert tuple(a[0] for a in handed) == order
        end = 0
        for name, offset, nbytes in handed:
            assert offset % align == 0 and offset >= end, (name, offset, end)     # aligned, behind its predecessor: no overlap
            end = offset + nbytes
        reserved = sum(a[2] for a in arena.arrays if a[1] is None)
        assert end + reserved <= arena.bytes <= arena.allocBytes, (end, reserved, arena.bytes)
    assert [a[0] for a in got.results.arrays if a[1] is None] == ([] if bin_gi else ["giPerm"])     # giPerm: always reserved, handed out under RT_BIN_GI


def test_what_the_cases_are_there_for():
    """The cases reach the paths they were chosen for (so that a change of a default cannot quietly empty them)."""
    by = {c[0]: _plan(*c[1:]) for c in CASES}
    assert by["one_tile_no_ao"].perHit == 12 * 36 + 16 + 16 + 6 + 12 + 6     # 6 + 6 light rays, one bounce ray, ONE origin group (no aoOrg), results
    assert by["160x96_1mb"].chBudget == 4096 and by["160x96_1mb"].nChunks == 4           # the 4096-hit minimum chunk: four chunks at most
    assert by["160x96_1mb_hits"].nChunks == 2 and by["160x96_1mb_hits"].ch == 3840       # 7234 hits in two equal chunks, a multiple of 256
    assert by["160x96_1mb_no_hits"].nChunks == 0
    assert by["160x96_1mb_from_slots"].nChunks == 4
    assert by["spp3_q2_cap_64"].q2Entries == 64 and by["spp3_q2_cap_clamped"].q2Entries == 4096 * 3
    assert by["batch8_default"].deferred and by["batch8_6144mb"].deferred
    assert not by["below_comfort"].deferred and by["above_comfort"].deferred and ABOVE - BELOW == 256
    one, mid, big = by["batch8_6144mb_1_hit"], by["batch8_6144mb_7.4m"], by["batch8_6144mb_20m"]
    assert (one.nChunks, one.ch, one.room) == (1, 256, 512)
    assert mid.nChunks > 1 and big.nChunks > mid.nChunks
    for p, hits in ((mid, 7_400_000), (big, 20_000_000)):
        assert p.ch % 256 == 0 and p.nChunks * p.ch >= hits > (p.nChunks - 1) * p.ch and p.ch <= p.chBudget == p.room
    single = by["batch8_default_7.4m"]
    assert single.nChunks == 1 and single.room == min(single.chBudget, (single.ch + single.ch // 16 + 255) // 256 * 256)
    worst = single.ch * 4
    assert by["q2_share_0"].q2Entries == worst == by["q2_predict_off"].q2Entries
    assert by["q2_share_0.01"].q2Entries == (max(int(2.0 * 0.01 * worst) + 65536, worst // 32) + 63) // 64 * 64
    assert by["q2_share_0.05"].q2Entries == (int(2.0 * 0.05 * worst) + 65536 + 63) // 64 * 64 > worst // 32 + 64      # the prediction decides
    assert by["q2_share_floor"].q2Entries == (worst // 32 + 63) // 64 * 64 > 65536 + 64
    assert by["q2_share_cap"].q2Entries == 64


def test_a_chunk_of_2_to_the_31_entries_is_refused_with_the_parents_message():
    slots, spp, ao, budget_mb = 256 * 400_000, 4, 4, 1 << 20
    assert ref.plan(slots, spp, ao, budget_bytes=budget_mb << 20)["tooLarge"]
    with pytest.raises(rt.RtError) as e:
        rt.wave_plan(slots, spp, ao, budget_mb=budget_mb)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED and ref.TOO_LARGE_MESSAGE in str(e.value)
    below = (1 << 31) // 24 // 256 * 256          # S2 = 24 entries per hit: the largest chunk that is accepted
    assert not ref.plan(below, spp, ao, budget_bytes=budget_mb << 20)["tooLarge"]
    assert rt.wave_plan(below, spp, ao, budget_mb=budget_mb).chBudget == below


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_totals_equal_what_the_parent_allocated(name):
    """tests/golden/wave_plan_parent.json: rt_get_memory_info of the commit before the planner, one lane, one frame."""
    rec = GOLDEN[name]
    case = next(c for c in wave_plan_cases.GPU_CASES if c[0] == name)
    assert (rec["slots"], rec["spp"], rec["ao"], rec["env"]) == (case[1] * case[2], case[3], case[4], case[5])
    options = wave_plan_cases.options_of(rec["env"])
    for hits in (None, rec["hitPixels"]):
        p = _plan(rec["slots"], rec["spp"], rec["ao"], options, hits, 0.0)
        assert p.rays.allocBytes * rec["queueArenas"] == rec["queueArenaBytes"]
        assert p.frame.bytes + p.results.allocBytes == rec["frameArrayBytes"]
    assert -(-rec["hitPixels"] // p.chBudget) == rec["bounceLaunches"] == p.nChunks


# variable -> (value, the same as keywords of rt.wave_plan)
ENV = {
    "RT_QUEUE_BUDGET_MB": ("1", {"budget_mb": 1}),
    "RT_BIN_GI": ("1", {"binGi": 1}),
    "RT_PACKET_AO": ("1", {"packetAO": 1}),
    "RT_BOUNCE_PROBE": ("0", {"probeMode": 0}),
    "RT_CHUNKS_FROM_SLOTS": ("1", {"chunksFromSlots": 1}),
    "RT_CU_SPLIT": ("9", {"cuSplit": 7}),
    "RT_SHADE_PRIORITY": ("-1", {"shadePrioritySet": 1, "shadePriority": -1}),
    "RT_DEBUG_SKIP_TRAVERSAL": ("1", {"skipTraversalSet": 1, "skipTraversal": 1}),
    "RT_Q2_PREDICT": ("0", {"q2Predict": 0}),
    "RT_Q2_CAP": ("64", {"q2_cap": 64}),
    "RT_GRID_PCT": ("60", {"gridPct": 60}),
    "RT_GRID_PCT_PRIMARY": ("0", {"gridPctPrimary": 1}),
    "RT_CHUNK_PRIMARY": ("128", {"chunkPrimarySet": 1, "chunkPrimary": 128}),
    "RT_TRACE_STATS": ("2", {"traceStatsSet": 1, "traceStats": 2}),
    "RT_TRACE_TIMING": ("1", {"traceTimingSet": 1, "traceTiming": 1}),
}


def test_every_option_variable_is_covered():
    assert set(ENV) == set(wave_plan_cases.OPTION_VARS)


@pytest.mark.parametrize("var", [None, "RT_BOUNCE_PROBE=auto"] + sorted(ENV))
def test_options_come_from_the_environment_when_none_are_given(monkeypatch, var):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    if var is None:
        keywords = {"probeMode": -1}                  # the defaults
    elif "=" in var:
        monkeypatch.setenv(*var.split("="))
        keywords = {"probeMode": -1}
    else:
        monkeypatch.setenv(var, ENV[var][0])
        keywords = ENV[var][1]
    args = dict(hits=7234, share=0.01)
    from_env, explicit = rt.wave_plan(15360, 2, 3, **args), rt.wave_plan(15360, 2, 3, **args, **keywords)
    assert from_env == explicit
    defaults = rt.wave_plan(15360, 2, 3, **args, probeMode=-1)
    assert (from_env.options != defaults.options) == (var in ENV), "the variable is read"
    assert defaults.options["budgetBytes"] == 16 << 30 and defaults.options["q2Predict"] == 1
