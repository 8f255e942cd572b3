"""The ray-queue planner against the device: after one frame of each case of tests/wave_plan_cases.py on one lane, rt_get_memory_info equals
rt.wave_plan's totals and tests/golden/wave_plan_parent.json (what the commit before the planner allocated), and a frame cut into chunks launches the
chunk loop as often as the plan says."""
import json
from pathlib import Path

import pytest

import opengl_raytracing_amd as rt
import wave_plan_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).parent / "golden" / "wave_plan_parent.json").read_text())


@pytest.mark.parametrize("case", cases.GPU_CASES, ids=[c[0] for c in cases.GPU_CASES])
def test_memory_info_equals_the_plan_and_the_parents_record(monkeypatch, case):
    for v in cases.OPTION_VARS:
        monkeypatch.delenv(v, raising=False)
    name, W, H, spp, ao, env = case
    got, rec = cases.render_one_frame(case, monkeypatch.setenv), GOLDEN[name]
    plan = rt.wave_plan(W * H, spp, ao, hits=got["hitPixels"])      # the options from the environment, as the lane read them
    assert plan.options["budgetBytes"] == int(env.get("RT_QUEUE_BUDGET_MB", 16 << 10)) << 20 and plan.options["binGi"] == int(env.get("RT_BIN_GI", 0))
    assert got["queueArenas"] == 1 and got["queueArenaBytes"] == plan.rays.allocBytes
    assert got["frameArrayBytes"] == plan.frame.bytes + plan.results.allocBytes
    for k in ("queueArenaBytes", "queueArenas", "frameArrayBytes", "hitPixels"):
        assert got[k] == rec[k], k
    # the chunk loop: one bounce launch (probed or closest-hit) per chunk that holds hits
    assert got["bounceLaunches"] == plan.nChunks == -(-got["hitPixels"] // plan.chBudget) == rec["bounceLaunches"]
    if "RT_QUEUE_BUDGET_MB" in env:
        assert plan.nChunks > 1
