"""Records tests/golden/api_parent.json: what every call of tests/api_cases.py returns in every state it belongs to -- the return code, the text of
rt_last_error, what the calls leave in their outputs -- and the sums of the four lane-summed getters after api_cases.lane_sums()'s fixed render.

Run on a GPU against a build of the commit BEFORE the one that splits csrc/rt_api.hip (it uses the exported entry points and the Renderer methods
of that commit only), from the root of that commit's tree with this file and tests/api_cases.py copied into it:

    python tests/golden/make_api_golden.py [out.json]

tests/test_gpu_api_contract.py then holds the library to the record."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import opengl_raytracing_amd as rt   # noqa: E402
import api_cases as cases            # noqa: E402


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "api_parent.json"
    refusals = {state: cases.run(state) for state in cases.STATES}
    for state, calls in refusals.items():
        for name, got in calls.items():
            assert name in cases.QUIET or got["rc"] != rt.RT_OK, f"{state}: {name} was not refused"
            assert got["untouched"] and got.get("out7_untouched", True), f"{state}: {name} wrote to an output"
    sums = cases.lane_sums()
    assert sums == cases.lane_sums(), "the lane sums of the fixed render do not repeat"
    assert sums["rt_get_traced_rays"]["frames"] == 3 and sums["rt_get_traced_rays"]["primary"] > 0, sums
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"refusals": refusals, "lane_sums": sums}, indent=1, sort_keys=True) + "\n")
    print(f"{sum(len(c) for c in refusals.values())} records in {len(refusals)} states, {sum(len(s) for s in sums.values())} sums -> {out}")


if __name__ == "__main__":
    main()
