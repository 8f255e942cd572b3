"""Records tests/golden/wave_plan_parent.json: what the ray-queue arenas and the per-lane frame arrays came to (rt_get_memory_info: queueArenaBytes,
queueArenas, frameArrayBytes) after one frame of each case of tests/wave_plan_cases.py on one lane, with the frame's hit pixels and bounce launches.

Run on a GPU against a build of the commit BEFORE the planner (csrc/rt_wave_plan.cpp) existed -- it uses render_frame, memory_info, traced_rays and
bounce_probe only, which that commit has -- from the root of that commit's tree with this file and tests/wave_plan_cases.py copied into it:

    python tests/golden/make_wave_plan_golden.py [out.json]

tests/test_wave_plan_host.py then holds rt.wave_plan's totals to the record without a GPU, tests/test_gpu_wave_plan.py holds the device to both."""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import wave_plan_cases as cases   # noqa: E402


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "wave_plan_parent.json"
    record = {}
    for case in cases.GPU_CASES:
        for v in cases.OPTION_VARS + ("RT_LANES",):
            os.environ.pop(v, None)
        name, W, H, spp, ao, env = case
        record[name] = dict(cases.render_one_frame(case, os.environ.__setitem__), slots=W * H, spp=spp, ao=ao, env=env)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=1, sort_keys=True) + "\n")
    print(f"{len(record)} records -> {out}")


if __name__ == "__main__":
    main()
