"""Records tests/golden/mesh_api_parent.json: what every call of tests/mesh_api_cases.py returns in every state it belongs to -- the return code, the
text of rt_last_error, what the accessors leave in their outputs.

Run on a GPU against a build of the commit BEFORE the one that reorganises the dynamic-mesh API (it uses the exported rt_mesh_* entry points and the
Renderer methods of that commit only), from the root of that commit's tree with this file and tests/mesh_api_cases.py copied into it.  The record
was made before the API moved to csrc/rt_api_mesh.hip, and again -- the UV and texture cases added, every earlier entry unchanged -- before colours
and UVs became one corner-attribute path:

    python tests/golden/make_mesh_api_golden.py [out.json]

tests/test_gpu_mesh_api_contract.py then holds the library to the record."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import opengl_raytracing_amd as rt   # noqa: E402
import mesh_api_cases as cases       # noqa: E402


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "mesh_api_parent.json"
    record = {state: cases.run(state) for state in cases.STATES}
    for state, calls in record.items():
        for name, got in calls.items():
            quiet = name.endswith("/n_zero") or name in cases.QUIET
            assert quiet or got["rc"] != rt.RT_OK, f"{state}: {name} was not refused"
            assert got.get("untouched", True), f"{state}: {name} wrote to an output"
    if out.exists():                                                # what an earlier parent recorded stays as it was recorded: a later one only adds
        for state, calls in json.loads(out.read_text()).items():
            record.setdefault(state, {}).update(calls)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=1, sort_keys=True) + "\n")
    print(f"{sum(len(c) for c in record.values())} records in {len(record)} states -> {out}")


if __name__ == "__main__":
    main()
