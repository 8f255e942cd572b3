"""Records tests/golden/scene_pack_parent.json: what rt_upload_bvh leaves on the device for every mesh and option set of tests/scene_pack_cases.py --
the sha256 of each of the seven arrays rt_debug_read_scene could read before the packers moved to csrc/rt_scene_pack.cpp, and RtSceneInfo.

Run on a GPU against a build of the commit BEFORE that move (it uses upload_bvh, debug_read_scene and scene_info only, which that commit has), from the
root of that commit's tree with this file and tests/scene_pack_cases.py copied into it:

    python tests/golden/make_scene_pack_golden.py [out.json]

tests/test_scene_pack_host.py then holds rt.pack_scene to the record without a GPU."""
import hashlib
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import opengl_raytracing_amd as rt   # noqa: E402
import scene_pack_cases as cases     # noqa: E402

ARRAYS = ("tris", "pairs", "nodes2", "nodes2w", "nodes4", "qnodes4", "leafbox")


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "scene_pack_parent.json"
    record = {}
    for oname, (env, _) in cases.OPTION_SETS.items():
        for v in cases.PACK_VARS:
            os.environ.pop(v, None)
        os.environ.update(env)
        with rt.Renderer() as r:
            for mname in cases.MESHES:
                nodes, tris = cases.mesh(mname)
                r.upload_bvh(nodes, tris)
                info = r.scene_info()
                record[f"{mname}/{oname}"] = {
                    "sha256": {a: hashlib.sha256(r.debug_read_scene(a).tobytes()).hexdigest() for a in ARRAYS},
                    "bytes": {a: int(r.debug_read_scene(a).size) for a in ARRAYS},
                    "info": {f: int(getattr(info, f)) for f in cases.INFO_FIELDS},
                }
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=1, sort_keys=True) + "\n")
    print(f"{len(record)} records -> {out}")


if __name__ == "__main__":
    main()
