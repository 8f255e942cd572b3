"""The box query's definition (csrc/rt_overlap_query.cpp: rt_box_overlaps) compiled on its own with AddressSanitizer + UndefinedBehaviorSanitizer into a
stand-alone program (tests/box_query_sanitize.cpp) that drives it over a single leaf, the 36-triangle layer stack and a leaf with zero-area rows --
box strides 6, 7 and 12, the counts alone, the exact list in two passes, capacities 0, 1, 3 and 8, counts NULL and non-NULL, NaN, infinite, huge and
inverted boxes, slots of negative length, nodes that are no tree, every refusal -- on arrays exactly as long as the call may read or write.  It also
shows that rt_overlap_query.cpp links without any other object of the library."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_box_definition_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "box_query_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "box_query_sanitize.cpp"),
           str(ROOT / "opengl-raytracing_amd" / "csrc" / "rt_overlap_query.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "box query host: all checks passed" in r.stdout
