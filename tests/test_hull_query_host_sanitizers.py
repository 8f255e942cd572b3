"""The hull query's definition (csrc/rt_overlap_query.cpp: rt_hull_overlaps) and the corner makers (csrc/rt_hull_corners.cpp: rt_box_corners,
rt_rect_frusta) compiled on their own with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program (tests/hull_query_sanitize.cpp) that
drives them over a single leaf, the 36-triangle layer stack and a leaf with zero-area rows -- query strides 24, 25 and 32, the counts alone, the exact
list in two passes, capacities 0, 1, 3 and 8, counts NULL and non-NULL, NaN, infinite, huge and collapsed hulls, hulls at a row's own points, slots of
negative length, nodes that are no tree, strided boxes and rects, every refusal -- on arrays exactly as long as the call may read or write.  It also
shows that the two files link without any other object of the library."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_hull_definition_and_corner_makers_are_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "hull_query_sanitize"
    csrc = ROOT / "opengl-raytracing_amd" / "csrc"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "hull_query_sanitize.cpp"), str(csrc / "rt_overlap_query.cpp"), str(csrc / "rt_hull_corners.cpp"),
           "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "hull query host: all checks passed" in r.stdout
