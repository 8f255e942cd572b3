"""The per-vertex colour host code (csrc/rt_mesh_colors.cpp: rt_hit_colors and rt_color_rows, with the arithmetic of csrc/rt_mesh_colors.hpp) compiled
on its own with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program (tests/colors_sanitize.cpp) that drives it over its edge
cases -- vertex counts about 64, shuffled orders, hits with NaN and infinite barycentrics and prims off the mesh (-1, nTris, INT_MAX, INT_MIN), the flat
rule, arrays that must be refused -- on arrays exactly as long as the call may read.  It also shows that rt_mesh_colors.cpp links without any other
object of the library."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_colors_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "colors_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "colors_sanitize.cpp"), str(ROOT / "opengl-raytracing_amd" / "csrc" / "rt_mesh_colors.cpp"),
           "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "colors host: all checks passed" in r.stdout
