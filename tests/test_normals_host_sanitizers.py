"""The smooth-normal host code (csrc/rt_normal_pack.cpp: the check, the packer, rt_vertex_normals and rt_hit_normals, with the arithmetic of
csrc/rt_mesh_normals.hpp) compiled on its own with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program
(tests/normals_sanitize.cpp) that drives it over its edge cases -- vertex counts at the slice edges, a vertex named twice, a high-valence fan, hits
with NaN and infinite barycentrics and prims off the mesh, index buffers that must be refused, the 2^31 refusal -- and checks the packed form against
the definition.  It also shows that rt_normal_pack.cpp links without any other object of the library."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_normals_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "normals_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "normals_sanitize.cpp"), str(ROOT / "opengl-raytracing_amd" / "csrc" / "rt_normal_pack.cpp"),
           "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "normals host: all checks passed" in r.stdout
