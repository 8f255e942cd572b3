"""The morph-target host code (csrc/rt_morph_pack.cpp: the checks, the packer and rt_morph_positions) compiled on its own with AddressSanitizer +
UndefinedBehaviorSanitizer into a stand-alone program (tests/morph_sanitize.cpp) that drives it over its edge cases -- vertex counts at the slice
edges, empty targets, repeated vertices, targets that must be refused, the 2^31 refusal -- and checks the packed form against the definition.  It
also shows that rt_morph_pack.cpp links without any other object of the library."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_morph_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "morph_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "morph_sanitize.cpp"), str(ROOT / "opengl-raytracing_amd" / "csrc" / "rt_morph_pack.cpp"),
           "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "morph host: all checks passed" in r.stdout
