"""The beam cull's host definition (csrc/rt_beam.cpp with csrc/rt_beam.hpp: rt_debug_beam_cull, rt_debug_beam_slab, rt_debug_beam_walk) compiled on its own
with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program (tests/beam_cull_sanitize.cpp) that drives it over frames that are no multiple
of the tile, one pixel wide, ranks of a world, batches of 1 and 16, a root that is a leaf, no tree, references outside the records, a frontier overflow,
intervals and bounds outside the argument and every refusal -- on arrays exactly as long as the call may read or write.  It also shows that rt_beam.cpp
links without any other object of the library."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_beam_cull_definition_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "beam_cull_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "beam_cull_sanitize.cpp"),
           str(ROOT / "opengl-raytracing_amd" / "csrc" / "rt_beam.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "beam cull host: all checks passed" in r.stdout
