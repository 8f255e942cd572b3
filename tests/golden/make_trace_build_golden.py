"""Records tests/golden/trace_build_parent.json: what launch_trace of commit 8c53523 -- the last one that chose the k_trace build inside the HIP header --
chose for every case of tests/trace_build_cases.py: the RT_BUILD_* bits of the build, the arrays it handed the kernel, the stack entries and the LDS bytes.

Needs a checkout of that commit and hipcc, no GPU:

    python tests/golden/make_trace_build_golden.py PARENT_TREE [out.json]

A probe is compiled from PARENT_TREE's own csrc/rt_wave.hip and csrc/rt_trace.hpp, host side only, in a temporary copy: in launch_trace's `go` the
persistent_grid / hipLaunchKernelGGL lines give way to a printf of `built`, nodes, pairRecords, leafBoxes, stack and ldsBytes, and a main() is appended that
fills a DevScene with one distinct fake address per array, reads tune_from_env() and calls launch_trace_kind.  Nothing touches a device.  The probe runs
once per case under that case's environment; its tune goes into the record too.
tests/test_trace_build_host.py holds rt.trace_build to the record."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_options as gpu_options   # noqa: E402
import trace_build_cases                  # noqa: E402

GO_OLD = """        const auto kernel = decltype(k)::fn;
        built = decltype(k)::bits;
        unsigned blocks = persistent_grid(kernel, ldsBytes, t.cus, t.gridPct);
        if (t.maxBlocks) blocks = std::min(blocks, t.maxBlocks);   // (ray queries: no more waves than the rays can occupy)
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), ldsBytes, t.st, t.fr, nodes, pairRecords, src, t.head, t.tally, t.gatherLoads, tune, stack, stats, leafBoxes);
"""
GO_NEW = """        built = decltype(k)::bits;
        printf("built %u nodes %ld pairs %ld leafBoxes %ld stack %d lds %zu\\n", built, (long)nodes, (long)pairRecords, (long)leafBoxes, stack, ldsBytes);
"""
ADDRESS = {"wnodesW": 0x10, "wF": 0x20, "iN2": 0x30, "w4": 0x40, "q4": 0x50, "iN4": 0x60, "iQ4": 0x70, "pairs": 0x100, "iPairs": 0x110, "leafBox": 0x200,
           "iLeafBox": 0x210}
MAIN = """
int main(int argc, char **argv) {   // any stats depth anyStack q4 wF iN2 iN4 iQ4
    if (argc < 10) return 2;
    DevScene sc{};
    sc.anyStack = atoi(argv[4]);
    sc.wnodesW = (const float4 *)%(wnodesW)d; sc.w4 = (const float4 *)%(w4)d; sc.pairs = (const float4 *)%(pairs)d; sc.leafBox = (const float4 *)%(leafBox)d;
    sc.iPairs = (const float4 *)%(iPairs)d; sc.iLeafBox = (const float4 *)%(iLeafBox)d;
    if (atoi(argv[5])) sc.q4 = (const float4 *)%(q4)d;
    if (atoi(argv[6])) sc.wF = (const float4 *)%(wF)d;
    if (atoi(argv[7])) sc.iN2 = (const float4 *)%(iN2)d;
    if (atoi(argv[8])) sc.iN4 = (const float4 *)%(iN4)d;
    if (atoi(argv[9])) sc.iQ4 = (const float4 *)%(iQ4)d;
    const TraceTune tn = tune_from_env();
    printf("tune timing %%d coop %%d nearFirst %%d qnodes %%d fused %%d impl %%d leafb %%d leafbClosest %%d\\n", tn.timing, tn.coop, tn.nearFirst, tn.qnodes, tn.fused,
           tn.impl, tn.leafb, tn.leafbClosest);
    TraceLaunch t{nullptr, 256, 100, atoi(argv[3]), nullptr, sc, nullptr, tn};
    if (atoi(argv[2])) t.stats = (unsigned long long *)8;
    QueueSrc q{};
    launch_trace_kind(atoi(argv[1]) != 0, t, q);
    return 0;
}
""" % ADDRESS


def build_probe(parent: Path, work: Path) -> Path:
    shutil.copytree(parent / "opengl-raytracing_amd" / "csrc", work / "opengl-raytracing_amd" / "csrc")
    shutil.copytree(parent / "include", work / "include")
    csrc = work / "opengl-raytracing_amd" / "csrc"
    hpp = (csrc / "rt_trace.hpp").read_text()
    assert hpp.count(GO_OLD) == 1, "PARENT_TREE is not a checkout of 8c53523: launch_trace's `go` reads differently"
    (csrc / "rt_trace.hpp").write_text(hpp.replace(GO_OLD, GO_NEW))
    with open(csrc / "rt_wave.hip", "a") as f:
        f.write(MAIN)
    hipcc = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "bin" / "hipcc"
    # host side only; the unit's references into the other units are never called
    subprocess.run([str(hipcc), "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function", str(csrc / "rt_wave.hip"), "-o",
                    str(work / "probe"), "-Wl,--unresolved-symbols=ignore-all"], check=True)
    return work / "probe"


def main():
    parent = Path(sys.argv[1])
    out = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "tests" / "golden" / "trace_build_parent.json"
    names = {v: k for k, v in ADDRESS.items()}
    record = {}
    with tempfile.TemporaryDirectory() as td:
        probe = build_probe(parent, Path(td))
        for name, env, any_, stats, depth, any_stack, forms, _ in trace_build_cases.cases():
            e = {k: v for k, v in os.environ.items() if k not in gpu_options.OPTION_VARS}
            e.update(env)
            args = [int(any_), int(stats), depth, any_stack] + [int(f in forms) for f in ("q4", "wF", "iN2", "iN4", "iQ4")]
            lines = subprocess.run([str(probe)] + [str(a) for a in args], env=e, check=True, capture_output=True, text=True).stdout.splitlines()
            tune, built = lines[0].split(), lines[1].split()
            assert tune[0] == "tune" and built[0] == "built" and len(lines) == 2, lines
            b = dict(zip(built[0::2], (int(v) for v in built[1::2])))
            bits = b["built"] >> (16 if any_ else 0)
            assert bits & 1 and bits < (1 << 16), b            # RT_BUILD_LAUNCHED, on this hit kind's half
            record[name] = dict(env=env, any=bool(any_), stats=bool(stats), depth=depth, anyStack=any_stack, forms=list(forms),
                                tune=dict(zip(tune[1::2], (int(v) for v in tune[2::2]))),
                                expect=dict(opt=bits & ~1, nodes=names[b["nodes"]], implPairs=names[b["pairs"]] == "iPairs",
                                            implLeafBoxes=names[b["leafBoxes"]] == "iLeafBox", stack=b["stack"], ldsBytes=b["lds"]))
    out.write_text(json.dumps(record, indent=1, sort_keys=True) + "\n")
    print(f"{len(record)} records -> {out}")


if __name__ == "__main__":
    main()
