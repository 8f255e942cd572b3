#!/usr/bin/env python3
"""Machine-code diff of the gfx950 kernels of two builds of librt_mi355.so.

    python tools/isa_diff.py OLD.so NEW.so        # two libraries
    python tools/isa_diff.py --rev HEAD~1         # build REV in a temporary worktree, compare with the in-tree library

Every function symbol of the OLD library's gfx950 code objects is disassembled (llvm-objdump -d) in both libraries and compared instruction
by instruction, encodings included; only the absolute addresses llvm-objdump prints in its comments and the "..." it prints for zero
padding behind a section's last function are dropped (a kernel that merely moved inside its code object is the same code).  A symbol
that disappeared is paired with a symbol of the same code object that only the NEW library has when their instruction streams are
identical apart from the symbol's own name in branch-target comments, one to one, and reported as renamed (a template's arguments changed, its code did not).
A symbol that left its code object and appears in another one under the same name with identical instructions is reported as moved (its
translation unit changed, its code did not).  Symbols only the NEW library has and
that no such pair accounts for are listed as added.  Exit status 0 when no existing symbol changed or disappeared without an identical
partner, 1 otherwise.  The code objects are read straight from the .hip_fatbin section (clang offload bundles, one per translation unit), so nothing beyond the ROCm LLVM tools
is needed.
"""
import argparse
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
LLVM = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "gfx950"


def fatbin(lib: Path) -> bytes:
    with tempfile.TemporaryDirectory() as td:
        out = Path(td) / "fatbin"
        subprocess.run([str(LLVM / "llvm-objcopy"), "--dump-section", f".hip_fatbin={out}", str(lib), str(Path(td) / "ignored")], check=True,
                       capture_output=True)
        return out.read_bytes()


def code_objects(lib: Path):
    """The gfx950 code objects of lib, in bundle order (one per translation unit with device code)."""
    data, cos, pos = fatbin(lib), [], 0
    while True:
        pos = data.find(MAGIC, pos)
        if pos < 0:
            return cos
        (n,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", data, p)
            ident = data[p + 24:p + 24 + idlen].decode()
            p += 24 + idlen
            if ident.endswith(TARGET) or ident.endswith(TARGET + ":xnack-") or (TARGET + ":") in ident:
                cos.append(data[pos + off:pos + off + size])
        pos += len(MAGIC)


ADDR = re.compile(r"//\s*[0-9A-Fa-f]+:\s*")


def disassemble(co: bytes):
    """{symbol: [instruction lines without addresses]} of one code object."""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co)
        f.flush()
        txt = subprocess.run([str(LLVM / "llvm-objdump"), "-d", f.name], check=True, capture_output=True, text=True).stdout
    syms, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-fA-F]+ <(.+)>:$", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
            continue
        if cur is not None and line.strip() and line.strip() != "...":   # "...": zero padding after the last function of a section
            cur.append(ADDR.sub("// ", line.strip()))
    return syms


def library_symbols(lib: Path):
    out = {}
    for i, co in enumerate(code_objects(lib)):
        for name, body in disassemble(co).items():
            out[(i, name)] = body
    return out


def build_rev(rev: str, work: Path) -> Path:
    subprocess.run(["git", "-C", str(ROOT), "worktree", "add", "--detach", str(work), rev], check=True, capture_output=True)
    subprocess.run(["make", "-C", str(work / "opengl-raytracing_amd"), "-j", str(min(16, os.cpu_count() or 2)), "ARCH=gfx950", "librt_mi355.so"],
                   check=True, capture_output=True)
    return work / "opengl-raytracing_amd" / "librt_mi355.so"


def pair_renamed(before, after, gone, added):
    """(gone, added, renamed) with every removed symbol that has an added symbol of identical code in its code object taken out of both lists, one to one."""
    def stream(k, body):   # (llvm-objdump names a branch's target <symbol+offset> in its comment: the symbol's own name is not part of its code)
        return k[0], tuple(line.replace(f"<{k[1]}+", "<.+").replace(f"<{k[1]}>", "<.>") for line in body)

    pool = {}
    for k in added:
        pool.setdefault(stream(k, after[k]), []).append(k)
    renamed, left = [], []
    for k in gone:
        partners = pool.get(stream(k, before[k]))
        if partners:
            renamed.append((k, partners.pop(0)))
        else:
            left.append(k)
    taken = {k2 for _, k2 in renamed}
    return left, [k for k in added if k not in taken], renamed


def pair_moved(before, after, gone, added):
    """(gone, added, moved) with every removed symbol that another code object now holds under the same name and with identical instructions taken
    out of both lists, one to one: its translation unit changed, its code did not."""
    pool = {}
    for k in added:
        pool.setdefault((k[1], tuple(after[k])), []).append(k)
    moved, left = [], []
    for k in gone:
        partners = pool.get((k[1], tuple(before[k])))
        if partners:
            moved.append((k, partners.pop(0)))
        else:
            left.append(k)
    taken = {k2 for _, k2 in moved}
    return left, [k for k in added if k not in taken], moved


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old", nargs="?")
    ap.add_argument("new", nargs="?", default=str(ROOT / "opengl-raytracing_amd" / "librt_mi355.so"))
    ap.add_argument("--rev", help="build this git revision as OLD (temporary worktree)")
    a = ap.parse_args()
    tmp = None
    try:
        if a.rev:
            tmp = Path(tempfile.mkdtemp(prefix="isa_diff_"))
            old = build_rev(a.rev, tmp / "tree")
        elif a.old:
            old = Path(a.old)
        else:
            ap.error("give OLD.so or --rev REV")
        before, after = library_symbols(old), library_symbols(Path(a.new))
        changed = [k for k in before if k in after and before[k] != after[k]]
        gone = [k for k in before if k not in after]
        added = [k for k in after if k not in before]
        same = len(before) - len(changed) - len(gone)
        gone, added, renamed = pair_renamed(before, after, gone, added)
        gone, added, moved = pair_moved(before, after, gone, added)
        print(f"old: {old}\nnew: {a.new}")
        print(f"symbols before: {len(before)} in {len({k[0] for k in before})} code objects; identical: {same}; renamed: {len(renamed)}; "
              f"moved: {len(moved)}; changed: {len(changed)}; removed: {len(gone)}; added: {len(added)}")
        for k, k2 in renamed:
            print(f"  renamed  [{k[0]}] {k[1]} -> {k2[1]}  ({len(before[k])} instructions)")
        for k, k2 in moved:
            print(f"  moved    [{k[0]}] -> [{k2[0]}] {k[1]}  ({len(before[k])} instructions)")
        for k in changed:
            print(f"  CHANGED  [{k[0]}] {k[1]}  ({len(before[k])} -> {len(after[k])} instructions)")
        for k in gone:
            print(f"  REMOVED  [{k[0]}] {k[1]}")
        for k in added:
            print(f"  added    [{k[0]}] {k[1]}  ({len(after[k])} instructions)")
        return 1 if (changed or gone) else 0
    finally:
        if tmp:
            subprocess.run(["git", "-C", str(ROOT), "worktree", "remove", "--force", str(tmp / "tree")], capture_output=True)
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
