"""Records tests/golden/oracle_undressed_64x48.npz: the two undressed frames of tests/test_oracle_dressed.py::undressed_frames -- a BVH frame over a
history and a hybrid frame of the flat floor-and-ceiling mesh, all four targets and the counters -- as orc_render gives them.

Recorded with the oracle library of the commit BEFORE the dressed mode (oracle/orc_dress.h) existed: build that commit's oracle/ sources with
oracle/Makefile's flags and pass the library:

    python tests/golden/make_oracle_undressed_golden.py path/to/liborc_of_the_parent.so [out.npz]

tests/test_oracle_dressed.py::test_off_is_off then holds orc_render without a dress, and with a dress of null pointers, to these bits.  Needs no GPU."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle as orc   # noqa: E402
import test_oracle_dressed as cases   # noqa: E402


def main():
    L = orc.load(sys.argv[1])
    out = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "tests" / "golden" / "oracle_undressed_64x48.npz"
    frames = cases.undressed_frames(lambda u, n, t, e, p: orc.render(u, n, t, e, p, L=L))
    np.savez_compressed(out, **frames)
    print(out, {k: v.shape for k, v in frames.items()})


if __name__ == "__main__":
    main()
