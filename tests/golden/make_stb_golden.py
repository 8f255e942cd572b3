"""Generates tests/golden/stb_png/: small PNGs of every colour type / filter the product's reader accepts, and what the reference's own
decoder (oracle/_ref/libstb_ref.so, `make -C oracle ref`) makes of them and of the two cube-map crosses under assets/cubemaps/ --
shape and sha256 of the decoded bytes.  tests/test_host_parity.py compares rt_load_png with these where that library cannot be built.

    make -C oracle ref && python tests/golden/make_stb_golden.py        # rewrites the fixtures
"""
import ctypes as C
import hashlib
import json
from pathlib import Path

import numpy as np
from PIL import Image

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
OUT = HERE / "stb_png"
LIB = ROOT / "oracle" / "_ref" / "libstb_ref.so"

# the synthetic PNGs of test_png_reader_matches_the_references_own_decoder: (file, PIL mode, shape)
SYNTHETIC = (("t0.png", "RGBA", (31, 17, 4)), ("t1.png", "RGB", (64, 64, 3)), ("t2.png", "L", (5, 9)), ("t3.png", "RGB", (1, 1, 3)))


def stb_loader():
    L = C.CDLL(str(LIB))
    L.stbi_load.restype = C.POINTER(C.c_ubyte)
    L.stbi_load.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    L.stbi_image_free.argtypes = [C.c_void_p]

    def stb(path):
        w, h, n = C.c_int(), C.c_int(), C.c_int()
        p = L.stbi_load(str(path).encode(), C.byref(w), C.byref(h), C.byref(n), 0)
        assert p, path
        a = np.ctypeslib.as_array(p, shape=(h.value, w.value, n.value)).copy()
        L.stbi_image_free(p)
        return a
    return stb


def digest(a):
    return {"shape": list(a.shape), "sha256": hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()}


def main():
    OUT.mkdir(exist_ok=True)
    rng = np.random.default_rng(9)
    for i, (name, mode, shape) in enumerate(SYNTHETIC):
        a = rng.integers(0, 256, size=shape, dtype=np.uint8)
        if i == 1:
            a = np.sort(a, axis=1)                      # smooth rows: the encoder picks Sub / Up / Average / Paeth filters
        Image.fromarray(a, mode).save(OUT / name, optimize=bool(i % 2))
    stb = stb_loader()
    decoded = {name: digest(stb(ROOT / "assets" / "cubemaps" / name)) for name in ("Sky_01.png", "Sky_16.png")}
    decoded.update({name: digest(stb(OUT / name)) for name, _, _ in SYNTHETIC})
    (OUT / "decoded.json").write_text(json.dumps(decoded, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
