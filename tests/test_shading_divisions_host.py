"""The shading stages' arithmetic without divisions, as the host compiles it: no GPU, no context.

(a) the cube-map texel decode (texel_unorm8, rt_device_shade.hpp) equals float32 c / 255 for all 256 codes;
(b) the multiply-high form of the three run-time divisors of the slot <-> pixel arithmetic (rt_frame.hpp: max(nLocalTiles, 1), tilesX, world) equals
    // and %, and the host stores the fallback word 0 exactly when the stated condition -- d >= 2 and nMax * d < 2^32 -- fails;
(c) the halton pairs the host writes into the frame descriptor equal the scalar function of rt_common.glsl:106-116, restated here in float32.

How (b) covers "every index up to the bound".  umulhi(n, M) is non-decreasing in n and so is n // d, which steps only at multiples of d.  If the two agree
at n = k d and at n = k d + d - 1 for every k up to the bound, every n between is squeezed between equal values: agreement at those 2 (nMax / d + 1) points
is agreement at every n <= nMax.  That is what is checked for every divisor of the ranges the issue names (tilesX 1..512, nLocalTiles 1..70 000, world
1..8) with nMax the largest dividend the kernels form (frame_geom_set_reciprocals), and every single n is checked besides for the small divisors
(nLocalTiles <= 1024 with a batch of 16, every tilesX with 135 tile rows, every world) and for the shapes of the benchmark (1080p, 4K)."""
import numpy as np
import pytest

import opengl_raytracing_amd as rt
from opengl_raytracing_amd import tiles

MAX_BATCH = 16     # RT_MAX_BATCH
ROW_SHIFT = tiles.ROW_SHIFT


def test_texel_decode_equals_the_division_for_every_code():
    got = rt.texel_unorm8()
    want = np.arange(256, dtype=np.float32) / np.float32(255)
    assert want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    # the correction step is not optional: the plain product with fl(1 / 255) differs for many codes
    plain = np.arange(256, dtype=np.float32) * (np.float32(1) / np.float32(255))
    assert (plain.view(np.uint32) != want.view(np.uint32)).sum() == 126


def _halton32(i, b):
    f, r, n = np.float32(1), np.float32(0), int(i)
    while n > 0:
        f = np.float32(f / np.float32(b))
        r = np.float32(r + np.float32(f * np.float32(n % b)))
        n //= b
    return r


def test_host_halton_table_equals_the_scalar_function():
    got = rt.halton_pairs(0, 4097)          # uFrameIndex 0 .. 4096 -> halton(index + 1, base)
    want = np.array([[_halton32(f + 1, 2), _halton32(f + 1, 3)] for f in range(4097)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0, 0] == 0.5 and got[0, 1] == np.float32(np.float32(1) / np.float32(3))
    # a table that starts in the middle (a batch deep into an accumulation) holds the same values
    assert np.array_equal(rt.halton_pairs(1000, 16), got[1000:1016])


def _expected_reciprocal(d, n_max):
    return (2**32 // d + 1) if (d >= 2 and n_max * d < 2**32) else 0


def _check_breakpoints(d, rcp, n_max):
    k = np.arange(0, n_max // d + 1, dtype=np.uint64)
    n = np.concatenate([k * d, np.minimum(k * d + (d - 1), n_max)]).astype(np.uint32)
    q, r = rt.div_by(d, rcp, n)
    assert np.array_equal(q, n // np.uint32(d)) and np.array_equal(r, n % np.uint32(d)), (d, rcp, n_max)


def _check_every(d, rcp, n_max):
    n = np.arange(0, n_max + 1, dtype=np.uint32)
    q, r = rt.div_by(d, rcp, n)
    assert np.array_equal(q, n // np.uint32(d)) and np.array_equal(r, n % np.uint32(d)), (d, rcp, n_max)


def test_local_tile_reciprocal():
    """d = max(nLocalTiles, 1), dividend = a local tile index of a batch: n <= d * batch - 1."""
    fallbacks = 0
    for d in range(1, 70_001):
        n_max = d * MAX_BATCH - 1
        rcp = rt.div_reciprocal(d, n_max)
        assert rcp == _expected_reciprocal(d, n_max), d
        fallbacks += rcp == 0
        _check_breakpoints(d, rcp, n_max)
        if d <= 1024 or d in (8160, 32400):            # every index: the small divisors; 1080p and 4K on one rank
            _check_every(d, rcp, n_max)
    # 16 d^2 < 2^32 up to d = 16 383: the divisors beyond fall back, and d = 1 has no 32-bit reciprocal
    assert rt.div_reciprocal(16_383, 16_383 * 16 - 1) != 0 and rt.div_reciprocal(16_384, 16_384 * 16 - 1) != 0 and rt.div_reciprocal(16_385, 16_385 * 16 - 1) == 0
    assert fallbacks == 1 + (70_000 - 16_384)
    # the same divisor with the batch it is really used with: 4K, batches of 4 and of 5
    assert rt.div_reciprocal(32_400, 32_400 * 4 - 1) != 0 and rt.div_reciprocal(32_400, 32_400 * 5 - 1) == 0


def test_reciprocal_is_wrong_beyond_its_condition():
    """One case beyond the bound: the word the condition refuses does give a wrong quotient there, so the fallback is needed and the bound is not slack by
    orders of magnitude.  d = 70 000, M = floor(2^32 / d) + 1: e = M d - 2^32 = 22 704, and the first wrong quotient is at the first n = k d - 1 with
    n e >= 2^32, the first k d - 1 above 189 172 -- far below the 1 119 999 a batch of 16 reaches."""
    d = 70_000
    m = 2**32 // d + 1
    e = m * d - 2**32
    assert 0 < e <= d
    n = np.arange(d - 1, 16 * d, d, dtype=np.uint32)              # k d - 1
    q, _ = rt.div_by(d, m, n)
    bad = np.flatnonzero(q != n // np.uint32(d))
    assert bad.size > 0
    first = int(n[bad[0]])
    assert first * e >= 2**32 > (first - d) * e                   # exactly where the proof says it starts
    assert rt.div_reciprocal(d, 16 * d - 1) == 0                  # ... and the host does not store that word
    q0, r0 = rt.div_by(d, 0, n)                                   # the fallback divides
    assert np.array_equal(q0, n // np.uint32(d)) and np.array_equal(r0, n % np.uint32(d))


def test_tiles_x_reciprocal():
    """d = tilesX; dividends: a global tile index t < tilesX * tilesY, and 11 ty with ty < tilesY (the row shift)."""
    for d in range(1, 513):
        for tiles_y in (1, 7, 135, 512):
            n_max = max(d * tiles_y - 1, ROW_SHIFT * (tiles_y - 1))
            rcp = rt.div_reciprocal(d, n_max)
            assert rcp == _expected_reciprocal(d, n_max) and (rcp != 0) == (d >= 2), (d, tiles_y)   # 512 * 512 * 512 < 2^32: only d = 1 falls back
            _check_breakpoints(d, rcp, n_max)
            if tiles_y == 135:
                _check_every(d, rcp, n_max)


def test_world_reciprocal():
    for d in range(1, 9):
        n_max = 512 * 512 - 1
        rcp = rt.div_reciprocal(d, n_max)
        assert rcp == _expected_reciprocal(d, n_max) and (rcp != 0) == (d >= 2)
        _check_every(d, rcp, n_max)


def test_reciprocal_condition_at_its_edge():
    """The word is stored exactly while nMax * d < 2^32."""
    for d in (2, 3, 255, 256, 4097, 65_535, 65_536, 70_000, 2**31 - 1):
        edge = (2**32 - 1) // d                   # the largest nMax with nMax * d < 2^32 ...
        if edge * d == 2**32:
            edge -= 1
        assert edge * d < 2**32 <= (edge + 1) * d
        assert rt.div_reciprocal(d, edge) == 2**32 // d + 1
        assert rt.div_reciprocal(d, edge + 1) == 0
        n = np.unique(np.clip(np.array([0, 1, d - 1, d, d + 1, edge - d, edge - 1, edge], dtype=np.int64), 0, edge)).astype(np.uint32)
        q, r = rt.div_by(d, rt.div_reciprocal(d, edge), n)
        assert np.array_equal(q, n // np.uint32(d)) and np.array_equal(r, n % np.uint32(d)), d
    assert rt.div_reciprocal(1, 0) == 0 and rt.div_reciprocal(1, 100) == 0


def _geom_words(w, h, rank, world, batch):
    g = tiles.geometry(w, h, world)
    n_local = max((g["nTiles"] - rank + world - 1) // world, 0)
    nl = max(n_local, 1)
    t_max = max(g["nTiles"] - 1, ROW_SHIFT * (g["tilesY"] - 1))
    return g, n_local, (_expected_reciprocal(nl, nl * batch - 1), _expected_reciprocal(g["tilesX"], t_max), _expected_reciprocal(world, g["nTiles"] - 1))


@pytest.mark.parametrize("w,h", [(160, 96), (200, 120), (16, 16), (17, 300), (1920, 1080)])
@pytest.mark.parametrize("world,rank", [(1, 0), (2, 1), (3, 1), (7, 6), (8, 0)])
def test_frame_geometry_and_its_slots_agree_with_the_tile_layout(w, h, world, rank):
    """The geometry rt_resize sets up carries the reciprocal words the rule gives, and pixel_of_slot -- with them and in its dividing form -- maps every
    slot of a batch to the pixel tiles.slot_map puts there."""
    batch = 1 if (w, h) == (1920, 1080) else 3
    g, n_local, words = _geom_words(w, h, rank, world, batch)
    owner, slot = tiles.slot_map(w, h, world)
    want = np.full((n_local * 256, 2), -1, np.int64)
    ys, xs = np.nonzero(owner == rank)
    want[slot[ys, xs], 0] = xs
    want[slot[ys, xs], 1] = ys
    for reciprocals in (True, False):
        info, xy = rt.frame_geom(w, h, rank, world, batch, reciprocals=reciprocals, slots=True)
        assert (info.tilesX, info.tilesY, info.nTiles, info.nLocalTiles) == (g["tilesX"], g["tilesY"], g["nTiles"], n_local)
        assert (info.rcpLocalTiles, info.rcpTilesX, info.rcpWorld) == (words if reciprocals else (0, 0, 0))
        xy = xy.reshape(batch, n_local * 256, 3)
        for k in range(batch):
            assert np.array_equal(xy[k, :, :2], want), (reciprocals, k)
            live = want[:, 0] >= 0
            assert np.all(xy[k, live, 2] == k) and np.all(xy[k, ~live, 2] == -1)


def test_frame_geometry_falls_back_for_a_large_batched_frame():
    """4K on one rank: 32 400 local tiles.  Batches of up to 4 keep the reciprocal of nLocalTiles, longer ones divide; tilesX keeps its own either way."""
    a, _ = rt.frame_geom(3840, 2160, batch=4)
    b, _ = rt.frame_geom(3840, 2160, batch=8)
    assert a.nLocalTiles == b.nLocalTiles == 32_400
    assert a.rcpLocalTiles == 2**32 // 32_400 + 1 and b.rcpLocalTiles == 0
    assert a.rcpTilesX == b.rcpTilesX == 2**32 // 240 + 1 and a.rcpWorld == b.rcpWorld == 0   # world == 1
