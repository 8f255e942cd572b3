"""bench.py --dump-outputs, the writer alone (CPU-only, synthetic targets): half bit patterns become exact float32 arrays; a frame whose
targets exceed the budget is written as the same fixed, seeded pixel sample of every target, with the pixel indices beside it."""
import numpy as np

import bench

NAMES = ("color", "motion", "gpos", "gnrm")


def _targets(h, w, seed):
    rng = np.random.default_rng(seed)
    halfs = [rng.uniform(-4, 4, size=(h, w, ch)).astype(np.float16) for ch in (4, 2, 4, 4)]
    return [a.view(np.uint16) for a in halfs], halfs


def test_small_frame_is_written_whole(tmp_path):
    bits, halfs = _targets(36, 64, 1)
    bench.dump_outputs(tmp_path, bits, NAMES)
    for name, want in zip(NAMES, halfs):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got, want.astype(np.float32))
    assert not (tmp_path / "pixel_index.npy").exists()


def test_1080p_frame_is_a_fixed_sample_under_64_mb(tmp_path):
    h, w = 1080, 1920
    bits, halfs = _targets(h, w, 2)
    bench.dump_outputs(tmp_path / "a", bits, NAMES)
    bench.dump_outputs(tmp_path / "b", bits, NAMES)
    files = sorted((tmp_path / "a").glob("*.npy"))
    assert sum(f.stat().st_size for f in files) < 64 * 10**6
    idx = np.load(tmp_path / "a" / "pixel_index.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(tmp_path / "b" / "pixel_index.npy"))
    k = idx.shape[0]
    assert k > (h * w) // 3 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < h * w
    flat = idx.astype(np.int64)
    for name, want in zip(NAMES, halfs):
        got = np.load(tmp_path / "a" / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == (k, want.shape[2])
        assert np.array_equal(got, want.reshape(h * w, -1)[flat].astype(np.float32)), name
