"""Linear-blend skinning as include/rt_mi355.h defines it for rt_skin_positions, restated in numpy float32: the same association
per component, the same skip of +-0 weights, the first unskipped term initialising the sum, the rest position's bits where nothing is left.  Every
numpy operation on float32 arrays rounds once to float32 and nothing is fused, which is the float model of the library's host and device code."""
import numpy as np

F1 = np.float32(1.0)


def skin_ref(rest, bone_idx, weights, bones):
    """rest [V,3], bone_idx [V,4], weights [V,4], bones [nBones,16] column-major -> positions [V,3] float32"""
    p = np.ascontiguousarray(rest, np.float32).reshape(-1, 3)
    bi = np.asarray(bone_idx).reshape(-1, 4).astype(np.int64)
    w = np.ascontiguousarray(weights, np.float32).reshape(-1, 4)
    B = np.ascontiguousarray(bones, np.float32).reshape(-1, 16)
    assert bi.shape[0] == p.shape[0] == w.shape[0] and bi.min() >= 0 and bi.max() < B.shape[0] and np.isfinite(w).all()
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    acc = np.zeros_like(p)
    have = np.zeros(p.shape[0], bool)
    with np.errstate(all="ignore"):
        for k in range(4):
            M = B[bi[:, k]]
            wk = w[:, k]
            use = wk != 0                     # false for +0 and for -0
            for c in range(3):
                q = (M[:, c] * x + M[:, 4 + c] * y) + (M[:, 8 + c] * z + M[:, 12 + c] * F1)
                term = wk * q
                new = np.where(have, acc[:, c] + term, term)
                acc[:, c] = np.where(use, new, acc[:, c])
            have |= use
    out = p.copy()                            # no influence: the rest position, bit for bit
    out[have] = acc[have]
    return out
