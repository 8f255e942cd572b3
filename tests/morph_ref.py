"""Morph-target blending as include/rt_mi355.h defines it for rt_morph_positions, restated in numpy float32, and the packed form of
the targets as rt_debug_morph_pack hands it out.  Every numpy operation on float32 arrays rounds once to float32 and nothing is fused, which is the
float model of the library's host and device code: the product and the sum below are two operations with two roundings."""
import numpy as np

SLICE = 64
PAD = 0xFFFFFFFF


def _by_vertex(n_verts, target_first, vert_idx):
    """The entries in the definition's order per vertex: (order, count, rank) with order a stable sort of the entries by vertex (input order is
    ascending target, then position within the target), count[v] the entries of vertex v, rank[i] the position of entry order[i] in its vertex's list;
    and the target of every entry."""
    tf = np.asarray(target_first, np.int64)
    vi = np.asarray(vert_idx, np.int64).reshape(-1)
    assert tf[0] == 0 and (np.diff(tf) >= 0).all() and tf[-1] == vi.size and (vi.size == 0 or (vi.min() >= 0 and vi.max() < n_verts))
    target = np.repeat(np.arange(tf.size - 1), np.diff(tf))
    order = np.argsort(vi, kind="stable")
    count = np.bincount(vi, minlength=n_verts)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    rank = np.arange(vi.size) - start[vi[order]]
    return order, count, rank, target


def morph_ref(base, target_first, vert_idx, deltas, weights):
    """base [V,3]; entries target_first [T+1], vert_idx [E], deltas [E,3]; weights [T] -> positions [V,3] float32"""
    p = np.ascontiguousarray(base, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(deltas, np.float32).reshape(-1, 3)
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    vi = np.asarray(vert_idx, np.int64).reshape(-1)
    order, count, rank, target = _by_vertex(p.shape[0], target_first, vi)
    assert w.size == np.asarray(target_first).size - 1 and np.isfinite(d).all()
    acc = p.copy()
    with np.errstate(all="ignore"):
        for k in range(int(count.max()) if count.size else 0):     # the k-th entry of every vertex that has one
            e = order[rank == k]
            v, wk = vi[e], w[target[e]]
            skip = wk == 0                                             # true for +0 and for -0
            for c in range(3):
                term = wk * d[e, c]
                acc[v, c] = np.where(skip, acc[v, c], acc[v, c] + term)
    return acc


def pack_ref(n_verts, target_first, vert_idx, deltas):
    """-> (slice_first uint32 [nSlices+1], entries uint32 [padded,4], info dict): slices of 64 vertices, each with as many rows as its longest entry
    list; record (slice_first[s] + k) * 64 + l = the k-th entry of vertex 64 s + l as {delta bits, target}, else the pad record."""
    d = np.ascontiguousarray(deltas, np.float32).reshape(-1, 3)
    vi = np.asarray(vert_idx, np.int64).reshape(-1)
    order, count, rank, target = _by_vertex(n_verts, target_first, vi)
    n_slices = (n_verts + SLICE - 1) // SLICE
    padded = np.zeros(n_slices * SLICE, np.int64)
    padded[:n_verts] = count
    rows = padded.reshape(n_slices, SLICE).max(axis=1)
    slice_first = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint32)
    entries = np.zeros((int(slice_first[-1]) * SLICE, 4), np.uint32)
    entries[:, 3] = PAD
    v = vi[order]
    at = (slice_first[v // SLICE].astype(np.int64) + rank) * SLICE + v % SLICE
    entries[at, :3] = d[order].view(np.uint32)
    entries[at, 3] = target[order]
    n_targets = np.asarray(target_first).size - 1
    info = {"nVerts": n_verts, "nTargets": n_targets, "nSlices": n_slices, "maxPerVertex": int(count.max()) if count.size else 0,
            "entries": int(vi.size), "paddedEntries": int(entries.shape[0]),
            "bytes": int(entries.shape[0]) * 16 + (n_slices + 1) * 4 + n_verts * 12 + n_targets * 4}
    return slice_first, entries, info
