"""numpy definition of a raster draw list that names slots bound to the dynamic mesh (rt_raster_mesh_dynamic).

A bound draw is, by definition, the run of static draws -- one per non-empty part, in part order -- that rt_render_raster would execute from
slots holding the mesh's positions and the part's index triples, with model = rt_mat4_mul(draw.model, table[p]) and the part's colour when a
colour table is set.  expand() writes that run out and raster_ref.render draws it: numpy and raster_ref only.
"""
from __future__ import annotations

import numpy as np

import raster_ref as rr


class Bound:
    """What a slot is bound as: parts=False is RT_RASTER_BIND_SINGLE; colors: None or [nParts,3] floats (parts mode only)."""

    def __init__(self, parts=False, colors=None):
        self.parts = bool(parts)
        self.colors = None if colors is None else np.asarray(colors, np.float32).reshape(-1, 3)


def _fields(d):
    return (d.mesh, list(d.model), list(d.color)) if hasattr(d, "mesh") else d


def expand(meshes, draws, bound, dyn):
    """meshes: {slot: (positions, indices)} of the static slots; draws: the draw list (RtRasterDraw-like objects or (slot, model16, color3));
    bound: {slot: Bound}; dyn = (positions [V,3], indices, part_first [nParts+1], table [nParts,16]) -- the dynamic mesh as it stands.
    -> (meshes, draws, bases) for raster_ref.render: the expanded list, and bases[k] = global primitive index of the first triangle of draws[k]."""
    out_meshes, out_draws, bases, base = dict(meshes), [], [], 0
    for k, d in enumerate(draws):
        slot, model, color = _fields(d)
        bases.append(base)
        if slot not in bound:
            out_draws.append((slot, model, color))
            base += np.asarray(meshes[slot][1]).size // 3
            continue
        pos, idx, pf, table = dyn
        idx = np.asarray(idx, np.uint32).reshape(-1, 3)
        pf = np.asarray(pf, np.int64)
        b = bound[slot]
        if not b.parts:
            out_meshes[("dyn", k)] = (pos, idx)
            out_draws.append((("dyn", k), model, color))
        else:
            table = np.asarray(table, np.float32).reshape(-1, 16)
            assert table.shape[0] == pf.size - 1 and (b.colors is None or b.colors.shape[0] == pf.size - 1)
            for p in range(pf.size - 1):
                if pf[p + 1] == pf[p]:
                    continue   # an empty part contributes nothing
                out_meshes[("dyn", k, p)] = (pos, idx[pf[p]:pf[p + 1]])
                with np.errstate(all="ignore"):   # non-finite matrix entries are legal input
                    m = rr.mat4_mul(model, table[p])
                out_draws.append((("dyn", k, p), m, color if b.colors is None else list(b.colors[p])))
        base += idx.shape[0]
    return out_meshes, out_draws, bases


def render(meshes, draws, bound, dyn, view, proj, W, H, window=None):
    """-> (rgba8, prim_id, depth24, stats, bases) of the draw list with its bound draws expanded."""
    m, d, bases = expand(meshes, draws, bound, dyn)
    with np.errstate(all="ignore"):
        rgba, prim, depth, stats = rr.render(m, d, view, proj, W, H, window=window, return_stats=True)
    return rgba, prim, depth, stats, bases


def prim_parts(prim_id, base, part_first):
    """searchsorted restatement of raster_prim_parts: (part, triangle of the part), -1 outside [base, base + nTris) and on the background."""
    pf = np.asarray(part_first, np.int64)
    t = np.asarray(prim_id).astype(np.int64) - int(base)
    ok = (np.asarray(prim_id) != rr.BACKGROUND) & (t >= 0) & (t < pf[-1])
    part = np.searchsorted(pf, np.where(ok, t, 0), "right") - 1
    return np.where(ok, part, -1).astype(np.int32), np.where(ok, t - pf[part], -1).astype(np.int32)
