"""What the definitions of the three overlap queries share, restated in numpy once: the small float32 helpers, the explicit
right-child-first walk -- `order`, the path mask and `visits` -- over whatever node test a shape has, and the answer that a row test and a walk make
together.  What differs per shape -- which slots are live, the query's box, the row test Sat, the node test and the query sets -- stays in
box_query_ref.py, tri_query_ref.py and hull_query_ref.py, whose Walk and Answer forward here."""
import numpy as np

import nearest_ref

f32 = np.float32
_idx = nearest_ref._idx


def min3(a, b, c):
    return np.fmin(np.fmin(a, b), c)                       # a NaN operand is ignored


def max3(a, b, c):
    return np.fmax(np.fmax(a, b), c)


def sub(a, b):
    with np.errstate(all="ignore"):
        return (a - b).astype(f32)


def row_points(tris12):
    """a, b, c of every row: one rounded add per component."""
    t = np.asarray(tris12, f32)
    with np.errstate(all="ignore"):
        return t[:, 0:3], (t[:, 0:3] + t[:, 4:7]).astype(f32), (t[:, 0:3] + t[:, 8:11]).astype(f32)


def rows_as_tris(tris12):
    return np.concatenate(row_points(tris12), 1)


def boxes_overlap(bmin, bmax, lo, hi):
    """Closed boxes [M,3] against queries [N,3] -> [N,M]: comparisons only."""
    with np.errstate(all="ignore"):
        return (~(bmax[None] < lo[:, None]) & ~(hi[:, None] < bmin[None])).all(-1)


def leaves(nodes):
    return np.array([k for k in range(nodes.shape[0]) if _idx(nodes[k, 9]) > 0])


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def box_enter(nodes12, box, alive):
    """[N,M] bool, the node test of the box and triangle queries: the node box overlaps the query's box [N,6] and the query is live."""
    nodes12 = np.asarray(nodes12, f32)
    return boxes_overlap(nodes12[:, 0:3], nodes12[:, 4:7], box[:, 0:3], box[:, 3:6]) & alive[:, None]


class Walk:
    """An explicit depth-first walk of nodes12 for all queries at once, the right child before the left.  enter [N,M] bool: the nodes a query enters
    once the walk reaches them -- dead queries enter none; alive [N] bool.  `order` [T], the rows in the order the walk of a query that enters
    everything meets them (any query's walk meets a subsequence of it); path [N,T] bool, every node from the root to the row's leaf is entered;
    visits [N], the boxes tested: 1 + twice the inner nodes entered, 0 for an empty slot.  With by_normal [N,M] -- the nodes a hull's face normal
    rejects although their boxes overlap its [lo, hi] -- also culled [N,M], those of them that the walk reached."""

    def __init__(self, nodes12, n_tris, enter, alive, by_normal=None):
        nodes12 = np.asarray(nodes12, f32)
        self.path = np.zeros((enter.shape[0], n_tris), bool)
        self.visits = alive.astype(np.int32)               # the root box
        if by_normal is not None:
            self.culled = np.zeros_like(by_normal)
            self.culled[:, 0] = by_normal[:, 0]
        order = []
        stack = [(0, enter[:, 0])]
        while stack:
            ni, entered = stack.pop()
            count = _idx(nodes12[ni, 9])
            if count > 0:
                first = _idx(nodes12[ni, 8])
                order.extend(range(first, first + count))
                self.path[:, first:first + count] = entered[:, None]
            else:
                self.visits += 2 * entered.astype(np.int32)
                l, r = _idx(nodes12[ni, 3]), _idx(nodes12[ni, 7])
                if by_normal is not None:
                    self.culled[:, l] = entered & by_normal[:, l]
                    self.culled[:, r] = entered & by_normal[:, r]
                stack.append((l, entered & enter[:, l]))
                stack.append((r, entered & enter[:, r]))      # popped first
        self.order = np.array(order, np.int64)


class Answer:
    """The definition's answer from a shape's row test `sat` (accept [N,T]) and its `walk`: accepted = sat.accept & walk.path [N,T], count [N] int32,
    and lists -- lists[i] the accepted rows of query i in walk order (int32 arrays)."""

    def __init__(self, sat, walk):
        self.sat, self.walk = sat, walk
        self.accepted = sat.accept & walk.path
        self.count = self.accepted.sum(1).astype(np.int32)
        in_order = self.accepted[:, walk.order]
        self.lists = [walk.order[in_order[i]].astype(np.int32) for i in range(self.accepted.shape[0])]
        self.visits = walk.visits

    def offsets(self):
        return np.concatenate([[0], np.cumsum(self.count)]).astype(np.int32)

    def filled(self, offsets=None, cap=None, sentinel=-77):
        """What a call leaves of a prims array pre-filled with `sentinel`: slot i (offsets, or i * cap) holds the first min(capacity, count) rows."""
        n = len(self.lists)
        if offsets is None:
            offsets = (np.arange(n + 1, dtype=np.int64) * cap)
        out = np.full(int(max(offsets[-1], 0)), sentinel, np.int32)
        for i, rows in enumerate(self.lists):
            room = max(int(offsets[i + 1]) - int(offsets[i]), 0)
            k = min(room, rows.size)
            out[int(offsets[i]):int(offsets[i]) + k] = rows[:k]
        return out

    def pairs(self):
        return np.array([(i, t) for i, rows in enumerate(self.lists) for t in rows], np.int32).reshape(-1, 2)
