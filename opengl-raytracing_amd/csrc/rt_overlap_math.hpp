// rt_overlap_math.hpp -- the float operations of the overlap queries' definitions: the 13-axis test of a row against a box, the
// 20-axis test of a row against a query triangle, and the two query shapes the walks run over.  One text for both
// sides, as rt_nearest_math.hpp, whose primitives these functions are written in: device functions over rtd::V3 for rt_overlap_query.hip, inline host
// functions for rt_overlap_query.cpp.  Nothing contracted.
#pragma once
#include "rt_nearest_math.hpp"

namespace rtoverlap {

using namespace rtnear;

RT_Q float min3(float a, float b, float c) { return fminr(fminr(a, b), c); }   // a NaN operand is ignored
RT_Q float max3(float a, float b, float c) { return fmaxr(fmaxr(a, b), c); }
RT_Q V add(V a, V b) { return V{a.x + b.x, a.y + b.y, a.z + b.z}; }
RT_Q V crs(V x, V y) { return V{pd(x.y, y.z, x.z, y.y), pd(x.z, y.x, x.x, y.z), pd(x.x, y.y, x.y, y.x)}; }

// closed boxes: comparisons only
RT_Q bool boxes_overlap(V bmin, V bmax, V lo, V hi) {
    return !(bmax.x < lo.x) && !(hi.x < bmin.x) && !(bmax.y < lo.y) && !(hi.y < bmin.y) && !(bmax.z < lo.z) && !(hi.z < bmin.z);
}

// ---- a row against the closed box [lo, hi]
// One axis cross(unit_k, f): components n1, n2 on the coordinates i, j != k.  a1 .. c2: the vertices' coordinates i and j; l1 .. h2: the box's.
// A point projects to fma(p_j, n2, p_i * n1); the box to the least and the greatest of its corners under the same two steps, the least and the greatest
// product kept after the first.  Both steps are monotone, so a vertex inside the closed box never projects outside it.  True when the axis separates.
RT_Q bool edge_axis_separates(float n1, float n2, float a1, float a2, float b1, float b2, float c1, float c2, float l1, float h1, float l2, float h2) {
    const float pa = fmar(a2, n2, a1 * n1), pb = fmar(b2, n2, b1 * n1), pc = fmar(c2, n2, c1 * n1);
    const float tmin = min3(pa, pb, pc), tmax = max3(pa, pb, pc);
    const float l1p = l1 * n1, h1p = h1 * n1;
    const float m1 = fminr(l1p, h1p), M1 = fmaxr(l1p, h1p);
    const float bmin = fminr(fmar(l2, n2, m1), fmar(h2, n2, m1)), bmax = fmaxr(fmar(l2, n2, M1), fmar(h2, n2, M1));
    return tmax < bmin || bmax < tmin;
}

// cross(unit_x, f), cross(unit_y, f), cross(unit_z, f) = (0, -f.z, f.y), (f.z, 0, -f.x), (-f.y, f.x, 0): written out
RT_Q bool edge_separates(V f, V a, V b, V c, V lo, V hi) {
    return edge_axis_separates(-f.z, f.y, a.y, a.z, b.y, b.z, c.y, c.z, lo.y, hi.y, lo.z, hi.z) ||
           edge_axis_separates(-f.x, f.z, a.z, a.x, b.z, b.x, c.z, c.x, lo.z, hi.z, lo.x, hi.x) ||
           edge_axis_separates(-f.y, f.x, a.x, a.y, b.x, b.y, c.x, c.y, lo.x, hi.x, lo.y, hi.y);
}

// The triangle test of DESIGN.md 23.1: true when none of the 13 axes separates the row from [lo, hi]
RT_Q bool tri_overlaps(V v0, V e1, V e2, V lo, V hi) {
    const V a = v0, b = add(v0, e1), c = add(v0, e2);
    const V tmin = {min3(a.x, b.x, c.x), min3(a.y, b.y, c.y), min3(a.z, b.z, c.z)}, tmax = {max3(a.x, b.x, c.x), max3(a.y, b.y, c.y), max3(a.z, b.z, c.z)};
    if (!boxes_overlap(tmin, tmax, lo, hi)) return false;
    const V n = crs(e1, e2);
    const float d = dot(n, a);
    const float lx = n.x * lo.x, hx = n.x * hi.x;   // the box's corners through dot's own three steps, the least and the greatest kept at each
    const float mx = fminr(lx, hx), Mx = fmaxr(lx, hx);
    const float my = fminr(fmar(n.y, lo.y, mx), fmar(n.y, hi.y, mx)), My = fmaxr(fmar(n.y, lo.y, Mx), fmar(n.y, hi.y, Mx));
    const float bmin = fminr(fmar(n.z, lo.z, my), fmar(n.z, hi.z, my)), bmax = fmaxr(fmar(n.z, lo.z, My), fmar(n.z, hi.z, My));
    if (d < bmin || bmax < d) return false;
    if (edge_separates(e1, a, b, c, lo, hi)) return false;
    if (edge_separates(sub(e2, e1), a, b, c, lo, hi)) return false;
    return !edge_separates(e2, a, b, c, lo, hi);
}

// ---- a row against the query triangle (p0, p1, p2)
// The query's own values: its points, its edges g1 = p1 - p0, g2 = p2 - p1, g3 = p2 - p0, its normal m = cross(g1, g3), the three in-plane axes
// cross(m, g_j), the box of its points, and its intervals on m and on cross(m, g_j): the axes that do not depend on the row
struct Query {
    V p0, p1, p2, g1, g2, g3, m, mg1, mg2, mg3, lo, hi;
    float mLo, mHi, mg1Lo, mg1Hi, mg2Lo, mg2Hi, mg3Lo, mg3Hi;
};

// The row's interval on ax against [qmin, qmax].  True when the axis separates; a NaN never does
RT_Q bool row_separates(V ax, V a, V b, V c, float qmin, float qmax) {
    const float ta = dot(ax, a), tb = dot(ax, b), tc = dot(ax, c);
    return max3(ta, tb, tc) < qmin || qmax < min3(ta, tb, tc);
}

// One projected axis: the row's points and the query's points through the same dot
RT_Q bool axis_separates(V ax, V a, V b, V c, const Query &Q) {
    const float q0 = dot(ax, Q.p0), q1 = dot(ax, Q.p1), q2 = dot(ax, Q.p2);
    return row_separates(ax, a, b, c, min3(q0, q1, q2), max3(q0, q1, q2));
}

// The triangle test of DESIGN.md 24.1: true when none of the 20 axes separates the row from the query.  The box axes first: they reject most rows
RT_Q bool tri_overlaps(V v0, V e1, V e2, const Query &Q) {
    const V a = v0, b = add(v0, e1), c = add(v0, e2);
    const V tmin = {min3(a.x, b.x, c.x), min3(a.y, b.y, c.y), min3(a.z, b.z, c.z)}, tmax = {max3(a.x, b.x, c.x), max3(a.y, b.y, c.y), max3(a.z, b.z, c.z)};
    if (!boxes_overlap(tmin, tmax, Q.lo, Q.hi)) return false;
    const V f1 = e1, f2 = sub(e2, e1), f3 = e2;
    const V n = crs(e1, e2);
    if (axis_separates(n, a, b, c, Q)) return false;
    if (row_separates(Q.m, a, b, c, Q.mLo, Q.mHi)) return false;
    if (axis_separates(crs(f1, Q.g1), a, b, c, Q) || axis_separates(crs(f1, Q.g2), a, b, c, Q) || axis_separates(crs(f1, Q.g3), a, b, c, Q)) return false;
    if (axis_separates(crs(f2, Q.g1), a, b, c, Q) || axis_separates(crs(f2, Q.g2), a, b, c, Q) || axis_separates(crs(f2, Q.g3), a, b, c, Q)) return false;
    if (axis_separates(crs(f3, Q.g1), a, b, c, Q) || axis_separates(crs(f3, Q.g2), a, b, c, Q) || axis_separates(crs(f3, Q.g3), a, b, c, Q)) return false;
    if (axis_separates(crs(n, f1), a, b, c, Q) || axis_separates(crs(n, f2), a, b, c, Q) || axis_separates(crs(n, f3), a, b, c, Q)) return false;
    return !(row_separates(Q.mg1, a, b, c, Q.mg1Lo, Q.mg1Hi) || row_separates(Q.mg2, a, b, c, Q.mg2Lo, Q.mg2Hi) || row_separates(Q.mg3, a, b, c, Q.mg3Lo, Q.mg3Hi));
}

// ---- the query shapes.  A walk calls load() on the query's floats, walks the nodes whose boxes overlap [lo(), hi()], calls prepare()
// once before the first row, and row() on every row of an entered leaf
struct BoxShape {
    V blo, bhi;   // the query's floats: lo.xyz, hi.xyz
    RT_Q bool load(const float *q) {   // false: a NaN component or lo > hi, an empty slot
        blo = ld(q); bhi = ld(q + 3);
        return blo.x <= bhi.x && blo.y <= bhi.y && blo.z <= bhi.z;
    }
    RT_Q V lo() const { return blo; }
    RT_Q V hi() const { return bhi; }
    RT_Q void prepare() {}
    RT_Q bool row(V v0, V e1, V e2) const { return tri_overlaps(v0, e1, e2, blo, bhi); }
};

struct TriShape {
    Query Q;   // the query's floats: p0.xyz, p1.xyz, p2.xyz
    RT_Q bool load(const float *q) {   // false: a NaN component, an empty slot
        Q.p0 = ld(q); Q.p1 = ld(q + 3); Q.p2 = ld(q + 6);
        const bool nan = Q.p0.x != Q.p0.x || Q.p0.y != Q.p0.y || Q.p0.z != Q.p0.z || Q.p1.x != Q.p1.x || Q.p1.y != Q.p1.y || Q.p1.z != Q.p1.z ||
                         Q.p2.x != Q.p2.x || Q.p2.y != Q.p2.y || Q.p2.z != Q.p2.z;
        Q.lo = V{min3(Q.p0.x, Q.p1.x, Q.p2.x), min3(Q.p0.y, Q.p1.y, Q.p2.y), min3(Q.p0.z, Q.p1.z, Q.p2.z)};   // (of no use where a component is NaN)
        Q.hi = V{max3(Q.p0.x, Q.p1.x, Q.p2.x), max3(Q.p0.y, Q.p1.y, Q.p2.y), max3(Q.p0.z, Q.p1.z, Q.p2.z)};
        return !nan;
    }
    RT_Q V lo() const { return Q.lo; }
    RT_Q V hi() const { return Q.hi; }
    RT_Q void interval(V ax, float &qmin, float &qmax) const {
        const float q0 = dot(ax, Q.p0), q1 = dot(ax, Q.p1), q2 = dot(ax, Q.p2);
        qmin = min3(q0, q1, q2); qmax = max3(q0, q1, q2);
    }
    RT_Q void prepare() {
        Q.g1 = sub(Q.p1, Q.p0); Q.g2 = sub(Q.p2, Q.p1); Q.g3 = sub(Q.p2, Q.p0);
        Q.m = crs(Q.g1, Q.g3);
        Q.mg1 = crs(Q.m, Q.g1); Q.mg2 = crs(Q.m, Q.g2); Q.mg3 = crs(Q.m, Q.g3);
        interval(Q.m, Q.mLo, Q.mHi); interval(Q.mg1, Q.mg1Lo, Q.mg1Hi); interval(Q.mg2, Q.mg2Lo, Q.mg2Hi); interval(Q.mg3, Q.mg3Lo, Q.mg3Hi);
    }
    RT_Q bool row(V v0, V e1, V e2) const { return tri_overlaps(v0, e1, e2, Q); }
};

}  // namespace rtoverlap
