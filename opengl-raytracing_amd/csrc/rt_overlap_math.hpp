// rt_overlap_math.hpp -- the float operations of the overlap queries' definitions: the 13-axis test of a row against a box, the
// 20-axis test of a row against a query triangle, the 46-axis test of a row against a convex hexahedron, and the
// three query shapes the walks run over.  One text for both sides, as rt_nearest_math.hpp, whose primitives these functions are written in: device functions over rtd::V3 for rt_overlap_query.hip, inline host
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

// ---- the query shapes.  A walk calls load() on the query's floats, enters the nodes whose boxes pass node() -- for a box and a
// triangle the overlap with [lo(), hi()] --, calls prepare() once before the first row (kPrepareFirst: before the first node(), which reads what
// prepare() forms), and row() on every row of an entered leaf
struct BoxShape {
    V blo, bhi;   // the query's floats: lo.xyz, hi.xyz
    RT_Q bool load(const float *q) {   // false: a NaN component or lo > hi, an empty slot
        blo = ld(q); bhi = ld(q + 3);
        return blo.x <= bhi.x && blo.y <= bhi.y && blo.z <= bhi.z;
    }
    RT_Q V lo() const { return blo; }
    RT_Q V hi() const { return bhi; }
    RT_Q void prepare() {}
    static constexpr bool kPrepareFirst = false;
    RT_Q bool node(V bmin, V bmax) const { return boxes_overlap(bmin, bmax, blo, bhi); }
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
    static constexpr bool kPrepareFirst = false;
    RT_Q bool node(V bmin, V bmax) const { return boxes_overlap(bmin, bmax, Q.lo, Q.hi); }
    RT_Q bool row(V v0, V e1, V e2) const { return tri_overlaps(v0, e1, e2, Q); }
};

// ---- a row, and a node's box, against the convex hull of eight points
// On the hull's axes only finite projections separate.  A face normal or an edge product of a hull some 1e19 across overflows, and then dot() gives
// inf or NaN (inf * 0, inf - inf) for some points and not for others; min and max, which pass over a NaN, would build an interval from the points
// that happened to stay, and an inf may carry the wrong sign (fma(1e30, -1e30, inf) = inf).  So each side's interval is made NaN -- it then never
// separates -- unless every projection that went into it is finite: s - s is added to its ends, with s the sum of those projections in a fixed order.
// An inf or a NaN among them stays in s, so s - s is NaN then, and 0 otherwise -- or, harmlessly, NaN again where finite projections sum to inf.  A
// node's box counts only when it and its interval lie within +-1e38, by comparisons, which a NaN fails: three projections inside such an interval have
// a finite sum, so a row under a rejected node is rejected by the row test too.
constexpr float kHullLimit = 1e38f;   // (< FLT_MAX / 3)
RT_Q bool within_limit(V lo, V hi) {
    return lo.x >= -kHullLimit && lo.y >= -kHullLimit && lo.z >= -kHullLimit && hi.x <= kHullLimit && hi.y <= kHullLimit && hi.z <= kHullLimit;
}

// The closed box [lo, hi] on the axis n: its corners through dot's own three steps, the least and the greatest kept at each -- the operations
// tri_overlaps(.., lo, hi) above performs for the row's normal.  Every step is monotone in the point, so dot(n, p) of a point p inside the box lies in
// [bmin, bmax] as computed, in the extended reals; with n, lo and hi finite no step gives a NaN, and an overflow reaches bmin or bmax as an inf or is
// passed over on the side where that is right (min(+inf, x) = x)
RT_Q void box_interval(V n, V lo, V hi, float &bmin, float &bmax) {
    const float lx = n.x * lo.x, hx = n.x * hi.x;
    const float mx = fminr(lx, hx), Mx = fmaxr(lx, hx);
    const float my = fminr(fmar(n.y, lo.y, mx), fmar(n.y, hi.y, mx)), My = fmaxr(fmar(n.y, lo.y, Mx), fmar(n.y, hi.y, Mx));
    bmin = fminr(fmar(n.z, lo.z, my), fmar(n.z, hi.z, my));
    bmax = fmaxr(fmar(n.z, lo.z, My), fmar(n.z, hi.z, My));
}
// True when the axis n parts the box, which lies within the limit, from the hull's interval [hmin, hmax] on it; a NaN never does, nor an interval of
// the box beyond the limit.  [hmin, hmax] is NaN where n is not finite (HullShape::interval)
RT_Q bool box_separates(V n, V lo, V hi, float hmin, float hmax) {
    float bmin, bmax;
    box_interval(n, lo, hi, bmin, bmax);
    return (bmax < hmin || hmax < bmin) && bmin >= -kHullLimit && bmax <= kHullLimit;
}
// The row's interval on ax against [hmin, hmax], only where the three projections and their sum are finite (row_separates above is the triangle
// query's, which passes over a NaN)
RT_Q bool finite_row_separates(V ax, V a, V b, V c, float hmin, float hmax) {
    const float ta = dot(ax, a), tb = dot(ax, b), tc = dot(ax, c);
    const float sum = (ta + tb) + tc, bad = sum - sum;
    return (max3(ta, tb, tc) + bad) < hmin || hmax < (min3(ta, tb, tc) + bad);
}

// The hull of the eight corners c0 .. c7 (query floats c0.xyz .. c7.xyz): corner k has bit 0 for the low or high end along the shape's first parameter,
// bit 1 along the second, bit 2 along the third -- a box under an affine or projective map: an oriented box, a sheared one, a frustum, a pyramid whose
// near face is its apex.  The caller supplies planar, convex faces.  Where the faces are not planar the test still never misses a real overlap: every
// axis it tries projects all eight points, the true hull, so a wrong face normal is a worse axis, never a wrong verdict -- it errs towards overlap.
// Infinite and huge corners are legal: an axis on which any projection is not finite does not separate (above), so they err towards overlap too.
//   Kept across the walk: the corners, their box, the six face normals -- the cross product of each face's diagonals, so that a face collapsed to a
// point leaves its neighbours' normals intact and has the zero normal itself, which never separates -- and the hull's interval on each.  The twelve
// edges are formed again for every row that reaches them: the same subtractions of the same corners, so no bit differs, and 36 registers less
struct HullShape {
    V c0, c1, c2, c3, c4, c5, c6, c7, hlo, hhi;
    V n0, n1, n2, n3, n4, n5;
    float n0Lo, n0Hi, n1Lo, n1Hi, n2Lo, n2Hi, n3Lo, n3Hi, n4Lo, n4Hi, n5Lo, n5Hi;
    static RT_Q bool nan3(V p) { return p.x != p.x || p.y != p.y || p.z != p.z; }
    RT_Q bool load(const float *q) {   // false: a NaN among the 24 floats, an empty slot
        c0 = ld(q); c1 = ld(q + 3); c2 = ld(q + 6); c3 = ld(q + 9); c4 = ld(q + 12); c5 = ld(q + 15); c6 = ld(q + 18); c7 = ld(q + 21);
        const bool nan = nan3(c0) || nan3(c1) || nan3(c2) || nan3(c3) || nan3(c4) || nan3(c5) || nan3(c6) || nan3(c7);
        hlo = V{fminr(fminr(min3(c0.x, c1.x, c2.x), min3(c3.x, c4.x, c5.x)), fminr(c6.x, c7.x)), fminr(fminr(min3(c0.y, c1.y, c2.y), min3(c3.y, c4.y, c5.y)), fminr(c6.y, c7.y)),
                fminr(fminr(min3(c0.z, c1.z, c2.z), min3(c3.z, c4.z, c5.z)), fminr(c6.z, c7.z))};   // (of no use where a component is NaN)
        hhi = V{fmaxr(fmaxr(max3(c0.x, c1.x, c2.x), max3(c3.x, c4.x, c5.x)), fmaxr(c6.x, c7.x)), fmaxr(fmaxr(max3(c0.y, c1.y, c2.y), max3(c3.y, c4.y, c5.y)), fmaxr(c6.y, c7.y)),
                fmaxr(fmaxr(max3(c0.z, c1.z, c2.z), max3(c3.z, c4.z, c5.z)), fmaxr(c6.z, c7.z))};
        return !nan;
    }
    RT_Q V lo() const { return hlo; }
    RT_Q V hi() const { return hhi; }
    // The hull's interval on ax: all eight corners through dot; NaN unless the eight projections and their sum are finite (an axis with a component
    // that is not finite gives none that is)
    RT_Q void interval(V ax, float &hmin, float &hmax) const {
        const float p0 = dot(ax, c0), p1 = dot(ax, c1), p2 = dot(ax, c2), p3 = dot(ax, c3), p4 = dot(ax, c4), p5 = dot(ax, c5), p6 = dot(ax, c6), p7 = dot(ax, c7);
        const float sum = ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), bad = sum - sum;   // (an inf or a NaN among them stays in the sum)
        hmin = fminr(fminr(min3(p0, p1, p2), min3(p3, p4, p5)), fminr(p6, p7)) + bad;
        hmax = fmaxr(fmaxr(max3(p0, p1, p2), max3(p3, p4, p5)), fmaxr(p6, p7)) + bad;
    }
    // The normal of the face (a, b, c, d): the cross product of its diagonals d - a and c - b
    static RT_Q V face(V a, V b, V c, V d) { return crs(sub(d, a), sub(c, b)); }
    static constexpr bool kPrepareFirst = true;
    RT_Q void prepare() {
        n0 = face(c0, c2, c4, c6); n1 = face(c1, c3, c5, c7); n2 = face(c0, c1, c4, c5); n3 = face(c2, c3, c6, c7); n4 = face(c0, c1, c2, c3); n5 = face(c4, c5, c6, c7);
        interval(n0, n0Lo, n0Hi); interval(n1, n1Lo, n1Hi); interval(n2, n2Lo, n2Hi); interval(n3, n3Lo, n3Hi); interval(n4, n4Lo, n4Hi); interval(n5, n5Lo, n5Hi);
    }
    // A node is entered when its box overlaps [lo, hi] and none of the six face normals parts it from the hull
    RT_Q bool node(V bmin, V bmax) const {
        if (!boxes_overlap(bmin, bmax, hlo, hhi)) return false;
        if (!within_limit(bmin, bmax)) return true;   // (a box beyond the limit is entered)
        return !(box_separates(n0, bmin, bmax, n0Lo, n0Hi) || box_separates(n1, bmin, bmax, n1Lo, n1Hi) || box_separates(n2, bmin, bmax, n2Lo, n2Hi) ||
                 box_separates(n3, bmin, bmax, n3Lo, n3Hi) || box_separates(n4, bmin, bmax, n4Lo, n4Hi) || box_separates(n5, bmin, bmax, n5Lo, n5Hi));
    }
    // One projected axis: the hull's eight corners and the row's three points through the same dot
    RT_Q bool axis_separates(V ax, V a, V b, V c) const {
        float hmin, hmax;
        interval(ax, hmin, hmax);
        return finite_row_separates(ax, a, b, c, hmin, hmax);
    }
    // The three axes cross(f_i, d) of one hull edge d
    RT_Q bool edge_separates(V d, V f1, V f2, V f3, V a, V b, V c) const {
        return axis_separates(crs(f1, d), a, b, c) || axis_separates(crs(f2, d), a, b, c) || axis_separates(crs(f3, d), a, b, c);
    }
    // The triangle test of DESIGN.md 26.1: true when none of the 46 axes separates the row from the hull.  The cheap axes first: they reject most rows
    RT_Q bool row(V v0, V e1, V e2) const {
        const V a = v0, b = add(v0, e1), c = add(v0, e2);
        const V tmin = {min3(a.x, b.x, c.x), min3(a.y, b.y, c.y), min3(a.z, b.z, c.z)}, tmax = {max3(a.x, b.x, c.x), max3(a.y, b.y, c.y), max3(a.z, b.z, c.z)};
        if (!boxes_overlap(tmin, tmax, hlo, hhi)) return false;
        if (finite_row_separates(n0, a, b, c, n0Lo, n0Hi) || finite_row_separates(n1, a, b, c, n1Lo, n1Hi) || finite_row_separates(n2, a, b, c, n2Lo, n2Hi)) return false;
        if (finite_row_separates(n3, a, b, c, n3Lo, n3Hi) || finite_row_separates(n4, a, b, c, n4Lo, n4Hi) || finite_row_separates(n5, a, b, c, n5Lo, n5Hi)) return false;
        if (axis_separates(crs(e1, e2), a, b, c)) return false;
        const V f1 = e1, f2 = sub(e2, e1), f3 = e2;
        if (edge_separates(sub(c1, c0), f1, f2, f3, a, b, c) || edge_separates(sub(c3, c2), f1, f2, f3, a, b, c)) return false;   // along the first parameter
        if (edge_separates(sub(c5, c4), f1, f2, f3, a, b, c) || edge_separates(sub(c7, c6), f1, f2, f3, a, b, c)) return false;
        if (edge_separates(sub(c2, c0), f1, f2, f3, a, b, c) || edge_separates(sub(c3, c1), f1, f2, f3, a, b, c)) return false;   // along the second
        if (edge_separates(sub(c6, c4), f1, f2, f3, a, b, c) || edge_separates(sub(c7, c5), f1, f2, f3, a, b, c)) return false;
        if (edge_separates(sub(c4, c0), f1, f2, f3, a, b, c) || edge_separates(sub(c5, c1), f1, f2, f3, a, b, c)) return false;   // along the third
        return !(edge_separates(sub(c6, c2), f1, f2, f3, a, b, c) || edge_separates(sub(c7, c3), f1, f2, f3, a, b, c));
    }
};

}  // namespace rtoverlap
