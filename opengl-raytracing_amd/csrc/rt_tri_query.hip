// rt_tri_query.hip -- the triangle query (rt_query_tris): per query triangle the rows of the triangle array that it intersects, as
// rt_tri_overlaps (rt_tri_query.cpp) defines them, in walk order.  One lane per query walks sc.wnodes / sc.tris exactly as the box query walks them for
// the box [qlo, qhi] of the query's three points: depth first, the right child before the left, both children of an inner node tested, the left one
// pushed only when both overlap.  At a leaf the rows are tested ascending: the three box axes by comparisons, then the seventeen projected axes.
//   Registers: the query's points, its edges g, its normal m, the three in-plane axes cross(m, g_j) and the query's intervals on those four axes are
// formed once per lane, before the walk -- the definition's operations on the definition's operands, so no bit changes by where they stand.
//   LDS, sized by the launch: the stack, one 4-byte ref per entry laid out [entry][lane] per wave.  A listing lane issues one 4-byte store per listed
// row and one for its count.  No dynamically indexed register array, no scratch, no atomics.
#include "rt_tri_query.hpp"
#include "rt_nearest_dev.hpp"

#pragma clang fp contract(off)

namespace rtd {
namespace {

using nearest::pd;

RT_DEV float min3(float a, float b, float c) { return fminr(fminr(a, b), c); }   // a NaN operand is ignored
RT_DEV float max3(float a, float b, float c) { return fmaxr(fmaxr(a, b), c); }

// closed boxes: comparisons only
RT_DEV bool boxes_overlap(V3 bmin, V3 bmax, V3 lo, V3 hi) {
    return !(bmax.x < lo.x) && !(hi.x < bmin.x) && !(bmax.y < lo.y) && !(hi.y < bmin.y) && !(bmax.z < lo.z) && !(hi.z < bmin.z);
}

RT_DEV V3 crs(V3 x, V3 y) { return mk3(pd(x.y, y.z, x.z, y.y), pd(x.z, y.x, x.x, y.z), pd(x.x, y.y, x.y, y.x)); }

// What a lane keeps of its query across the walk
struct Query {
    V3 p0, p1, p2, g1, g2, g3, m, mg1, mg2, mg3, lo, hi;
    float mLo, mHi, mg1Lo, mg1Hi, mg2Lo, mg2Hi, mg3Lo, mg3Hi;   // the query's intervals on m and on cross(m, g_j)
};

// The row's interval on ax against [qmin, qmax].  True when the axis separates; a NaN never does
RT_DEV bool row_separates(V3 ax, V3 a, V3 b, V3 c, float qmin, float qmax) {
    const float ta = dot(ax, a), tb = dot(ax, b), tc = dot(ax, c);
    return max3(ta, tb, tc) < qmin || qmax < min3(ta, tb, tc);
}

// One projected axis, operation for operation as rt_tri_query.cpp has it
RT_DEV bool axis_separates(V3 ax, V3 a, V3 b, V3 c, const Query &Q) {
    const float q0 = dot(ax, Q.p0), q1 = dot(ax, Q.p1), q2 = dot(ax, Q.p2);
    return row_separates(ax, a, b, c, min3(q0, q1, q2), max3(q0, q1, q2));
}

// The triangle test of DESIGN.md 24.1: true when none of the 20 axes separates the row from the query.  The box axes first: they reject most rows
RT_DEV bool tri_overlaps(V3 v0, V3 e1, V3 e2, const Query &Q) {
    const V3 a = v0, b = v0 + e1, c = v0 + e2;
    const V3 tmin = mk3(min3(a.x, b.x, c.x), min3(a.y, b.y, c.y), min3(a.z, b.z, c.z)), tmax = mk3(max3(a.x, b.x, c.x), max3(a.y, b.y, c.y), max3(a.z, b.z, c.z));
    if (!boxes_overlap(tmin, tmax, Q.lo, Q.hi)) return false;
    const V3 f1 = e1, f2 = e2 - e1, f3 = e2;
    const V3 n = crs(e1, e2);
    if (axis_separates(n, a, b, c, Q)) return false;
    if (row_separates(Q.m, a, b, c, Q.mLo, Q.mHi)) return false;
    if (axis_separates(crs(f1, Q.g1), a, b, c, Q) || axis_separates(crs(f1, Q.g2), a, b, c, Q) || axis_separates(crs(f1, Q.g3), a, b, c, Q)) return false;
    if (axis_separates(crs(f2, Q.g1), a, b, c, Q) || axis_separates(crs(f2, Q.g2), a, b, c, Q) || axis_separates(crs(f2, Q.g3), a, b, c, Q)) return false;
    if (axis_separates(crs(f3, Q.g1), a, b, c, Q) || axis_separates(crs(f3, Q.g2), a, b, c, Q) || axis_separates(crs(f3, Q.g3), a, b, c, Q)) return false;
    if (axis_separates(crs(n, f1), a, b, c, Q) || axis_separates(crs(n, f2), a, b, c, Q) || axis_separates(crs(n, f3), a, b, c, Q)) return false;
    return !(row_separates(Q.mg1, a, b, c, Q.mg1Lo, Q.mg1Hi) || row_separates(Q.mg2, a, b, c, Q.mg2Lo, Q.mg2Hi) || row_separates(Q.mg3, a, b, c, Q.mg3Lo, Q.mg3Hi));
}

// The scene (root box included) into the query's frame descriptor: the walk reads it through scalar loads
__global__ void k_tri_prep(DevFrame *fr, DevScene sc) {
    if (threadIdx.x == 0) { fr->sc = sc; scene_take_root_box(fr->sc); }
}

// stackEntries: entries per lane of the stack (the tree's depth: depth first, at most one deferred sibling per level).  LIST = false: the counts alone
template <bool LIST>
__global__ __launch_bounds__(256) void k_tri_query(const DevFrame *fr, TriQuery r, int stackEntries) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    int *stk = reinterpret_cast<int *>(lds) + (threadIdx.x >> 6) * (stackEntries * 64) + (threadIdx.x & 63);   // entry e at stk[e * 64]
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= r.n) return;
    const DevScene &sc = fr->sc;
    const float *q = r.t + (size_t)i * r.ts;
    Query Q;
    Q.p0 = ld3(q); Q.p1 = ld3(q + 3); Q.p2 = ld3(q + 6);
    int32_t *out = nullptr;   // the slot: `room` entries from `out`
    int room = 0;
    if (LIST) {
        if (r.offsets) {
            const int o0 = r.offsets[i], o1 = r.offsets[i + 1];
            if (o0 >= 0 && o1 > o0) { out = r.prims + o0; room = o1 - o0; }
        } else {
            out = r.prims + (size_t)i * (size_t)r.cap;
            room = r.cap;
        }
    }
    int found = 0, visits = 0;
    const bool nan = Q.p0.x != Q.p0.x || Q.p0.y != Q.p0.y || Q.p0.z != Q.p0.z || Q.p1.x != Q.p1.x || Q.p1.y != Q.p1.y || Q.p1.z != Q.p1.z ||
                     Q.p2.x != Q.p2.x || Q.p2.y != Q.p2.y || Q.p2.z != Q.p2.z;
    if (!nan) {   // a NaN component: an empty slot
        visits = 1;
        Q.lo = mk3(min3(Q.p0.x, Q.p1.x, Q.p2.x), min3(Q.p0.y, Q.p1.y, Q.p2.y), min3(Q.p0.z, Q.p1.z, Q.p2.z));
        Q.hi = mk3(max3(Q.p0.x, Q.p1.x, Q.p2.x), max3(Q.p0.y, Q.p1.y, Q.p2.y), max3(Q.p0.z, Q.p1.z, Q.p2.z));
        if (boxes_overlap(ld3(sc.rootMin), ld3(sc.rootMax), Q.lo, Q.hi)) {
            Q.g1 = Q.p1 - Q.p0; Q.g2 = Q.p2 - Q.p1; Q.g3 = Q.p2 - Q.p0;
            Q.m = crs(Q.g1, Q.g3);
            Q.mg1 = crs(Q.m, Q.g1); Q.mg2 = crs(Q.m, Q.g2); Q.mg3 = crs(Q.m, Q.g3);
            {
                const float q0 = dot(Q.m, Q.p0), q1 = dot(Q.m, Q.p1), q2 = dot(Q.m, Q.p2);
                Q.mLo = min3(q0, q1, q2); Q.mHi = max3(q0, q1, q2);
            }
            {
                const float q0 = dot(Q.mg1, Q.p0), q1 = dot(Q.mg1, Q.p1), q2 = dot(Q.mg1, Q.p2);
                Q.mg1Lo = min3(q0, q1, q2); Q.mg1Hi = max3(q0, q1, q2);
            }
            {
                const float q0 = dot(Q.mg2, Q.p0), q1 = dot(Q.mg2, Q.p1), q2 = dot(Q.mg2, Q.p2);
                Q.mg2Lo = min3(q0, q1, q2); Q.mg2Hi = max3(q0, q1, q2);
            }
            {
                const float q0 = dot(Q.mg3, Q.p0), q1 = dot(Q.mg3, Q.p1), q2 = dot(Q.mg3, Q.p2);
                Q.mg3Lo = min3(q0, q1, q2); Q.mg3Hi = max3(q0, q1, q2);
            }
            int ref = sc.rootRef;
            int sp = 0;
            for (;;) {
                if (ref >= 0) {
                    const float4 *nd = sc.wnodes + (size_t)ref * 4;
                    const float4 a = nd[0], bb = nd[1], c = nd[2], d = nd[3];
                    const bool goL = boxes_overlap(f4xyz(a), f4xyz(bb), Q.lo, Q.hi), goR = boxes_overlap(f4xyz(c), f4xyz(d), Q.lo, Q.hi);
                    visits += 2;
                    const int refL = (int)f2u(a.w), refR = (int)f2u(bb.w);
                    if (goL && goR && sp < stackEntries) {   // (the depth bounds the deferred siblings: one per level)
                        stk[sp * 64] = refL;
                        sp++;
                        ref = refR;
                        continue;
                    }
                    if (goL || goR) {
                        ref = goR ? refR : refL;
                        continue;
                    }
                } else {
                    const int v = -ref - 1;
                    const int first = v >> 3, count = (v & 7) + 1;
                    for (int k = 0; k < count; ++k) {
                        const float4 *t = sc.tris + (size_t)(first + k) * 3;
                        if (!tri_overlaps(f4xyz(t[0]), f4xyz(t[1]), f4xyz(t[2]), Q)) continue;
                        if (LIST && found < room) out[found] = first + k;
                        found++;
                    }
                }
                if (sp == 0) break;
                sp--;
                ref = stk[sp * 64];
            }
        }
    }
    if (r.counts) r.counts[i] = found;
    if (r.visits) r.visits[i] = visits;
}

}  // namespace
}  // namespace rtd

using namespace rtd;

hipError_t rt_tri_query_launch(hipStream_t st, int treeDepth, DevFrame *dFrame, const DevScene &sc, const TriQuery &q) {
    hipLaunchKernelGGL(k_tri_prep, dim3(1), dim3(64), 0, st, dFrame, sc);
    const int stackEntries = std::min(std::max(treeDepth, 1), 64);
    const size_t ldsBytes = (size_t)stackEntries * 256 * sizeof(int);   // at most 64 KiB
    const unsigned blocks = (q.n + 255u) / 256u;
    if (q.prims) hipLaunchKernelGGL(k_tri_query<true>, dim3(blocks), dim3(256), ldsBytes, st, (const DevFrame *)dFrame, q, stackEntries);
    else hipLaunchKernelGGL(k_tri_query<false>, dim3(blocks), dim3(256), ldsBytes, st, (const DevFrame *)dFrame, q, stackEntries);
    return hipGetLastError();
}
