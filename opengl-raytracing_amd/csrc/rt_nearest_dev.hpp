// rt_nearest_dev.hpp -- what is device-only of the nearest-point queries, for rt_nearest.hip and rt_nearest_multi.hip: the
// stack entry and the walk both kernels run.  The float operations are rt_nearest_math.hpp's, one text for host and device.
#pragma once
#include "rt_frame.hpp"
#include "rt_nearest_math.hpp"

#pragma clang fp contract(off)

namespace rtd {
namespace nearest {

using rtnear::box_lb;
using rtnear::closest_uv;
using rtnear::point_at;

RT_DEV unsigned long long entry(int ref, float lbEff) { return (unsigned long long)(uint32_t)ref | ((unsigned long long)f2u(lbEff) << 32); }   // a stack entry
RT_DEV bool finite1(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }

// The walk of one lane from the root: depth first over sc.wnodes / sc.tris, carrying lbEff = the largest box bound on the way down.  A node is
// skipped when lbEff > b, at the test and again at the pop; row(prim, e) is called for every row of an entered leaf, ascending, with the row's e, and
// may lower b.  e(t) never lies below lbEff of a node above t, so the cull is exact for any child order: the near child first,
// FARFIRST for the tests.  stk: the lane's stack (lane_stack), entry e at stk[e * 64], ref in the low word, the bits of lbEff in the high word;
// stackEntries: its entries (the tree's depth: at most one deferred sibling per level).  Returns the boxes tested.
template <bool FARFIRST, class Row>
RT_DEV int nearest_walk(const DevScene &sc, unsigned long long *stk, int stackEntries, V3 p, float &b, Row row) {
    float lbCur = box_lb(ld3(sc.rootMin), ld3(sc.rootMax), p);
    int visits = 1;
    if (lbCur > b) return visits;
    int ref = sc.rootRef;
    int sp = 0;
    for (;;) {
        if (ref >= 0) {
            const float4 *nd = sc.wnodes + (size_t)ref * 4;
            const float4 a = nd[0], bb = nd[1], c = nd[2], d = nd[3];
            const float lbL = fmaxr(lbCur, box_lb(f4xyz(a), f4xyz(bb), p));
            const float lbR = fmaxr(lbCur, box_lb(f4xyz(c), f4xyz(d), p));
            visits += 2;
            const bool goL = !(lbL > b), goR = !(lbR > b);
            const int refL = (int)f2u(a.w), refR = (int)f2u(bb.w);
            if (goL && goR && sp < stackEntries) {   // (the depth bounds the deferred siblings: one per level)
                const bool rightFirst = FARFIRST ? lbL < lbR : lbR < lbL;
                stk[sp * 64] = rightFirst ? entry(refL, lbL) : entry(refR, lbR);
                sp++;
                ref = rightFirst ? refR : refL;
                lbCur = rightFirst ? lbR : lbL;
                continue;
            }
            if (goL || goR) {
                ref = goL ? refL : refR;
                lbCur = goL ? lbL : lbR;
                continue;
            }
        } else {
            const int v = -ref - 1;
            const int first = v >> 3, count = (v & 7) + 1;
            for (int k = 0; k < count; ++k) {
                const float4 *t = sc.tris + (size_t)(first + k) * 3;
                row(first + k, rtnear::row_e(p, f4xyz(t[0]), f4xyz(t[1]), f4xyz(t[2]), lbCur));
            }
        }
        bool more = false;
        while (sp > 0) {   // a deferred sibling the bound has overtaken meanwhile is dropped without a box test
            sp--;
            const unsigned long long s = stk[sp * 64];
            ref = (int)(uint32_t)s;
            lbCur = u2f((uint32_t)(s >> 32));
            if (lbCur > b) continue;
            more = true;
            break;
        }
        if (!more) return visits;
    }
}

}  // namespace nearest
}  // namespace rtd
