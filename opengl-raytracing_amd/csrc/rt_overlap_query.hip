// rt_overlap_query.hip -- the box query (rt_query_boxes), the triangle query (rt_query_tris) and the hull query
// (rt_query_hulls, rt_pick_rects): per query the rows of the triangle array that overlap the box, that the query triangle intersects, or
// that overlap the convex hull of the query's eight corners, as rt_box_overlaps, rt_tri_overlaps and rt_hull_overlaps (rt_overlap_query.cpp) define
// them, in walk order.  One lane per query walks the two arrays every scene has -- the 64-byte two-child records with exact boxes (sc.wnodes) and the
// 48-byte triangle rows (sc.tris) -- depth first, the right child before the left.  The query never shrinks, so nothing culls by what was found: the
// walk enters exactly the nodes that pass the shape's node test -- their boxes overlap the query's and, for a hull, none of its six face normals parts
// them from it --, tests both children of each, and pushes the left one only when both pass.  What a query is -- its floats, its box, its node test,
// what it keeps across the walk and its test of a row -- is the shape's (rt_overlap_math.hpp), the same text the definitions run.
// A triangle forms its edges, its normal, the three in-plane axes and its intervals on those four once, after the root box test; a hull forms its six
// face normals and its intervals on them once, before it, and its twelve edges again for every row that reaches them.
//   LDS, sized by the launch: the stack, one 4-byte ref per entry laid out [entry][lane] per wave -- one wave's push or pop is one conflict-free 4-byte
// write or read.  The shape, the write cursor and the count live in registers; a listing lane issues one 4-byte store per listed row and one for its
// count.  No dynamically indexed register array, no scratch, no atomics.
#include "rt_overlap_query.hpp"

#include "rt_overlap_math.hpp"
#include "rt_query_launch.hpp"

#pragma clang fp contract(off)

namespace rtd {
namespace {

// stackEntries: entries per lane of the stack (the tree's depth: depth first, at most one deferred sibling per level).  LIST = false: the counts alone
template <class Shape, bool LIST>
__global__ __launch_bounds__(256) void k_overlap_query(const DevFrame *fr, OverlapQuery r, int stackEntries) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    int *stk = lane_stack(reinterpret_cast<int *>(lds), stackEntries);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= r.n) return;
    const DevScene &sc = fr->sc;
    Shape S;
    const bool live = S.load(r.q + (size_t)i * r.qs);
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
    if (live) {
        visits = 1;
        if constexpr (Shape::kPrepareFirst) S.prepare();   // (a hull's node test reads its face normals)
        if (S.node(ld3(sc.rootMin), ld3(sc.rootMax))) {
            if constexpr (!Shape::kPrepareFirst) S.prepare();
            int ref = sc.rootRef;
            int sp = 0;
            for (;;) {
                if (ref >= 0) {
                    const float4 *nd = sc.wnodes + (size_t)ref * 4;
                    const float4 a = nd[0], bb = nd[1], c = nd[2], d = nd[3];
                    const bool goL = S.node(f4xyz(a), f4xyz(bb)), goR = S.node(f4xyz(c), f4xyz(d));
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
                        if (!S.row(f4xyz(t[0]), f4xyz(t[1]), f4xyz(t[2]))) continue;
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

// rt_rect_frusta's 24 floats per rect (rt_hull_corners.hpp), the root box from the frame descriptor
__global__ __launch_bounds__(256) void k_rect_frusta(const DevFrame *fr, rthull::RectCam cam, const float *rects, int stride, uint32_t n, float tNear, float tFar,
                                                     float *corners) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float far = rthull::rect_far(cam, ld3(fr->sc.rootMin), ld3(fr->sc.rootMax), tNear, tFar);
    rthull::rect_frustum(cam, rects + (size_t)i * stride, tNear, far, corners + (size_t)i * 24);
}

template <class Shape>
void launch(hipStream_t st, int treeDepth, DevFrame *dFrame, const OverlapQuery &q) {
    const int stackEntries = rt_query_stack_entries(treeDepth);
    const size_t ldsBytes = (size_t)stackEntries * 256 * sizeof(int);   // at most 64 KiB
    if (q.prims) rt_query_launch(&k_overlap_query<Shape, true>, st, 256, ldsBytes, dFrame, q, stackEntries);
    else rt_query_launch(&k_overlap_query<Shape, false>, st, 256, ldsBytes, dFrame, q, stackEntries);
}

}  // namespace
}  // namespace rtd

using namespace rtd;

hipError_t rt_overlap_launch(OverlapShape shape, hipStream_t st, int treeDepth, DevFrame *dFrame, const DevScene &sc, const OverlapQuery &q, bool prepared) {
    if (!prepared) rt_query_prep(st, dFrame, sc);
    if (shape == RT_OVERLAP_HULL) launch<rtoverlap::HullShape>(st, treeDepth, dFrame, q);
    else if (shape == RT_OVERLAP_TRI) launch<rtoverlap::TriShape>(st, treeDepth, dFrame, q);
    else launch<rtoverlap::BoxShape>(st, treeDepth, dFrame, q);
    return hipGetLastError();
}

hipError_t rt_rect_frusta_launch(hipStream_t st, DevFrame *dFrame, const DevScene &sc, const rthull::RectCam &cam, const float *rects, int stride, uint32_t n,
                                 float tNear, float tFar, float *corners) {
    rt_query_prep(st, dFrame, sc);
    hipLaunchKernelGGL(k_rect_frusta, dim3((n + 255u) / 256u), dim3(256), 0, st, (const DevFrame *)dFrame, cam, rects, stride, n, tNear, tFar, corners);
    return hipGetLastError();
}
