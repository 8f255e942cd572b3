// rt_box_query.hip -- the box query (rt_query_boxes): per axis-aligned box the rows of the triangle array that overlap it, as rt_box_overlaps
// (rt_box_query.cpp) defines them, in walk order.  One lane per box walks the two arrays every scene has -- the 64-byte two-child records with exact
// boxes (sc.wnodes) and the 48-byte triangle rows (sc.tris) -- depth first, the right child before the left.  The box never shrinks, so nothing culls:
// the walk enters exactly the nodes whose boxes overlap the query, tests both children of each, and pushes the left one only when it overlaps too.
//   LDS, sized by the launch: the stack, one 4-byte ref per entry laid out [entry][lane] per wave -- one wave's push or pop is one conflict-free 4-byte
// write or read.  lo, hi, the write cursor and the count live in registers; a listing lane issues one 4-byte store per listed row and one for its count.
// No dynamically indexed register array, no scratch, no atomics.
#include "rt_box_query.hpp"
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

// One axis cross(unit_k, f), operation for operation as rt_box_query.cpp has it: components n1, n2 on the coordinates i, j != k
RT_DEV bool edge_axis_separates(float n1, float n2, float a1, float a2, float b1, float b2, float c1, float c2, float l1, float h1, float l2, float h2) {
    const float pa = __builtin_fmaf(a2, n2, a1 * n1), pb = __builtin_fmaf(b2, n2, b1 * n1), pc = __builtin_fmaf(c2, n2, c1 * n1);
    const float tmin = min3(pa, pb, pc), tmax = max3(pa, pb, pc);
    const float l1p = l1 * n1, h1p = h1 * n1;
    const float m1 = fminr(l1p, h1p), M1 = fmaxr(l1p, h1p);
    const float bmin = fminr(__builtin_fmaf(l2, n2, m1), __builtin_fmaf(h2, n2, m1)), bmax = fmaxr(__builtin_fmaf(l2, n2, M1), __builtin_fmaf(h2, n2, M1));
    return tmax < bmin || bmax < tmin;
}

// cross(unit_x, f), cross(unit_y, f), cross(unit_z, f) = (0, -f.z, f.y), (f.z, 0, -f.x), (-f.y, f.x, 0): written out
RT_DEV bool edge_separates(V3 f, V3 a, V3 b, V3 c, V3 lo, V3 hi) {
    return edge_axis_separates(-f.z, f.y, a.y, a.z, b.y, b.z, c.y, c.z, lo.y, hi.y, lo.z, hi.z) ||
           edge_axis_separates(-f.x, f.z, a.z, a.x, b.z, b.x, c.z, c.x, lo.z, hi.z, lo.x, hi.x) ||
           edge_axis_separates(-f.y, f.x, a.x, a.y, b.x, b.y, c.x, c.y, lo.x, hi.x, lo.y, hi.y);
}

// The triangle test of DESIGN.md 23.1: true when none of the 13 axes separates the row from [lo, hi]
RT_DEV bool tri_overlaps(V3 v0, V3 e1, V3 e2, V3 lo, V3 hi) {
    const V3 a = v0, b = v0 + e1, c = v0 + e2;
    const V3 tmin = mk3(min3(a.x, b.x, c.x), min3(a.y, b.y, c.y), min3(a.z, b.z, c.z)), tmax = mk3(max3(a.x, b.x, c.x), max3(a.y, b.y, c.y), max3(a.z, b.z, c.z));
    if (!boxes_overlap(tmin, tmax, lo, hi)) return false;
    const V3 n = mk3(pd(e1.y, e2.z, e1.z, e2.y), pd(e1.z, e2.x, e1.x, e2.z), pd(e1.x, e2.y, e1.y, e2.x));
    const float d = dot(n, a);
    const float lx = n.x * lo.x, hx = n.x * hi.x;   // the box's corners through dot's own three steps, the least and the greatest kept at each
    const float mx = fminr(lx, hx), Mx = fmaxr(lx, hx);
    const float my = fminr(__builtin_fmaf(n.y, lo.y, mx), __builtin_fmaf(n.y, hi.y, mx)), My = fmaxr(__builtin_fmaf(n.y, lo.y, Mx), __builtin_fmaf(n.y, hi.y, Mx));
    const float bmin = fminr(__builtin_fmaf(n.z, lo.z, my), __builtin_fmaf(n.z, hi.z, my)), bmax = fmaxr(__builtin_fmaf(n.z, lo.z, My), __builtin_fmaf(n.z, hi.z, My));
    if (d < bmin || bmax < d) return false;
    if (edge_separates(e1, a, b, c, lo, hi)) return false;
    if (edge_separates(e2 - e1, a, b, c, lo, hi)) return false;
    return !edge_separates(e2, a, b, c, lo, hi);
}

// The scene (root box included) into the query's frame descriptor: the walk reads it through scalar loads
__global__ void k_box_prep(DevFrame *fr, DevScene sc) {
    if (threadIdx.x == 0) { fr->sc = sc; scene_take_root_box(fr->sc); }
}

// stackEntries: entries per lane of the stack (the tree's depth: depth first, at most one deferred sibling per level).  LIST = false: the counts alone
template <bool LIST>
__global__ __launch_bounds__(256) void k_box_query(const DevFrame *fr, BoxQuery r, int stackEntries) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    int *stk = reinterpret_cast<int *>(lds) + (threadIdx.x >> 6) * (stackEntries * 64) + (threadIdx.x & 63);   // entry e at stk[e * 64]
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= r.n) return;
    const DevScene &sc = fr->sc;
    const float *q = r.b + (size_t)i * r.bs;
    const V3 lo = ld3(q), hi = ld3(q + 3);
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
    if (lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z) {   // a NaN component or lo > hi: an empty slot
        visits = 1;
        if (boxes_overlap(ld3(sc.rootMin), ld3(sc.rootMax), lo, hi)) {
            int ref = sc.rootRef;
            int sp = 0;
            for (;;) {
                if (ref >= 0) {
                    const float4 *nd = sc.wnodes + (size_t)ref * 4;
                    const float4 a = nd[0], bb = nd[1], c = nd[2], d = nd[3];
                    const bool goL = boxes_overlap(f4xyz(a), f4xyz(bb), lo, hi), goR = boxes_overlap(f4xyz(c), f4xyz(d), lo, hi);
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
                        if (!tri_overlaps(f4xyz(t[0]), f4xyz(t[1]), f4xyz(t[2]), lo, hi)) continue;
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

hipError_t rt_box_query_launch(hipStream_t st, int treeDepth, DevFrame *dFrame, const DevScene &sc, const BoxQuery &q) {
    hipLaunchKernelGGL(k_box_prep, dim3(1), dim3(64), 0, st, dFrame, sc);
    const int stackEntries = std::min(std::max(treeDepth, 1), 64);
    const size_t ldsBytes = (size_t)stackEntries * 256 * sizeof(int);   // at most 64 KiB
    const unsigned blocks = (q.n + 255u) / 256u;
    if (q.prims) hipLaunchKernelGGL(k_box_query<true>, dim3(blocks), dim3(256), ldsBytes, st, (const DevFrame *)dFrame, q, stackEntries);
    else hipLaunchKernelGGL(k_box_query<false>, dim3(blocks), dim3(256), ldsBytes, st, (const DevFrame *)dFrame, q, stackEntries);
    return hipGetLastError();
}
