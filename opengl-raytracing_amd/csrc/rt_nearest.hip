// rt_nearest.hip -- the nearest-point query (rt_query_nearest): per point the triangle least under (e(t), prim) with e(t) <= L, as
// rt_nearest_points (rt_nearest.cpp) defines it.  One lane per point walks the two arrays every scene has -- the 64-byte two-child records with exact
// boxes (sc.wnodes) and the 48-byte triangle rows (sc.tris) -- depth first, carrying lbEff = the largest box bound on the way down, and skips a node
// when lbEff > the best e so far, at the test and again at the pop.  e(t) never lies below lbEff of a node above t, so the cull is exact for any child
// order; the order is a performance choice, near child first, FARFIRST for the tests.
//   LDS, sized by the launch: the stack, (ref, lbEff) per entry laid out [entry][lane] per wave -- one wave's push or pop is one conflict-free 8-byte
// write or read.  The best pair lives in registers; u, v and the point are recomputed for the winner alone.  No dynamically indexed register array,
// no scratch.
#include "rt_nearest.hpp"
#include "rt_nearest_dev.hpp"

#pragma clang fp contract(off)

namespace rtd {
namespace {

using namespace nearest;

// The scene (root box included) into the query's frame descriptor: the walk reads it through scalar loads
__global__ void k_nearest_prep(DevFrame *fr, DevScene sc) {
    if (threadIdx.x == 0) { fr->sc = sc; scene_take_root_box(fr->sc); }
}

// stackEntries: entries per lane of the stack (the tree's depth: depth first, at most one deferred sibling per level)
template <bool FARFIRST>
__global__ __launch_bounds__(256) void k_nearest(const DevFrame *fr, NearestQuery r, int stackEntries) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    // entry e at stk[e * 64]: ref in the low word, the bits of lbEff in the high word
    unsigned long long *stk = reinterpret_cast<unsigned long long *>(lds) + (threadIdx.x >> 6) * (stackEntries * 64) + (threadIdx.x & 63);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= r.n) return;
    const DevScene &sc = fr->sc;
    const V3 p = ld3(r.p + (size_t)i * r.ps);
    const float md = r.md ? r.md[i] : 0.0f;
    float b = r.md ? md * md : __builtin_inff();   // the best pair (b, bprim), initially (L, INT32_MAX)
    int bprim = INT32_MAX;
    int visits = 0;
    if (!(r.md && md < 0.0f) && finite1(p.x) && finite1(p.y) && finite1(p.z)) {   // else an empty slot
        float lbCur = box_lb(ld3(sc.rootMin), ld3(sc.rootMax), p);
        visits = 1;
        if (!(lbCur > b)) {
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
                        const V3 v0 = f4xyz(t[0]), e1 = f4xyz(t[1]), e2 = f4xyz(t[2]);
                        float uu, vv;
                        closest_uv(p, v0, e1, e2, uu, vv);
                        const V3 diff = p - point_at(v0, e1, e2, uu, vv);
                        const float d2 = dot(diff, diff);
                        const float e = (d2 < lbCur) ? lbCur : d2;   // a NaN d2 stays NaN, and is never taken
                        if (e < b || (e == b && first + k < bprim)) { b = e; bprim = first + k; }
                    }
                }
                bool more = false;
                while (sp > 0) {   // a deferred sibling the best has overtaken meanwhile is dropped without a box test
                    sp--;
                    const unsigned long long s = stk[sp * 64];
                    ref = (int)(uint32_t)s;
                    lbCur = u2f((uint32_t)(s >> 32));
                    if (lbCur > b) continue;
                    more = true;
                    break;
                }
                if (!more) break;
            }
        }
    }
    float4 h = make_float4(__builtin_inff(), __int_as_float(-1), 0.0f, 0.0f);
    V3 c = mk3(0.0f);
    if (bprim != INT32_MAX) {
        const float4 *t = sc.tris + (size_t)bprim * 3;
        const V3 v0 = f4xyz(t[0]), e1 = f4xyz(t[1]), e2 = f4xyz(t[2]);
        float uu, vv;
        closest_uv(p, v0, e1, e2, uu, vv);
        c = point_at(v0, e1, e2, uu, vv);
        h = make_float4(b, __int_as_float(bprim), uu, vv);
    }
    r.hits[i] = h;
    if (r.closest) { float *o = r.closest + (size_t)i * 3; o[0] = c.x; o[1] = c.y; o[2] = c.z; }
    if (r.visits) r.visits[i] = visits;
}

}  // namespace
}  // namespace rtd

using namespace rtd;

hipError_t rt_nearest_launch(hipStream_t st, int treeDepth, DevFrame *dFrame, const DevScene &sc, bool farFirst, const NearestQuery &q) {
    hipLaunchKernelGGL(k_nearest_prep, dim3(1), dim3(64), 0, st, dFrame, sc);
    const int stackEntries = std::min(std::max(treeDepth, 1), 64);
    const size_t ldsBytes = (size_t)stackEntries * 256 * sizeof(unsigned long long);
    const unsigned blocks = (q.n + 255u) / 256u;
    auto go = [&](auto *kernel) {
        if (ldsBytes > ((size_t)64 << 10)) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), ldsBytes, st, (const DevFrame *)dFrame, q, stackEntries);
    };
    if (farFirst) go(&k_nearest<true>); else go(&k_nearest<false>);
    return hipGetLastError();
}
