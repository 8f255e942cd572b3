// rt_nearest.hip -- the nearest-point query (rt_query_nearest): per point the triangle least under (e(t), prim) with e(t) <= L, as
// rt_nearest_points (rt_nearest.cpp) defines it.  One lane per point walks the two arrays every scene has -- the 64-byte two-child records with exact
// boxes (sc.wnodes) and the 48-byte triangle rows (sc.tris) -- depth first, carrying lbEff = the largest box bound on the way down, and skips a node
// when lbEff > the best e so far, at the test and again at the pop.  e(t) never lies below lbEff of a node above t, so the cull is exact for any child
// order; the order is a performance choice, near child first, FARFIRST for the tests.  The walk itself is nearest_walk
// (rt_nearest_dev.hpp), which k_nearest_multi runs too.
//   LDS, sized by the launch: the stack, (ref, lbEff) per entry laid out [entry][lane] per wave -- one wave's push or pop is one conflict-free 8-byte
// write or read.  The best pair lives in registers; u, v and the point are recomputed for the winner alone.  No dynamically indexed register array,
// no scratch.
#include "rt_nearest.hpp"
#include "rt_nearest_dev.hpp"
#include "rt_query_launch.hpp"

#pragma clang fp contract(off)

namespace rtd {
namespace {

using namespace nearest;

// stackEntries: entries per lane of the stack (the tree's depth: depth first, at most one deferred sibling per level)
template <bool FARFIRST>
__global__ __launch_bounds__(256) void k_nearest(const DevFrame *fr, NearestQuery r, int stackEntries) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned long long *stk = lane_stack(reinterpret_cast<unsigned long long *>(lds), stackEntries);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= r.n) return;
    const DevScene &sc = fr->sc;
    const V3 p = ld3(r.p + (size_t)i * r.ps);
    const float md = r.md ? r.md[i] : 0.0f;
    float b = r.md ? md * md : __builtin_inff();   // the best pair (b, bprim), initially (L, INT32_MAX)
    int bprim = INT32_MAX;
    int visits = 0;
    if (!(r.md && md < 0.0f) && finite1(p.x) && finite1(p.y) && finite1(p.z))   // else an empty slot
        visits = nearest_walk<FARFIRST>(sc, stk, stackEntries, p, b, [&](int prim, float e) {   // a NaN e is never taken
            if (e < b || (e == b && prim < bprim)) { b = e; bprim = prim; }
        });
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
    rt_query_prep(st, dFrame, sc);
    const int stackEntries = rt_query_stack_entries(treeDepth);
    const size_t ldsBytes = (size_t)stackEntries * 256 * sizeof(unsigned long long);
    if (farFirst) rt_query_launch(&k_nearest<true>, st, 256, ldsBytes, dFrame, q, stackEntries);
    else rt_query_launch(&k_nearest<false>, st, 256, ldsBytes, dFrame, q, stackEntries);
    return hipGetLastError();
}
