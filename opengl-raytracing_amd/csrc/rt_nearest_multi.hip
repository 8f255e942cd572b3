// rt_nearest_multi.hip -- the proximity query (rt_query_nearest_multi): per point the K rows least under (e(t), prim) among those with
// e(t) <= L, and the count of all of them, as rt_nearest_points_multi (rt_nearest_multi.cpp) defines them.  The walk is k_nearest's, the
// one function nearest_walk (rt_nearest_dev.hpp): one lane per point over the two-child records with exact boxes (sc.wnodes) and the triangle rows (sc.tris), depth first, carrying lbEff = the largest
// box bound on the way down.  A node is skipped when lbEff > b, at the test and again at the pop.  b is the limit L while the count is asked for (ALL:
// every accepted row matters), else L until the buffer holds K rows and the K-th row's e from then on.  e(t) never lies below lbEff of a node above t,
// so the cull is exact for any child order; the order is a performance choice, near child first, FARFIRST for the tests.
//   LDS, sized by the launch: the K-buffer, one 64-bit word bits(e) << 32 | prim per entry laid out [slot][thread] -- an accepted e is neither NaN nor
// negative, so the words order as (e, prim) -- then the stack, (ref, lbEff) per entry laid out [entry][lane] per wave.  The block is a multiple of 32
// threads, so a lane's bank depends on its index alone and not on the slot or entry: lanes at different slots do not conflict either.  u, v and the
// point are recomputed for the winners alone.  No dynamically indexed register array, no scratch.
#include "rt_nearest_multi.hpp"

#include "rt_nearest_dev.hpp"
#include "rt_nearest_multi_block.hpp"
#include "rt_query_launch.hpp"

#pragma clang fp contract(off)

namespace rtd {
namespace {

using namespace nearest;

// stackEntries: entries per lane of the stack (the tree's depth: depth first, at most one deferred sibling per level).  blockDim.x: 64, 128 or 256.
template <bool FARFIRST, bool ALL>
__global__ __launch_bounds__(256) void k_nearest_multi(const DevFrame *fr, NearestMultiQuery r, int stackEntries) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int K = r.K;
    const uint32_t bs = blockDim.x;
    unsigned long long *kb = reinterpret_cast<unsigned long long *>(lds) + threadIdx.x;   // slot s at kb[s * bs]
    unsigned long long *stk = lane_stack(reinterpret_cast<unsigned long long *>(lds) + (size_t)K * bs, stackEntries);
    const uint32_t i = blockIdx.x * bs + threadIdx.x;
    if (i >= r.n) return;
    const DevScene &sc = fr->sc;
    const V3 p = ld3(r.p + (size_t)i * r.ps);
    const float md = r.md ? r.md[i] : 0.0f;
    const float L = r.md ? md * md : __builtin_inff();
    float b = L;   // the cull bound: never increases
    int total = 0, kept = 0, visits = 0;
    if (!(r.md && md < 0.0f) && finite1(p.x) && finite1(p.y) && finite1(p.z))   // else an empty slot
        visits = nearest_walk<FARFIRST>(sc, stk, stackEntries, p, b, [&](int prim, float e) {
            if (!(e <= L)) return;   // a NaN e is never accepted
            total++;
            // sorted insertion: the buffer holds the `kept` least so far, ascending
            const unsigned long long w = ((unsigned long long)f2u(e) << 32) | (uint32_t)prim;
            if (kept == K && (K == 0 || w >= kb[(K - 1) * bs])) return;
            int j = kept < K ? kept : K - 1;
            while (j > 0) {
                const unsigned long long q = kb[(j - 1) * bs];
                if (w >= q) break;
                kb[j * bs] = q;
                j--;
            }
            kb[j * bs] = w;
            if (kept < K) kept++;
            if (!ALL && kept == K) b = u2f((uint32_t)(kb[(K - 1) * bs] >> 32));   // the K-th best: at most L, and at most what it was
        });
    if (r.counts) r.counts[i] = total;
    if (r.visits) r.visits[i] = visits;
    // u, v and c of the winners alone, by the same closest_uv on the same operands; one 16-byte store per slot, misses included
    for (int j = 0; j < K; ++j) {
        const size_t slot = (size_t)i * (size_t)K + (size_t)j;
        float4 h = make_float4(__builtin_inff(), __int_as_float(-1), 0.0f, 0.0f);
        V3 c = mk3(0.0f);
        if (j < kept) {
            const unsigned long long w = kb[j * bs];
            const int prim = (int)(uint32_t)w;
            const float4 *t = sc.tris + (size_t)prim * 3;
            const V3 v0 = f4xyz(t[0]), e1 = f4xyz(t[1]), e2 = f4xyz(t[2]);
            float uu, vv;
            closest_uv(p, v0, e1, e2, uu, vv);
            c = point_at(v0, e1, e2, uu, vv);
            h = make_float4(u2f((uint32_t)(w >> 32)), __int_as_float(prim), uu, vv);
        }
        r.hits[slot] = h;
        if (r.closest) { float *o = r.closest + slot * 3; o[0] = c.x; o[1] = c.y; o[2] = c.z; }
    }
}

}  // namespace
}  // namespace rtd

using namespace rtd;

hipError_t rt_nearest_multi_launch(hipStream_t st, int treeDepth, DevFrame *dFrame, const DevScene &sc, bool farFirst, const NearestMultiQuery &q) {
    static_assert(RT_NEAREST_MULTI_STACK_MAX == 64, "the block size is chosen for rt_query_stack_entries' ceiling");
    rt_query_prep(st, dFrame, sc);
    const int stackEntries = rt_query_stack_entries(treeDepth);
    const unsigned threads = (unsigned)rt_nearest_multi_block(stackEntries, q.K);
    const size_t ldsBytes = rt_nearest_multi_lds((int)threads, stackEntries, q.K);
    const bool all = q.counts != nullptr || q.K == 0;   // the count needs every accepted row: cull against the limit alone
    auto go = [&](auto *kernel) { rt_query_launch(kernel, st, threads, ldsBytes, dFrame, q, stackEntries); };
    if (farFirst) { if (all) go(&k_nearest_multi<true, true>); else go(&k_nearest_multi<true, false>); }
    else { if (all) go(&k_nearest_multi<false, true>); else go(&k_nearest_multi<false, false>); }
    return hipGetLastError();
}
