// rt_nearest_multi.hip -- the proximity query (rt_query_nearest_multi): per point the K rows least under (e(t), prim) among those with
// e(t) <= L, and the count of all of them, as rt_nearest_points_multi (rt_nearest_multi.cpp) defines them.  The walk is k_nearest's (rt_nearest.hip): one
// lane per point over the two-child records with exact boxes (sc.wnodes) and the triangle rows (sc.tris), depth first, carrying lbEff = the largest
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

#pragma clang fp contract(off)

namespace rtd {
namespace {

using namespace nearest;

// The scene (root box included) into the query's frame descriptor: the walk reads it through scalar loads
__global__ void k_nearest_multi_prep(DevFrame *fr, DevScene sc) {
    if (threadIdx.x == 0) { fr->sc = sc; scene_take_root_box(fr->sc); }
}

// stackEntries: entries per lane of the stack (the tree's depth: depth first, at most one deferred sibling per level).  blockDim.x: 64, 128 or 256.
template <bool FARFIRST, bool ALL>
__global__ __launch_bounds__(256) void k_nearest_multi(const DevFrame *fr, NearestMultiQuery r, int stackEntries) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int K = r.K;
    const uint32_t bs = blockDim.x;
    unsigned long long *kb = reinterpret_cast<unsigned long long *>(lds) + threadIdx.x;   // slot s at kb[s * bs]
    // entry e at stk[e * 64]: ref in the low word, the bits of lbEff in the high word
    unsigned long long *stk = reinterpret_cast<unsigned long long *>(lds) + (size_t)K * bs + (threadIdx.x >> 6) * (stackEntries * 64) + (threadIdx.x & 63);
    const uint32_t i = blockIdx.x * bs + threadIdx.x;
    if (i >= r.n) return;
    const DevScene &sc = fr->sc;
    const V3 p = ld3(r.p + (size_t)i * r.ps);
    const float md = r.md ? r.md[i] : 0.0f;
    const float L = r.md ? md * md : __builtin_inff();
    float b = L;   // the cull bound: never increases
    int total = 0, kept = 0, visits = 0;
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
                        const float e = (d2 < lbCur) ? lbCur : d2;   // a NaN d2 stays NaN, and is never accepted
                        if (!(e <= L)) continue;
                        total++;
                        // sorted insertion: the buffer holds the `kept` least so far, ascending
                        const unsigned long long w = ((unsigned long long)f2u(e) << 32) | (uint32_t)(first + k);
                        if (kept == K && (K == 0 || w >= kb[(K - 1) * bs])) continue;
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
                if (!more) break;
            }
        }
    }
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
    hipLaunchKernelGGL(k_nearest_multi_prep, dim3(1), dim3(64), 0, st, dFrame, sc);
    const int stackEntries = std::min(std::max(treeDepth, 1), RT_NEAREST_MULTI_STACK_MAX);
    const unsigned threads = (unsigned)rt_nearest_multi_block(stackEntries, q.K);
    const size_t ldsBytes = rt_nearest_multi_lds((int)threads, stackEntries, q.K);
    const unsigned blocks = (q.n + threads - 1u) / threads;
    const bool all = q.counts != nullptr || q.K == 0;   // the count needs every accepted row: cull against the limit alone
    auto go = [&](auto *kernel) {
        if (ldsBytes > ((size_t)64 << 10)) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), ldsBytes, st, (const DevFrame *)dFrame, q, stackEntries);
    };
    if (farFirst) { if (all) go(&k_nearest_multi<true, true>); else go(&k_nearest_multi<true, false>); }
    else { if (all) go(&k_nearest_multi<false, true>); else go(&k_nearest_multi<false, false>); }
    return hipGetLastError();
}
