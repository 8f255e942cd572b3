// rt_multi_hit.hip -- the multi-hit query (rt_trace_rays_multi, rt_pick_pixels_multi): per ray the K nearest accepted triangles and the
// count of all of them, as rt_multi_hits (rt_multi_hit.cpp) defines them.  One lane per ray walks the two arrays every scene has -- the 64-byte
// two-child records with exact boxes (sc.wnodes) and the 48-byte triangle rows (sc.tris) -- with traceBVHShadow's tests at the ray's limit T and no
// cull against a found hit.  The answer is a set, so the child order is free and the stack holds references alone.
//   LDS, sized by the launch: the K-buffer, (key(t), prim) per entry laid out [slot][thread] -- one wave's access to a slot is one conflict-free
// 8-byte read or write -- then the stack, [entry][lane] per wave as the frame kernels lay theirs out.  No dynamically indexed register array, no scratch.
#include "rt_multi_hit.hpp"

#pragma clang fp contract(off)

namespace rtd {
namespace {

// key(t): ascending keys are ascending t for every ordinary t; it orders NaNs too (positive ones last)
RT_DEV uint32_t key_of(float t) { const uint32_t b = f2u(t); return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
RT_DEV float t_of(uint32_t k) { return u2f(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
RT_DEV bool before(uint2 a, uint2 b) { return a.x != b.x ? a.x < b.x : a.y < b.y; }   // (key, prim) ascending

// The scene (root box included) and, for pixel rays, the uniform block into the query's frame descriptor: the walk reads both through scalar loads
__global__ __launch_bounds__(256) void k_multi_prep(DevFrame *fr, DevScene sc, const RtUniforms u, int withCam) {
    if (withCam) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(&u);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&fr->u);
        for (uint32_t k = threadIdx.x; k < sizeof(RtUniforms) / 4; k += blockDim.x) dst[k] = src[k];
    }
    if (threadIdx.x == 0) { fr->sc = sc; scene_take_root_box(fr->sc); }
}

// PIX: pixel rays from fr->u, as SceneSrc builds them.  stackEntries: entries per lane of the stack (the tree's depth).  live: the scene has a BVH.
template <bool PIX>
__global__ __launch_bounds__(256) void k_multi_hit(const DevFrame *fr, MultiHitQuery r, int stackEntries, int live) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int K = r.K;
    uint2 *kb = reinterpret_cast<uint2 *>(lds) + threadIdx.x;                                      // slot s at kb[s * 256]
    uint32_t *stk = reinterpret_cast<uint32_t *>(lds + (size_t)K * 256 * sizeof(uint2)) + (threadIdx.x >> 6) * (stackEntries * 64) + (threadIdx.x & 63);   // entry e at stk[e * 64]
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= r.n) return;
    const float T = r.tm ? r.tm[i] : r.inf;
    V3 ro = mk3(0.0f), rd = mk3(0.0f);
    int total = 0, kept = 0;
    if (live && !(r.tm && T < 0.0f)) {
        if (PIX) {
            ro = ld3(fr->u.camPos);
            rd = primaryDirJ(fr->u, (float)r.xy[(size_t)i * 2] + 0.5f, (float)r.xy[(size_t)i * 2 + 1] + 0.5f, fr->u.jitter[0], fr->u.jitter[1]);
        } else {
            ro = ld3(r.o + (size_t)i * r.os);
            rd = ld3(r.d + (size_t)i * r.ds);
        }
        const DevScene &sc = fr->sc;
        const V3 rdInv = mk3(1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z);
        float tminCur;
        if (slab(ro, rdInv, ld3(sc.rootMin), ld3(sc.rootMax), tminCur) && tminCur <= T) {
            int ref = sc.rootRef;
            int sp = 0;
            for (;;) {
                if (ref >= 0) {
                    const float4 *nd = sc.wnodes + (size_t)ref * 4;
                    const float4 a = nd[0], b = nd[1], c = nd[2], d = nd[3];
                    float tL, tR;
                    const bool hitL = slab(ro, rdInv, f4xyz(a), f4xyz(b), tL) && tL <= T;
                    const bool hitR = slab(ro, rdInv, f4xyz(c), f4xyz(d), tR) && tR <= T;
                    const int refL = (int)f2u(a.w), refR = (int)f2u(b.w);
                    if (hitL && hitR && sp < stackEntries) {   // (the depth bounds the deferred siblings: one per level)
                        stk[sp * 64] = (uint32_t)refR;
                        sp++;
                        ref = refL;
                        continue;
                    }
                    if (hitL || hitR) {
                        ref = hitL ? refL : refR;
                        continue;
                    }
                } else {
                    const int v = -ref - 1;
                    const int first = v >> 3, count = (v & 7) + 1;
                    for (int k = 0; k < count; ++k) {
                        const float4 *t = sc.tris + (size_t)(first + k) * 3;
                        const float4 p0 = t[0], p1 = t[1], p2 = t[2];
                        float tt;
                        if (!tri_hit(ro, rd, f4xyz(p0), f4xyz(p1), f4xyz(p2), r.eps, T, tt)) continue;
                        total++;
                        // sorted insertion: the buffer holds the `kept` smallest so far, ascending
                        const uint2 e = make_uint2(key_of(tt), (uint32_t)(first + k));
                        if (kept == K && (K == 0 || !before(e, kb[(K - 1) * 256]))) continue;
                        int j = kept < K ? kept : K - 1;
                        while (j > 0) {
                            const uint2 p = kb[(j - 1) * 256];
                            if (!before(e, p)) break;
                            kb[j * 256] = p;
                            j--;
                        }
                        kb[j * 256] = e;
                        if (kept < K) kept++;
                    }
                }
                if (sp == 0) break;
                sp--;
                ref = (int)stk[sp * 64];
            }
        }
    }
    if (r.counts) r.counts[i] = total;
    // u, v of the winners alone, with triHit's operations in their order (QuerySrc::store_closest); one 16-byte store per slot, misses included
    float4 *out = r.hits + (size_t)i * (size_t)K;
    for (int j = 0; j < K; ++j) {
        float4 h = make_float4(r.inf, __int_as_float(-1), 0.0f, 0.0f);
        if (j < kept) {
            const uint2 e = kb[j * 256];
            const float4 *Tr = fr->sc.tris + (size_t)e.y * 3;
            const V3 v0 = f4xyz(Tr[0]), e1 = f4xyz(Tr[1]), e2 = f4xyz(Tr[2]);
            const V3 pvec = cross(rd, e2);
            const float invDet = 1.0f / dot(e1, pvec);
            const V3 tvec = ro - v0;
            h = make_float4(t_of(e.x), __int_as_float((int)e.y), dot(tvec, pvec) * invDet, dot(rd, cross(tvec, e1)) * invDet);
        }
        out[j] = h;
    }
}

}  // namespace
}  // namespace rtd

using namespace rtd;

hipError_t rt_multi_hit_launch(hipStream_t st, int treeDepth, DevFrame *dFrame, const DevScene &sc, bool hasBVH, const MultiHitQuery &q) {
    RtUniforms u = {};
    if (q.xy) u = *q.cam;
    hipLaunchKernelGGL(k_multi_prep, dim3(1), dim3(256), 0, st, dFrame, sc, u, q.xy ? 1 : 0);
    const int stackEntries = std::min(std::max(treeDepth, 1), 64);
    const size_t ldsBytes = (size_t)q.K * 256 * sizeof(uint2) + (size_t)stackEntries * 256 * sizeof(uint32_t);
    const unsigned blocks = (q.n + 255u) / 256u;   // grid by the work: a one-pixel pick starts one block
    auto go = [&](auto *kernel) {
        if (ldsBytes > ((size_t)64 << 10)) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), ldsBytes, st, (const DevFrame *)dFrame, q, stackEntries, hasBVH ? 1 : 0);
    };
    if (q.xy) go(&k_multi_hit<true>); else go(&k_multi_hit<false>);
    return hipGetLastError();
}
