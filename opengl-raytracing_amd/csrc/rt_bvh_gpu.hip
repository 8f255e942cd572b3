// rt_bvh_gpu.hip -- the reference's median-split BVH (src/scene/bvh.cpp:41-135) built on the GPU ("GPU
// builder as an optional fast path"; the reference builds on the CPU only).
//
// The builder splits a range [begin,end) at mid = (begin+end)/2 and makes a leaf of <= 8 triangles (bvh.cpp:62,73), so the
// SHAPE of the tree -- node numbering (pre-order), ranges, leaf slots after the LIFO re-packing (:109-135) -- depends on
// the triangle count alone and is laid out on the host (skeleton()).  What depends on the data is done on the device,
// level by level, for all nodes of a depth at once:
//   * node bounds = min / max over the triangles of its range (bvh.cpp:49-54), block-reduced, one atomic per block and node;
//   * split axis = largest extent (:72);
//   * the partition about the median centroid (:75-80).  The reference uses std::nth_element; here every range is SORTED by
//     the same key (one global radix sort per level on (node rank, centroid[axis]) pairs).  The lower half holds the same
//     triangles whenever the median key is unique, so nodes, boxes and the set of triangles of every leaf are then identical
//     to the CPU build's; the order of triangles inside a leaf differs from it (nth_element's arrangement is unspecified), which
//     can change the winner of an exact-t tie between two triangles of one leaf, nothing else.  rt_build_bvh stays the
//     parity path; this is the fast one (1 M triangles: ~0.9 s on the host).
// THE TIE RULE (restated in tests/bvh_build_ref.py and compared bit for bit).  This builder is deterministic, ties
// included: level 0 starts from input order (k_iota); each level is ONE STABLE radix sort on (start of the item's range, sortable key
// of its centroid along the range's axis), applied to the permutation the level above left; items of leaves keep their place.  Items
// with bit-equal keys therefore keep their order, the lower half of a tied median takes the earlier ones, and the order of the rows
// inside a leaf is specified.  Boxes are min / max in the keys' order, in which -0 lies below +0; equal extents fall to the later axis.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/rt_mi355.h"
#include "rt_bvh_build.hpp"   // skeleton() and the per-level kernels, shared with the device-resident rebuild (rt_mesh.hip)

#pragma clang fp contract(off)

#define BG_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err = hipGetErrorString(e_); goto done; } } while (0)

namespace rtl {

// -> number of nodes, or a negative RtStatus; *errOut names a HIP error
int build_bvh_gpu(int device, const float *tris9, int nTris, float *nodes12, float *tris12, const char **errOut) {
    if (nTris < 0 || (nTris > 0 && (!tris9 || !nodes12 || !tris12))) return RT_ERR_INVALID;
    if (nTris == 0) return 0;
    const char *err = nullptr;
    std::vector<SkNode> sk;
    skeleton(nTris, sk);
    int maxDepth = 0;
    for (const SkNode &nd : sk) maxDepth = std::max(maxDepth, nd.depth);
    std::vector<std::vector<int>> byDepth((size_t)maxDepth + 1);
    for (int i = 0; i < (int)sk.size(); ++i) byDepth[(size_t)sk[(size_t)i].depth].push_back(i);
    for (auto &v : byDepth) std::sort(v.begin(), v.end(), [&](int a, int b) { return sk[(size_t)a].begin < sk[(size_t)b].begin; });
    size_t maxSeg = 0;
    for (auto &v : byDepth) maxSeg = std::max(maxSeg, v.size());
    std::vector<int> outOfPos((size_t)nTris);
    for (const SkNode &nd : sk)
        if (nd.left < 0) for (int k = 0; k < nd.end - nd.begin; ++k) outOfPos[(size_t)(nd.begin + k)] = nd.firstOut + k;

    const int n = nTris;
    const unsigned gN = (unsigned)((n + 255) / 256);
    float *dT9 = nullptr, *dMn = nullptr, *dMx = nullptr, *dCen = nullptr, *dT12 = nullptr;
    int *dPerm[2] = {nullptr, nullptr}, *dSegB = nullptr, *dSegE = nullptr, *dSegI = nullptr, *dOut = nullptr;
    unsigned long long *dKeys[2] = {nullptr, nullptr};
    uint32_t *dBounds = nullptr;
    void *dTemp = nullptr;
    size_t tempBytes = 0;
    std::vector<uint32_t> hostBounds(sk.size() * 6);
    std::vector<int> segB, segE, segI;
    int cur = 0;
    (void)hipSetDevice(device);
    hipStream_t st = nullptr;
    BG_TRY(hipStreamCreate(&st));
    BG_TRY(hipMalloc(&dT9, (size_t)n * 9 * 4)); BG_TRY(hipMalloc(&dMn, (size_t)n * 3 * 4)); BG_TRY(hipMalloc(&dMx, (size_t)n * 3 * 4));
    BG_TRY(hipMalloc(&dCen, (size_t)n * 3 * 4)); BG_TRY(hipMalloc(&dT12, (size_t)n * 12 * 4));
    BG_TRY(hipMalloc(&dPerm[0], (size_t)n * 4)); BG_TRY(hipMalloc(&dPerm[1], (size_t)n * 4));
    BG_TRY(hipMalloc(&dKeys[0], (size_t)n * 8)); BG_TRY(hipMalloc(&dKeys[1], (size_t)n * 8));
    BG_TRY(hipMalloc(&dSegB, maxSeg * 4)); BG_TRY(hipMalloc(&dSegE, maxSeg * 4)); BG_TRY(hipMalloc(&dSegI, maxSeg * 4));
    BG_TRY(hipMalloc(&dBounds, maxSeg * 6 * 4)); BG_TRY(hipMalloc(&dOut, (size_t)n * 4));
    BG_TRY(hipMemcpyAsync(dT9, tris9, (size_t)n * 9 * 4, hipMemcpyHostToDevice, st));
    BG_TRY(hipMemcpyAsync(dOut, outOfPos.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_tri_prep, dim3(gN), dim3(256), 0, st, dT9, n, dMn, dMx, dCen);
    hipLaunchKernelGGL(k_iota, dim3(gN), dim3(256), 0, st, dPerm[0], n);
    {
        rocprim::double_buffer<unsigned long long> kb(dKeys[0], dKeys[1]);
        rocprim::double_buffer<int> vb(dPerm[0], dPerm[1]);
        BG_TRY(rocprim::radix_sort_pairs(nullptr, tempBytes, kb, vb, (size_t)n, 0, 64, st));
        BG_TRY(hipMalloc(&dTemp, std::max<size_t>(tempBytes, 16)));
    }
    for (int d = 0; d <= maxDepth; ++d) {
        const std::vector<int> &ids = byDepth[(size_t)d];
        const int nSeg = (int)ids.size();
        segB.resize((size_t)nSeg); segE.resize((size_t)nSeg); segI.resize((size_t)nSeg);
        bool anyInner = false;
        for (int s = 0; s < nSeg; ++s) {
            const SkNode &nd = sk[(size_t)ids[(size_t)s]];
            segB[(size_t)s] = nd.begin; segE[(size_t)s] = nd.end; segI[(size_t)s] = nd.left >= 0;
            anyInner = anyInner || nd.left >= 0;
        }
        BG_TRY(hipMemcpyAsync(dSegB, segB.data(), (size_t)nSeg * 4, hipMemcpyHostToDevice, st));
        BG_TRY(hipMemcpyAsync(dSegE, segE.data(), (size_t)nSeg * 4, hipMemcpyHostToDevice, st));
        BG_TRY(hipMemcpyAsync(dSegI, segI.data(), (size_t)nSeg * 4, hipMemcpyHostToDevice, st));
        // identity of min over sortable uints = 0xffffffff, of max = 0: fill [min,min,min,max,max,max] per node
        {
            std::vector<uint32_t> init((size_t)nSeg * 6);
            for (int s = 0; s < nSeg; ++s) for (int c = 0; c < 6; ++c) init[(size_t)s * 6 + c] = c < 3 ? 0xffffffffu : 0u;
            BG_TRY(hipMemcpyAsync(dBounds, init.data(), init.size() * 4, hipMemcpyHostToDevice, st));
            BG_TRY(hipStreamSynchronize(st));   // `init` and the seg vectors are reused next level
        }
        hipLaunchKernelGGL(k_level_bounds, dim3(gN), dim3(256), 0, st, dPerm[cur], n, dMn, dMx, dSegB, dSegE, nSeg, dBounds);
        {
            std::vector<uint32_t> got((size_t)nSeg * 6);
            BG_TRY(hipMemcpyAsync(got.data(), dBounds, got.size() * 4, hipMemcpyDeviceToHost, st));
            BG_TRY(hipStreamSynchronize(st));
            for (int s = 0; s < nSeg; ++s) std::memcpy(&hostBounds[(size_t)ids[(size_t)s] * 6], &got[(size_t)s * 6], 24);
        }
        if (!anyInner) continue;
        hipLaunchKernelGGL(k_level_keys, dim3(gN), dim3(256), 0, st, dPerm[cur], n, dCen, dSegB, dSegE, dSegI, nSeg, dBounds, dKeys[cur]);
        {
            rocprim::double_buffer<unsigned long long> kb(dKeys[cur], dKeys[cur ^ 1]);
            rocprim::double_buffer<int> vb(dPerm[cur], dPerm[cur ^ 1]);
            BG_TRY(rocprim::radix_sort_pairs(dTemp, tempBytes, kb, vb, (size_t)n, 0, 64, st));
            cur = (vb.current() == dPerm[0]) ? 0 : 1;
        }
    }
    hipLaunchKernelGGL(k_emit_tris, dim3(gN), dim3(256), 0, st, dT9, dPerm[cur], dOut, n, dT12);
    BG_TRY(hipMemcpyAsync(tris12, dT12, (size_t)n * 12 * 4, hipMemcpyDeviceToHost, st));
    BG_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < sk.size(); ++i) {   // upload_bvh_tbo node texels, bvh.cpp:153-168
        const SkNode &nd = sk[i];
        float *o = nodes12 + i * 12;
        for (int c = 0; c < 6; ++c) {
            const uint32_t s = hostBounds[i * 6 + (size_t)c];
            const uint32_t u = (s & 0x80000000u) ? (s & 0x7fffffffu) : ~s;
            std::memcpy(&o[c < 3 ? c : c + 1], &u, 4);
        }
        o[3] = (float)nd.left; o[7] = (float)nd.right;
        o[8] = nd.left < 0 ? (float)nd.firstOut : -1.0f;
        o[9] = nd.left < 0 ? (float)(nd.end - nd.begin) : 0.0f;
        o[10] = o[11] = 0.0f;
    }
done:
    for (void *p : {(void *)dT9, (void *)dMn, (void *)dMx, (void *)dCen, (void *)dT12, (void *)dPerm[0], (void *)dPerm[1], (void *)dKeys[0], (void *)dKeys[1],
                    (void *)dSegB, (void *)dSegE, (void *)dSegI, (void *)dBounds, (void *)dOut, dTemp})
        if (p) (void)hipFree(p);
    if (st) (void)hipStreamDestroy(st);
    if (err) { if (errOut) *errOut = err; return RT_ERR_HIP; }
    return (int)sk.size();
}

}  // namespace rtl
