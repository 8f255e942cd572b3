// rt_bvh_build.hpp -- what the two GPU builders of the reference's median-split BVH share: the host-side skeleton (the SHAPE of the tree, which
// depends on the triangle count alone) and the per-level device kernels.  Included by rt_bvh_gpu.hip (rt_build_bvh_gpu: host arrays in, host
// arrays out) and rt_mesh.hip (the device-resident rebuild); one source, so that both sort the same keys and ties fall alike.
#pragma once
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace {

struct SkNode { int begin, end, left, right, depth, firstOut; };

// pre-order numbering, exactly rt_host.cpp build_nodes / bvh.cpp build_recursive
void skeleton(int n, std::vector<SkNode> &nodes) {
    struct Work { int begin, end, parent, depth; bool isRight; };
    std::vector<Work> todo{{0, n, -1, 0, false}};
    while (!todo.empty()) {
        const Work w = todo.back();
        todo.pop_back();
        const int self = (int)nodes.size();
        nodes.push_back({w.begin, w.end, -1, -1, w.depth, -1});
        if (w.parent >= 0) (w.isRight ? nodes[(size_t)w.parent].right : nodes[(size_t)w.parent].left) = self;
        if (w.end - w.begin <= 8) continue;
        const int mid = (w.begin + w.end) / 2;
        todo.push_back({mid, w.end, self, w.depth + 1, true});
        todo.push_back({w.begin, mid, self, w.depth + 1, false});
    }
    // leaf re-packing: LIFO walk that pushes left then right (bvh.cpp:109-135)
    int out = 0;
    std::vector<int> walk{0};
    while (!walk.empty()) {
        const int i = walk.back();
        walk.pop_back();
        SkNode &nd = nodes[(size_t)i];
        if (nd.left < 0) { nd.firstOut = out; out += nd.end - nd.begin; }
        else { walk.push_back(nd.left); walk.push_back(nd.right); }
    }
}

__device__ __forceinline__ uint32_t f2sortable(float f) { uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float sortable2f(uint32_t s) { return __uint_as_float((s & 0x80000000u) ? (s & 0x7fffffffu) : ~s); }

// per triangle: bounds and centroid, the reference's expressions (bvh.cpp:10-26)
__global__ void k_tri_prep(const float *__restrict__ t9, int n, float *__restrict__ mn, float *__restrict__ mx, float *__restrict__ cen) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *t = t9 + (size_t)i * 9;
    for (int a = 0; a < 3; ++a) {
        const float v0 = t[a], v1 = v0 + t[3 + a], v2 = v0 + t[6 + a];
        mn[(size_t)a * n + i] = fminf(v0, fminf(v1, v2));
        mx[(size_t)a * n + i] = fmaxf(v0, fmaxf(v1, v2));
        cen[(size_t)a * n + i] = ((v0 + v1) + v2) * (1.0f / 3.0f);
    }
}

// item position -> rank of the node of this level that contains it (levelBegin sorted ascending, binary search)
__device__ int find_seg(const int *__restrict__ segBegin, int nSeg, int pos) {
    int lo = 0, hi = nSeg - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (segBegin[mid] <= pos) lo = mid; else hi = mid - 1; }
    return lo;
}

// bounds of every node of one level: sortable-uint atomics, pre-reduced per wave when the whole wave lies in one node
__global__ void k_level_bounds(const int *__restrict__ perm, int n, const float *__restrict__ mn, const float *__restrict__ mx,
                               const int *__restrict__ segBegin, const int *__restrict__ segEnd, int nSeg, uint32_t *__restrict__ bounds /* [nSeg][6] */) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    int seg = -1;
    if (live) { seg = find_seg(segBegin, nSeg, i); if (i < segBegin[seg] || i >= segEnd[seg]) seg = -1; }   // positions of finished leaves belong to no node of this level
    uint32_t v[6];
    for (int a = 0; a < 3; ++a) {
        const int t = live ? perm[i] : 0;
        v[a] = seg >= 0 ? f2sortable(mn[(size_t)a * n + t]) : 0xffffffffu;
        v[3 + a] = seg >= 0 ? f2sortable(mx[(size_t)a * n + t]) : 0u;
    }
    const int seg0 = __shfl(seg, 0, 64);
    const bool uniform = __ballot(seg != seg0) == 0ull;
    if (uniform) {
        if (seg0 < 0) return;
        for (int c = 0; c < 6; ++c) {
            uint32_t x = v[c];
            for (int off = 32; off > 0; off >>= 1) { const uint32_t y = __shfl_down(x, off, 64); x = c < 3 ? min(x, y) : max(x, y); }
            if ((threadIdx.x & 63) == 0) { if (c < 3) atomicMin(&bounds[(size_t)seg0 * 6 + c], x); else atomicMax(&bounds[(size_t)seg0 * 6 + c], x); }
        }
    } else if (seg >= 0) {
        for (int c = 0; c < 3; ++c) { atomicMin(&bounds[(size_t)seg * 6 + c], v[c]); atomicMax(&bounds[(size_t)seg * 6 + 3 + c], v[3 + c]); }
    }
}

// sort key of every item: (rank of its node at this level, centroid along that node's axis); items of nodes that are leaves
// at this level or were finished earlier keep their place (key = their position)
__global__ void k_level_keys(const int *__restrict__ perm, int n, const float *__restrict__ cen, const int *__restrict__ segBegin,
                             const int *__restrict__ segEnd, const int *__restrict__ segInner, int nSeg, const uint32_t *__restrict__ bounds,
                             unsigned long long *__restrict__ keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int seg = find_seg(segBegin, nSeg, i);
    // the high word orders ranges by where they start, so every range stays in place; the low word orders inside a range
    uint32_t lowKey = (uint32_t)i;
    uint32_t high = (uint32_t)i;                     // finished item: unique key = its own position
    if (i >= segBegin[seg] && i < segEnd[seg]) {
        high = (uint32_t)segBegin[seg];
        if (segInner[seg]) {
            const float ex = sortable2f(bounds[(size_t)seg * 6 + 3]) - sortable2f(bounds[(size_t)seg * 6 + 0]);
            const float ey = sortable2f(bounds[(size_t)seg * 6 + 4]) - sortable2f(bounds[(size_t)seg * 6 + 1]);
            const float ez = sortable2f(bounds[(size_t)seg * 6 + 5]) - sortable2f(bounds[(size_t)seg * 6 + 2]);
            const int axis = (ex > ey) ? ((ex > ez) ? 0 : 2) : ((ey > ez) ? 1 : 2);   // bvh.cpp:72
            lowKey = f2sortable(cen[(size_t)axis * n + perm[i]]);
        }
    }
    keys[i] = ((unsigned long long)high << 32) | lowKey;
}

__global__ void k_iota(int *p, int n) { const int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) p[i] = i; }

__global__ void k_emit_tris(const float *__restrict__ t9, const int *__restrict__ perm, const int *__restrict__ outOfPos, int n, float *__restrict__ t12) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *t = t9 + (size_t)perm[i] * 9;
    float *o = t12 + (size_t)outOfPos[i] * 12;
    o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = 0.0f;
    o[4] = t[3]; o[5] = t[4]; o[6] = t[5]; o[7] = 0.0f;
    o[8] = t[6]; o[9] = t[7]; o[10] = t[8]; o[11] = 0.0f;
}

}  // namespace
