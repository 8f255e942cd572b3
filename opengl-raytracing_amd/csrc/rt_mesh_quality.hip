// rt_mesh_quality.hip -- the device measurement of the BVH quality metric: rt_bvh_cost's integer sums over the tree a rebuild or a
// refit left in the bounds array.  A translation unit of its own, so that the code objects of rt_mesh.hip, rt_mesh_refit.hip and rt_mesh_parts.hip stay
// the machine code they were (tools/isa_diff.py).  rt_mesh.hip owns the mesh, the tables and the result slots; this file only launches.
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "rt_bvh_cost.hpp"
#include "rt_mesh.hpp"

#pragma clang fp contract(off)

namespace {

// the sortable key of rt_bvh_build.hpp back to its float
__device__ __forceinline__ float sortable2f(uint32_t s) { return __uint_as_float((s & 0x80000000u) ? (s & 0x7fffffffu) : ~s); }

__device__ __forceinline__ double slot_area(const uint32_t *__restrict__ bounds, int slot) {
    const uint32_t *b = bounds + (size_t)slot * 6;
    return rtcost::half_area(sortable2f(b[3]) - sortable2f(b[0]), sortable2f(b[4]) - sortable2f(b[1]), sortable2f(b[5]) - sortable2f(b[2]));
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;   // lane 0 holds the wave's sum
}

// Thread i takes bounds slot i when that slot is an inner node (the refit's child table says which), and leaf i of the refit's leaf table: both tables
// exist already, nNodes >= nLeaves, and every node is counted once.  The root's half-area comes from slot 0 in every thread (a uniform load).  Integer
// sums: wave by shuffles, block through 2 x 4 words of LDS, then one 64-bit atomicAdd per sum and block -- in whatever order, the same bits.
// acc: [inner sum, leaf sum, the root's six keys as three 64-bit words] -- the record the host copies out.
__global__ void __launch_bounds__(256) k_mesh_quality(const uint32_t *__restrict__ bounds, const rtl::RefitKids *__restrict__ kids, int nNodes,
                                                      const rtl::RefitLeaf *__restrict__ leaves, int nLeaves, unsigned long long *__restrict__ acc) {
    __shared__ unsigned long long part[2][4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 6) reinterpret_cast<uint32_t *>(acc + 2)[i] = bounds[i];
    const double A = slot_area(bounds, 0);
    if (A == 0.0) return;   // degenerate (uniform): the sums stay zero
    const int e = rtcost::root_exp(A);
    unsigned long long qi = 0ull, ql = 0ull;
    if (i < nNodes && kids[i].l >= 0) qi = rtcost::quantise(slot_area(bounds, i), e);
    if (i < nLeaves) { const rtl::RefitLeaf lf = leaves[i]; ql = rtcost::quantise(slot_area(bounds, lf.slot), e) * (unsigned long long)lf.count; }
    qi = wave_sum(qi);
    ql = wave_sum(ql);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { part[0][wave] = qi; part[1][wave] = ql; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned long long s = (part[threadIdx.x][0] + part[threadIdx.x][1]) + (part[threadIdx.x][2] + part[threadIdx.x][3]);
        if (s) atomicAdd(acc + threadIdx.x, s);
    }
}

}  // namespace

namespace rtl {

// Clears the accumulators on `st` itself, measures, and copies the record to the pinned slot: three stream operations, no host wait.
hipError_t quality_launch(hipStream_t st, const uint32_t *bounds, const RefitKids *kids, int nNodes, const RefitLeaf *leaves, int nLeaves, unsigned long long *acc,
                          void *pinned) {
    hipError_t e = hipMemsetAsync(acc, 0, kQualityRecordBytes, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mesh_quality, dim3((unsigned)std::max(1, (nNodes + 255) / 256)), dim3(256), 0, st, bounds, kids, nNodes, leaves, nLeaves, acc);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(pinned, acc, kQualityRecordBytes, hipMemcpyDeviceToHost, st);
}

}  // namespace rtl
