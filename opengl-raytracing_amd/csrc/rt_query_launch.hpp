// rt_query_launch.hpp -- what the launches of the mesh queries share, for rt_nearest.hip, rt_nearest_multi.hip and rt_overlap_query.hip:
// the prep launch, the lane stack's place in LDS, the stack's size and the launch of a walk kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rt_frame.hpp"

// Enqueues one thread that writes the scene (root box included) into the query's frame descriptor: the walks read it through scalar loads
// (rt_query_prep.hip)
void rt_query_prep(hipStream_t st, rtd::DevFrame *dFrame, const rtd::DevScene &sc);

// Entries per lane of a walk's stack: the tree's depth (depth first, at most one deferred sibling per level), at most 64
inline int rt_query_stack_entries(int treeDepth) { return std::min(std::max(treeDepth, 1), 64); }

// One thread per query, `threads` per block, ldsBytes of dynamic LDS: opted in to where they exceed 64 KiB
template <class Kernel, class Query>
void rt_query_launch(Kernel *kernel, hipStream_t st, unsigned threads, size_t ldsBytes, rtd::DevFrame *dFrame, const Query &q, int stackEntries) {
    if (ldsBytes > ((size_t)64 << 10)) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes);
    hipLaunchKernelGGL(kernel, dim3((q.n + threads - 1u) / threads), dim3(threads), ldsBytes, st, (const rtd::DevFrame *)dFrame, q, stackEntries);
}

namespace rtd {

// A lane's stack of T in LDS, from `base`, the first entry of the block's stacks: laid out [entry][lane] per wave, entry e at [e * 64] -- one wave's
// push or pop is one conflict-free write or read
template <class T>
RT_DEV T *lane_stack(T *base, int stackEntries) {
    return base + (threadIdx.x >> 6) * (stackEntries * 64) + (threadIdx.x & 63);
}

}  // namespace rtd
