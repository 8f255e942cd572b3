// rt_nearest_multi_block.hpp -- the block size of the proximity query's launch (rt_nearest_multi.hip), in plain C++: the launch calls
// it, rt_debug_nearest_multi_block (rt_nearest_multi.cpp) shows it to the tests without a GPU.
#pragma once
#include <cstddef>

constexpr int RT_NEAREST_MULTI_STACK_MAX = 64;                 // the stack's ceiling, entries per lane
constexpr size_t RT_NEAREST_MULTI_LDS_MAX = (size_t)160 << 10;   // gfx950: 160 KiB of LDS per workgroup

// LDS of one block: per thread the stack's entries and the K-buffer's slots, 8 bytes each
constexpr size_t rt_nearest_multi_lds(int threads, int stackEntries, int maxHits) { return (size_t)threads * 8u * (size_t)(stackEntries + maxHits); }

// 256 threads where their LDS fits a workgroup's, else 128, else 64.  At the ceilings (64 entries, 32 slots) 128 threads take 96 KiB: every legal pair fits.
constexpr int rt_nearest_multi_block(int stackEntries, int maxHits) {
    for (int threads = 256; threads > 64; threads >>= 1)
        if (rt_nearest_multi_lds(threads, stackEntries, maxHits) <= RT_NEAREST_MULTI_LDS_MAX) return threads;
    return 64;
}
static_assert(rt_nearest_multi_lds(rt_nearest_multi_block(RT_NEAREST_MULTI_STACK_MAX, 32), RT_NEAREST_MULTI_STACK_MAX, 32) <= RT_NEAREST_MULTI_LDS_MAX, "every legal launch fits");
