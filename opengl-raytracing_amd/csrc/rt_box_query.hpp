// rt_box_query.hpp -- the launch of the box query (rt_box_query.hip), for rt_api_query.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_frame.hpp"

// The boxes and outputs of one box query.  Box i is b[i * bs .. + 5] (lo.xyz, hi.xyz; stride in floats).  prims (may be null: the counts alone): slot i
// starts at offsets[i] and holds offsets[i + 1] - offsets[i] entries, or, without offsets, starts at i * cap and holds cap.  counts and visits may be
// null.  The kernel takes the struct as it is.
struct BoxQuery {
    const float *b;
    int bs;
    uint32_t n;
    const int32_t *offsets;
    int cap;
    int32_t *prims;
    int32_t *counts;
    int32_t *visits;
};

// Enqueues the query on `st`: one thread writes the scene (root box included) into dFrame, then one lane per box walks sc.wnodes / sc.tris, the right
// child before the left, entering exactly the nodes whose boxes overlap its box.  Returns the launch's error, hipSuccess when enqueued.
hipError_t rt_box_query_launch(hipStream_t st, int treeDepth, rtd::DevFrame *dFrame, const rtd::DevScene &sc, const BoxQuery &q);
