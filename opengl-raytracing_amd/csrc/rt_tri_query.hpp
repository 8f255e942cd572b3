// rt_tri_query.hpp -- the launch of the triangle query (rt_tri_query.hip), for rt_api_query.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_frame.hpp"

// The query triangles and outputs of one triangle query.  Triangle i is t[i * ts .. + 8] (p0.xyz, p1.xyz, p2.xyz; stride in floats).  prims (may be
// null: the counts alone): slot i starts at offsets[i] and holds offsets[i + 1] - offsets[i] entries, or, without offsets, starts at i * cap and holds
// cap.  counts and visits may be null.  The kernel takes the struct as it is.
struct TriQuery {
    const float *t;
    int ts;
    uint32_t n;
    const int32_t *offsets;
    int cap;
    int32_t *prims;
    int32_t *counts;
    int32_t *visits;
};

// Enqueues the query on `st`: one thread writes the scene (root box included) into dFrame, then one lane per query triangle walks sc.wnodes / sc.tris,
// the right child before the left, entering exactly the nodes whose boxes overlap the box of its three points.  Returns the launch's error, hipSuccess
// when enqueued.
hipError_t rt_tri_query_launch(hipStream_t st, int treeDepth, rtd::DevFrame *dFrame, const rtd::DevScene &sc, const TriQuery &q);
