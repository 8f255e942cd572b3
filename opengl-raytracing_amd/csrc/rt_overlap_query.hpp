// rt_overlap_query.hpp -- the launch of the overlap queries (rt_overlap_query.hip), for rt_api_query.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_frame.hpp"

// The queries and outputs of one box or triangle query.  Query i is q[i * qs ..] (stride in floats): a box's lo.xyz, hi.xyz or a triangle's p0.xyz,
// p1.xyz, p2.xyz.  prims (may be null: the counts alone): slot i starts at offsets[i] and holds offsets[i + 1] - offsets[i] entries, or, without
// offsets, starts at i * cap and holds cap.  counts and visits may be null.  The kernel takes the struct as it is.
struct OverlapQuery {
    const float *q;
    int qs;
    uint32_t n;
    const int32_t *offsets;
    int cap;
    int32_t *prims;
    int32_t *counts;
    int32_t *visits;
};

enum OverlapShape { RT_OVERLAP_BOX, RT_OVERLAP_TRI };

// Enqueues the query on `st`: one thread writes the scene (root box included) into dFrame, then one lane per query walks sc.wnodes / sc.tris, the right
// child before the left, entering exactly the nodes whose boxes overlap its box -- a triangle's is the box of its three points.  Returns the launch's
// error, hipSuccess when enqueued.
hipError_t rt_overlap_launch(OverlapShape shape, hipStream_t st, int treeDepth, rtd::DevFrame *dFrame, const rtd::DevScene &sc, const OverlapQuery &q);
