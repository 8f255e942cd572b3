// rt_overlap_query.hpp -- the launches of the overlap queries (rt_overlap_query.hip), for rt_api_query.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_frame.hpp"
#include "rt_hull_corners.hpp"

// The queries and outputs of one box, triangle or hull query.  Query i is q[i * qs ..] (stride in floats): a box's lo.xyz, hi.xyz, a triangle's p0.xyz,
// p1.xyz, p2.xyz or a hull's c0.xyz .. c7.xyz.  prims (may be null: the counts alone): slot i starts at offsets[i] and holds offsets[i + 1] - offsets[i] entries, or, without
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

enum OverlapShape { RT_OVERLAP_BOX, RT_OVERLAP_TRI, RT_OVERLAP_HULL };

// Enqueues the query on `st`: one thread writes the scene (root box included) into dFrame, then one lane per query walks sc.wnodes / sc.tris, the right
// child before the left, entering exactly the nodes that pass its shape's node test: their boxes overlap its box -- a triangle's is the box of its
// three points, a hull's of its eight corners -- and, for a hull, none of its six face normals parts them from it.  Returns the launch's error,
// hipSuccess when enqueued.  prepared: dFrame already holds the scene, written by an earlier launch on `st` (rt_rect_frusta_launch): no prep launch.
hipError_t rt_overlap_launch(OverlapShape shape, hipStream_t st, int treeDepth, rtd::DevFrame *dFrame, const rtd::DevScene &sc, const OverlapQuery &q,
                             bool prepared = false);

// Enqueues on `st` the prep launch and the kernel that writes rt_rect_frusta's 24 floats per rect into corners: one lane per rect, the root box read
// from dFrame, where the prep launch has left it.  Returns the launch's error.
hipError_t rt_rect_frusta_launch(hipStream_t st, rtd::DevFrame *dFrame, const rtd::DevScene &sc, const rthull::RectCam &cam, const float *rects, int stride, uint32_t n,
                                 float tNear, float tFar, float *corners);
