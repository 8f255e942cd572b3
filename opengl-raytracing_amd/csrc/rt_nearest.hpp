// rt_nearest.hpp -- the launch of the nearest-point query (rt_nearest.hip), for rt_api_query.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_frame.hpp"

// The points and outputs of one nearest-point query.  Point i is p[i * ps] (stride in floats).  md (may be null): the per-point distance limit, < 0 an
// empty slot.  hits: n records; closest (3 floats per point) and visits may be null.  The kernel takes the struct as it is.
struct NearestQuery {
    const float *p;
    const float *md;
    int ps;
    uint32_t n;
    float4 *hits;
    float *closest;
    int32_t *visits;
};

// Enqueues the query on `st`: one thread writes the scene (root box included) into dFrame, then one lane per point walks sc.wnodes / sc.tris, culling
// against its best.  farFirst: the farther child first (RT_NEAREST_FAR_FIRST, for the tests: the answer does not depend on it, `visits` does).
// Returns the launch's error, hipSuccess when enqueued.
hipError_t rt_nearest_launch(hipStream_t st, int treeDepth, rtd::DevFrame *dFrame, const rtd::DevScene &sc, bool farFirst, const NearestQuery &q);
