// rt_nearest_multi.hpp -- the launch of the proximity query (rt_nearest_multi.hip), for rt_api_query.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_frame.hpp"

// The points and outputs of one proximity query.  Point i is p[i * ps] (stride in floats).  md (may be null): the per-point distance limit, < 0 an
// empty slot.  K: records per point, 0 .. RT_NEAREST_MULTI_MAX.  hits: n * K records (null when K == 0); closest: 3 floats per record; counts, closest
// and visits may be null, counts not when K == 0.  The kernel takes the struct as it is.
struct NearestMultiQuery {
    const float *p;
    const float *md;
    int ps;
    uint32_t n;
    int K;
    float4 *hits;
    int32_t *counts;
    float *closest;
    int32_t *visits;
};

// Enqueues the query on `st`: one thread writes the scene (root box included) into dFrame, then one lane per point walks sc.wnodes / sc.tris, culling
// against the limit when counts are asked for (or K == 0) and against its K-th best otherwise.  farFirst: the farther child first
// (RT_NEAREST_FAR_FIRST, for the tests: the answer does not depend on it, `visits` does).  Returns the launch's error, hipSuccess when enqueued.
hipError_t rt_nearest_multi_launch(hipStream_t st, int treeDepth, rtd::DevFrame *dFrame, const rtd::DevScene &sc, bool farFirst, const NearestMultiQuery &q);
