// rt_multi_hit.hpp -- the launch of the multi-hit query (rt_multi_hit.hip), for rt_api_query.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_frame.hpp"

// The rays and outputs of one multi-hit query.  Ray i is o[i * os] / d[i * ds] (strides in floats), or -- xy non-null -- the primary ray of pixel
// (xy[2i], xy[2i + 1]) under the uniform block *cam, which the launch copies into the query's frame descriptor.  tm (may be null): the per-ray limit,
// < 0 an empty slot.  hits: n * K records (null with K == 0); counts may be null.  The kernel takes the struct as it is.
struct MultiHitQuery {
    const float *o, *d;
    const int32_t *xy;
    const RtUniforms *cam;   // a host address: read by the launch, never on the device
    const float *tm;
    int os, ds;
    uint32_t n;
    int K;
    float eps, inf;
    float4 *hits;
    int32_t *counts;
};

// Enqueues the query on `st`: one block writes the scene (root box included) and, for pixel rays, the uniform block into dFrame, then one lane per ray
// walks sc.wnodes / sc.tris.  hasBVH false: every ray is answered as an empty slot.  Returns the launch's error, hipSuccess when enqueued.
hipError_t rt_multi_hit_launch(hipStream_t st, int treeDepth, rtd::DevFrame *dFrame, const rtd::DevScene &sc, bool hasBVH, const MultiHitQuery &q);
