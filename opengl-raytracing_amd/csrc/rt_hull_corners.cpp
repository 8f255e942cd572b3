// rt_hull_corners.cpp -- rt_box_corners and rt_rect_frusta (include/rt_mi355.h): the hulls of the hull query made from boxes under model
// matrices and from rectangles of the frame.  Host only, no context, no GPU; every float operation is rt_hull_corners.hpp's, the text the device
// compiles too (rt_pick_rects' kernel).
#include <cstddef>
#include <cstdint>

#include "../../include/rt_mi355.h"
#include "rt_hull_corners.hpp"

using namespace rthull;

extern "C" int rt_box_corners(const float *boxes, int stride, int n, const float *M16s, int matStride, float *corners24) {
    if (n < 0 || stride < 6 || (matStride != 0 && matStride != 16)) return RT_ERR_INVALID;
    if (n > 0 && (!boxes || !corners24)) return RT_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        box_corners(boxes + (size_t)i * stride, M16s ? M16s + (size_t)i * matStride : nullptr, corners24 + (size_t)i * 24);
    return RT_OK;
}

extern "C" int rt_rect_frusta(const RtUniforms *u, const float *rootMin, const float *rootMax, const float *rects, int stride, int n, float tNear, float tFar,
                              float *corners24) {
    if (n < 0 || !rect_args_ok(u, stride, tNear, tFar) || !rootMin || !rootMax) return RT_ERR_INVALID;
    if (n > 0 && (!rects || !corners24)) return RT_ERR_INVALID;
    const RectCam cam = rect_cam(*u);
    const float far = rect_far(cam, ld(rootMin), ld(rootMax), tNear, tFar);
    for (int i = 0; i < n; ++i) rect_frustum(cam, rects + (size_t)i * stride, tNear, far, corners24 + (size_t)i * 24);
    return RT_OK;
}
