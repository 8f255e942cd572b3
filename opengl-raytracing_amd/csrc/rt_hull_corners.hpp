// rt_hull_corners.hpp -- the float operations of the corner makers of the hull query: the eight corners of a box under a model
// matrix (rt_box_corners) and of the frustum behind a rectangle of the frame (rt_rect_frusta, rt_pick_rects).  One text for both sides, as
// rt_nearest_math.hpp, whose primitives these functions are written in: device functions for the rect kernel of rt_overlap_query.hip, inline host
// functions for rt_hull_corners.cpp.  Nothing contracted.
#pragma once
#include "rt_nearest_math.hpp"

namespace rthull {

using namespace rtnear;

// What the frustum of a rect reads of the frame's uniforms: the camera alone
struct RectCam {
    float camPos[3], camRight[3], camUp[3], camFwd[3];
    float resX, resY, jx, jy, sx, sy;   // jx, jy: the jitter in force (0 with enableJitter != 1); sx = tanHalfFov * aspect, sy = tanHalfFov
};

// (host, both sides) the camera of the uniforms u (an RtUniforms); only these fields are read
template <class U>
inline RectCam rect_cam(const U &u) {
    RectCam c;
    for (int a = 0; a < 3; ++a) { c.camPos[a] = u.camPos[a]; c.camRight[a] = u.camRight[a]; c.camUp[a] = u.camUp[a]; c.camFwd[a] = u.camFwd[a]; }
    c.resX = u.resolution[0]; c.resY = u.resolution[1];
    c.jx = (u.enableJitter == 1) ? u.jitter[0] : 0.0f; c.jy = (u.enableJitter == 1) ? u.jitter[1] : 0.0f;
    c.sx = u.tanHalfFov * u.aspect; c.sy = u.tanHalfFov;
    return c;
}
// (host, both sides) what rt_rect_frusta and rt_pick_rects refuse of the camera and the depths
template <class U>
inline bool rect_args_ok(const U *u, int stride, float tNear, float tFar) {
    return u && u->resolution[0] > 0.0f && u->resolution[1] > 0.0f && tNear >= 0.0f && tFar == tFar && stride >= 4;
}

RT_Q void empty24(float *o) {
    const float nan = __builtin_nanf("");
    for (int k = 0; k < 24; ++k) o[k] = nan;
}

// Corner k of the box (lo.xyz, hi.xyz) under M (column-major 4 x 4, null: the identity, which copies): the point (k&1 ? hi.x : lo.x, k&2 ? hi.y : lo.y,
// k&4 ? hi.z : lo.z) in rt_gather_triangles' expression.  A NaN component or lo > hi: 24 NaNs
RT_Q void box_corners(const float *box, const float *M, float *o) {
    if (!(box[0] <= box[3] && box[1] <= box[4] && box[2] <= box[5])) { empty24(o); return; }
    for (int k = 0; k < 8; ++k) {
        const float p0 = box[(k & 1) ? 3 : 0], p1 = box[(k & 2) ? 4 : 1], p2 = box[(k & 4) ? 5 : 2];
        float *c = o + k * 3;
        if (!M) { c[0] = p0; c[1] = p1; c[2] = p2; continue; }
        for (int a = 0; a < 3; ++a) c[a] = (M[a] * p0 + M[4 + a] * p1) + (M[8 + a] * p2 + M[12 + a] * 1.0f);
    }
}

// "To the far side of the scene": the greatest depth along camFwd of the root box's corners, widened by 2^-10 of itself so that rounding cannot cut
// off the farthest vertex, and no nearer than tNear
RT_Q float scene_far(const RectCam &cam, V rootMin, V rootMax, float tNear) {
    const V fwd = ld(cam.camFwd), pos = ld(cam.camPos);
    float s = dot(fwd, sub(rootMin, pos));
    s = fmaxr(s, dot(fwd, sub(V{rootMax.x, rootMin.y, rootMin.z}, pos)));
    s = fmaxr(s, dot(fwd, sub(V{rootMin.x, rootMax.y, rootMin.z}, pos)));
    s = fmaxr(s, dot(fwd, sub(V{rootMax.x, rootMax.y, rootMin.z}, pos)));
    s = fmaxr(s, dot(fwd, sub(V{rootMin.x, rootMin.y, rootMax.z}, pos)));
    s = fmaxr(s, dot(fwd, sub(V{rootMax.x, rootMin.y, rootMax.z}, pos)));
    s = fmaxr(s, dot(fwd, sub(V{rootMin.x, rootMax.y, rootMax.z}, pos)));
    s = fmaxr(s, dot(fwd, sub(rootMax, pos)));
    return fmaxr(fmar(s < 0.0f ? -s : s, 0.0009765625f, s), tNear);
}

// The far depth of a call: tFar where it is given (never nearer than tNear), else the scene's
RT_Q float rect_far(const RectCam &cam, V rootMin, V rootMax, float tNear, float tFar) {
    return tFar < 0.0f ? scene_far(cam, rootMin, rootMax, tNear) : fmaxr(tFar, tNear);
}

// The frustum behind the rect (x0, y0, x1, y1) in pixel-corner coordinates, row 0 at the bottom, between the depths tNear and far along camFwd.  The
// direction through the frame point (fx, fy) is primaryDirJ's before its normalize -- D[a] = (camFwd[a] + (nx * camRight[a]) * sx) + (ny * camUp[a]) * sy,
// nx = ((fx + jx) / resX) * 2 - 1 -- whose depth along camFwd is 1, so near and far faces are planes of constant depth.  Corner k is
// fma(D(k&1 ? x1 : x0, k&2 ? y1 : y0)[a], k&4 ? far : tNear, camPos[a]).  A NaN, x1 < x0 or y1 < y0: 24 NaNs
RT_Q void rect_frustum(const RectCam &cam, const float *rect, float tNear, float far, float *o) {
    if (!(rect[0] <= rect[2] && rect[1] <= rect[3])) { empty24(o); return; }
    for (int k = 0; k < 8; ++k) {
        const float fx = rect[(k & 1) ? 2 : 0], fy = rect[(k & 2) ? 3 : 1], t = (k & 4) ? far : tNear;
        const float uvx = (fx + cam.jx) / cam.resX, uvy = (fy + cam.jy) / cam.resY;
        const float nx = uvx * 2.0f - 1.0f, ny = uvy * 2.0f - 1.0f;
        for (int a = 0; a < 3; ++a) {
            const float d = (cam.camFwd[a] + (nx * cam.camRight[a]) * cam.sx) + (ny * cam.camUp[a]) * cam.sy;
            o[k * 3 + a] = fmar(d, t, cam.camPos[a]);
        }
    }
}

}  // namespace rthull
