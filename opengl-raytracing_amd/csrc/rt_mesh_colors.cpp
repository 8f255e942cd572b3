// rt_mesh_colors.cpp -- per-vertex colours of the dynamic mesh on host arrays: the definitions the device's colour rows
// (k_corner_rows<ColorAttr>), rt_mesh_hit_colors and the frames' albedo are held to.  Plain C++: no HIP header, links on its own (tests/colors_sanitize.cpp).
// The arithmetic is rt_mesh_colors.hpp's, shared with the device.
#include <cstdint>
#include <cstring>

#include "../../include/rt_mi355.h"
#include "rt_mesh_colors.hpp"

#pragma clang fp contract(off)

// The colour of hits: the corner colours of the hit row's input triangle blended at the hit's barycentrics.  A prim outside [0, nTris): zeros, nothing
// read.  tris12 is not read: the barycentrics come with the hit.
int rt_hit_colors(const float *tris12, int nTris, const int32_t *order, const uint32_t *indices, const float *colors, int nVerts, const RtHit *hits, int n,
                  float *out3) {
    (void)tris12;
    if (!order || !indices || !colors || nTris <= 0 || nVerts <= 0 || n < 0 || (n > 0 && (!hits || !out3))) return RT_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        const int p = hits[i].prim;
        if (p < 0 || p >= nTris) continue;
        const int k = order[p];
        if (k < 0 || k >= nTris) return RT_ERR_INVALID;
        for (int c = 0; c < 3; ++c)
            if (indices[3 * (size_t)k + c] >= (uint32_t)nVerts) return RT_ERR_INVALID;
    }
    for (int i = 0; i < n; ++i) {
        float out[3] = {0.0f, 0.0f, 0.0f};
        const int p = hits[i].prim;
        if (p >= 0 && p < nTris) {
            const uint32_t *ix = indices + 3 * (size_t)order[p];
            rtcolor::blend_colors(colors + (size_t)ix[0] * 3, colors + (size_t)ix[1] * 3, colors + (size_t)ix[2] * 3, hits[i].u, hits[i].v, out);
        }
        std::memcpy(out3 + (size_t)i * 3, out, sizeof out);
    }
    return RT_OK;
}

// The device row array: row i holds the corner colours of input triangle order[i], three (r, g, b, 0).
int rt_color_rows(const int32_t *order, const uint32_t *indices, const float *colors, int nTris, int nVerts, float *rows12) {
    if (!order || !indices || !colors || !rows12 || nTris <= 0 || nVerts <= 0) return RT_ERR_INVALID;
    for (int r = 0; r < nTris; ++r) {
        if (order[r] < 0 || order[r] >= nTris) return RT_ERR_INVALID;
        for (int c = 0; c < 3; ++c)
            if (indices[3 * (size_t)r + c] >= (uint32_t)nVerts) return RT_ERR_INVALID;
    }
    for (int r = 0; r < nTris; ++r) {
        const uint32_t *ix = indices + 3 * (size_t)order[r];
        float *o = rows12 + (size_t)r * 12;
        for (int c = 0; c < 3; ++c) {
            std::memcpy(o + 4 * c, colors + (size_t)ix[c] * 3, 12);
            o[4 * c + 3] = 0.0f;
        }
    }
    return RT_OK;
}
