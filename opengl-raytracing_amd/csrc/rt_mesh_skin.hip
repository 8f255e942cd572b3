// rt_mesh_skin.hip -- linear-blend skinning of the dynamic mesh: positions := sum over four influences of w * (bone * rest), written
// where rebuild, refit and the bound raster draws read them.  A translation unit of its own for the reason rt_mesh_parts.hip is one: the code objects
// of the other mesh files stay the machine code they were.  rt_mesh.hip owns the arrays.
//
// One thread per vertex.  It reads 12 B of rest position, the vertex's four 16-bit bone indices as one 8-byte load, its four weights as one 16-byte
// load and four 64-byte entries of the bone table, each as four 16-byte loads of which the xyz lanes are used, as k_parts_gather reads a matrix; it
// writes 12 B.  All sixteen matrix loads are issued before the first use: the upload has checked every index, whatever its weight, so an influence
// that is skipped is loaded like the others and dropped by a select, and a wave never waits for one matrix after another.  Neighbouring vertices
// mostly share bones, so a wave's matrix loads fall on few cache lines; the table (256 KiB at 4096 bones) sits in L2.  No LDS, no atomics, no scratch.
//
// The arithmetic is rt_skin_positions' (rt_host.cpp), operation for operation: nothing is fused, the first unskipped term initialises the sum, and a
// vertex without one keeps its rest position's bits.
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/rt_mi355.h"
#include "rt_mesh.hpp"

#pragma clang fp contract(off)

namespace {

__global__ void k_mesh_skin(const float *__restrict__ rest, const uint2 *__restrict__ idx4, const float4 *__restrict__ w4, const float4 *__restrict__ bones,
                            int nVerts, float *__restrict__ pos) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nVerts) return;
    const float *p = rest + (size_t)i * 3;
    const float x = p[0], y = p[1], z = p[2];
    const uint2 id = idx4[i];
    const float4 wv = w4[i];
    const uint32_t bone[RT_SKIN_INFLUENCES] = {id.x & 0xffffu, id.x >> 16, id.y & 0xffffu, id.y >> 16};
    const float w[RT_SKIN_INFLUENCES] = {wv.x, wv.y, wv.z, wv.w};
    float4 c[RT_SKIN_INFLUENCES][4];
    for (int k = 0; k < RT_SKIN_INFLUENCES; ++k) {
        const float4 *B = bones + (size_t)bone[k] * 4;
        c[k][0] = B[0]; c[k][1] = B[1]; c[k][2] = B[2]; c[k][3] = B[3];
    }
    float ax = x, ay = y, az = z;   // no influence: the rest position, bit for bit
    bool any = false;
    for (int k = 0; k < RT_SKIN_INFLUENCES; ++k) {
        const bool use = w[k] != 0.0f;   // +0 and -0 are skipped; the upload has refused NaN
        const float tx = w[k] * ((c[k][0].x * x + c[k][1].x * y) + (c[k][2].x * z + c[k][3].x * 1.0f));
        const float ty = w[k] * ((c[k][0].y * x + c[k][1].y * y) + (c[k][2].y * z + c[k][3].y * 1.0f));
        const float tz = w[k] * ((c[k][0].z * x + c[k][1].z * y) + (c[k][2].z * z + c[k][3].z * 1.0f));
        const float sx = any ? ax + tx : tx, sy = any ? ay + ty : ty, sz = any ? az + tz : tz;
        ax = use ? sx : ax; ay = use ? sy : ay; az = use ? sz : az;
        any = any || use;
    }
    float *o = pos + (size_t)i * 3;
    o[0] = ax; o[1] = ay; o[2] = az;
}

inline unsigned blocks_for(size_t n) { return (unsigned)std::max<size_t>(1, (n + 255) / 256); }

}  // namespace

namespace rtl {

void skin_launch(hipStream_t st, const float *rest, const uint16_t *idx4, const float *w4, const float *bones, int nVerts, float *pos) {
    hipLaunchKernelGGL(k_mesh_skin, dim3(blocks_for((size_t)nVerts)), dim3(256), 0, st, rest, reinterpret_cast<const uint2 *>(idx4),
                       reinterpret_cast<const float4 *>(w4), reinterpret_cast<const float4 *>(bones), nVerts, pos);
}

}  // namespace rtl
