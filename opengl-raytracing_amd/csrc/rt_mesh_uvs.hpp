// rt_mesh_uvs.hpp -- vertex UVs and the albedo texture of the dynamic mesh, once, for the host definitions (rt_uv_rows, rt_hit_uvs and
// rt_sample_texture, rt_mesh_uvs.cpp), the device kernels (rt_mesh_corner.hip) and the frames (hitAlbedoTex, rt_device_shade.hpp).
//
// A vertex UV is two floats.  At a hit the three corner UVs are blended component by component under rt_mesh_corner.hpp's rule.
// A texture is W x H RGBA8 texels, row 0 at v = 0, decoded through a 256-entry float table (c / 255, or the sRGB curve: one code path for both) and
// sampled NEAREST or LINEAR under REPEAT or CLAMP; a LINEAR channel whose four decoded values are bit-equal hands that value back bit for bit -- the
// four weights do not sum to 1 in float32, and a texture of one value must sample as that value.  fp32, every product and sum rounded on its own,
// nothing fused (the one exception is unorm8's Newton step, which is texel_unorm8's).
#pragma once
#include <cstddef>
#include <cstdint>

#include "rt_mesh_corner.hpp"

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_UV_HD __host__ __device__
#else
#define RT_UV_HD
#endif

#pragma clang fp contract(off)

namespace rtuv {

// the flag bits of include/rt_mi355.h (RT_TEX_*), and the largest edge
constexpr uint32_t kNearest = 1u, kClamp = 2u, kSrgb = 4u, kAllFlags = 7u;
constexpr int kMaxEdge = 16384;

// What a sampler needs: the texels (W x H RGBA8, 4-byte aligned on the device), the decode table and the flags.  The frames carry one in DevFrame.
struct Texture {
    const void *texels = nullptr;
    const float *table = nullptr;
    int W = 0, H = 0;
    uint32_t flags = 0;
};

// c / 255.0f without the division: texel_unorm8 (rt_device_shade.hpp), operation for operation
RT_UV_HD inline float unorm8(uint8_t code) {
    const float c = (float)code, r = 1.0f / 255.0f;
    const float q = c * r;
    const float e = __builtin_fmaf(-255.0f, q, c);
    return __builtin_fmaf(e, r, q);
}

// the blend of a row's three corner UVs at barycentrics (a, b)
RT_UV_HD inline void blend_uvs(const float *c0, const float *c1, const float *c2, float a, float b, float *out) { rtcorner::blend_corners<2>(c0, c1, c2, a, b, out); }

// One axis of a lookup: the coordinate u on an edge of N texels.  i0, i1: the two texels (equal under NEAREST), f: the weight of i1.
RT_UV_HD inline int wrap_index(int i, int N, bool clamp) {
    if (clamp) return i < 0 ? 0 : (i > N - 1 ? N - 1 : i);
    return ((i % N) + N) % N;
}
RT_UV_HD inline void axis(float u, int N, bool nearest, bool clamp, int &i0, int &i1, float &f) {
    if (!rtcorner::finite_bits(u)) u = 0.0f;
    float s;
    if (clamp) { s = u < 0.0f ? 0.0f : u; s = s > 1.0f ? 1.0f : s; }
    else s = u - __builtin_floorf(u);
    if (nearest) {
        i0 = i1 = wrap_index((int)__builtin_floorf(s * (float)N), N, clamp);
        f = 0.0f;
        return;
    }
    const float x = s * (float)N - 0.5f;
    const float fl = __builtin_floorf(x);
    f = x - fl;
    const int i = (int)fl;
    i0 = wrap_index(i, N, clamp);
    i1 = wrap_index(i + 1, N, clamp);
}

// texel (i, j) of the texture as its four bytes, r lowest
RT_UV_HD inline uint32_t texel_at(const Texture &t, int i, int j) {
    const size_t at = (size_t)j * (size_t)t.W + (size_t)i;
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<const uint32_t *>(t.texels)[at];
#else
    const uint8_t *p = static_cast<const uint8_t *>(t.texels) + at * 4;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
#endif
}

// The sample at (u, v): decoded RGB, alpha ignored.  Every index is inside the texture whatever (u, v) is.
RT_UV_HD inline void sample(const Texture &t, float u, float v, float *out) {
    const bool nearest = (t.flags & kNearest) != 0u, clamp = (t.flags & kClamp) != 0u;
    int i0, i1, j0, j1;
    float a, b;
    axis(u, t.W, nearest, clamp, i0, i1, a);
    axis(v, t.H, nearest, clamp, j0, j1, b);
    if (nearest) {
        const uint32_t c = texel_at(t, i0, j0);
        for (int k = 0; k < 3; ++k) out[k] = t.table[(c >> (8 * k)) & 255u];
        return;
    }
    const uint32_t c00 = texel_at(t, i0, j0), c10 = texel_at(t, i1, j0), c01 = texel_at(t, i0, j1), c11 = texel_at(t, i1, j1);
    const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    for (int k = 0; k < 3; ++k) {
        const float t00 = t.table[(c00 >> (8 * k)) & 255u], t10 = t.table[(c10 >> (8 * k)) & 255u];
        const float t01 = t.table[(c01 >> (8 * k)) & 255u], t11 = t.table[(c11 >> (8 * k)) & 255u];
        const bool flat = rtcorner::same_bits(t00, t10) && rtcorner::same_bits(t00, t01) && rtcorner::same_bits(t00, t11);
        const float m = ((t00 * w00 + t10 * w10) + t01 * w01) + t11 * w11;
        out[k] = flat ? t00 : m;
    }
}

}  // namespace rtuv
