// oracle/orc_dress.h -- TEST INFRASTRUCTURE ONLY (parity oracle). Never linked into the product.
//
// EXTENSION, not in the reference: the "dress" of the dynamic mesh -- smooth corner normals, corner colours, corner UVs with an albedo texture and the
// previous pose -- restated from DESIGN.md 14.12-14.15 and the numpy definitions tests/{normals,colors,uvs,motion}_ref.py, for the dressed mode of
// rt_oracle.cpp.  Nothing here comes from the product's sources: the rules are written out again so that a frame of the device can be compared with an
// independent answer.  Float model (orc_math.h): every product and sum is rounded on its own; a fused multiply-add stands only inside dot and cross.
//
// Rows lie beside the rows of the triangle array (tris12: [v0 -][e1 -][e2 -]), row for row:
//   nrmRows  12 floats: the three corner normals (x, y, z, -)          colRows  12 floats: the three corner colours (r, g, b, 0)
//   uvRows    8 floats: (u0, v0, u1, v1), (u2, v2, 0, 0)               prevTris 12 floats: the row the same input triangle had in the previous pose
// (a, b) are the barycentrics of a hit on its row: triHit's u and v.
#pragma once
#include <algorithm>
#include <cstddef>

#include "orc_math.h"

extern "C" {
struct OrcDress {
    int nTris;
    const float *nrmRows;
    const float *colRows;
    const float *uvRows;
    const uint8_t *texels;      // texH x texW x 4, row 0 at v = 0
    int texW, texH, texFlags;   // 1 NEAREST (else LINEAR), 2 CLAMP (else REPEAT); 4 SRGB only names the table the caller passes
    const float *table;         // 256 decoded values, read only with texels
    const float *prevTris;
};
}

namespace orc {

enum { kTexNearest = 1, kTexClamp = 2 };

static inline bool sameBits(float p, float q) { return f2u(p) == f2u(q); }
static inline bool finiteBits(float p) { return (f2u(p) & 0x7f800000u) != 0x7f800000u; }
static inline bool dressHasTexture(const OrcDress &d) { return d.uvRows && d.texels && d.table && d.texW > 0 && d.texH > 0; }
static inline bool dressHasAlbedo(const OrcDress &d) { return d.colRows || dressHasTexture(d); }

// DESIGN.md 14.13.  Nine bit-equal corner floats give n0 (unless it is zero); otherwise the blend, normalised, when it has a direction; in every
// remaining case the face normal normalize(cross(e1, e2)), the reference's.
static inline vec3 dressFaceNormal(const float *row) { return normalize(cross(v3(row[4], row[5], row[6]), v3(row[8], row[9], row[10]))); }
static inline vec3 dressNormal(const float *row, const float *nrow, float a, float b) {
    const float *n0 = nrow, *n1 = nrow + 4, *n2 = nrow + 8;
    bool same = true;
    for (int c = 0; c < 3; ++c) same = same && sameBits(n0[c], n1[c]) && sameBits(n0[c], n2[c]);
    if (same) {
        if (n0[0] == 0.0f && n0[1] == 0.0f && n0[2] == 0.0f) return dressFaceNormal(row);
        return v3(n0[0], n0[1], n0[2]);
    }
    const float w = (1.0f - a) - b;
    float m[3];
    for (int c = 0; c < 3; ++c) m[c] = (n0[c] * w + n1[c] * a) + n2[c] * b;
    const vec3 M = v3(m[0], m[1], m[2]);
    const float d = dot(M, M);
    if (!(d > 0.0f) || !(d < INFINITY)) return dressFaceNormal(row);
    return M * (1.0f / std::sqrt(d));
}

// DESIGN.md 14.14 / 14.15, per channel: the first corner where a barycentric is not finite or the three corner values are bit-equal, else
// (c0 * ((1 - a) - b) + c1 * a) + c2 * b.
static inline float dressBlend1(float c0, float c1, float c2, float a, float b) {
    if (!finiteBits(a) || !finiteBits(b)) return c0;
    if (sameBits(c0, c1) && sameBits(c0, c2)) return c0;
    const float w = (1.0f - a) - b;
    return (c0 * w + c1 * a) + c2 * b;
}
static inline vec3 dressColor(const float *crow, float a, float b) {
    return v3(dressBlend1(crow[0], crow[4], crow[8], a, b), dressBlend1(crow[1], crow[5], crow[9], a, b), dressBlend1(crow[2], crow[6], crow[10], a, b));
}
static inline vec2 dressUV(const float *urow, float a, float b) {
    return vec2{dressBlend1(urow[0], urow[2], urow[4], a, b), dressBlend1(urow[1], urow[3], urow[5], a, b)};
}

// one axis of a lookup on an edge of N texels -> the two texels and the weight of the second
static inline int dressWrap(int i, int N, bool clamp) {
    if (clamp) return std::min(std::max(i, 0), N - 1);
    return ((i % N) + N) % N;
}
static inline void dressAxis(float u, int N, bool nearest, bool clamp, int &i0, int &i1, float &f) {
    if (!finiteBits(u)) u = 0.0f;
    float s;
    if (clamp) s = (u < 0.0f) ? 0.0f : ((u > 1.0f) ? 1.0f : u);
    else s = u - std::floor(u);
    if (nearest) {
        i0 = i1 = dressWrap((int)std::floor(s * (float)N), N, clamp);
        f = 0.0f;
        return;
    }
    const float x = s * (float)N - 0.5f;
    const float fl = std::floor(x);
    f = x - fl;
    i0 = dressWrap((int)fl, N, clamp);
    i1 = dressWrap((int)fl + 1, N, clamp);
}
static inline vec3 dressTexel(const OrcDress &d, vec2 uv) {
    const bool nearest = (d.texFlags & kTexNearest) != 0, clamp = (d.texFlags & kTexClamp) != 0;
    int i0, i1, j0, j1;
    float a, b;
    dressAxis(uv.x, d.texW, nearest, clamp, i0, i1, a);
    dressAxis(uv.y, d.texH, nearest, clamp, j0, j1, b);
    auto at = [&](int i, int j) { return d.texels + ((size_t)j * (size_t)d.texW + (size_t)i) * 4; };
    float out[3];
    if (nearest) {
        const uint8_t *p = at(i0, j0);
        return v3(d.table[p[0]], d.table[p[1]], d.table[p[2]]);
    }
    const uint8_t *p00 = at(i0, j0), *p10 = at(i1, j0), *p01 = at(i0, j1), *p11 = at(i1, j1);
    const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    for (int k = 0; k < 3; ++k) {
        const float t00 = d.table[p00[k]], t10 = d.table[p10[k]], t01 = d.table[p01[k]], t11 = d.table[p11[k]];
        const bool flat = sameBits(t00, t10) && sameBits(t00, t01) && sameBits(t00, t11);   // four weights do not sum to 1 in float32
        out[k] = flat ? t00 : ((t00 * w00 + t10 * w10) + t01 * w01) + t11 * w11;
    }
    return v3(out[0], out[1], out[2]);
}

// The albedo of a hit on row prim: base (the colours' blend, or the reference's 0.85) times the texel where there is a texture, one rounded product.
static inline vec3 dressAlbedo(const OrcDress &d, int prim, float a, float b) {
    vec3 base = v3(0.85f);
    if (d.colRows) base = dressColor(d.colRows + (size_t)prim * 12, a, b);
    if (!dressHasTexture(d)) return base;
    return base * dressTexel(d, dressUV(d.uvRows + (size_t)prim * 8, a, b));
}

// where the hit point x on row T was when the row was P.  Nine bit-equal geometry floats hand x back; otherwise x moves by the
// difference of the two rows at (a, b): x + (((P.v0 - T.v0) + (P.e1 - T.e1) * a) + (P.e2 - T.e2) * b).
static inline vec3 dressPrevPoint(const float *T, const float *P, float a, float b, vec3 x) {
    bool same = true;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) same = same && sameBits(T[4 * r + c], P[4 * r + c]);
    if (same) return x;
    float d[3];
    for (int c = 0; c < 3; ++c) d[c] = ((P[c] - T[c]) + (P[4 + c] - T[4 + c]) * a) + (P[8 + c] - T[8 + c]) * b;
    return v3(x.x + d[0], x.y + d[1], x.z + d[2]);
}

}  // namespace orc
