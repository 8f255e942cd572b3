// rt_mesh_uvs.cpp -- vertex UVs and the albedo texture of the dynamic mesh on host arrays: the definitions the device's UV rows
// (k_corner_rows<UvAttr>), rt_mesh_hit_uvs, rt_mesh_hit_texels and the frames' texel are held to, the sRGB decode table, and the .obj reader that keeps vt.
// Plain C++: no HIP header, links on its own (tests/uvs_sanitize.cpp).  The arithmetic is rt_mesh_uvs.hpp's, shared with the device.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../include/rt_mi355.h"
#include "rt_mesh_uvs.hpp"

#pragma clang fp contract(off)

// The device row array: row i holds the corner UVs of input triangle order[i], (u0, v0, u1, v1), (u2, v2, 0, 0).
int rt_uv_rows(const int32_t *order, const uint32_t *indices, const float *uvs, int nTris, int nVerts, float *out) {
    if (!order || !indices || !uvs || !out || nTris <= 0 || nVerts <= 0) return RT_ERR_INVALID;
    for (int r = 0; r < nTris; ++r) {
        if (order[r] < 0 || order[r] >= nTris) return RT_ERR_INVALID;
        for (int c = 0; c < 3; ++c)
            if (indices[3 * (size_t)order[r] + c] >= (uint32_t)nVerts) return RT_ERR_INVALID;
    }
    for (int r = 0; r < nTris; ++r) {
        const uint32_t *ix = indices + 3 * (size_t)order[r];
        float *o = out + (size_t)r * 8;
        for (int c = 0; c < 3; ++c) std::memcpy(o + 2 * c, uvs + (size_t)ix[c] * 2, 8);
        o[6] = 0.0f; o[7] = 0.0f;
    }
    return RT_OK;
}

// The UV of hits: the corner UVs of the hit row's input triangle blended at the hit's barycentrics.  A prim outside [0, nTris): zeros, nothing read.
int rt_hit_uvs(const RtHit *hits, int n, const int32_t *order, const uint32_t *indices, const float *uvs, int nTris, int nVerts, float *out2) {
    if (!order || !indices || !uvs || nTris <= 0 || nVerts <= 0 || n < 0 || (n > 0 && (!hits || !out2))) return RT_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        const int p = hits[i].prim;
        if (p < 0 || p >= nTris) continue;
        const int k = order[p];
        if (k < 0 || k >= nTris) return RT_ERR_INVALID;
        for (int c = 0; c < 3; ++c)
            if (indices[3 * (size_t)k + c] >= (uint32_t)nVerts) return RT_ERR_INVALID;
    }
    for (int i = 0; i < n; ++i) {
        float out[2] = {0.0f, 0.0f};
        const int p = hits[i].prim;
        if (p >= 0 && p < nTris) {
            const uint32_t *ix = indices + 3 * (size_t)order[p];
            rtuv::blend_uvs(uvs + (size_t)ix[0] * 2, uvs + (size_t)ix[1] * 2, uvs + (size_t)ix[2] * 2, hits[i].u, hits[i].v, out);
        }
        std::memcpy(out2 + (size_t)i * 2, out, sizeof out);
    }
    return RT_OK;
}

// The sRGB decode of every texel code: the piecewise curve in double, rounded to float once.
int rt_srgb_table(float *out256) {
    if (!out256) return RT_ERR_INVALID;
    for (int c = 0; c < 256; ++c) {
        const double x = (double)c / 255.0;
        out256[c] = (float)(x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4));
    }
    return RT_OK;
}

int rt_sample_texture(const uint8_t *texels, int W, int H, int flags, const float *uv2, int n, float *out3) {
    if (!texels || W < 1 || H < 1 || W > rtuv::kMaxEdge || H > rtuv::kMaxEdge || ((uint32_t)flags & ~rtuv::kAllFlags) || n < 0 || (n > 0 && (!uv2 || !out3)))
        return RT_ERR_INVALID;
    float table[256];
    if ((uint32_t)flags & rtuv::kSrgb) (void)rt_srgb_table(table);
    else for (int c = 0; c < 256; ++c) table[c] = rtuv::unorm8((uint8_t)c);
    rtuv::Texture t;
    t.texels = texels; t.table = table; t.W = W; t.H = H; t.flags = (uint32_t)flags;
    for (int i = 0; i < n; ++i) {
        float out[3];
        rtuv::sample(t, uv2[2 * (size_t)i], uv2[2 * (size_t)i + 1], out);
        std::memcpy(out3 + (size_t)i * 3, out, sizeof out);
    }
    return RT_OK;
}

// rt_load_obj's reader, keeping vt: a vertex per distinct (v, vt) pair in order of first use by the faces; a corner without vt pairs as vt = none.
namespace {
int load_obj_uv(FILE *f, char *&line, size_t &cap, float **positions, float **uvs, int *nVerts, uint32_t **indices, int *nIdx) {
    std::vector<float> pos, tex, outPos, outUv;
    std::vector<uint32_t> idx, face;
    std::map<std::pair<long, long>, uint32_t> seen;   // (v, vt) zero-based, vt = -1: none
    while (getline(&line, &cap, f) >= 0) {
        const char *s = line;
        while (*s == ' ' || *s == '\t') ++s;
        if (s[0] == 'v' && (s[1] == ' ' || s[1] == '\t')) {
            float x = 0, y = 0, z = 0;
            if (std::sscanf(s + 2, "%f %f %f", &x, &y, &z) == 3) { pos.push_back(x); pos.push_back(y); pos.push_back(z); }
        } else if (s[0] == 'v' && s[1] == 't' && (s[2] == ' ' || s[2] == '\t')) {
            float u = 0, v = 0;
            if (std::sscanf(s + 3, "%f %f", &u, &v) >= 1) { tex.push_back(u); tex.push_back(v); }
        } else if (s[0] == 'f' && (s[1] == ' ' || s[1] == '\t')) {
            face.clear();
            const char *q = s + 2;
            while (*q) {
                while (*q == ' ' || *q == '\t') ++q;
                if (*q == '\0' || *q == '\n' || *q == '\r' || *q == '#') break;
                char *end = nullptr;
                long v = std::strtol(q, &end, 10);   // "v", "v/vt", "v//vn", "v/vt/vn"
                if (end == q) break;
                const long nv = (long)(pos.size() / 3), nt = (long)(tex.size() / 2);
                if (v < 0) v = nv + v + 1;           // relative index
                if (v < 1 || v > nv) return RT_ERR_IO;
                q = end;
                long t = 0;                          // 0: none
                if (*q == '/' && q[1] != '/') {
                    ++q;
                    if (*q == '-' || *q == '+' || (*q >= '0' && *q <= '9')) {   // (strtol would skip blanks into the next corner)
                        t = std::strtol(q, &end, 10);
                        if (end != q) {
                            if (t < 0) t = nt + t + 1;
                            if (t < 1 || t > nt) return RT_ERR_IO;
                        } else t = 0;
                        q = end;
                    }
                }
                while (*q && *q != ' ' && *q != '\t' && *q != '\n' && *q != '\r') ++q;
                const std::pair<long, long> key(v - 1, t - 1);
                auto it = seen.find(key);
                if (it == seen.end()) {
                    it = seen.emplace(key, (uint32_t)(outPos.size() / 3)).first;
                    for (int k = 0; k < 3; ++k) outPos.push_back(pos[(size_t)(v - 1) * 3 + (size_t)k]);
                    outUv.push_back(t > 0 ? tex[(size_t)(t - 1) * 2] : 0.0f);
                    outUv.push_back(t > 0 ? tex[(size_t)(t - 1) * 2 + 1] : 0.0f);
                }
                face.push_back(it->second);
            }
            for (size_t k = 1; k + 1 < face.size(); ++k) {   // fan, as rt_load_obj
                idx.push_back(face[0]); idx.push_back(face[k]); idx.push_back(face[k + 1]);
            }
        }
    }
    *nVerts = (int)(outPos.size() / 3);
    *nIdx = (int)idx.size();
    *positions = (float *)std::malloc((outPos.size() + 1) * sizeof(float));
    *uvs = (float *)std::malloc((outUv.size() + 1) * sizeof(float));
    *indices = (uint32_t *)std::malloc((idx.size() + 1) * sizeof(uint32_t));
    if (!*positions || !*uvs || !*indices) {
        std::free(*positions); std::free(*uvs); std::free(*indices);
        *positions = nullptr; *uvs = nullptr; *indices = nullptr;
        return RT_ERR_IO;
    }
    if (!outPos.empty()) std::memcpy(*positions, outPos.data(), outPos.size() * sizeof(float));
    if (!outUv.empty()) std::memcpy(*uvs, outUv.data(), outUv.size() * sizeof(float));
    if (!idx.empty()) std::memcpy(*indices, idx.data(), idx.size() * sizeof(uint32_t));
    return RT_OK;
}
}  // namespace

int rt_load_obj_uv(const char *path, float **positions, float **uvs, int *nVerts, uint32_t **indices, int *nIdx) {
    if (!path || !positions || !uvs || !nVerts || !indices || !nIdx) return RT_ERR_INVALID;
    *positions = nullptr; *uvs = nullptr; *indices = nullptr; *nVerts = 0; *nIdx = 0;
    FILE *f = std::fopen(path, "rb");
    if (!f) return RT_ERR_IO;
    char *line = nullptr;
    size_t cap = 0;
    int rc;
    try { rc = load_obj_uv(f, line, cap, positions, uvs, nVerts, indices, nIdx); }
    catch (...) { rc = RT_ERR_IO; }
    std::free(line);
    std::fclose(f);
    return rc;
}
