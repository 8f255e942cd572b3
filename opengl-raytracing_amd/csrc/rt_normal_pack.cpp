// rt_normal_pack.cpp -- smooth vertex normals on the host: rt_vertex_normals and rt_hit_normals, the definitions the device kernels
// and the frames are held to, and the packer of the sliced adjacency k_vertex_normals reads, handed out by rt_debug_normal_pack.  Plain C++ that
// links on its own (rt_normal_pack.hpp); the arithmetic is rt_mesh_normals.hpp's, the expressions the device compiles.
#include "rt_normal_pack.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>

#include "rt_mesh_normals.hpp"

namespace rtl {

int normal_validate(const uint32_t *indices, int nIdx, int nVerts, std::string &err) {
    char buf[160];
    auto bad = [&](const char *msg) { err = msg; return (int)RT_ERR_INVALID; };
    if (!indices) return bad("null indices");
    if (nVerts <= 0) return bad("no vertices");
    if (nIdx <= 0 || nIdx % 3 != 0) {
        snprintf(buf, sizeof buf, "%d indices are not a list of triangles", nIdx);
        return bad(buf);
    }
    for (int k = 0; k < nIdx; ++k)
        if (indices[k] >= (uint32_t)nVerts) {
            snprintf(buf, sizeof buf, "index %d names vertex %u of %d", k, indices[k], nVerts);
            return bad(buf);
        }
    return RT_OK;
}

int normal_plan(const uint32_t *indices, int nIdx, int nVerts, NormalPlan &plan, std::string &err) {
    const size_t nSlices = ((size_t)nVerts + kNormalSlice - 1) / kNormalSlice;
    plan.count.assign((size_t)nVerts, 0u);
    for (int k = 0; k < nIdx; ++k) ++plan.count[indices[k]];
    plan.sliceFirst.assign(nSlices + 1, 0u);
    uint64_t total = 0;
    uint32_t maxPer = 0;
    for (size_t s = 0; s < nSlices; ++s) {
        const size_t v1 = std::min((size_t)nVerts, (s + 1) * kNormalSlice);
        uint32_t width = 0;
        for (size_t v = s * kNormalSlice; v < v1; ++v) width = std::max(width, plan.count[v]);
        maxPer = std::max(maxPer, width);
        total += (uint64_t)width * kNormalSlice;
        if (total >= (1ull << 31)) {
            err = "the padded adjacency reaches 2^31 entries (one vertex of a slice of 64 sets the width of all of them)";
            return RT_ERR_UNSUPPORTED;
        }
        plan.sliceFirst[s + 1] = (uint32_t)total;
    }
    RtNormalInfo &I = plan.info;
    I.nVerts = nVerts; I.nTris = nIdx / 3; I.nSlices = (int32_t)nSlices; I.maxPerVertex = (int32_t)maxPer;
    I.incidences = (uint64_t)nIdx; I.paddedEntries = total;
    I.bytes = total * 4 + (uint64_t)(nSlices + 1) * 4 + (uint64_t)I.nTris * 16 + (uint64_t)nVerts * 16 + (uint64_t)I.nTris * 48;
    return RT_OK;
}

void normal_fill(const NormalPlan &plan, const uint32_t *indices, int nIdx, std::vector<int32_t> &entries) {
    entries.assign((size_t)plan.info.paddedEntries, kNormalPad);
    std::vector<uint32_t> next(plan.count.size(), 0u);   // per vertex: the step its next incidence takes; input order is k ascending, then c
    for (int k = 0; k < nIdx; ++k) {
        const uint32_t v = indices[k];
        entries[(size_t)plan.sliceFirst[v / kNormalSlice] + (size_t)next[v]++ * kNormalSlice + v % kNormalSlice] = k / 3;
    }
}

}  // namespace rtl

// Area-weighted vertex normals, and the definition the device's vertex normals are held to: the face vector of input triangle k is cross(e1, e2) of the
// row r with order[r] == k; a vertex sums the face vectors of its incidences with k ascending, then c, the first term initialising the sum.
int rt_vertex_normals(const float *tris12, const int32_t *order, int nTris, const uint32_t *indices, int nVerts, float *normals3) {
    if (!tris12 || !order || !normals3 || nTris <= 0) return RT_ERR_INVALID;
    try {
        std::string err;
        const int rc = rtl::normal_validate(indices, nTris * 3, nVerts, err);
        if (rc != RT_OK) return rc;
        for (int r = 0; r < nTris; ++r)
            if (order[r] < 0 || order[r] >= nTris) return RT_ERR_INVALID;
        std::vector<float> face((size_t)nTris * 3, 0.0f);
        for (int r = 0; r < nTris; ++r) rtnormal::face_vector(tris12 + (size_t)r * 12, face.data() + (size_t)order[r] * 3);
        std::vector<float> sum((size_t)nVerts * 3, 0.0f);
        std::vector<char> any((size_t)nVerts, 0);
        for (int k = 0; k < nTris; ++k)
            for (int c = 0; c < 3; ++c) {
                const uint32_t v = indices[3 * (size_t)k + c];
                float *S = sum.data() + (size_t)v * 3;
                const float *f = face.data() + (size_t)k * 3;
                for (int d = 0; d < 3; ++d) S[d] = any[v] ? S[d] + f[d] : f[d];
                any[v] = 1;
            }
        for (int v = 0; v < nVerts; ++v) rtnormal::vertex_normal(sum.data() + (size_t)v * 3, normals3 + (size_t)v * 3);
        return RT_OK;
    } catch (const std::bad_alloc &) { return RT_ERR_IO; }
}

// Shading normals of hits, and the definition rt_mesh_hit_normals and the frames' normals are held to: the corner normals of the hit row's input triangle
// blended at the hit's barycentrics (rt_mesh_normals.hpp).  A prim outside [0, nTris): zeros, nothing read.
int rt_hit_normals(const float *tris12, const int32_t *order, int nTris, const uint32_t *indices, const float *normals3, int nVerts, const RtHit *hits, int n,
                   float *out3) {
    if (!tris12 || !order || !indices || !normals3 || nTris <= 0 || nVerts <= 0 || n < 0 || (n > 0 && (!hits || !out3))) return RT_ERR_INVALID;
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
            rtnormal::hit_normal(tris12 + (size_t)p * 12, normals3 + (size_t)ix[0] * 3, normals3 + (size_t)ix[1] * 3, normals3 + (size_t)ix[2] * 3, hits[i].u,
                                 hits[i].v, out);
        }
        std::memcpy(out3 + (size_t)i * 3, out, sizeof out);
    }
    return RT_OK;
}

int rt_debug_normal_pack(const uint32_t *indices, int nIdx, int nVerts, int which, void *dst, size_t capacity, size_t *bytes) {
    if (!bytes) return RT_ERR_INVALID;
    *bytes = 0;
    try {
        std::string err;
        int rc = rtl::normal_validate(indices, nIdx, nVerts, err);
        if (rc != RT_OK) return rc;
        rtl::NormalPlan plan;
        rc = rtl::normal_plan(indices, nIdx, nVerts, plan, err);
        if (rc != RT_OK) return rc;
        std::vector<int32_t> entries;
        const void *src = nullptr;
        size_t n = 0;
        switch (which) {
            case RT_NORMAL_ARRAY_SLICE_FIRST: src = plan.sliceFirst.data(); n = plan.sliceFirst.size() * 4; break;
            case RT_NORMAL_ARRAY_ENTRIES:
                n = (size_t)plan.info.paddedEntries * 4;
                if (dst && capacity >= n) { rtl::normal_fill(plan, indices, nIdx, entries); src = entries.data(); }   // a size query packs nothing
                break;
            case RT_NORMAL_ARRAY_INFO: src = &plan.info; n = sizeof plan.info; break;
            default: return RT_ERR_INVALID;
        }
        *bytes = n;
        if (!dst) return RT_OK;
        if (capacity < n) return RT_ERR_INVALID;
        if (n) std::memcpy(dst, src, n);
        return RT_OK;
    } catch (const std::bad_alloc &) { return RT_ERR_IO; }
}
