// rt_morph_pack.cpp -- sparse morph targets on the host: rt_morph_positions, the definition rt_mesh_morph is held to, and the packer
// of the sliced layout k_mesh_morph reads, handed out by rt_debug_morph_pack.  Plain C++ that links on its own (rt_morph_pack.hpp).
#include "rt_morph_pack.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

namespace rtl {

int morph_validate(int nVerts, const int32_t *targetFirst, const uint32_t *vertIdx, const float *deltas, int nTargets, std::string &err) {
    char buf[160];
    auto bad = [&](const char *msg) { err = msg; return (int)RT_ERR_INVALID; };
    if (nVerts <= 0) return bad("no vertices");
    if (nTargets < 1 || nTargets > RT_MAX_MORPH_TARGETS) {
        snprintf(buf, sizeof buf, "%d targets (1 .. %d)", nTargets, RT_MAX_MORPH_TARGETS);
        return bad(buf);
    }
    if (!targetFirst || !vertIdx || !deltas) return bad(!targetFirst ? "null targetFirst" : !vertIdx ? "null vertIdx" : "null deltas");
    if (targetFirst[0] != 0) {
        snprintf(buf, sizeof buf, "targetFirst starts at %d, not at 0", targetFirst[0]);
        return bad(buf);
    }
    for (int t = 0; t < nTargets; ++t)
        if (targetFirst[t + 1] < targetFirst[t]) {
            snprintf(buf, sizeof buf, "targetFirst decreases at target %d (%d after %d)", t, targetFirst[t + 1], targetFirst[t]);
            return bad(buf);
        }
    const size_t n = (size_t)targetFirst[nTargets];
    for (size_t e = 0; e < n; ++e) {
        if (vertIdx[e] >= (uint32_t)nVerts) {
            snprintf(buf, sizeof buf, "entry %zu names vertex %u of %d", e, vertIdx[e], nVerts);
            return bad(buf);
        }
        if (!std::isfinite(deltas[3 * e]) || !std::isfinite(deltas[3 * e + 1]) || !std::isfinite(deltas[3 * e + 2])) {
            snprintf(buf, sizeof buf, "the delta of entry %zu is not finite", e);
            return bad(buf);
        }
    }
    return RT_OK;
}

int morph_plan(int nVerts, const int32_t *targetFirst, const uint32_t *vertIdx, int nTargets, MorphPlan &plan, std::string &err) {
    const size_t n = (size_t)targetFirst[nTargets];
    const size_t nSlices = ((size_t)nVerts + kMorphSlice - 1) / kMorphSlice;
    plan.count.assign((size_t)nVerts, 0u);
    for (size_t e = 0; e < n; ++e) ++plan.count[vertIdx[e]];
    plan.sliceFirst.assign(nSlices + 1, 0u);
    uint64_t rowsTotal = 0;
    uint32_t maxPer = 0;
    for (size_t s = 0; s < nSlices; ++s) {
        const size_t v1 = std::min((size_t)nVerts, (s + 1) * kMorphSlice);
        uint32_t rows = 0;
        for (size_t v = s * kMorphSlice; v < v1; ++v) rows = std::max(rows, plan.count[v]);
        maxPer = std::max(maxPer, rows);
        rowsTotal += rows;
        if (rowsTotal * kMorphSlice >= (1ull << 31)) {
            err = "the padded entry records reach 2^31 (one vertex of a slice of 64 sets the rows of all of them)";
            return RT_ERR_UNSUPPORTED;
        }
        plan.sliceFirst[s + 1] = (uint32_t)rowsTotal;
    }
    RtMorphInfo &I = plan.info;
    I.nVerts = nVerts; I.nTargets = nTargets; I.nSlices = (int32_t)nSlices; I.maxPerVertex = (int32_t)maxPer;
    I.entries = n; I.paddedEntries = rowsTotal * kMorphSlice;
    I.bytes = I.paddedEntries * sizeof(MorphRecord) + (uint64_t)(nSlices + 1) * 4 + (uint64_t)nVerts * 12 + (uint64_t)nTargets * 4;
    return RT_OK;
}

void morph_fill(const MorphPlan &plan, const int32_t *targetFirst, const uint32_t *vertIdx, const float *deltas, std::vector<MorphRecord> &records) {
    const MorphRecord pad = {0u, 0u, 0u, kMorphPadTarget};
    records.assign((size_t)plan.info.paddedEntries, pad);
    std::vector<uint32_t> next(plan.count.size(), 0u);   // per vertex: the row its next entry takes; input order is the definition's order
    for (int t = 0; t < plan.info.nTargets; ++t)
        for (size_t e = (size_t)targetFirst[t]; e < (size_t)targetFirst[t + 1]; ++e) {
            const uint32_t v = vertIdx[e];
            MorphRecord &r = records[((size_t)plan.sliceFirst[v / kMorphSlice] + next[v]++) * kMorphSlice + v % kMorphSlice];
            std::memcpy(&r, deltas + 3 * e, 12);
            r.target = (uint32_t)t;
        }
}

}  // namespace rtl

// Morph-target blending, and the definition rt_mesh_morph is held to: the entries in input order, each adding weight * delta to its vertex as a
// rounded product and a rounded sum; an entry whose weight is +-0 is skipped, so a vertex without any other keeps its base bits.
int rt_morph_positions(const float *base, int nVerts, const int32_t *targetFirst, const uint32_t *vertIdx, const float *deltas, int nTargets, const float *weights,
                       float *out) {
    if (!base || !weights || !out) return RT_ERR_INVALID;
    try {
        std::string err;
        const int rc = rtl::morph_validate(nVerts, targetFirst, vertIdx, deltas, nTargets, err);
        if (rc != RT_OK) return rc;
    } catch (const std::bad_alloc &) { return RT_ERR_IO; }
    if (out != base) std::memmove(out, base, (size_t)nVerts * 12);
    for (int t = 0; t < nTargets; ++t) {
        const float w = weights[t];
        if (w == 0.0f) continue;
        for (size_t e = (size_t)targetFirst[t]; e < (size_t)targetFirst[t + 1]; ++e) {
            float *acc = out + (size_t)vertIdx[e] * 3;
            for (int c = 0; c < 3; ++c) {
                const float term = w * deltas[3 * e + c];
                acc[c] = acc[c] + term;
            }
        }
    }
    return RT_OK;
}

int rt_debug_morph_pack(int nVerts, const int32_t *targetFirst, const uint32_t *vertIdx, const float *deltas, int nTargets, int which, void *dst, size_t capacity,
                        size_t *bytes) {
    if (!bytes) return RT_ERR_INVALID;
    *bytes = 0;
    try {
        std::string err;
        int rc = rtl::morph_validate(nVerts, targetFirst, vertIdx, deltas, nTargets, err);
        if (rc != RT_OK) return rc;
        rtl::MorphPlan plan;
        rc = rtl::morph_plan(nVerts, targetFirst, vertIdx, nTargets, plan, err);
        if (rc != RT_OK) return rc;
        std::vector<rtl::MorphRecord> records;
        const void *src = nullptr;
        size_t n = 0;
        switch (which) {
            case RT_MORPH_ARRAY_SLICE_FIRST: src = plan.sliceFirst.data(); n = plan.sliceFirst.size() * 4; break;
            case RT_MORPH_ARRAY_ENTRIES:
                n = (size_t)plan.info.paddedEntries * sizeof(rtl::MorphRecord);
                if (dst && capacity >= n) { rtl::morph_fill(plan, targetFirst, vertIdx, deltas, records); src = records.data(); }   // a size query packs nothing
                break;
            case RT_MORPH_ARRAY_INFO: src = &plan.info; n = sizeof plan.info; break;
            default: return RT_ERR_INVALID;
        }
        *bytes = n;
        if (!dst) return RT_OK;
        if (capacity < n) return RT_ERR_INVALID;
        if (n) std::memcpy(dst, src, n);
        return RT_OK;
    } catch (const std::bad_alloc &) { return RT_ERR_IO; }
}
