// rt_morph_pack.hpp -- sparse morph targets of the dynamic mesh on the host: the checks rt_morph_positions and rt_mesh_morph_upload
// share, and the packer that turns the targets' entry lists into the wave-shaped layout k_mesh_morph (rt_mesh_morph.hip) reads.  Plain C++: no HIP,
// no context, no other object of the library; rt_morph_pack.cpp links on its own.
//
// The packed form is sliced ELLPACK with slices of 64 vertices, one slice per wave.  Slice s holds vertices 64s .. 64s+63 and has rows[s] rows, the
// largest entry count of any of its vertices (0 is legal); sliceFirst holds the nSlices + 1 prefix sums of rows.  Record (sliceFirst[s] + k) * 64 + l
// is the k-th entry of vertex 64s + l in the definition's order (ascending target, then position within the target), so the 64 lanes of a wave read
// 64 consecutive 16-byte records per row.  Where a vertex has fewer than k + 1 entries, or lies at or past nVerts, the record is the pad record.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_mi355.h"

namespace rtl {

constexpr int kMorphSlice = 64;                       // vertices per slice: one wave
constexpr uint32_t kMorphPadTarget = 0xFFFFFFFFu;     // target of the pad record {+0, +0, +0, pad}
struct MorphRecord { uint32_t dx, dy, dz, target; };  // the delta's three floats by their bits, the target whose weight scales it
static_assert(sizeof(MorphRecord) == 16, "one 16-byte load per lane");

struct MorphPlan {
    RtMorphInfo info = {};
    std::vector<uint32_t> count;        // per vertex: its entries
    std::vector<uint32_t> sliceFirst;   // nSlices + 1 prefix sums of the slices' rows
};

// RT_OK or RT_ERR_INVALID with a message: a null array, nVerts <= 0, nTargets outside 1 .. RT_MAX_MORPH_TARGETS, a targetFirst that does not start at 0
// or decreases, a vertIdx >= nVerts, a delta that is not finite.
int morph_validate(int nVerts, const int32_t *targetFirst, const uint32_t *vertIdx, const float *deltas, int nTargets, std::string &err);
// Counts and prefix sums for validated targets; allocates nVerts + nSlices words, never the records.  RT_ERR_UNSUPPORTED when the padded record count
// reaches 2^31.
int morph_plan(int nVerts, const int32_t *targetFirst, const uint32_t *vertIdx, int nTargets, MorphPlan &plan, std::string &err);
// The records of a plan: a stable counting sort of the entries by vertex into the slices, pad records elsewhere.
void morph_fill(const MorphPlan &plan, const int32_t *targetFirst, const uint32_t *vertIdx, const float *deltas, std::vector<MorphRecord> &records);

}  // namespace rtl
