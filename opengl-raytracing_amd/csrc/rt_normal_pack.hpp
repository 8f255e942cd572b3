// rt_normal_pack.hpp -- the vertex -> triangle adjacency of the dynamic mesh on the host: the check rt_vertex_normals and
// rt_mesh_normals_enable share, and the packer that turns an index buffer into the wave-shaped layout k_vertex_normals (rt_mesh_normals.hip) reads.
// Plain C++: no HIP, no context, no other object of the library; rt_normal_pack.cpp links on its own.
//
// An incidence is a pair (input triangle k, corner c) with indices[3k + c] == v; a vertex's incidences are ordered by k, then c, and a triangle that
// names v twice is two of them.  The packed form is sliced ELLPACK with slices of 64 vertices, one slice per wave.  Slice s holds vertices
// 64s .. 64s+63 and is as wide as the largest number of incidences any of them has (0 is legal); sliceFirst holds the nSlices + 1 prefix sums of
// width * 64, in entries.  Entry sliceFirst[s] + j * 64 + l is the input triangle of the j-th incidence of vertex 64s + l, or -1 where that vertex
// has no j-th incidence or does not exist: the 64 lanes of a wave read 256 consecutive bytes per step, the step count is wave-uniform, and one
// high-valence vertex widens only its own slice.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_mi355.h"

namespace rtl {

constexpr int kNormalSlice = 64;       // vertices per slice: one wave
constexpr int32_t kNormalPad = -1;     // the entry of an incidence that does not exist

struct NormalPlan {
    RtNormalInfo info = {};
    std::vector<uint32_t> count;        // per vertex: its incidences
    std::vector<uint32_t> sliceFirst;   // nSlices + 1 prefix sums, in entries
};

// RT_OK or RT_ERR_INVALID with a message: null indices, nIdx <= 0 or no multiple of 3, nVerts <= 0, an index >= nVerts.
int normal_validate(const uint32_t *indices, int nIdx, int nVerts, std::string &err);
// Counts and prefix sums for a validated index buffer; allocates nVerts + nSlices words, never the entries.  RT_ERR_UNSUPPORTED when the padded entry
// count reaches 2^31.
int normal_plan(const uint32_t *indices, int nIdx, int nVerts, NormalPlan &plan, std::string &err);
// The entries of a plan: the incidences in input order, which is their order per vertex, pad entries elsewhere.
void normal_fill(const NormalPlan &plan, const uint32_t *indices, int nIdx, std::vector<int32_t> &entries);

}  // namespace rtl
