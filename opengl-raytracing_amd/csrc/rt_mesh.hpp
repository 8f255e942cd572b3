// rt_mesh.hpp -- the dynamic mesh: positions and indices stay on the device, the topology of the reference's median-split BVH is laid
// out once per mesh as index tables, and a rebuild is a fixed sequence of kernels that fills every device record form of rt_upload_bvh with floats.
// rt_mesh.hip owns the device code and the mesh's memory; rt_api.hip owns the context, the ordering against frames and queries and the C ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace rtl {

// What the triangle count alone determines (the builder splits every range at its middle and stops at <= 8 triangles).
struct BvhLayout {
    int nTris = 0, nNodes = 0, nInner = 0, treeDepth = 0, anyStack = 0;
    int rootRef = 0, rootRefW = 0, rootRef4 = 0;   // as rt_upload_bvh derives them
    size_t nPairs = 0, nWide4 = 0, nLeaves = 0;
    int minLeafRecords = 0;                         // fewest pair records any leaf owns (the leaf-box index divides by it)
};
// RT_OK, RT_ERR_INVALID (nTris <= 0) or RT_ERR_UNSUPPORTED (>= 2^28 triangles, depth > 32); O(log n) time and memory
int bvh_layout(int nTris, BvhLayout &out);

// The scene arrays a rebuild fills: rt_upload_bvh's device layout, allocated once per mesh (zero padding included).
struct MeshScene {
    float4 *wnodes = nullptr, *wnodesW = nullptr, *w4 = nullptr, *q4 = nullptr, *leafBox = nullptr, *pairs = nullptr, *tris = nullptr;
    float *rootBox = nullptr;   // six floats: min.xyz, max.xyz of node 0
    size_t leafBoxBytes = 0;
    uint32_t leafBoxMagic = 0;
};

struct Mesh;
// positions / indices: validated host arrays.  quantised: build the quantised any-hit form as well.  May allocate and synchronise.
int mesh_create(const float *positions, int nVerts, const uint32_t *indices, int nIdx, bool quantised, Mesh **out, const char **err);
void mesh_destroy(Mesh *m);
const BvhLayout &mesh_layout(const Mesh *m);
const MeshScene &mesh_scene(const Mesh *m);
float *mesh_positions(Mesh *m);
int mesh_verts(const Mesh *m);
uint64_t mesh_allocations(const Mesh *m);
size_t mesh_scratch_bytes(const Mesh *m);
size_t mesh_scene_bytes(const Mesh *m);
// Enqueues gather (model matrix M16, column-major), build and record emission on `st`: no allocation, no host wait.
int mesh_rebuild(Mesh *m, hipStream_t st, const float *M16, const char **err);
// Quantised form only: enqueue the read of the status word behind the rebuild, wait for `st`, and say whether every node could be quantised.
int mesh_quantised_ok(Mesh *m, hipStream_t st, bool &ok, const char **err);

}  // namespace rtl
