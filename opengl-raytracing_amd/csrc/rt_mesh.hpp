// rt_mesh.hpp -- the dynamic mesh: positions and indices stay on the device, the topology of the reference's median-split BVH is laid
// out once per mesh as index tables, and a rebuild is a fixed sequence of kernels that fills every device record form of rt_upload_bvh with floats.
// rt_mesh.hip owns the device code and the mesh's memory; rt_api.hip owns the context, the ordering against frames and queries and the C ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/rt_mi355.h"

namespace rtuv { struct Texture; }   // rt_mesh_uvs.hpp

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
// positions / indices: validated host arrays.  partFirst: nParts + 1 validated part boundaries in triangle units; the parts table, the
// per-triangle part lookup and the matrix table (identities) go to the device here.  quantised: build the quantised any-hit form as well; sparseLeafBoxes: its leaf
// boxes one slot per pair record (PackOptions).  May allocate and synchronise.
int mesh_create(const float *positions, int nVerts, const uint32_t *indices, int nIdx, const int32_t *partFirst, int nParts, bool quantised, bool sparseLeafBoxes,
                Mesh **out, const char **err);
void mesh_destroy(Mesh *m);
const BvhLayout &mesh_layout(const Mesh *m);
const MeshScene &mesh_scene(const Mesh *m);
float *mesh_positions(Mesh *m);
int mesh_verts(const Mesh *m);
uint64_t mesh_allocations(const Mesh *m);
size_t mesh_scratch_bytes(const Mesh *m);
size_t mesh_scene_bytes(const Mesh *m);
int mesh_part_count(const Mesh *m);
const int32_t *mesh_part_first(const Mesh *m);   // host copy, nParts + 1 entries
float *mesh_part_matrices(Mesh *m);               // device, nParts x 16 floats, column-major
const uint32_t *mesh_indices(const Mesh *m);      // device, the uploaded index triples (validated on upload)
const uint16_t *mesh_part_of(const Mesh *m);      // device, [input triangle] -> part
// Enqueues gather, build and record emission on `st`: no allocation, no host wait.  The gather is the single-matrix one under M16 (column-major), or,
// with M16 == nullptr, the part-aware one under the matrix table as it stands when the kernel runs.  mesh_refit takes the same argument.
int mesh_rebuild(Mesh *m, hipStream_t st, const float *M16, const char **err);
// A rebuild of this mesh has run: there is a tree to refit and an order to hand out.
bool mesh_has_tree(const Mesh *m);
// Enqueues the refit on `st`: the tree of the last rebuild (numbering, links, leaf ranges, which input triangle sits in which row) kept, triangles
// re-gathered under M16 into their rows, boxes bottom-up, every record form re-emitted.  No allocation, no host wait.  RT_ERR_INVALID without a tree.
int mesh_refit(Mesh *m, hipStream_t st, const float *M16, const char **err);
// *order: device array, order[row of the triangle array] = input triangle, derived on `st` at the first call after a rebuild into the permutation
// buffer that is idle between rebuilds; valid until the next rebuild.  RT_ERR_INVALID without a tree.
int mesh_order(Mesh *m, hipStream_t st, const int **order, const char **err);
bool mesh_order_written(const Mesh *m);   // the order array of the current tree has been derived (by whichever call asked first)
// Enqueues the hit -> (part, triangle of the part) map on `st` for n RtHit records (device pointers; either output may be null): order[prim] through the
// part lookup, (-1, -1) for a prim outside [0, nTris).  The caller has made the order array visible on `st` (mesh_order).
int mesh_hit_parts(Mesh *m, hipStream_t st, const int *order, const void *hits, int n, int32_t *parts, int32_t *tris, const char **err);

// rt_mesh_refit.hip: the refit's kernels behind plain launch functions (raw device pointers; bounds are the builder's sortable uints, six per slot)
struct RefitLeaf { int slot, first, count; };   // one leaf: bounds slot, its rows of the triangle array
struct RefitKids { int l, r; };                 // per bounds slot: the children's slots (-1, -1: a leaf)
void refit_launch_tris(hipStream_t st, const float *pos, const uint32_t *idx, const int *perm, const int *outOfPos, int nTris, const float *M16, float4 *t12);
void refit_launch_leaves(hipStream_t st, const float4 *t12, const RefitLeaf *leaves, int nLeaves, uint32_t *bounds, uint32_t *status);   // clears *status
void refit_launch_inner(hipStream_t st, const RefitKids *kids, int firstSlot, int nSlots, uint32_t *bounds);                             // one level
void refit_launch_order(hipStream_t st, const int *perm, const int *outOfPos, int nTris, int *order);

// rt_mesh_parts.hip: the part-aware kernels behind plain launch functions.  partOf[input triangle] = its part; mats = the matrix table
void parts_launch_gather(hipStream_t st, const float *pos, const uint32_t *idx, const uint16_t *partOf, const float *mats, int nTris, float *t9);
void parts_launch_refit_tris(hipStream_t st, const float *pos, const uint32_t *idx, const int *perm, const int *outOfPos, const uint16_t *partOf, const float *mats,
                             int nTris, float4 *t12);
void parts_launch_hit_parts(hipStream_t st, const void *hits, int n, const int *order, int nTris, const uint16_t *partOf, const int32_t *partFirst, int32_t *parts,
                            int32_t *tris);

// rt_mesh_quality.hip: the quality metric of the tree in the bounds array.  One record = the two integer sums of rt_bvh_cost and the
// root's six sortable keys, from which the host derives everything else.
constexpr int kQualityRing = 8;                 // result slots: measurements that may be in flight at once
constexpr size_t kQualityRecordBytes = 64;
struct QualityRecord { uint64_t innerQ, leafQ; uint32_t rootKeys[6]; };
hipError_t quality_launch(hipStream_t st, const uint32_t *bounds, const RefitKids *kids, int nNodes, const RefitLeaf *leaves, int nLeaves, unsigned long long *acc,
                          void *pinned);
// Enqueues the measurement of the current tree on `st` into result slot `slot` (its own accumulators, its own pinned record) and records the slot's
// event behind it: no allocation, no host wait.  RT_ERR_INVALID without a tree.  mesh_quality_event / mesh_quality_record: what the host polls and reads.
int mesh_measure(Mesh *m, hipStream_t st, int slot, const char **err);
hipEvent_t mesh_quality_event(const Mesh *m, int slot);
const QualityRecord *mesh_quality_record(const Mesh *m, int slot);

// Skinning.  mesh_skin_create: validated host tables for the mesh's vertices; rest == nullptr snapshots the device positions.  Replaces
// a skin the mesh already has.  Allocates, copies and waits for the device; the caller has waited for every lane.  mesh_skin_release: the four arrays
// freed (callers have synchronised).  mesh_skin enqueues positions := skin(rest, tables, bone table) on `st`: no allocation, no host wait;
// RT_ERR_INVALID without a skin.
int mesh_skin_create(Mesh *m, const float *rest, const uint16_t *boneIdx4, const float *weights4, int nBones, const char **err);
void mesh_skin_release(Mesh *m);
int mesh_bone_count(const Mesh *m);          // 0: no skin
float *mesh_bones(Mesh *m);                  // device, nBones x 16 floats, column-major
float *mesh_rest_positions(Mesh *m);         // device, nVerts x 3 floats
int mesh_skin(Mesh *m, hipStream_t st, const char **err);
// rt_mesh_skin.hip: the kernel behind a plain launch function (raw device pointers; idx4 / w4: four influences per vertex)
void skin_launch(hipStream_t st, const float *rest, const uint16_t *idx4, const float *w4, const float *bones, int nVerts, float *pos);

// Morph targets.  mesh_morph_create: the packed form rt_morph_pack.cpp made of validated targets for the mesh's vertices (sliceFirst:
// info.nSlices + 1 words; records: info.paddedEntries 16-byte records); base == nullptr snapshots the rest array when the mesh has a skin, else the
// positions.  The weight table starts all zero.  Replaces a morph the mesh already has.  Allocates, copies and waits for the device; the caller has
// waited for every lane.  mesh_morph_release: the four arrays freed (callers have synchronised).  mesh_morph enqueues dst := morph(base, records,
// weight table) on `st`, dst the rest array (toRest) or the positions: no allocation, no host wait; RT_ERR_INVALID without a morph, or toRest
// without a skin.
int mesh_morph_create(Mesh *m, const float *base, const uint32_t *sliceFirst, const void *records, const RtMorphInfo &info, const char **err);
void mesh_morph_release(Mesh *m);
int mesh_morph_target_count(const Mesh *m);  // 0: no morph
const RtMorphInfo &mesh_morph_info(const Mesh *m);
float *mesh_morph_base(Mesh *m);             // device, nVerts x 3 floats
float *mesh_morph_weights(Mesh *m);          // device, nTargets floats
int mesh_morph(Mesh *m, hipStream_t st, bool toRest, const char **err);
// rt_mesh_morph.hip: the kernel behind a plain launch function (raw device pointers; entries: the packed records)
void morph_launch(hipStream_t st, const float *base, const uint32_t *sliceFirst, const void *entries, const float *weights, int nVerts, float *dst);

// The previous pose: prevTris, nTris rows of the triangle array's layout, row i = the row input triangle order[i] had before the most
// recent update.  mesh_motion_create allocates it and the remap scratch (old rows by input triangle) and, when there is a tree, latches; allocates and
// waits for the device; the caller has waited for every lane.  mesh_motion_release: both arrays freed (callers have synchronised).  While the arrays
// exist mesh_rebuild and mesh_refit move the previous pose on their stream, inside their own sequence of launches.  mesh_motion_latch enqueues
// previous pose := current pose on `st`: no allocation, no host wait; RT_ERR_INVALID without the arrays or without a tree.
int mesh_motion_create(Mesh *m, const char **err);
void mesh_motion_release(Mesh *m);
const float4 *mesh_prev_tris(const Mesh *m);   // device; null: motion is not enabled
int mesh_motion_latch(Mesh *m, hipStream_t st, const char **err);
// Enqueues prevPoints[i] = where hit i's point was in the previous pose (rt_hit_motion's prevPoints) on `st` for n RtHit records and their points (device
// pointers).  RT_ERR_INVALID without the arrays or without a tree.
int mesh_hit_prev_points(Mesh *m, hipStream_t st, const void *hits, const float *points, int n, float *prevPoints, const char **err);
// rt_mesh_motion.hip: the kernels behind plain launch functions (raw device pointers; perm / outOfPos: the tables refit_launch_order composes)
void motion_launch_scatter(hipStream_t st, const float4 *tris, const int *perm, const int *outOfPos, int nTris, float4 *byInput);
void motion_launch_gather(hipStream_t st, const float4 *byInput, const int *perm, const int *outOfPos, int nTris, float4 *prev);
void motion_launch_hit_prev_points(hipStream_t st, const void *hits, const float *points, int n, const float4 *tris, const float4 *prevTris, int nTris,
                                   float *prevPoints);

// The corner attributes: smooth normals, colours and UVs are each a per-vertex array and a row array, row i beside row i of the triangle
// array, that holds the three corner values of the row's input triangle.  A kind is what tells them apart (corner_kind: rt_mesh_corner.hip's table,
// one row per traits type); everything else -- the arrays, the gather behind every update, the gather alone, the blend at a hit, the release -- is one path.
enum class Corner { normals, colors, uvs };   // the order an update walks them in
struct CornerKind {
    size_t vertBytes, rowBytes;   // per vertex (16, 16, 8) and per row (48, 48, 32)
    // the gather: rows[r] = the corner values of input triangle order[r] (raw device pointers; order: row -> input triangle)
    void (*launchRows)(hipStream_t st, const int *order, const uint32_t *idx, const void *vert, int nTris, int nVerts, float4 *rows);
    // the blend at n RtHit records, kChannels floats each; null: the attribute has a query of its own (normals: k_hit_normals)
    void (*launchHitBlend)(hipStream_t st, const void *hits, int n, const float4 *rows, int nTris, float *values);
};
const CornerKind &corner_kind(Corner which);
// mesh_corner_create (colours and UVs): allocates the vertex array (zeros; colours: every one (0.85, 0.85, 0.85, 0)) and the row array and, when there
// is a tree, gathers the rows on `st`; allocates and waits for the device; the caller has waited for every lane.  mesh_corner_release: the attribute's
// arrays freed (callers have synchronised).  While the arrays exist mesh_rebuild and mesh_refit gather the rows again behind their new rows on their
// stream, inside their own sequence of launches, normals (recomputed first), then colours, then UVs: no allocation, no host wait.
int mesh_corner_create(Mesh *m, Corner which, hipStream_t st, const char **err);
void mesh_corner_release(Mesh *m, Corner which);
void *mesh_corner_vertices(const Mesh *m, Corner which);   // device; null: the attribute is not enabled
// Enqueues the row gather alone on `st` (deriving the order array first where the tree has none yet; normals: the two kernels that recompute them in
// front of it).  RT_ERR_INVALID without the arrays or a tree.
int mesh_corner_refresh(Mesh *m, Corner which, hipStream_t st, const char **err);
// Enqueues values[i] = the attribute at hit i (rt_hit_colors' out3, rt_hit_uvs' out2) on `st` for n RtHit records (device pointers).  RT_ERR_INVALID
// without the arrays, without a tree or for normals.
int mesh_hit_blend(Mesh *m, Corner which, hipStream_t st, const void *hits, int n, float *values, const char **err);
const float4 *mesh_vertex_normals(const Mesh *m);   // device, nVerts float4 (xyz, w = 0); null: normals are not enabled
const float4 *mesh_normal_rows(const Mesh *m);      // device, nTris x 3 float4; null: normals are not enabled
float4 *mesh_vertex_colors(const Mesh *m);          // device, nVerts float4 (rgb, w = 0); null: colours are not enabled
const float4 *mesh_color_rows(const Mesh *m);       // device, nTris x 3 float4; null: colours are not enabled
float2 *mesh_vertex_uvs(const Mesh *m);             // device, nVerts float2; null: UVs are not enabled
const float4 *mesh_uv_rows(const Mesh *m);          // device, nTris x 2 float4, (u0, v0, u1, v1), (u2, v2, 0, 0); null: UVs are not enabled

// Smooth vertex normals: the one attribute a kernel writes.  mesh_normals_create: the packed adjacency rt_normal_pack.cpp made of the
// mesh's own index buffer (sliceFirst: info.nSlices + 1 words; entries: info.paddedEntries words); allocates it, the face vectors by input triangle and
// the attribute's two arrays and, when there is a tree, computes the normals and gathers the rows on `st`; allocates, copies and waits for the device;
// the caller has waited for every lane.  mesh_corner_release frees all five.
int mesh_normals_create(Mesh *m, hipStream_t st, const uint32_t *sliceFirst, const int32_t *entries, const RtNormalInfo &info, const char **err);
// Enqueues normals[i] = the shading normal of hit i (rt_hit_normals' out3) on `st` for n RtHit records (device pointers).  RT_ERR_INVALID without the
// arrays or without a tree.
int mesh_hit_normals(Mesh *m, hipStream_t st, const void *hits, int n, float *normals, const char **err);
// rt_mesh_normals.hip: the kernels behind plain launch functions (raw device pointers; order: row -> input triangle)
void normals_launch_update(hipStream_t st, const float4 *tris, const int *order, int nTris, const uint32_t *sliceFirst, const int32_t *entries, int nVerts,
                           float4 *faceByInput, float4 *vertNrm);
void normals_launch_hit_normals(hipStream_t st, const void *hits, int n, const float4 *tris, const float4 *nrmRows, int nTris, float *normals);

// The albedo texture: an attachment of its own, the texels (W x H RGBA8) and the 256-float decode table.  mesh_texture_create
// allocates (a block of the same size is kept), copies both from host memory and waits for the device; the caller has waited for every lane.
// mesh_texture: null without one.
int mesh_texture_create(Mesh *m, const uint8_t *rgba8, int W, int H, uint32_t flags, const float *table256, const char **err);
void mesh_texture_release(Mesh *m);
const rtuv::Texture *mesh_texture(const Mesh *m);
// Enqueues texels[i] = the texture's sample at the UV of hit i on `st` for n RtHit records (device pointers).  RT_ERR_INVALID without the UVs, the
// texture or a tree.
int mesh_hit_texels(Mesh *m, hipStream_t st, const void *hits, int n, float *texels, const char **err);
// rt_mesh_corner.hip: the two kernels beside the table's
void corner_launch_color_fill(hipStream_t st, float4 *vertCol, int nVerts);
void corner_launch_hit_texels(hipStream_t st, const void *hits, int n, const float4 *uvRows, int nTris, const rtuv::Texture &tex, float *texels);

// Quantised form only: enqueue the read of the status word behind the rebuild, wait for `st`, and say whether every node could be quantised.
int mesh_quantised_ok(Mesh *m, hipStream_t st, bool &ok, const char **err);

}  // namespace rtl
