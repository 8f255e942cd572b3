// rt_mesh.hip -- the dynamic mesh: rt_gather_triangles -> rt_build_bvh_gpu -> rt_upload_bvh as one fixed sequence of kernels on one
// stream, with no copy of geometry or records to or from the host, no allocation and no host wait.
//
// The reference's builder splits every range at its middle and stops at <= 8 triangles (bvh.cpp:62-76), so node numbering, links, leaf ranges and with
// them every reference, record slot, stack need and array size of every device record form depend on the triangle count alone.  mesh_create lays that
// out once on the host (the derivations of rt_scene_pack, applied to the skeleton instead of to decoded nodes) and keeps it on the device as index
// tables; what depends on the geometry -- node boxes and the order of the triangles -- is computed by the level kernels of rt_bvh_build.hpp, and one
// emission kernel per record form then writes whole records through the tables.  Every array ends up byte for byte as rt_upload_bvh would have left it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/rt_mi355.h"
#include "rt_bvh_build.hpp"
#include "rt_mesh.hpp"
#include "rt_mesh_uvs.hpp"
#include "rt_qnode.hpp"
#include "rt_scene_pack.hpp"

#pragma clang fp contract(off)


namespace {

struct Mat16 { float m[16]; };
struct Wn2Tab { int slotL, slotR, refL, refR, refLW, refRW; };   // one two-child record: bounds slots of the children, their references in both encodings
struct W4Tab { int slot[4]; int ref[4]; };                       // one four-child record: bounds slot (-1: absent) and reference per child
struct LeafTab { int slot; uint32_t at; };                       // one leaf box: bounds slot -> index in leafBox

// rt_gather_triangles (rt_host.cpp): glm's mat4 * vec4 order per vertex, then e1 = b - a, e2 = c - a
__global__ void k_mesh_gather(const float *__restrict__ pos, const uint32_t *__restrict__ idx, int nTris, Mat16 M, float *__restrict__ t9) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nTris) return;
    float v[3][3];
    for (int c = 0; c < 3; ++c) {
        const float *p = pos + (size_t)idx[(size_t)i * 3 + c] * 3;
        const float x = p[0], y = p[1], z = p[2];
        for (int k = 0; k < 3; ++k) v[c][k] = (M.m[k] * x + M.m[4 + k] * y) + (M.m[8 + k] * z + M.m[12 + k] * 1.0f);
    }
    float *o = t9 + (size_t)i * 9;
    for (int j = 0; j < 3; ++j) { o[j] = v[0][j]; o[3 + j] = v[1][j] - v[0][j]; o[6 + j] = v[2][j] - v[0][j]; }
}

// identity of min over sortable uints = 0xffffffff, of max = 0: [min, min, min, max, max, max] per node; the status word of the quantiser cleared
__global__ void k_mesh_init(uint32_t *__restrict__ bounds, int nWords, uint32_t *__restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *status = 0u;
    if (i < nWords) bounds[i] = (i % 6) < 3 ? 0xffffffffu : 0u;
}

__device__ __forceinline__ float bnd(const uint32_t *__restrict__ bounds, int slot, int c) { return sortable2f(bounds[(size_t)slot * 6 + c]); }

__global__ void k_mesh_root(const uint32_t *__restrict__ bounds, float *__restrict__ rootBox) {
    if (threadIdx.x < 6) rootBox[threadIdx.x] = sortable2f(bounds[threadIdx.x]);
}

// 80-byte triangle-pair records (rt_upload_bvh): [v0 e1 e2][v0 e1 e2][index of the first][-]; a record with one triangle repeats the index in its tenth float
__global__ void k_mesh_pairs(const float4 *__restrict__ tris, const uint32_t *__restrict__ tab, int nPairs, float4 *__restrict__ pairs) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nPairs) return;
    const uint32_t e = tab[r], orig = e & 0x7fffffffu;
    const bool single = (e >> 31) != 0u;
    const float fo = __uint_as_float(orig);
    const float4 a0 = tris[(size_t)orig * 3], a1 = tris[(size_t)orig * 3 + 1], a2 = tris[(size_t)orig * 3 + 2];
    float4 *o = pairs + (size_t)r * 5;
    o[0] = make_float4(a0.x, a0.y, a0.z, a1.x);
    o[1] = make_float4(a1.y, a1.z, a2.x, a2.y);
    if (single) {
        o[2] = make_float4(a2.z, fo, 0.0f, 0.0f);
        o[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        o[4] = make_float4(0.0f, 0.0f, fo, 0.0f);
    } else {
        const float4 b0 = tris[(size_t)orig * 3 + 3], b1 = tris[(size_t)orig * 3 + 4], b2 = tris[(size_t)orig * 3 + 5];
        o[2] = make_float4(a2.z, b0.x, b0.y, b0.z);
        o[3] = make_float4(b1.x, b1.y, b1.z, b2.x);
        o[4] = make_float4(b2.y, b2.z, fo, 0.0f);
    }
}

// 64-byte two-child records in both reference encodings: [L.min, ref L][L.max, ref R][R.min, 0][R.max, 0]
__global__ void k_mesh_nodes2(const uint32_t *__restrict__ bounds, const Wn2Tab *__restrict__ tab, int nInner, float4 *__restrict__ wn, float4 *__restrict__ wnW) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nInner) return;
    const Wn2Tab t = tab[k];
    const float lx = bnd(bounds, t.slotL, 0), ly = bnd(bounds, t.slotL, 1), lz = bnd(bounds, t.slotL, 2);
    const float Lx = bnd(bounds, t.slotL, 3), Ly = bnd(bounds, t.slotL, 4), Lz = bnd(bounds, t.slotL, 5);
    const float4 q2 = make_float4(bnd(bounds, t.slotR, 0), bnd(bounds, t.slotR, 1), bnd(bounds, t.slotR, 2), 0.0f);
    const float4 q3 = make_float4(bnd(bounds, t.slotR, 3), bnd(bounds, t.slotR, 4), bnd(bounds, t.slotR, 5), 0.0f);
    float4 *o = wn + (size_t)k * 4, *w = wnW + (size_t)k * 4;
    o[0] = make_float4(lx, ly, lz, __int_as_float(t.refL)); o[1] = make_float4(Lx, Ly, Lz, __int_as_float(t.refR)); o[2] = q2; o[3] = q3;
    w[0] = make_float4(lx, ly, lz, __int_as_float(t.refLW)); w[1] = make_float4(Lx, Ly, Lz, __int_as_float(t.refRW)); w[2] = q2; w[3] = q3;
}

// 128-byte four-child any-hit records, component-wise with NaN boxes for absent children, and (q4 != null) the same node quantised by the function
// rt_upload_bvh quantises it with (rt_qnode.hpp).  A node that cannot be quantised sets *status; the host then walks the exact records, as after an
// upload.
__global__ void k_mesh_nodes4(const uint32_t *__restrict__ bounds, const W4Tab *__restrict__ tab, int n4, float4 *__restrict__ w4, uint4 *__restrict__ q4,
                              uint32_t *__restrict__ status) {
    const int nn = blockIdx.x * blockDim.x + threadIdx.x;
    if (nn >= n4) return;
    const W4Tab t = tab[nn];
    const float qnan = __uint_as_float(0x7fc00000u);
    float o[24];
    for (int i = 0; i < 4; ++i)
        for (int c = 0; c < 6; ++c) o[4 * c + i] = t.slot[i] >= 0 ? bnd(bounds, t.slot[i], c) : qnan;
    float4 *w = w4 + (size_t)nn * 8;
    for (int c = 0; c < 6; ++c) w[c] = make_float4(o[4 * c], o[4 * c + 1], o[4 * c + 2], o[4 * c + 3]);
    w[6] = make_float4(__int_as_float(t.ref[0]), __int_as_float(t.ref[1]), __int_as_float(t.ref[2]), __int_as_float(t.ref[3]));
    w[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!q4) return;
    uint32_t q[16];
    const bool okQ = rt_quantise_node4(o, t.ref, q);
    for (int i = 0; i < 4; ++i) q[12 + i] = (uint32_t)t.ref[i];
    if (!okQ) atomicOr(status, 1u);
    uint4 *d = q4 + (size_t)nn * 4;
    for (int k = 0; k < 4; ++k) d[k] = make_uint4(q[4 * k], q[4 * k + 1], q[4 * k + 2], q[4 * k + 3]);
}

// the leaves' exact boxes for the quantised walk: [lo.xyz hi.x][hi.yz 0 0]
__global__ void k_mesh_leafbox(const uint32_t *__restrict__ bounds, const LeafTab *__restrict__ tab, int nLeaves, float4 *__restrict__ leafBox) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nLeaves) return;
    const LeafTab t = tab[j];
    float4 *o = leafBox + (size_t)t.at * 2;
    o[0] = make_float4(bnd(bounds, t.slot, 0), bnd(bounds, t.slot, 1), bnd(bounds, t.slot, 2), bnd(bounds, t.slot, 3));
    o[1] = make_float4(bnd(bounds, t.slot, 4), bnd(bounds, t.slot, 5), 0.0f, 0.0f);
}

inline unsigned blocks_for(size_t n) { return (unsigned)std::max<size_t>(1, (n + 255) / 256); }

}  // namespace

namespace rtl {

int bvh_layout(int nTris, BvhLayout &out) {
    out = BvhLayout{};
    if (nTris <= 0) return RT_ERR_INVALID;
    if (nTris >= (1 << 28)) return RT_ERR_UNSUPPORTED;
    // a subtree's shape depends on its triangle count alone, and a level holds at most two distinct counts
    struct Sub { long long nodes, inner, pairs, leaves; int depth, minRec; };
    struct Wide { long long n4; int stack; };
    std::map<int, Sub> sub;
    std::map<int, Wide> wide;
    auto subOf = [&](auto &&self, int s) -> Sub {
        auto it = sub.find(s);
        if (it != sub.end()) return it->second;
        Sub r;
        if (s <= 8) r = {1, 0, (s + 1) / 2, 1, 1, (s + 1) / 2};
        else {
            const Sub a = self(self, s / 2), b = self(self, s - s / 2);
            r = {1 + a.nodes + b.nodes, 1 + a.inner + b.inner, a.pairs + b.pairs, a.leaves + b.leaves, 1 + std::max(a.depth, b.depth), std::min(a.minRec, b.minRec)};
        }
        sub[s] = r;
        return r;
    };
    // four-child record of an inner node of s triangles: it absorbs its inner children (rt_upload_bvh); stack need = children - 1 + the deepest inner child's
    auto wideOf = [&](auto &&self, int s) -> Wide {
        auto it = wide.find(s);
        if (it != wide.end()) return it->second;
        int kids[4], nk = 0;
        for (int ch : {s / 2, s - s / 2}) {
            if (ch <= 8) kids[nk++] = ch;
            else { kids[nk++] = ch / 2; kids[nk++] = ch - ch / 2; }
        }
        Wide r{1, 0};
        int deepest = 0;
        for (int i = 0; i < nk; ++i)
            if (kids[i] > 8) { const Wide k = self(self, kids[i]); r.n4 += k.n4; deepest = std::max(deepest, k.stack); }
        r.stack = std::max(nk - 1, 0) + deepest;
        wide[s] = r;
        return r;
    };
    const Sub root = subOf(subOf, nTris);
    if (root.depth > 32) return RT_ERR_UNSUPPORTED;
    out.nTris = nTris; out.nNodes = (int)root.nodes; out.nInner = (int)root.inner; out.treeDepth = root.depth;
    out.nPairs = (size_t)root.pairs; out.nLeaves = (size_t)root.leaves; out.minLeafRecords = root.minRec;
    if (out.nPairs + 8 >= ((size_t)1 << 28)) return RT_ERR_UNSUPPORTED;
    const int leafRef = -(((0 << 3) | (nTris - 1)) + 1);   // the root as a leaf: first = 0 in both encodings
    if (nTris <= 8) { out.nWide4 = 1; out.anyStack = 0; out.rootRef = out.rootRefW = out.rootRef4 = leafRef; }
    else { const Wide w = wideOf(wideOf, nTris); out.nWide4 = (size_t)w.n4; out.anyStack = std::max(w.stack, 1); out.rootRef = out.rootRefW = out.rootRef4 = 0; }
    return RT_OK;
}

// The device memory of one optional feature (skin, morph, motion, normals, colours, UVs, the texture): the blocks its create call allocated beyond `owned`, each with the
// member that points at it, and their byte count.  attach / detach below are the only code that allocates, counts and frees them.
struct Attachment {
    struct Block { void *mem; void *member; void (*forget)(void *member); };
    Block blocks[5] = {};
    int n = 0;
    size_t bytes = 0;
};

struct Mesh {
    BvhLayout lay;
    MeshScene sc;
    int nVerts = 0, nLevels = 0;
    bool quantised = false;
    std::vector<int> levelOff, levelSegs;   // per level: first bounds slot / segment, number of nodes
    std::vector<char> levelInner;           // per level: some node of it is split
    // geometry and build scratch
    float *dPos = nullptr, *dT9 = nullptr, *dMn = nullptr, *dMx = nullptr, *dCen = nullptr;
    uint32_t *dIdx = nullptr, *dBounds = nullptr, *dStatus = nullptr;
    int *dPerm[2] = {nullptr, nullptr}, *dSegB = nullptr, *dSegE = nullptr, *dSegI = nullptr, *dOut = nullptr;
    unsigned long long *dKeys[2] = {nullptr, nullptr};
    void *dTemp = nullptr;
    size_t tempBytes = 0;
    // index tables
    uint32_t *dPairTab = nullptr;
    Wn2Tab *dWn2Tab = nullptr;
    W4Tab *dW4Tab = nullptr;
    LeafTab *dLeafTab = nullptr;
    RefitLeaf *dRefitLeaf = nullptr;
    RefitKids *dRefitKids = nullptr;
    // parts: boundaries in triangle units (host copy and device), the part of every input triangle, one model matrix per part
    std::vector<int32_t> partFirst;
    int32_t *dPartFirst = nullptr;
    uint16_t *dPartOf = nullptr;
    float *dPartM = nullptr;
    // skin: rest positions, four bone indices and weights per vertex, one matrix per bone; allocated by mesh_skin_create, not in `owned`
    float *dRest = nullptr, *dSkinW = nullptr, *dBones = nullptr;
    uint16_t *dSkinIdx = nullptr;
    int nBones = 0;
    Attachment skin;
    // morph targets: base positions, the packed records with their slice table, one weight per target; allocated by
    // mesh_morph_create, not in `owned`
    float *dMorphBase = nullptr, *dMorphW = nullptr;
    uint32_t *dMorphSliceFirst = nullptr;
    void *dMorphEntries = nullptr;
    RtMorphInfo morph = {};   // nTargets == 0: no morph
    Attachment morphMem;
    // previous pose: the rows before the most recent update, in the current order, and the old rows by input triangle a rebuild
    // carries them across in; allocated by mesh_motion_create, not in `owned`
    float4 *dPrevTris = nullptr, *dPrevByInput = nullptr;
    Attachment motion;
    // the corner attributes, indexed by Corner -- smooth normals, colours, UVs: one value per vertex and the corner values row for row
    // beside the triangle array, corner_kind's bytes each; allocated by mesh_normals_create and mesh_corner_create, not in `owned`
    struct CornerArrays { void *vert = nullptr; float4 *rows = nullptr; Attachment mem; };
    CornerArrays corner[3];
    // what the normals are computed from: the packed vertex -> triangle adjacency and the face vectors by input triangle; with
    // the normals' attachment
    uint32_t *dNrmSliceFirst = nullptr;
    int32_t *dNrmEntries = nullptr;
    float4 *dFaceByInput = nullptr;
    // the albedo texture: the texels and the decode table behind `tex` (mesh_texture_create), not in `owned`
    uint32_t *dTexels = nullptr;
    float *dTexTable = nullptr;
    rtuv::Texture tex;   // texels == null: no texture
    Attachment texture;
    // the tree a refit keeps: which of dPerm holds the last rebuild's permutation (-1: no rebuild yet); the other one is idle until the next rebuild
    // and holds, once asked for, the row -> input triangle map
    int permCur = -1;
    bool orderValid = false;
    uint32_t *hStatus = nullptr;   // pinned
    // quality measurements: per result slot its accumulators on the device, its pinned record and the event behind the copy
    unsigned long long *dQAcc = nullptr;
    char *hQRec = nullptr;         // pinned
    hipEvent_t evQ[kQualityRing] = {};
    std::vector<void *> owned;
    uint64_t allocations = 0;
    size_t scratchBytes = 0, sceneBytes = 0;
};

namespace {
template <class T> hipError_t dev_alloc(Mesh *m, T **p, size_t bytes, bool scene, bool zero) {
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(bytes, 16));
    if (e != hipSuccess) return e;
    m->owned.push_back(q);
    ++m->allocations;
    (scene ? m->sceneBytes : m->scratchBytes) += bytes;
    *p = reinterpret_cast<T *>(q);
    return zero ? hipMemset(q, 0, std::max<size_t>(bytes, 16)) : hipSuccess;
}
template <class T> hipError_t dev_upload(Mesh *m, T **p, const std::vector<T> &v) {
    hipError_t e = dev_alloc(m, p, v.size() * sizeof(T), false, false);
    if (e != hipSuccess || v.empty()) return e;
    return hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// One block of an attachment behind *p: at least 16 bytes, counted as one allocation and with the bytes asked for in scratchBytes; filled from host or
// device memory (nothing to copy when bytes == 0) or with zeros (all of the block; also what a null source means).  Synchronous: the create calls end
// with hipDeviceSynchronize.
enum class Fill { host, device, zeros };
template <class T> hipError_t attach(Mesh *m, Attachment &a, T **p, size_t bytes, Fill fill, const void *src = nullptr) {
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(bytes, 16));
    if (e != hipSuccess) return e;
    a.blocks[a.n++] = {q, p, [](void *member) { *static_cast<T **>(member) = nullptr; }};
    *p = static_cast<T *>(q);
    ++m->allocations;
    a.bytes += bytes; m->scratchBytes += bytes;
    if (fill == Fill::zeros || !src) return hipMemset(q, 0, std::max<size_t>(bytes, 16));   // (no source: an empty table, its 16 bytes zero)
    return bytes ? hipMemcpy(q, src, bytes, fill == Fill::host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice) : hipSuccess;
}
// ... and all of them freed, their members null, their bytes out of scratchBytes (allocations counts what was ever allocated)
void detach(Mesh *m, Attachment &a) {
    for (int i = 0; i < a.n; ++i) { (void)hipFree(a.blocks[i].mem); a.blocks[i].forget(a.blocks[i].member); }
    m->scratchBytes -= a.bytes;
    a = Attachment{};
}
}  // namespace

#define MESH_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { if (err) *err = hipGetErrorString(e_); mesh_destroy(m); return RT_ERR_HIP; } } while (0)

int mesh_create(const float *positions, int nVerts, const uint32_t *indices, int nIdx, const int32_t *partFirst, int nParts, bool quantised, bool sparseLeafBoxes,
                Mesh **out, const char **err) {
    *out = nullptr;
    const int n = nIdx / 3;
    Mesh *m = new Mesh();
    m->nVerts = nVerts; m->quantised = quantised;
    int rc = bvh_layout(n, m->lay);
    if (rc != RT_OK) { delete m; return rc; }
    // ---- the topology, node by node: rt_upload_bvh's derivations on the skeleton
    std::vector<SkNode> sk;
    skeleton(n, sk);
    const int nNodes = (int)sk.size();
    auto countOf = [&](int i) { return sk[(size_t)i].left < 0 ? sk[(size_t)i].end - sk[(size_t)i].begin : 0; };
    int maxDepth = 0;
    for (const SkNode &nd : sk) maxDepth = std::max(maxDepth, nd.depth);
    m->nLevels = maxDepth + 1;
    std::vector<std::vector<int>> byDepth((size_t)maxDepth + 1);
    for (int i = 0; i < nNodes; ++i) byDepth[(size_t)sk[(size_t)i].depth].push_back(i);
    for (auto &v : byDepth) std::sort(v.begin(), v.end(), [&](int a, int b) { return sk[(size_t)a].begin < sk[(size_t)b].begin; });
    std::vector<int> slotOf((size_t)nNodes), segB, segE, segI;
    for (int d = 0; d <= maxDepth; ++d) {
        m->levelOff.push_back((int)segB.size());
        m->levelSegs.push_back((int)byDepth[(size_t)d].size());
        bool anyInner = false;
        for (int id : byDepth[(size_t)d]) {
            const SkNode &nd = sk[(size_t)id];
            slotOf[(size_t)id] = (int)segB.size();
            segB.push_back(nd.begin); segE.push_back(nd.end); segI.push_back(nd.left >= 0);
            anyInner = anyInner || nd.left >= 0;
        }
        m->levelInner.push_back(anyInner ? 1 : 0);
    }
    std::vector<int> outOfPos((size_t)n);
    for (const SkNode &nd : sk)
        if (nd.left < 0) for (int k = 0; k < nd.end - nd.begin; ++k) outOfPos[(size_t)(nd.begin + k)] = nd.firstOut + k;
    std::vector<int> innerIdx((size_t)nNodes, -1), pairRefOf((size_t)nNodes, 0);
    int nInner = 0;
    std::vector<uint32_t> pairTab;
    int rmin = 8;
    size_t nLeaves = 0;
    for (int i = 0; i < nNodes; ++i) {
        const int cnt = countOf(i);
        if (cnt <= 0) { innerIdx[(size_t)i] = nInner++; continue; }
        ++nLeaves;
        rmin = std::min(rmin, (cnt + 1) / 2);
        const size_t rec = pairTab.size();
        pairRefOf[(size_t)i] = -((int)((rec << 3) | (size_t)(cnt - 1)) + 1);
        for (int t = 0; t < cnt; t += 2) pairTab.push_back((uint32_t)(sk[(size_t)i].firstOut + t) | (t + 1 >= cnt ? 0x80000000u : 0u));
    }
    auto refOf = [&](int node) { const int cnt = countOf(node); return cnt > 0 ? -(((sk[(size_t)node].firstOut << 3) | (cnt - 1)) + 1) : innerIdx[(size_t)node]; };
    auto refOfW = [&](int node) { return countOf(node) > 0 ? pairRefOf[(size_t)node] : innerIdx[(size_t)node]; };
    std::vector<Wn2Tab> wn2((size_t)nInner);
    for (int i = 0; i < nNodes; ++i) {
        if (innerIdx[(size_t)i] < 0) continue;
        const int L = sk[(size_t)i].left, R = sk[(size_t)i].right;
        wn2[(size_t)innerIdx[(size_t)i]] = {slotOf[(size_t)L], slotOf[(size_t)R], refOf(L), refOf(R), refOfW(L), refOfW(R)};
    }
    std::vector<RefitLeaf> refitLeaf;
    std::vector<RefitKids> refitKids((size_t)nNodes);
    for (int i = 0; i < nNodes; ++i) {
        if (countOf(i) > 0) { refitLeaf.push_back({slotOf[(size_t)i], sk[(size_t)i].firstOut, countOf(i)}); refitKids[(size_t)slotOf[(size_t)i]] = {-1, -1}; }
        else refitKids[(size_t)slotOf[(size_t)i]] = {slotOf[(size_t)sk[(size_t)i].left], slotOf[(size_t)sk[(size_t)i].right]};
    }
    std::vector<W4Tab> w4;
    int anyStack = 0;
    if (countOf(0) <= 0) {
        for (const Wide4 &w : collapse_to_four([&](int i) { return sk[(size_t)i].left; }, [&](int i) { return sk[(size_t)i].right; }, countOf, refOfW)) {
            W4Tab t;
            for (int i = 0; i < 4; ++i) { t.slot[i] = w.kid[i] >= 0 ? slotOf[(size_t)w.kid[i]] : -1; t.ref[i] = w.ref[i]; }
            w4.push_back(t);
        }
        anyStack = any_stack_need(w4.size(), [&](size_t nn, int i) { return w4[nn].ref[i]; });
    }
    const BvhLayout &L = m->lay;
    if (nNodes != L.nNodes || nInner != L.nInner || maxDepth + 1 != L.treeDepth || pairTab.size() != L.nPairs || std::max<size_t>(w4.size(), 1) != L.nWide4 ||
        anyStack != L.anyStack || nLeaves != L.nLeaves || rmin != L.minLeafRecords || refOf(0) != L.rootRef || refOfW(0) != L.rootRefW) {
        if (err) *err = "internal: the layout of the count and the layout of the skeleton disagree";
        delete m;
        return RT_ERR_STATE;
    }
    std::vector<LeafTab> leafTab;
    size_t leafBoxFloats = 0;
    if (quantised) {
        const LeafBoxRule rule(rmin, sparseLeafBoxes);
        m->sc.leafBoxMagic = rule.magic;
        leafBoxFloats = rule.floats(L.nPairs + 8);
        for (int i = 0; i < nNodes; ++i) {
            if (countOf(i) <= 0) continue;
            const size_t at = rule.index((size_t)(-pairRefOf[(size_t)i] - 1) >> 3);
            if (at * 8 + 8 > leafBoxFloats) { if (err) *err = "internal: leaf-box index out of range"; delete m; return RT_ERR_STATE; }
            leafTab.push_back({slotOf[(size_t)i], (uint32_t)at});
        }
        m->sc.leafBoxBytes = leafBoxFloats * 4;
    }
    // ---- device memory: geometry, tables, build scratch, scene arrays (padding zeroed here, once)
    const size_t N = (size_t)n;
    MESH_TRY(dev_alloc(m, &m->dPos, (size_t)nVerts * 12, false, false));
    MESH_TRY(hipMemcpy(m->dPos, positions, (size_t)nVerts * 12, hipMemcpyHostToDevice));
    MESH_TRY(dev_alloc(m, &m->dIdx, N * 12, false, false));
    MESH_TRY(hipMemcpy(m->dIdx, indices, N * 12, hipMemcpyHostToDevice));
    MESH_TRY(dev_upload(m, &m->dSegB, segB)); MESH_TRY(dev_upload(m, &m->dSegE, segE)); MESH_TRY(dev_upload(m, &m->dSegI, segI));
    MESH_TRY(dev_upload(m, &m->dOut, outOfPos));
    MESH_TRY(dev_upload(m, &m->dPairTab, pairTab)); MESH_TRY(dev_upload(m, &m->dWn2Tab, wn2)); MESH_TRY(dev_upload(m, &m->dW4Tab, w4));
    if (quantised) MESH_TRY(dev_upload(m, &m->dLeafTab, leafTab));
    MESH_TRY(dev_upload(m, &m->dRefitLeaf, refitLeaf)); MESH_TRY(dev_upload(m, &m->dRefitKids, refitKids));
    {   // parts: an empty part owns no triangle, so the lookup never names one
        m->partFirst.assign(partFirst, partFirst + nParts + 1);
        std::vector<uint16_t> partOf(N);
        std::vector<float> ident((size_t)nParts * 16, 0.0f);
        for (int p = 0; p < nParts; ++p) {
            for (int t = partFirst[p]; t < partFirst[p + 1]; ++t) partOf[(size_t)t] = (uint16_t)p;
            for (int k = 0; k < 4; ++k) ident[(size_t)p * 16 + 5 * k] = 1.0f;
        }
        MESH_TRY(dev_upload(m, &m->dPartFirst, m->partFirst)); MESH_TRY(dev_upload(m, &m->dPartOf, partOf)); MESH_TRY(dev_upload(m, &m->dPartM, ident));
    }
    MESH_TRY(dev_alloc(m, &m->dT9, N * 36, false, false));
    MESH_TRY(dev_alloc(m, &m->dMn, N * 12, false, false)); MESH_TRY(dev_alloc(m, &m->dMx, N * 12, false, false)); MESH_TRY(dev_alloc(m, &m->dCen, N * 12, false, false));
    MESH_TRY(dev_alloc(m, &m->dPerm[0], N * 4, false, false)); MESH_TRY(dev_alloc(m, &m->dPerm[1], N * 4, false, false));
    MESH_TRY(dev_alloc(m, &m->dKeys[0], N * 8, false, false)); MESH_TRY(dev_alloc(m, &m->dKeys[1], N * 8, false, false));
    MESH_TRY(dev_alloc(m, &m->dBounds, (size_t)nNodes * 24, false, false));
    MESH_TRY(dev_alloc(m, &m->dStatus, 16, false, true));
    {
        rocprim::double_buffer<unsigned long long> kb(m->dKeys[0], m->dKeys[1]);
        rocprim::double_buffer<int> vb(m->dPerm[0], m->dPerm[1]);
        MESH_TRY(rocprim::radix_sort_pairs(nullptr, m->tempBytes, kb, vb, N, 0, 64, (hipStream_t) nullptr));
        MESH_TRY(dev_alloc(m, reinterpret_cast<char **>(&m->dTemp), std::max<size_t>(m->tempBytes, 16), false, false));
    }
    MESH_TRY(hipHostMalloc(reinterpret_cast<void **>(&m->hStatus), 16, hipHostMallocDefault));
    ++m->allocations;
    *m->hStatus = 0u;
    MESH_TRY(dev_alloc(m, &m->dQAcc, kQualityRing * kQualityRecordBytes, false, true));
    MESH_TRY(hipHostMalloc(reinterpret_cast<void **>(&m->hQRec), kQualityRing * kQualityRecordBytes, hipHostMallocDefault));
    ++m->allocations;
    std::memset(m->hQRec, 0, kQualityRing * kQualityRecordBytes);
    for (int i = 0; i < kQualityRing; ++i) { MESH_TRY(hipEventCreateWithFlags(&m->evQ[i], hipEventDisableTiming)); ++m->allocations; }
    MESH_TRY(dev_alloc(m, &m->sc.wnodes, (size_t)std::max(nInner, 1) * 64, true, true));
    MESH_TRY(dev_alloc(m, &m->sc.wnodesW, (size_t)std::max(nInner, 1) * 64, true, true));
    MESH_TRY(dev_alloc(m, &m->sc.w4, L.nWide4 * 128, true, true));
    MESH_TRY(dev_alloc(m, &m->sc.pairs, (L.nPairs + 8) * 80, true, true));
    MESH_TRY(dev_alloc(m, &m->sc.tris, (N + 8) * 48, true, true));
    MESH_TRY(dev_alloc(m, &m->sc.rootBox, 32, true, true));
    if (quantised) {
        MESH_TRY(dev_alloc(m, &m->sc.q4, L.nWide4 * 64, true, true));
        MESH_TRY(dev_alloc(m, &m->sc.leafBox, leafBoxFloats * 4, true, true));
    }
    MESH_TRY(hipDeviceSynchronize());
    *out = m;
    return RT_OK;
}

void mesh_destroy(Mesh *m) {
    if (!m) return;
    mesh_skin_release(m);
    mesh_morph_release(m);
    mesh_motion_release(m);
    for (Corner which : {Corner::normals, Corner::colors, Corner::uvs}) mesh_corner_release(m, which);
    mesh_texture_release(m);
    for (void *p : m->owned) (void)hipFree(p);
    if (m->hStatus) (void)hipHostFree(m->hStatus);
    if (m->hQRec) (void)hipHostFree(m->hQRec);
    for (hipEvent_t e : m->evQ) if (e) (void)hipEventDestroy(e);
    delete m;
}

const BvhLayout &mesh_layout(const Mesh *m) { return m->lay; }
const MeshScene &mesh_scene(const Mesh *m) { return m->sc; }
float *mesh_positions(Mesh *m) { return m->dPos; }
int mesh_verts(const Mesh *m) { return m->nVerts; }
int mesh_part_count(const Mesh *m) { return (int)m->partFirst.size() - 1; }
const int32_t *mesh_part_first(const Mesh *m) { return m->partFirst.data(); }
float *mesh_part_matrices(Mesh *m) { return m->dPartM; }
const uint32_t *mesh_indices(const Mesh *m) { return m->dIdx; }
const uint16_t *mesh_part_of(const Mesh *m) { return m->dPartOf; }
uint64_t mesh_allocations(const Mesh *m) { return m->allocations; }
size_t mesh_scratch_bytes(const Mesh *m) { return m->scratchBytes; }
size_t mesh_scene_bytes(const Mesh *m) { return m->sceneBytes; }

#define REB_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { if (err) *err = hipGetErrorString(e_); return RT_ERR_HIP; } } while (0)

namespace {
// the tail of an update behind its new rows: the corner attributes that are enabled, in Corner's order and under the same order array --
// a rebuild moved every input triangle to another row; a refit's gather rewrites what it finds, which is what a caller who also changed colours or
// UVs wants
int attributes_update(Mesh *m, hipStream_t st, const char **err) {
    for (Corner which : {Corner::normals, Corner::colors, Corner::uvs}) {
        if (!m->corner[(int)which].rows) continue;
        const int rc = mesh_corner_refresh(m, which, st, err);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}
// every record form from the bounds and the triangle array, through the tables: the tail of a rebuild and of a refit
void emit_records(Mesh *m, hipStream_t st) {
    const BvhLayout &L = m->lay;
    hipLaunchKernelGGL(k_mesh_root, dim3(1), dim3(64), 0, st, m->dBounds, m->sc.rootBox);
    hipLaunchKernelGGL(k_mesh_pairs, dim3(blocks_for(L.nPairs)), dim3(256), 0, st, m->sc.tris, m->dPairTab, (int)L.nPairs, m->sc.pairs);
    if (L.nInner > 0) {
        hipLaunchKernelGGL(k_mesh_nodes2, dim3(blocks_for((size_t)L.nInner)), dim3(256), 0, st, m->dBounds, m->dWn2Tab, L.nInner, m->sc.wnodes, m->sc.wnodesW);
        hipLaunchKernelGGL(k_mesh_nodes4, dim3(blocks_for(L.nWide4)), dim3(256), 0, st, m->dBounds, m->dW4Tab, (int)L.nWide4, m->sc.w4,
                           reinterpret_cast<uint4 *>(m->sc.q4), m->dStatus);
        if (m->quantised)
            hipLaunchKernelGGL(k_mesh_leafbox, dim3(blocks_for(L.nLeaves)), dim3(256), 0, st, m->dBounds, m->dLeafTab, (int)L.nLeaves, m->sc.leafBox);
    }
}
}  // namespace

int mesh_rebuild(Mesh *m, hipStream_t st, const float *M16, const char **err) {
    const BvhLayout &L = m->lay;
    const int n = L.nTris;
    const unsigned gN = blocks_for((size_t)n);
    // previous pose: the rows that are about to be replaced, filed by input triangle while the old permutation still stands
    const bool carry = m->dPrevTris && m->permCur >= 0;
    if (carry) motion_launch_scatter(st, m->sc.tris, m->dPerm[m->permCur], m->dOut, n, m->dPrevByInput);
    m->permCur = -1; m->orderValid = false;   // the sorts below use both permutation buffers
    if (M16) {
        Mat16 M;
        std::memcpy(M.m, M16, sizeof M.m);
        hipLaunchKernelGGL(k_mesh_gather, dim3(gN), dim3(256), 0, st, m->dPos, m->dIdx, n, M, m->dT9);
    } else parts_launch_gather(st, m->dPos, m->dIdx, m->dPartOf, m->dPartM, n, m->dT9);
    hipLaunchKernelGGL(k_mesh_init, dim3(blocks_for((size_t)L.nNodes * 6)), dim3(256), 0, st, m->dBounds, L.nNodes * 6, m->dStatus);
    hipLaunchKernelGGL(k_tri_prep, dim3(gN), dim3(256), 0, st, m->dT9, n, m->dMn, m->dMx, m->dCen);
    hipLaunchKernelGGL(k_iota, dim3(gN), dim3(256), 0, st, m->dPerm[0], n);
    int cur = 0;
    for (int d = 0; d < m->nLevels; ++d) {   // the level loop of build_bvh_gpu (rt_bvh_gpu.hip) with its segment tables and bounds resident
        const int off = m->levelOff[(size_t)d], nSeg = m->levelSegs[(size_t)d];
        uint32_t *bounds = m->dBounds + (size_t)off * 6;
        hipLaunchKernelGGL(k_level_bounds, dim3(gN), dim3(256), 0, st, m->dPerm[cur], n, m->dMn, m->dMx, m->dSegB + off, m->dSegE + off, nSeg, bounds);
        if (!m->levelInner[(size_t)d]) continue;
        hipLaunchKernelGGL(k_level_keys, dim3(gN), dim3(256), 0, st, m->dPerm[cur], n, m->dCen, m->dSegB + off, m->dSegE + off, m->dSegI + off, nSeg, bounds,
                           m->dKeys[cur]);
        rocprim::double_buffer<unsigned long long> kb(m->dKeys[cur], m->dKeys[cur ^ 1]);
        rocprim::double_buffer<int> vb(m->dPerm[cur], m->dPerm[cur ^ 1]);
        REB_TRY(rocprim::radix_sort_pairs(m->dTemp, m->tempBytes, kb, vb, (size_t)n, 0, 64, st));
        cur = (vb.current() == m->dPerm[0]) ? 0 : 1;
    }
    hipLaunchKernelGGL(k_emit_tris, dim3(gN), dim3(256), 0, st, m->dT9, m->dPerm[cur], m->dOut, n, reinterpret_cast<float *>(m->sc.tris));
    emit_records(m, st);
    REB_TRY(hipGetLastError());
    if (m->dPrevTris) {   // ... and handed out in the new order; the first rebuild has no old rows: the new ones, zero motion
        if (carry) { motion_launch_gather(st, m->dPrevByInput, m->dPerm[cur], m->dOut, n, m->dPrevTris); REB_TRY(hipGetLastError()); }
        else REB_TRY(hipMemcpyAsync(m->dPrevTris, m->sc.tris, (size_t)n * 48, hipMemcpyDeviceToDevice, st));
    }
    m->permCur = cur;
    return attributes_update(m, st, err);
}

bool mesh_has_tree(const Mesh *m) { return m->permCur >= 0; }

int mesh_refit(Mesh *m, hipStream_t st, const float *M16, const char **err) {
    if (m->permCur < 0) return RT_ERR_INVALID;
    const BvhLayout &L = m->lay;
    const int n = L.nTris;
    // previous pose: a refit keeps every input triangle in its row, so the rows that are about to be rewritten are copied as they lie
    if (m->dPrevTris) REB_TRY(hipMemcpyAsync(m->dPrevTris, m->sc.tris, (size_t)n * 48, hipMemcpyDeviceToDevice, st));
    if (M16) refit_launch_tris(st, m->dPos, m->dIdx, m->dPerm[m->permCur], m->dOut, n, M16, m->sc.tris);
    else parts_launch_refit_tris(st, m->dPos, m->dIdx, m->dPerm[m->permCur], m->dOut, m->dPartOf, m->dPartM, n, m->sc.tris);
    refit_launch_leaves(st, m->sc.tris, m->dRefitLeaf, (int)L.nLeaves, m->dBounds, m->dStatus);
    for (int d = m->nLevels - 2; d >= 0; --d) {   // bottom-up, one launch per level: a kernel boundary makes the children's boxes visible
        if (!m->levelInner[(size_t)d]) continue;
        const int nSeg = m->levelSegs[(size_t)d];
        refit_launch_inner(st, m->dRefitKids, m->levelOff[(size_t)d], nSeg, m->dBounds);
    }
    emit_records(m, st);
    REB_TRY(hipGetLastError());
    return attributes_update(m, st, err);
}

int mesh_order(Mesh *m, hipStream_t st, const int **order, const char **err) {
    if (m->permCur < 0) return RT_ERR_INVALID;
    int *dst = m->dPerm[m->permCur ^ 1];
    if (!m->orderValid) {
        refit_launch_order(st, m->dPerm[m->permCur], m->dOut, m->lay.nTris, dst);
        REB_TRY(hipGetLastError());
        m->orderValid = true;
    }
    *order = dst;
    return RT_OK;
}

bool mesh_order_written(const Mesh *m) { return m->permCur >= 0 && m->orderValid; }

int mesh_hit_parts(Mesh *m, hipStream_t st, const int *order, const void *hits, int n, int32_t *parts, int32_t *tris, const char **err) {
    if (m->permCur < 0) return RT_ERR_INVALID;
    parts_launch_hit_parts(st, hits, n, order, m->lay.nTris, m->dPartOf, m->dPartFirst, parts, tris);
    REB_TRY(hipGetLastError());
    return RT_OK;
}

int mesh_measure(Mesh *m, hipStream_t st, int slot, const char **err) {
    if (m->permCur < 0 || slot < 0 || slot >= kQualityRing) return RT_ERR_INVALID;
    const BvhLayout &L = m->lay;
    REB_TRY(quality_launch(st, m->dBounds, m->dRefitKids, L.nNodes, m->dRefitLeaf, (int)L.nLeaves, m->dQAcc + (size_t)slot * (kQualityRecordBytes / 8),
                           m->hQRec + (size_t)slot * kQualityRecordBytes));
    REB_TRY(hipEventRecord(m->evQ[slot], st));
    return RT_OK;
}

hipEvent_t mesh_quality_event(const Mesh *m, int slot) { return m->evQ[slot]; }
const QualityRecord *mesh_quality_record(const Mesh *m, int slot) { return reinterpret_cast<const QualityRecord *>(m->hQRec + (size_t)slot * kQualityRecordBytes); }

void mesh_skin_release(Mesh *m) {
    detach(m, m->skin);
    m->nBones = 0;
}

int mesh_skin_create(Mesh *m, const float *rest, const uint16_t *boneIdx4, const float *weights4, int nBones, const char **err) {
    mesh_skin_release(m);
    const size_t nv = (size_t)m->nVerts;
    std::vector<float> ident((size_t)nBones * 16, 0.0f);
    for (int b = 0; b < nBones; ++b)
        for (int k = 0; k < 4; ++k) ident[(size_t)b * 16 + 5 * k] = 1.0f;
    Attachment &a = m->skin;
    hipError_t e = rest ? attach(m, a, &m->dRest, nv * 12, Fill::host, rest) : attach(m, a, &m->dRest, nv * 12, Fill::device, m->dPos);
    if (e == hipSuccess) e = attach(m, a, &m->dSkinIdx, nv * RT_SKIN_INFLUENCES * sizeof(uint16_t), Fill::host, boneIdx4);
    if (e == hipSuccess) e = attach(m, a, &m->dSkinW, nv * RT_SKIN_INFLUENCES * sizeof(float), Fill::host, weights4);
    if (e == hipSuccess) e = attach(m, a, &m->dBones, ident.size() * sizeof(float), Fill::host, ident.data());
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { if (err) *err = hipGetErrorString(e); mesh_skin_release(m); return RT_ERR_HIP; }
    m->nBones = nBones;
    return RT_OK;
}

int mesh_bone_count(const Mesh *m) { return m->nBones; }
float *mesh_bones(Mesh *m) { return m->dBones; }
float *mesh_rest_positions(Mesh *m) { return m->dRest; }

int mesh_skin(Mesh *m, hipStream_t st, const char **err) {
    if (m->nBones <= 0) return RT_ERR_INVALID;
    skin_launch(st, m->dRest, m->dSkinIdx, m->dSkinW, m->dBones, m->nVerts, m->dPos);
    REB_TRY(hipGetLastError());
    return RT_OK;
}

void mesh_morph_release(Mesh *m) {
    detach(m, m->morphMem);
    m->morph = RtMorphInfo{};
}

int mesh_morph_create(Mesh *m, const float *base, const uint32_t *sliceFirst, const void *records, const RtMorphInfo &info, const char **err) {
    mesh_morph_release(m);
    const size_t nv = (size_t)m->nVerts;
    Attachment &a = m->morphMem;
    hipError_t e = base ? attach(m, a, &m->dMorphBase, nv * 12, Fill::host, base)
                        : attach(m, a, &m->dMorphBase, nv * 12, Fill::device, m->nBones > 0 ? m->dRest : m->dPos);
    if (e == hipSuccess) e = attach(m, a, &m->dMorphSliceFirst, ((size_t)info.nSlices + 1) * 4, Fill::host, sliceFirst);
    if (e == hipSuccess) e = attach(m, a, &m->dMorphEntries, (size_t)info.paddedEntries * 16, Fill::host, records);
    if (e == hipSuccess) e = attach(m, a, &m->dMorphW, (size_t)info.nTargets * 4, Fill::zeros);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { if (err) *err = hipGetErrorString(e); mesh_morph_release(m); return RT_ERR_HIP; }
    m->morph = info;
    return RT_OK;
}

int mesh_morph_target_count(const Mesh *m) { return m->morph.nTargets; }
const RtMorphInfo &mesh_morph_info(const Mesh *m) { return m->morph; }
float *mesh_morph_base(Mesh *m) { return m->dMorphBase; }
float *mesh_morph_weights(Mesh *m) { return m->dMorphW; }

int mesh_morph(Mesh *m, hipStream_t st, bool toRest, const char **err) {
    if (m->morph.nTargets <= 0 || (toRest && m->nBones <= 0)) return RT_ERR_INVALID;
    morph_launch(st, m->dMorphBase, m->dMorphSliceFirst, m->dMorphEntries, m->dMorphW, m->nVerts, toRest ? m->dRest : m->dPos);
    REB_TRY(hipGetLastError());
    return RT_OK;
}

void mesh_motion_release(Mesh *m) { detach(m, m->motion); }

int mesh_motion_create(Mesh *m, const char **err) {
    mesh_motion_release(m);
    const size_t bytes = (size_t)m->lay.nTris * 48;
    hipError_t e = attach(m, m->motion, &m->dPrevTris, bytes, Fill::zeros);
    if (e == hipSuccess) e = attach(m, m->motion, &m->dPrevByInput, bytes, Fill::zeros);
    if (e == hipSuccess && m->permCur >= 0) e = hipMemcpy(m->dPrevTris, m->sc.tris, bytes, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { if (err) *err = hipGetErrorString(e); mesh_motion_release(m); return RT_ERR_HIP; }
    return RT_OK;
}

const float4 *mesh_prev_tris(const Mesh *m) { return m->dPrevTris; }

int mesh_motion_latch(Mesh *m, hipStream_t st, const char **err) {
    if (!m->dPrevTris || m->permCur < 0) return RT_ERR_INVALID;
    REB_TRY(hipMemcpyAsync(m->dPrevTris, m->sc.tris, (size_t)m->lay.nTris * 48, hipMemcpyDeviceToDevice, st));
    return RT_OK;
}

int mesh_hit_prev_points(Mesh *m, hipStream_t st, const void *hits, const float *points, int n, float *prevPoints, const char **err) {
    if (!m->dPrevTris || m->permCur < 0) return RT_ERR_INVALID;
    motion_launch_hit_prev_points(st, hits, points, n, m->sc.tris, m->dPrevTris, m->lay.nTris, prevPoints);
    REB_TRY(hipGetLastError());
    return RT_OK;
}

// ---- the corner attributes
void mesh_corner_release(Mesh *m, Corner which) { detach(m, m->corner[(int)which].mem); }

namespace {
// The attribute's two arrays, zeroed, behind the blocks its attachment already holds (e: what allocating those gave), the colours' grey fill, the
// rows at once when there is a tree, and the wait for the device.  A failure releases the attribute.
int corner_create(Mesh *m, Corner which, hipStream_t st, hipError_t e, const char **err) {
    Mesh::CornerArrays &a = m->corner[(int)which];
    const CornerKind &k = corner_kind(which);
    if (e == hipSuccess) e = attach(m, a.mem, &a.vert, (size_t)m->nVerts * k.vertBytes, Fill::zeros);
    if (e == hipSuccess) e = attach(m, a.mem, &a.rows, (size_t)m->lay.nTris * k.rowBytes, Fill::zeros);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && which == Corner::colors) { corner_launch_color_fill(st, static_cast<float4 *>(a.vert), m->nVerts); e = hipGetLastError(); }
    int rc = RT_OK;
    if (e == hipSuccess && m->permCur >= 0) rc = mesh_corner_refresh(m, which, st, err);
    if (e == hipSuccess && rc == RT_OK) e = hipDeviceSynchronize();
    if (rc != RT_OK || e != hipSuccess) { if (rc == RT_OK && err) *err = hipGetErrorString(e); mesh_corner_release(m, which); return rc != RT_OK ? rc : RT_ERR_HIP; }
    return RT_OK;
}
}  // namespace

int mesh_corner_create(Mesh *m, Corner which, hipStream_t st, const char **err) {
    if (which == Corner::normals) return RT_ERR_INVALID;   // (mesh_normals_create: they need their adjacency)
    mesh_corner_release(m, which);
    return corner_create(m, which, st, hipSuccess, err);
}

int mesh_normals_create(Mesh *m, hipStream_t st, const uint32_t *sliceFirst, const int32_t *entries, const RtNormalInfo &info, const char **err) {
    mesh_corner_release(m, Corner::normals);
    Attachment &a = m->corner[(int)Corner::normals].mem;
    hipError_t e = attach(m, a, &m->dNrmSliceFirst, ((size_t)info.nSlices + 1) * 4, Fill::host, sliceFirst);
    if (e == hipSuccess) e = attach(m, a, &m->dNrmEntries, (size_t)info.paddedEntries * 4, Fill::host, entries);
    if (e == hipSuccess) e = attach(m, a, &m->dFaceByInput, (size_t)m->lay.nTris * 16, Fill::zeros);
    return corner_create(m, Corner::normals, st, e, err);
}

void *mesh_corner_vertices(const Mesh *m, Corner which) { return m->corner[(int)which].vert; }
const float4 *mesh_vertex_normals(const Mesh *m) { return static_cast<const float4 *>(m->corner[(int)Corner::normals].vert); }
const float4 *mesh_normal_rows(const Mesh *m) { return m->corner[(int)Corner::normals].rows; }
float4 *mesh_vertex_colors(const Mesh *m) { return static_cast<float4 *>(m->corner[(int)Corner::colors].vert); }
const float4 *mesh_color_rows(const Mesh *m) { return m->corner[(int)Corner::colors].rows; }
float2 *mesh_vertex_uvs(const Mesh *m) { return static_cast<float2 *>(m->corner[(int)Corner::uvs].vert); }
const float4 *mesh_uv_rows(const Mesh *m) { return m->corner[(int)Corner::uvs].rows; }

// the gather under the order array -- derived first where a rebuild has just invalidated it -- and, in front of it, the two kernels that recompute the
// smooth normals from the rows of the triangle array
int mesh_corner_refresh(Mesh *m, Corner which, hipStream_t st, const char **err) {
    const Mesh::CornerArrays &a = m->corner[(int)which];
    if (!a.rows || m->permCur < 0) return RT_ERR_INVALID;
    const int *order = nullptr;
    const int rc = mesh_order(m, st, &order, err);
    if (rc != RT_OK) return rc;
    if (which == Corner::normals)
        normals_launch_update(st, m->sc.tris, order, m->lay.nTris, m->dNrmSliceFirst, m->dNrmEntries, m->nVerts, m->dFaceByInput, static_cast<float4 *>(a.vert));
    corner_kind(which).launchRows(st, order, m->dIdx, a.vert, m->lay.nTris, m->nVerts, a.rows);
    REB_TRY(hipGetLastError());
    return RT_OK;
}

int mesh_hit_blend(Mesh *m, Corner which, hipStream_t st, const void *hits, int n, float *values, const char **err) {
    const CornerKind &k = corner_kind(which);
    if (!k.launchHitBlend || !m->corner[(int)which].rows || m->permCur < 0) return RT_ERR_INVALID;
    k.launchHitBlend(st, hits, n, m->corner[(int)which].rows, m->lay.nTris, values);
    REB_TRY(hipGetLastError());
    return RT_OK;
}

int mesh_hit_normals(Mesh *m, hipStream_t st, const void *hits, int n, float *normals, const char **err) {
    if (!mesh_normal_rows(m) || m->permCur < 0) return RT_ERR_INVALID;
    normals_launch_hit_normals(st, hits, n, m->sc.tris, mesh_normal_rows(m), m->lay.nTris, normals);
    REB_TRY(hipGetLastError());
    return RT_OK;
}

void mesh_texture_release(Mesh *m) {
    detach(m, m->texture);
    m->tex = rtuv::Texture{};
}

int mesh_texture_create(Mesh *m, const uint8_t *rgba8, int W, int H, uint32_t flags, const float *table256, const char **err) {
    const size_t bytes = (size_t)W * (size_t)H * 4;
    hipError_t e = hipSuccess;
    if (m->dTexels && (size_t)m->tex.W * (size_t)m->tex.H * 4 == bytes) {   // the same size: the block is kept
        e = hipMemcpy(m->dTexels, rgba8, bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(m->dTexTable, table256, 1024, hipMemcpyHostToDevice);
    } else {
        mesh_texture_release(m);
        e = attach(m, m->texture, &m->dTexels, bytes, Fill::host, rgba8);
        if (e == hipSuccess) e = attach(m, m->texture, &m->dTexTable, 1024, Fill::host, table256);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { if (err) *err = hipGetErrorString(e); mesh_texture_release(m); return RT_ERR_HIP; }
    m->tex.texels = m->dTexels; m->tex.table = m->dTexTable; m->tex.W = W; m->tex.H = H; m->tex.flags = flags;
    return RT_OK;
}

const rtuv::Texture *mesh_texture(const Mesh *m) { return m->tex.texels ? &m->tex : nullptr; }

int mesh_hit_texels(Mesh *m, hipStream_t st, const void *hits, int n, float *texels, const char **err) {
    if (!mesh_uv_rows(m) || !m->tex.texels || m->permCur < 0) return RT_ERR_INVALID;
    corner_launch_hit_texels(st, hits, n, mesh_uv_rows(m), m->lay.nTris, m->tex, texels);
    REB_TRY(hipGetLastError());
    return RT_OK;
}

int mesh_quantised_ok(Mesh *m, hipStream_t st, bool &ok, const char **err) {
    REB_TRY(hipMemcpyAsync(m->hStatus, m->dStatus, 4, hipMemcpyDeviceToHost, st));
    REB_TRY(hipStreamSynchronize(st));
    ok = *m->hStatus == 0u;
    return RT_OK;
}

}  // namespace rtl
