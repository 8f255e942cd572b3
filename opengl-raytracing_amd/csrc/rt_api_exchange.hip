// rt_api_exchange.hip -- the multi-rank part of the C ABI (include/rt_mi355.h), what a single-rank user never calls: the RCCL binding and
// rt_comm_*, the gather of a frame's targets on rank 0 (k_assemble), the history exchange of a moving camera.
// Tile-parallel exchange over RCCL, owned by the library.  librccl is half a gigabyte and only multi-GPU
// runs need it, so it is bound on first use: an already loaded copy (e.g. the one a PyTorch wheel brought into the process) is
// reused by SONAME, otherwise librccl.so.1 is loaded from the ROCm installation.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>

#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: RCCL is bound at run time (rccl_api below), single-GPU users never load it

#include "rt_context.hpp"

using namespace rtd;
using namespace rtapi;

namespace {

// Gathered blocks (rank-major, blockBytes each, tile-major inside) -> row-major frame of halfs.
__global__ void k_assemble(const void *gathered, void *dst, FrameGeom g, int channels, size_t blockBytes) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.W * g.H) return;
    int x = i % g.W, y = i / g.W;
    int tx = x >> 4, ty = y >> 4;
    int t = tile_index(g, tx, ty);
    int owner = t % g.world, local = t / g.world;
    int lx = x & 15, ly = y & 15;
    int q = (lx >> 3) | ((ly >> 3) << 1);
    size_t slot = (size_t)local * 256 + q * 64 + (ly & 7) * 8 + (lx & 7);
    const uint16_t *in = (const uint16_t *)((const char *)gathered + (size_t)owner * blockBytes) + slot * channels;
    uint16_t *out = (uint16_t *)dst + (size_t)i * channels;
    for (int c = 0; c < channels; ++c) out[c] = in[c];
}

// Stage "assemble": k_assemble on `st`, every rank's block of `block` bytes at `gathered` into the row-major frame at `dst`
int assemble(RtContext *c, hipStream_t st, const void *gathered, void *dst, int ch, size_t block) {
    const size_t n = (size_t)c->g.W * c->g.H;
    rt_stage_begin(c, 10, st);
    hipLaunchKernelGGL(k_assemble, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, gathered, dst, c->g, ch, block);
    rt_stage_end(c, 10, 1, st);
    HIP_TRY(c, hipGetLastError());
    return RT_OK;
}

struct RcclApi {
    decltype(&ncclGetUniqueId) getUniqueId = nullptr;
    decltype(&ncclCommInitRank) commInitRank = nullptr;
    decltype(&ncclCommDestroy) commDestroy = nullptr;
    decltype(&ncclGroupStart) groupStart = nullptr;
    decltype(&ncclGroupEnd) groupEnd = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclAllGather) allGather = nullptr;
    decltype(&ncclGetErrorString) errorString = nullptr;
    decltype(&ncclCommCount) commCount = nullptr;          // optional (rt_comm_info)
    decltype(&ncclCommUserRank) commUserRank = nullptr;
    std::string err;
    bool ok = false;
};
void rccl_bind(RcclApi &a) {
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) { const char *e = dlerror(); a.err = std::string("librccl.so.1 could not be loaded: ") + (e ? e : "?"); return; }
#define RT_BIND(field, name) do { a.field = (decltype(a.field))dlsym(h, #name); if (!a.field) { a.err = "librccl lacks " #name; return; } } while (0)
    RT_BIND(getUniqueId, ncclGetUniqueId); RT_BIND(commInitRank, ncclCommInitRank); RT_BIND(commDestroy, ncclCommDestroy);
    RT_BIND(groupStart, ncclGroupStart); RT_BIND(groupEnd, ncclGroupEnd); RT_BIND(send, ncclSend); RT_BIND(recv, ncclRecv);
    RT_BIND(allGather, ncclAllGather); RT_BIND(errorString, ncclGetErrorString);
#undef RT_BIND
    a.commCount = (decltype(a.commCount))dlsym(h, "ncclCommCount");
    a.commUserRank = (decltype(a.commUserRank))dlsym(h, "ncclCommUserRank");
    a.ok = true;
}
RcclApi &rccl_api() {
    static RcclApi a;
    static std::once_flag once;              // contexts on different threads may reach their first rt_comm_* call together
    std::call_once(once, [] { rccl_bind(a); });
    return a;
}
#define NCCL_TRY(c, expr)                                                                                           \
    do {                                                                                                            \
        ncclResult_t r_ = (expr);                                                                                   \
        if (r_ != ncclSuccess) return fail((c), RT_ERR_HIP, "%s failed: %s", #expr, rccl_api().errorString(r_));     \
    } while (0)

}  // namespace

extern "C" {

int rt_history_exchange_buffer(RtContext *c, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_history_exchange_buffer before rt_resize");
    (void)hipSetDevice(c->cfg.device);
    const int lane = last_lane(c);
    const size_t n = (size_t)c->g.world * c->nSlots * 8;
    if (!c->dHistAll[lane]) HIP_TRY(c, hipMalloc(&c->dHistAll[lane], n));
    *devPtr = c->dHistAll[lane];
    *bytes = n;
    return RT_OK;
}
int rt_history_exchanged(RtContext *c) {
    if (!c) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_history_exchanged before rt_resize");
    (void)hipSetDevice(c->cfg.device);
    const int lane = last_lane(c);
    if (!c->dHistAll[lane]) return fail(c, RT_ERR_STATE, "rt_history_exchanged without rt_history_exchange_buffer");
    // the next frame's resolve waits on this event: it now also covers the all-gather the caller enqueued on rt_stream()
    HIP_TRY(c, hipEventRecord(c->evDone[lane], c->lanes[lane]));
    c->histExchanged[lane] = true;
    return RT_OK;
}

int rt_local_target(RtContext *c, int which, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_local_target before rt_resize");
    int ch;
    void *p = target_ptr(c, which, ch);
    if (!p) return fail(c, RT_ERR_INVALID, "rt_local_target: which=%d", which);
    *devPtr = p;
    *bytes = c->nSlots * ch * 2;
    return RT_OK;
}
int rt_gather_block_bytes(const RtContext *c, int which, size_t *bytes) {
    if (!c || !bytes || !c->sized) return RT_ERR_INVALID;
    const int ch = (which == RT_TARGET_MOTION) ? 2 : 4;
    *bytes = c->nSlots * ch * 2;
    return RT_OK;
}
int rt_assemble_gathered(RtContext *c, int which, const void *gatheredDev, void *dstDev) {
    if (!c || !gatheredDev || !dstDev) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_assemble_gathered before rt_resize");
    (void)hipSetDevice(c->cfg.device);
    const int ch = (which == RT_TARGET_MOTION) ? 2 : 4;
    return assemble(c, api_stream(c), gatheredDev, dstDev, ch, c->nSlots * ch * 2);   // behind the gather the caller enqueued on rt_stream()
}

int rt_comm_unique_id(void *id, size_t bytes) {
    if (!id || bytes < RT_COMM_ID_BYTES) return fail(nullptr, RT_ERR_INVALID, "rt_comm_unique_id: need %d bytes", RT_COMM_ID_BYTES);
    RcclApi &a = rccl_api();
    if (!a.ok) return fail(nullptr, RT_ERR_UNSUPPORTED, "rt_comm_unique_id: %s", a.err.c_str());
    static_assert(sizeof(ncclUniqueId) == RT_COMM_ID_BYTES, "RT_COMM_ID_BYTES");
    ncclUniqueId u;
    ncclResult_t r = a.getUniqueId(&u);
    if (r != ncclSuccess) return fail(nullptr, RT_ERR_HIP, "ncclGetUniqueId: %s", a.errorString(r));
    std::memcpy(id, &u, sizeof u);
    return RT_OK;
}

int rt_comm_init(RtContext *c, const void *id, size_t bytes) {
    if (!c || !id || bytes < RT_COMM_ID_BYTES) return RT_ERR_INVALID;
    if (c->comm) return fail(c, RT_ERR_STATE, "rt_comm_init: the context already has a communicator");
    RcclApi &a = rccl_api();
    if (!a.ok) return fail(c, RT_ERR_UNSUPPORTED, "rt_comm_init: %s", a.err.c_str());
    (void)hipSetDevice(c->cfg.device);
    HIP_TRY(c, sync_all(c));
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    ncclComm_t comm = nullptr;
    NCCL_TRY(c, a.commInitRank(&comm, c->cfg.worldSize, u, c->cfg.rank));   // collective over all ranks of the frame
    c->comm = (void *)comm;
    // the gathering rank's COLOR0 buffers for every frame lane now, not inside the frame loop (a first-gather hipMalloc would otherwise land in
    // whatever is being timed; the other targets are gathered for a present only and keep allocating on first use)
    if (c->sized && c->g.rank == 0) {
        const size_t block = c->nSlots * 8;
        for (int l = 0; l < c->nLanes; ++l) {
            if (!c->dGathered[l][RT_TARGET_COLOR]) HIP_TRY(c, hipMalloc(&c->dGathered[l][RT_TARGET_COLOR], block * (size_t)c->g.world));
            if (!c->dAssembled[l][RT_TARGET_COLOR]) HIP_TRY(c, hipMalloc(&c->dAssembled[l][RT_TARGET_COLOR], (size_t)c->g.W * c->g.H * 8));
        }
    }
    return RT_OK;
}

int rt_comm_destroy(RtContext *c) {
    if (!c) return RT_ERR_INVALID;
    if (!c->comm) return RT_OK;
    (void)hipSetDevice(c->cfg.device);
    (void)sync_all(c);
    ncclResult_t r = rccl_api().commDestroy((ncclComm_t)c->comm);
    c->comm = nullptr;
    if (r != ncclSuccess) return fail(c, RT_ERR_HIP, "ncclCommDestroy: %s", rccl_api().errorString(r));
    return RT_OK;
}

// One exchange per gathered frame: every rank sends the block of its tiles to rank 0 -- grouped point-to-point
// transfers, so the root's inbound xGMI links run in parallel and nothing is reduced -- and rank 0 un-tiles the blocks into a
// row-major frame.  Everything is enqueued on the lane (stream) of the frame rendered last and uses that lane's own buffers, so
// gathers of consecutive frames overlap like the frames themselves and never share a buffer.
int rt_gather_frame(RtContext *c, int which) {
    if (!c) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_gather_frame before rt_resize");
    if (c->frameIndex == 0) return fail(c, RT_ERR_STATE, "rt_gather_frame before the first frame");
    if (c->g.world > 1 && !c->comm) return fail(c, RT_ERR_STATE, "rt_gather_frame on a tile-parallel context without rt_comm_init");
    (void)hipSetDevice(c->cfg.device);
    const int lane = last_lane(c);
    int ch;
    void *local = lane_target(c, lane, which, ch);
    if (!local) return fail(c, RT_ERR_INVALID, "rt_gather_frame: which=%d", which);
    const size_t block = c->nSlots * (size_t)ch * 2;
    hipStream_t st = c->lanes[lane];
    const bool root = c->g.rank == 0;
    if (root) {
        if (!c->dGathered[lane][which]) HIP_TRY(c, hipMalloc(&c->dGathered[lane][which], block * (size_t)c->g.world));
        if (!c->dAssembled[lane][which]) HIP_TRY(c, hipMalloc(&c->dAssembled[lane][which], (size_t)c->g.W * c->g.H * ch * 2));
    }
    // stage "gather": from the point the lane's stream reaches the exchange (its frame is done) to the end of the un-tiling on the root / of
    // the send on the others -- on the root this is what the first 8-GPU run needs to see next to the ranks' frame times (bench.py)
    struct GatherSpan {
        RtContext *c; hipStream_t st;
        GatherSpan(RtContext *c_, hipStream_t s_) : c(c_), st(s_) { rt_stage_begin(c, 12, st); }
        ~GatherSpan() { rt_stage_end(c, 12, 1, st); }
    } span(c, st);
    c->gathers++;
    c->gatherBytes += root ? block * (size_t)(c->g.world - 1) : block;
    if (root) HIP_TRY(c, hipMemcpyAsync(c->dGathered[lane][which], local, block, hipMemcpyDeviceToDevice, st));
    if (c->g.world > 1) {
        RcclApi &a = rccl_api();
        ncclComm_t comm = (ncclComm_t)c->comm;
        NCCL_TRY(c, a.groupStart());
        // a failing send / recv must not leave the communicator inside an open group (later collectives and ncclCommDestroy would
        // hang): close the group first, then report the first error
        ncclResult_t r1 = ncclSuccess;
        if (root) {
            for (int r = 1; r < c->g.world && r1 == ncclSuccess; ++r)
                r1 = a.recv((char *)c->dGathered[lane][which] + (size_t)r * block, block, ncclUint8, r, comm, st);
        } else {
            r1 = a.send(local, block, ncclUint8, 0, comm, st);
        }
        const ncclResult_t r2 = a.groupEnd();
        if (r1 != ncclSuccess) return fail(c, RT_ERR_HIP, "ncclSend/ncclRecv failed: %s", a.errorString(r1));
        if (r2 != ncclSuccess) return fail(c, RT_ERR_HIP, "ncclGroupEnd failed: %s", a.errorString(r2));
    }
    if (root) {
        const int rc = assemble(c, st, c->dGathered[lane][which], c->dAssembled[lane][which], ch, block);
        if (rc != RT_OK) return rc;
    }
    c->gatheredLane[which] = lane;
    return RT_OK;
}

int rt_gathered_frame(RtContext *c, int which, void **devPtr, size_t *bytes) {
    if (!c || !devPtr || !bytes || which < 0 || which > 3) return RT_ERR_INVALID;
    if (c->g.rank != 0) return fail(c, RT_ERR_STATE, "rt_gathered_frame: only rank 0 holds the gathered frame");
    const int lane = c->gatheredLane[which];
    if (lane < 0 || !c->dAssembled[lane][which]) return fail(c, RT_ERR_STATE, "rt_gathered_frame: no rt_gather_frame(%d) since the last reset", which);
    *devPtr = c->dAssembled[lane][which];
    *bytes = (size_t)c->g.W * c->g.H * (which == RT_TARGET_MOTION ? 2 : 4) * 2;
    return RT_OK;
}

int rt_read_gathered(RtContext *c, int which, void *dstHalfs) {
    if (!c || !dstHalfs) return RT_ERR_INVALID;
    void *p;
    size_t n;
    int rc = rt_gathered_frame(c, which, &p, &n);
    if (rc != RT_OK) return rc;
    (void)hipSetDevice(c->cfg.device);
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(dstHalfs, p, n, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_present_last_gathered(RtContext *c, const RtPresentParams *p, uint8_t *dst) {
    if (!c || !p || !dst) return RT_ERR_INVALID;
    if (c->g.rank != 0) return fail(c, RT_ERR_STATE, "rt_present_last_gathered: only rank 0 holds the gathered targets");
    const int lane = c->gatheredLane[0];
    for (int w = 0; w < 4; ++w)
        if (c->gatheredLane[w] < 0 || c->gatheredLane[w] != lane || !c->dGathered[lane][w])
            return fail(c, RT_ERR_STATE, "rt_present_last_gathered: gather all four targets of the same frame first (rt_gather_frame 0..3)");
    return rt_present_gathered(c, p, c->dGathered[lane][0], c->dGathered[lane][1], c->dGathered[lane][2], c->dGathered[lane][3], dst);
}

// Moving camera on a tile-parallel frame: every rank needs the whole previous COLOR0 (rt_taa.glsl:116-179 reads it at arbitrary
// pixels) -> one all-gather of the ranks' blocks into this lane's exchange buffer, then the event the next frame's resolve waits on.
int rt_exchange_history(RtContext *c) {
    if (!c) return RT_ERR_INVALID;
    if (!c->sized) return fail(c, RT_ERR_STATE, "rt_exchange_history before rt_resize");
    if (c->g.world > 1 && !c->comm) return fail(c, RT_ERR_STATE, "rt_exchange_history on a tile-parallel context without rt_comm_init");
    void *buf;
    size_t bytes;
    int rc = rt_history_exchange_buffer(c, &buf, &bytes);
    if (rc != RT_OK) return rc;
    const int lane = last_lane(c);
    const size_t block = c->nSlots * 8;
    if (c->g.world > 1) NCCL_TRY(c, rccl_api().allGather(c->dColor[lane], buf, block, ncclUint8, (ncclComm_t)c->comm, c->lanes[lane]));
    else HIP_TRY(c, hipMemcpyAsync(buf, c->dColor[lane], block, hipMemcpyDeviceToDevice, c->lanes[lane]));
    c->historyExchanges++;
    return rt_history_exchanged(c);
}

int rt_comm_info(RtContext *c, RtCommInfo *out) {
    if (!c || !out) return RT_ERR_INVALID;
    out->commWorld = out->commRank = -1;
    out->rank = c->cfg.rank; out->worldSize = c->cfg.worldSize;
    out->gathers = c->gathers; out->gatherBytes = c->gatherBytes; out->historyExchanges = c->historyExchanges;
    if (c->comm) {
        RcclApi &a = rccl_api();
        int v = -1;
        if (a.commCount && a.commCount((ncclComm_t)c->comm, &v) == ncclSuccess) out->commWorld = v;
        v = -1;
        if (a.commUserRank && a.commUserRank((ncclComm_t)c->comm, &v) == ncclSuccess) out->commRank = v;
    }
    return RT_OK;
}

}  // extern "C"
