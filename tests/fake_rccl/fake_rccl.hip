// fake_rccl.hip — a test-only stand-in for librccl.so.1 that runs an N-rank "world" inside one process on one
// GPU, so the library's multi-GPU frame (rt_scene_attach_comm: trace -> grouped ncclSend / ncclRecv gather ->
// assemble, csrc/scene_comm.cpp) runs its world > 1 branch on a one-GPU box (verdict r3 item 2).
//
// Test infrastructure, never product: librtamd.so loads it only when RTAMD_RCCL_LIB names it (csrc/comm.cpp).
// It implements exactly the entry points comm.hpp resolves, with the semantics the library relies on:
//   * ncclCommInitRank / ncclCommSplit join a world keyed by the unique id (split worlds by split order and
//     colour), without blocking: the ranks are scenes driven from one host thread;
//   * point-to-point messages are matched per (world, source, destination) in posting order, as NCCL does;
//   * ncclSend stages the send buffer on the sender's stream (so the sender may reuse its slab at once) and
//     records an event; ncclRecv orders the receiver's stream after that event and copies the staged bytes;
//   * a receive posted before its send (the peer is late, or never sends) blocks the receiving stream on the
//     GPU like a real receive: a one-wave kernel polls a flag in coherent host memory, which the matching send
//     releases after its copy, or ncclCommAbort releases (the library's rt_comm_set_timeout path).  The poll
//     exits by itself after FAKE_RCCL_MAX_WAIT_S seconds (default 30), so no wave outlives the test;
//   * ncclCommGetAsyncError reports ncclSuccess (a late peer is not an error; the library's deadline is).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

namespace {

__global__ void wait_flag_kernel(const uint32_t *flag, uint64_t max_ticks) {
    // one wave polls a system-coherent host word (never writes it); s_memrealtime runs at 100 MHz
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
        __builtin_amdgcn_s_sleep(127);
        if (__builtin_amdgcn_s_memrealtime() - t0 > max_ticks) break;
    }
}

__global__ void set_flag_kernel(uint32_t *flag) {
    if (threadIdx.x == 0) __hip_atomic_store(flag, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct Msg {
    void *staging = nullptr;       // send first: the sender's bytes
    size_t bytes = 0;
    hipEvent_t ev = nullptr;       // send first: staging written
    bool sent = false, received = false;
    void *recv_dst = nullptr;      // receive first: where the sender copies to
    uint32_t *flag = nullptr;      // receive first: host word the waiting kernel polls (device view: flag_dev)
    uint32_t *flag_dev = nullptr;
    hipEvent_t done = nullptr;     // receive side complete (staging / flag reusable)
};

struct World {
    int nranks = 1;
    bool aborted = false;
    std::map<std::pair<int, int>, uint64_t> send_seq, recv_seq;
    std::map<std::tuple<int, int, uint64_t>, std::unique_ptr<Msg>> msgs;
    std::map<std::pair<uint64_t, int>, std::shared_ptr<World>> splits;   // (split index, colour)
};

struct PendingOp { bool send; void *buf; size_t bytes; int peer; ncclComm_t comm; hipStream_t stream; };

std::mutex g_mu;
std::map<uint64_t, std::shared_ptr<World>> g_worlds;
std::atomic<uint64_t> g_next_id{0x5EED000000000001ull};
thread_local int t_group_depth = 0;
thread_local std::vector<PendingOp> t_ops;

uint64_t max_wait_ticks() {
    const char *e = std::getenv("FAKE_RCCL_MAX_WAIT_S");
    const double s = e ? std::atof(e) : 30.0;
    return (uint64_t)((s > 0 ? s : 30.0) * 1e8);
}

size_t type_size(ncclDataType_t t) {
    switch (t) {
    case ncclInt8: case ncclUint8: return 1;
    case ncclFloat16: case ncclBfloat16: return 2;
    case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
    case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
    default: return 1;
    }
}

}  // namespace

struct ncclComm {
    std::shared_ptr<World> world;
    int rank = 0;
    uint64_t splits = 0;           // splits this rank made of this communicator (the split index of the next)
};

namespace {

// free the messages both sides are done with
void reap(World &w) {
    for (auto it = w.msgs.begin(); it != w.msgs.end();) {
        Msg &m = *it->second;
        if (m.sent && m.received && (!m.done || hipEventQuery(m.done) == hipSuccess)) {
            if (m.staging) (void)hipFree(m.staging);
            if (m.ev) (void)hipEventDestroy(m.ev);
            if (m.done) (void)hipEventDestroy(m.done);
            if (m.flag) (void)hipHostFree(m.flag);
            it = w.msgs.erase(it);
        } else {
            ++it;
        }
    }
}

Msg &msg_for(World &w, int src, int dst, bool send) {
    auto &seq = send ? w.send_seq[{src, dst}] : w.recv_seq[{src, dst}];
    auto &p = w.msgs[std::make_tuple(src, dst, seq++)];
    if (!p) p = std::make_unique<Msg>();
    return *p;
}

ncclResult_t do_send(const PendingOp &op) {
    World &w = *op.comm->world;
    Msg &m = msg_for(w, op.comm->rank, op.peer, true);
    m.sent = true;
    m.bytes = op.bytes;
    if (m.recv_dst) {                                  // the receiver is already waiting: copy, then release it
        if (hipMemcpyAsync(m.recv_dst, op.buf, op.bytes, hipMemcpyDeviceToDevice, op.stream) != hipSuccess)
            return ncclUnhandledCudaError;
        hipLaunchKernelGGL(set_flag_kernel, dim3(1), dim3(64), 0, op.stream, m.flag_dev);
        return hipGetLastError() == hipSuccess ? ncclSuccess : ncclUnhandledCudaError;
    }
    if (hipMalloc(&m.staging, op.bytes ? op.bytes : 1) != hipSuccess) return ncclUnhandledCudaError;
    if (hipMemcpyAsync(m.staging, op.buf, op.bytes, hipMemcpyDeviceToDevice, op.stream) != hipSuccess)
        return ncclUnhandledCudaError;
    if (hipEventCreateWithFlags(&m.ev, hipEventDisableTiming) != hipSuccess) return ncclUnhandledCudaError;
    return hipEventRecord(m.ev, op.stream) == hipSuccess ? ncclSuccess : ncclUnhandledCudaError;
}

ncclResult_t do_recv(const PendingOp &op) {
    World &w = *op.comm->world;
    Msg &m = msg_for(w, op.peer, op.comm->rank, false);
    m.received = true;
    if (m.sent) {                                      // the send was posted first: wait for its staging copy
        if (m.bytes != op.bytes) return ncclInvalidUsage;
        if (hipStreamWaitEvent(op.stream, m.ev, 0) != hipSuccess) return ncclUnhandledCudaError;
        if (hipMemcpyAsync(op.buf, m.staging, op.bytes, hipMemcpyDeviceToDevice, op.stream) != hipSuccess)
            return ncclUnhandledCudaError;
    } else {                                           // block this stream on the GPU until the send arrives
        if (hipHostMalloc(reinterpret_cast<void **>(&m.flag), 64, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
            return ncclUnhandledCudaError;
        *m.flag = 0u;
        if (hipHostGetDevicePointer(reinterpret_cast<void **>(&m.flag_dev), m.flag, 0) != hipSuccess)
            return ncclUnhandledCudaError;
        m.recv_dst = op.buf;
        m.bytes = op.bytes;
        if (w.aborted) *m.flag = 2u;
        hipLaunchKernelGGL(wait_flag_kernel, dim3(1), dim3(64), 0, op.stream, m.flag_dev, max_wait_ticks());
        if (hipGetLastError() != hipSuccess) return ncclUnhandledCudaError;
    }
    if (hipEventCreateWithFlags(&m.done, hipEventDisableTiming) != hipSuccess) return ncclUnhandledCudaError;
    return hipEventRecord(m.done, op.stream) == hipSuccess ? ncclSuccess : ncclUnhandledCudaError;
}

ncclResult_t run_ops(std::vector<PendingOp> ops) {
    std::lock_guard<std::mutex> lk(g_mu);
    ncclResult_t r = ncclSuccess;
    for (const PendingOp &op : ops) {                  // posting order within the group, sends and receives alike
        if (op.comm->world->aborted) return ncclInvalidUsage;
        r = op.send ? do_send(op) : do_recv(op);
        if (r != ncclSuccess) return r;
    }
    for (const PendingOp &op : ops) reap(*op.comm->world);
    return r;
}

ncclResult_t post(bool send, const void *buf, size_t count, ncclDataType_t t, int peer, ncclComm_t comm, hipStream_t st) {
    if (!comm || peer < 0 || peer >= comm->world->nranks || peer == comm->rank) return ncclInvalidArgument;
    PendingOp op{send, const_cast<void *>(buf), count * type_size(t), peer, comm, st};
    if (t_group_depth > 0) {
        t_ops.push_back(op);
        return ncclSuccess;
    }
    return run_ops({op});
}

}  // namespace

extern "C" {

ncclResult_t ncclGetUniqueId(ncclUniqueId *id) {
    if (!id) return ncclInvalidArgument;
    std::memset(id, 0, sizeof *id);
    const uint64_t v = g_next_id.fetch_add(1);
    std::memcpy(id->internal, "fake-rccl", 9);
    std::memcpy(id->internal + 16, &v, sizeof v);
    return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t *comm, int nranks, ncclUniqueId id, int rank) {
    if (!comm || nranks < 1 || rank < 0 || rank >= nranks || std::memcmp(id.internal, "fake-rccl", 9) != 0)
        return ncclInvalidArgument;
    uint64_t key;
    std::memcpy(&key, id.internal + 16, sizeof key);
    std::lock_guard<std::mutex> lk(g_mu);
    auto &w = g_worlds[key];
    if (!w) { w = std::make_shared<World>(); w->nranks = nranks; }
    if (w->nranks != nranks) return ncclInvalidArgument;
    auto *c = new ncclComm();
    c->world = w;
    c->rank = rank;
    *comm = c;
    return ncclSuccess;
}

ncclResult_t ncclCommSplit(ncclComm_t comm, int color, int key, ncclComm_t *newcomm, ncclConfig_t *config) {
    (void)config;
    if (!comm || !newcomm) return ncclInvalidArgument;
    std::lock_guard<std::mutex> lk(g_mu);
    auto &w = comm->world->splits[{comm->splits++, color}];
    if (!w) { w = std::make_shared<World>(); w->nranks = comm->world->nranks; }   // every rank joins with one colour
    auto *c = new ncclComm();
    c->world = w;
    c->rank = key;
    *newcomm = c;
    return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
    if (!comm) return ncclInvalidArgument;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        reap(*comm->world);
    }
    delete comm;
    return ncclSuccess;
}

ncclResult_t ncclCommAbort(ncclComm_t comm) {
    if (!comm) return ncclInvalidArgument;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        World &w = *comm->world;
        w.aborted = true;
        for (auto &kv : w.msgs)                        // release every receive still waiting on the GPU
            if (kv.second->flag) __atomic_store_n(kv.second->flag, 2u, __ATOMIC_RELEASE);
    }
    delete comm;
    return ncclSuccess;
}

ncclResult_t ncclCommGetAsyncError(ncclComm_t comm, ncclResult_t *err) {
    if (!comm || !err) return ncclInvalidArgument;
    *err = ncclSuccess;
    return ncclSuccess;
}

ncclResult_t ncclGroupStart() {
    t_group_depth++;
    return ncclSuccess;
}

ncclResult_t ncclGroupEnd() {
    if (t_group_depth <= 0) return ncclInvalidUsage;
    if (--t_group_depth > 0) return ncclSuccess;
    std::vector<PendingOp> ops;
    ops.swap(t_ops);
    return run_ops(std::move(ops));
}

ncclResult_t ncclSend(const void *buf, size_t count, ncclDataType_t t, int peer, ncclComm_t comm, hipStream_t st) {
    return post(true, buf, count, t, peer, comm, st);
}

ncclResult_t ncclRecv(void *buf, size_t count, ncclDataType_t t, int peer, ncclComm_t comm, hipStream_t st) {
    return post(false, buf, count, t, peer, comm, st);
}

const char *ncclGetErrorString(ncclResult_t r) {
    switch (r) {
    case ncclSuccess: return "no error (fake RCCL)";
    case ncclInvalidArgument: return "invalid argument (fake RCCL)";
    case ncclInvalidUsage: return "invalid usage (fake RCCL)";
    case ncclUnhandledCudaError: return "HIP error (fake RCCL)";
    default: return "error (fake RCCL)";
    }
}

}  // extern "C"
