// scene_comm.cpp — a multi-GPU frame over RCCL (comm.cpp loads it): attaching and detaching the communicators, the
// gather of the ranks' slabs behind a trace, and aborting them when a peer fails.
#include "launch.hpp"
#include "scene.hpp"

void rt_scene::release_comm() {
    if (!comm) return;
    for (int q = 0; q < CommState::NLANE; q++) {
        if (comm->comm[q]) (void)rccl().CommDestroy(comm->comm[q]);
        comm->slab[q].release();
        comm->gathered[q].release();
    }
    delete comm;
    comm = nullptr;
}
void rt_scene::abort_comm() {
    if (!comm) return;
    for (int q = 0; q < CommState::NLANE; q++)
        if (comm->comm[q]) (void)rccl().CommAbort(comm->comm[q]);
    delete comm;
    comm = nullptr;
    // the aborted frames' completion events are given up: nothing waits for them again, every staging buffer is free
    for (Lane &l : ln) l.reset();
    r_done = nullptr;
    for (FrameBlock &b : blk) b.reset();
    for (Stage &st : stg) st.reset();
}

namespace rtamd {

// Lane q's trace wrote this rank's slab: gather the ranks' slabs to rank 0 (grouped point-to-point over xGMI: each
// rank's bytes take their own link into rank 0), then scatter them into the frame there.
rt_status comm_gather(rt_scene *s, int q, uint8_t *frame_out, hipStream_t stream) {
    CommState *cm = s->comm;
    const Rccl &R = rccl();
    const size_t sb = cm->slab_bytes;
    if (cm->world > 1) {
        ncclResult_t e = R.GroupStart();
        if (cm->rank == 0) {
            for (int r = 1; r < cm->world && e == ncclSuccess; r++)
                e = R.Recv(cm->gathered[q].p + (size_t)r * sb, sb, ncclUint8, r, cm->comm[q % cm->ncomm], stream);
        } else if (e == ncclSuccess) {
            e = R.Send(cm->slab[q].p, sb, ncclUint8, 0, cm->comm[q % cm->ncomm], stream);
        }
        const ncclResult_t e2 = R.GroupEnd();
        if (e != ncclSuccess || e2 != ncclSuccess)
            return fail(RT_ERR_DEVICE, std::string("RCCL tile gather: ") + R.GetErrorString(e != ncclSuccess ? e : e2));
    }
    if (cm->rank == 0)
        HIP_TRY(launch_assemble(cm->gathered[q].p, (uint32_t)(sb / (4ull * cm->tile_w * cm->tile_h)), cm->tile_w,
                                cm->tile_h, (uint32_t)cm->world, s->width, s->height, frame_out, stream));
    return RT_OK;
}

}  // namespace rtamd

extern "C" {

rt_status rt_comm_unique_id(rt_comm_id *id) {
    if (!id) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    static_assert(sizeof(rt_comm_id) == sizeof(ncclUniqueId), "rt_comm_id must be an ncclUniqueId");
    const Rccl &R = rccl();
    if (!R.ok) return fail(RT_ERR_UNSUPPORTED, R.error);
    ncclUniqueId u;
    const ncclResult_t e = R.GetUniqueId(&u);
    if (e != ncclSuccess) return fail(RT_ERR_DEVICE, std::string("ncclGetUniqueId: ") + R.GetErrorString(e));
    std::memcpy(id, &u, sizeof u);
    return RT_OK;
}

rt_status rt_scene_attach_comm(rt_scene *s, const rt_comm_id *id, int rank, int world, uint32_t tw, uint32_t th) {
    if (!s || !id) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(RT_ERR_INVALID_ARGUMENT, "rank must be in [0, world)");
    if (tw == 0 || th == 0 || tw % 8 || th % 8) return fail(RT_ERR_INVALID_ARGUMENT, "tiles must be multiples of 8");
    const Rccl &R = rccl();
    if (!R.ok) return fail(RT_ERR_UNSUPPORTED, R.error);
    HIP_TRY(hipSetDevice(s->device));
    RT_TRY(drain(s));
    s->release_comm();
    auto *cm = new (std::nothrow) CommState();
    if (!cm) return fail(RT_ERR_OUT_OF_MEMORY, "host allocation failed");
    cm->rank = rank; cm->world = world; cm->tile_w = tw; cm->tile_h = th;
    // one per lane in use (auto lanes: the 8 a rank's share runs on, auto_lanes)
    cm->ncomm = (int)std::max<uint32_t>(1u, s->overlap_auto && world > 1 ? 8u : (s->overlap ? s->lanes : 1u));
    cm->timeout_ms = s->comm_timeout_ms;
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    ncclResult_t e = R.CommInitRank(&cm->comm[0], world, u, rank);
    for (int q = 1; q < cm->ncomm && e == ncclSuccess; q++) e = R.CommSplit(cm->comm[0], 0, rank, &cm->comm[q], nullptr);
    s->comm = cm;
    if (e != ncclSuccess) {
        const std::string msg = std::string("RCCL communicator: ") + R.GetErrorString(e);
        s->release_comm();
        return fail(RT_ERR_DEVICE, msg);
    }
    return RT_OK;
}

rt_status rt_comm_set_timeout(rt_scene *s, uint32_t timeout_ms) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "null scene");
    s->comm_timeout_ms = timeout_ms;
    if (s->comm) s->comm->timeout_ms = timeout_ms;
    return RT_OK;
}

rt_status rt_scene_detach_comm(rt_scene *s) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "null scene");
    if (!s->comm) return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    RT_TRY(drain(s));
    s->release_comm();
    return RT_OK;
}

}  // extern "C"
