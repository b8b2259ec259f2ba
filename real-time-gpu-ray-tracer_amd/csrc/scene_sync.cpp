// scene_sync.cpp — the scene's event and wait discipline: the host waits (bounded with a communicator attached), the
// stream-side waits that skip events already complete, and the destructor, which must outwait every launch.
#include "comm_wait.hpp"
#include "scene.hpp"

namespace {

int query_result(hipError_t r) { return r == hipSuccess ? 1 : (r == hipErrorNotReady ? 0 : -1); }

}  // namespace

rt_scene::~rt_scene() {
    (void)hipSetDevice(device);
    if (comm) {                            // a peer may be gone: bounded waits, abort instead of hanging
        bool ok = true;
        for (int q = 0; q < NLANE && ok; q++)
            if (ln[q].r_done) ok = poll_wait([&] { return query_result(hipEventQuery(ln[q].r_done)); }, [] { return 0; },
                                             comm->timeout_ms ? comm->timeout_ms : 10000u) == WaitResult::done;
        if (!ok) abort_comm();
    }
    if (stream) (void)hipStreamSynchronize(stream);
    for (const Lane &l : ln)                 // launches still running on caller streams
        if (l.r_done) (void)hipEventSynchronize(l.r_done);
    if (r_done) (void)hipEventSynchronize(r_done);
    for (hipEvent_t e : ev_query)            // ray queries still running on caller streams
        if (e) (void)hipEventSynchronize(e);
    release_comm();
    materials.release(); out_rgba.release(); out_rgb.release();
    timeline.release(); costmap.release();
    delete blas_builder; delete tlas_builder;
    raw_tris.release(); raw_verts.release(); raw_sph.release(); raw_quad.release(); inst_blas.release();
    blas_wide_refs.release();
    gpu_counts.release(); inst_params.release();
    ib_table.release(); ib_chunk_inst.release(); ib_multi.release(); ib_members.release(); ib_groups.release();
    ib_partials.release(); ib_cent.release();
    if (ib_cent_stage) (void)hipHostFree(ib_cent_stage);
    const auto drop = [](BlasSet &b) {             // every BLAS set, live or spare: its buffers and lane events
        b.release();
        for (hipEvent_t e : b.ev_lane)
            if (e) (void)hipEventDestroy(e);
    };
    drop(cur);
    for (BlasSet &sp : spare) drop(sp);
    if (ev_caller) (void)hipEventDestroy(ev_caller);
    if (ev_blas_built) (void)hipEventDestroy(ev_blas_built);
    if (ev_raw_staged) (void)hipEventDestroy(ev_raw_staged);
    if (ev_tri_update) (void)hipEventDestroy(ev_tri_update);
    if (raw_stage) (void)hipHostFree(raw_stage);
    for (Stage &st : stg) st.release();
    for (FrameBlock &b : blk) b.release();
    if (counters) (void)hipFree(counters);
    if (query_heads) (void)hipFree(query_heads);
    for (hipEvent_t e : ev_query)
        if (e) (void)hipEventDestroy(e);
    for (Lane &l : ln) l.release();          // queue heads, unit costs and orders
    if (counters_host) (void)hipHostFree(counters_host);
    for (uint32_t i = 0; i < RING; i++) {
        if (ring_start[i]) (void)hipEventDestroy(ring_start[i]);
        if (ring_stop[i]) (void)hipEventDestroy(ring_stop[i]);
        if (ring_post[i]) (void)hipEventDestroy(ring_post[i]);
    }
    if (stream) (void)hipStreamDestroy(stream);
    for (Lane &l : ln) l.destroy_stream();
}

namespace rtamd {

// Wait for a stream / an event of the scene.  With a communicator attached the wait polls (comm_wait.hpp):
// an asynchronous RCCL error or the rt_comm_set_timeout deadline aborts the communicators and fails with
// RT_ERR_DEVICE instead of blocking on a peer that will never send.
rt_status comm_poll(rt_scene *s, hipStream_t st, hipEvent_t ev) {
    CommState *cm = s->comm;
    const Rccl &R = rccl();
    int code = 0;
    const WaitResult w = poll_wait(
        [&] { return st ? query_result(hipStreamQuery(st)) : query_result(hipEventQuery(ev)); },
        [&] {
            return first_async_error(cm->ncomm, [&](int q, int *st) {
                ncclResult_t a = ncclSuccess;
                const ncclResult_t r = cm->comm[q] ? R.CommGetAsyncError(cm->comm[q], &a) : ncclSuccess;
                *st = (int)a;
                return (int)r;
            });
        },
        cm->timeout_ms, &code);
    if (w == WaitResult::done) return RT_OK;
    if (w == WaitResult::failed) {
        const hipError_t e = st ? hipStreamSynchronize(st) : hipEventSynchronize(ev);
        return fail(RT_ERR_DEVICE, std::string("multi-GPU frame: ") + hipGetErrorString(e));
    }
    const std::string why = w == WaitResult::timeout
        ? "multi-GPU frame not complete after " + std::to_string(cm->timeout_ms) + " ms (a peer stopped?)"
        : std::string("RCCL asynchronous error: ") + R.GetErrorString((ncclResult_t)code);
    s->abort_comm();
    return fail(RT_ERR_DEVICE, why + "; communicators aborted, scene detached");
}
rt_status wait_stream(rt_scene *s, hipStream_t st) {
    if (s->comm) return comm_poll(s, st, nullptr);
    const hipError_t e = hipStreamSynchronize(st);
    return e == hipSuccess ? RT_OK : fail(RT_ERR_DEVICE, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
}
rt_status wait_event(rt_scene *s, hipEvent_t ev) {
    if (s->comm) return comm_poll(s, nullptr, ev);
    const hipError_t e = hipEventSynchronize(ev);
    return e == hipSuccess ? RT_OK : fail(RT_ERR_DEVICE, std::string("hipEventSynchronize: ") + hipGetErrorString(e));
}
// Wait for every enqueued launch of the scene: its own stream, the last caller stream, every lane.
rt_status drain(rt_scene *s) {
    if (s->last_stream) RT_TRY(wait_stream(s, s->last_stream));
    if (s->stream) RT_TRY(wait_stream(s, s->stream));
    for (const Lane &l : s->ln)
        if (l.r_done) RT_TRY(wait_event(s, l.r_done));
    if (s->r_done) RT_TRY(wait_event(s, s->r_done));
    if (s->query_live) {                                  // ray queries on caller streams
        for (hipEvent_t e : s->ev_query)
            if (e) RT_TRY(wait_event(s, e));
        s->query_live = false;
    }
    return RT_OK;
}

// Order stream `st` after event `ev` unless it has already completed (a host query, ~1 us: whatever is enqueued now
// runs after it, and a cross-stream wait in front of a kernel costs GPU idle time).  *pending: a wait was enqueued.
rt_status wait_if_pending(hipStream_t st, hipEvent_t ev, bool *pending) {
    *pending = false;
    const hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) return RT_OK;
    if (q != hipErrorNotReady) return fail(RT_ERR_DEVICE, std::string("hipEventQuery: ") + hipGetErrorString(q));
    HIP_TRY(hipStreamWaitEvent(st, ev, 0));
    *pending = true;
    return RT_OK;
}

// Order stream `st` after every ray query still in flight (rt_query_rays; a finished one needs no wait: a host query).
rt_status wait_queries(rt_scene *s, hipStream_t st) {
    if (!s->query_live) return RT_OK;                      // no query since all were last seen complete: no host work
    bool live = false;
    for (hipEvent_t e : s->ev_query) {
        if (!e) continue;
        bool pending;
        RT_TRY(wait_if_pending(st, e, &pending));
        live = live || pending;
    }
    s->query_live = live;
    return RT_OK;
}

// Order stream `st` after the last GPU BLAS build (ev_blas_built, recorded on the scene stream).  A build that has
// already finished needs no wait (a host query, ~1 us): anything enqueued now runs after it.
rt_status wait_blas_built(rt_scene *s, hipStream_t st) {
    if (s->blas_build_done == s->blas_build_seq) return RT_OK;
    bool pending;
    RT_TRY(wait_if_pending(st, s->ev_blas_built, &pending));
    if (!pending) s->blas_build_done = s->blas_build_seq;
    return RT_OK;
}

// Order stream `st` after the record chains (instance update + TLAS build: microseconds, not the traces) of the GPU-built
// frames already enqueued on other streams: a block's ev_copied is recorded behind its chain.  What rewrites data every
// block's chain reads — the device-bounded centroids (RT_TRI_UPDATE_BOUNDS) — waits for them; a chain that has
// finished needs no wait (a host query).
rt_status wait_record_chains(rt_scene *s, hipStream_t st) {
    for (const FrameBlock &b : s->blk) {
        if (!b.chain || b.chain == st || !b.ev_copied) continue;
        bool pending;
        RT_TRY(wait_if_pending(st, b.ev_copied, &pending));
    }
    return RT_OK;
}

// Order stream `st` after what the caller enqueued on the null stream before the call: the scene's streams are
// non-blocking, which HIP does not order with it (rt_render explains when a caller expects that order).
rt_status order_after_null_stream(rt_scene *s, hipStream_t st) { return order_after_stream(s, nullptr, st); }

// Order stream `st` after what is enqueued on the caller's stream `from` now (ev_caller serves every such hand-over: a
// wait takes the record it finds, so the event may be recorded again straight after).
rt_status order_after_stream(rt_scene *s, hipStream_t from, hipStream_t st) {
    if (!s->ev_caller) HIP_TRY(hipEventCreateWithFlags(&s->ev_caller, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(s->ev_caller, from));
    HIP_TRY(hipStreamWaitEvent(st, s->ev_caller, 0));
    return RT_OK;
}

// Every enqueued launch of the scene and the build of the current frame block (GPU-built frames build it on the
// lane stream of the frame that staged it): the scene's own streams and events only, with the communicator's
// bounded polls when one is attached (never a device-wide synchronisation).
rt_status wait_frame_block(rt_scene *s) {
    RT_TRY(drain(s));
    if (s->active >= 0 && s->blk[s->active].r_copied) RT_TRY(wait_event(s, s->blk[s->active].r_copied));
    return RT_OK;
}

}  // namespace rtamd
