// render.cpp — the launches that take a scene: a frame (rt_render and its steps), the tile assembly, the ray queries;
// and the box test.  (The image filters, which take no scene: filters.cpp.)
// A frame issues its HIP calls in one fixed order on the frame's stream; the comments say what each wait and each
// event record costs, so a step moves as a whole or not at all.
#include "launch.hpp"
#include "scene.hpp"
#include "sched_phase.hpp"

namespace {

// The call's checks and its options: the caller's or the defaults; a multi-GPU frame takes its tiling from the
// communicator.
rt_status frame_options(const rt_scene *s, const rt_render_opts *opts, const float *rgb_host, rt_render_opts &o) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "null scene");
    if (!s->built) return fail(RT_ERR_STATE, "rt_scene_build has not been called");
    if (!s->cam_ok) return fail(RT_ERR_STATE, "rt_camera_set has not been called");
    if (opts) o = *opts;
    if (o.frame_seed == 0) o.frame_seed = 0x5EED;
    if (const CommState *cm = s->comm) {       // multi-GPU frame: the communicator owns the tiling
        if (o.tile_count) return fail(RT_ERR_INVALID_ARGUMENT, "tile options are set by rt_scene_attach_comm");
        if (o.rgb32_device || rgb_host) return fail(RT_ERR_UNSUPPORTED, "rgb32 outputs are not gathered across ranks");
        o.tile_w = cm->tile_w; o.tile_h = cm->tile_h;
        o.tile_rank = (uint32_t)cm->rank; o.tile_count = (uint32_t)cm->world;
    }
    return RT_OK;
}

// a trace that skipped the frame update after rt_scene_update_triangles would traverse the old trees while its hits
// read the new triangles (raw_tris): the next frame update rebuilds the BLASes first
rt_status fail_blas_dirty() {
    return fail(RT_ERR_STATE, "triangles were updated since the last frame update: render a frame with the update first");
}

// Option "overlap" -1: the lane count (and staging depth) bench.py measured best per frame kind:
// with a per-frame BLAS rebuild 2 lanes (the rebuild is the frame's critical path and starves behind traces in
// flight: C5 8.8 against 9.8 ms/frame with 4 lanes; a C5 1/8 share 4.1 against 5.5 with 8; C2-LBVH 0.38 against 1.04
// with 3; profiles/r04/c5_rebuild/, profiles/r05/c5_rebuild/); else a rank's share of a multi-GPU frame (tiles, or a
// communicator of world > 1) 8 lanes and 64 staging buffers, any other frame 4 lanes.  Changing the count drains the
// scene (a new frame kind, e.g. attaching a communicator).
rt_status auto_lanes(rt_scene *s, const rt_render_opts &o) {
    const bool share = o.tile_count > 0 || (s->comm && s->comm->world > 1);
    const uint32_t L = s->rebuild_blas ? 2u : (share ? 8u : 4u);
    const int depth = share ? rt_scene::NSTAGE : 16;
    if (L == s->lanes && (s->stage_depth_set || depth == s->stage_depth)) return RT_OK;
    RT_TRY(drain(s));
    s->lanes = L;
    s->overlap = L > 1;
    s->lane = 0;
    if (!s->stage_depth_set) {
        s->stage_depth = depth;
        s->stage_next = 0;
    }
    return RT_OK;
}

// The frame's stream: the caller's; else, with "overlap", the lane's own stream (created on first use), else the
// scene's stream (every frame of the scene in order).
rt_status frame_stream(rt_scene *s, const rt_render_opts &o, hipStream_t *stream) {
    *stream = static_cast<hipStream_t>(o.stream);
    if (!*stream && s->overlap) {
        hipStream_t &ls = s->ln[s->lane].st;
        if (!ls) {
            int lo = 0, hi = 0;                    // option "lane_priority": 1 = the device's highest stream priority
            HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
            HIP_TRY(hipStreamCreateWithPriority(&ls, hipStreamNonBlocking, s->lane_priority ? hi : 0));
        }
        *stream = ls;
    } else if (!*stream) {
        *stream = s->stream;
    }
    return RT_OK;
}

// The frame's geometry: the whole frame in 8 x 8 units, or this rank's tiles (with the kernels' fast divisions), and
// the pixels the launch writes.
rt_status frame_geometry(const rt_scene *s, const rt_render_opts &o, OutputGPU &out, size_t *pixels) {
    out.leaf_early = s->leaf_early >= 0 ? (uint32_t)s->leaf_early
                                        : (s->cam.depth * s->cam.sqrt_s * s->cam.sqrt_s <= 2u ? 0u : rt_scene::LEAF_EARLY_AUTO);
    const uint32_t W = s->width, H = s->height;
    size_t npix;
    if (o.tile_count == 0) {
        out.units_x = (W + 7) / 8;
        out.units = out.units_x * ((H + 7) / 8);
        npix = (size_t)W * H;
    } else {
        if (o.tile_w == 0 || o.tile_h == 0 || o.tile_w % 8 || o.tile_h % 8 || o.tile_rank >= o.tile_count)
            return fail(RT_ERR_INVALID_ARGUMENT, "tiles must be multiples of 8 and tile_rank < tile_count");
        const uint32_t mine = tiles_for_rank(W, H, o.tile_w, o.tile_h, o.tile_rank, o.tile_count);
        out.tile_w = o.tile_w; out.tile_h = o.tile_h; out.tile_rank = o.tile_rank; out.tile_count = o.tile_count;
        out.tiles_x = (W + o.tile_w - 1) / o.tile_w;
        out.units = mine * (o.tile_w / 8) * (o.tile_h / 8);
        npix = (size_t)mine * o.tile_w * o.tile_h;
        const uint32_t upr = o.tile_w / 8;
        out.div_upr = make_fastdiv(upr);
        out.div_upt = make_fastdiv(upr * (o.tile_h / 8));
        out.div_tiles_x = make_fastdiv(out.tiles_x);
        if ((uint64_t)out.tiles_x * ((H + o.tile_h - 1) / o.tile_h) >= (1ull << FASTDIV_BITS))
            return fail(RT_ERR_INVALID_ARGUMENT, "too many tiles");
    }
    if ((uint64_t)out.units * 64u >= (1ull << FASTDIV_BITS))       // work items index pixels of whole units
        return fail(RT_ERR_INVALID_ARGUMENT, "frame too large: more than 2^27 pixels per launch");
    out.div_units_x = make_fastdiv(out.units_x ? out.units_x : 1u);
    *pixels = npix;
    return RT_OK;
}

// Outputs: caller device buffers, else scene-owned; a rank of a multi-GPU frame traces into lane q's slab, and
// *frame_out is the assembled frame on rank 0.
rt_status frame_outputs(rt_scene *s, const rt_render_opts &o, int q, size_t npix, bool want_rgb, OutputGPU &out,
                        uint8_t **frame_out) {
    const uint32_t W = s->width, H = s->height;
    CommState *cm = s->comm;
    if (cm) {
        const size_t slab_bytes = (size_t)slab_tile_count(W, H, cm->tile_w, cm->tile_h, (uint32_t)cm->world) * cm->tile_w *
                                  cm->tile_h * 4;
        if (slab_bytes != cm->slab_bytes) {    // first frame, or the camera size changed: lanes may be in flight
            RT_TRY(drain(s));
            for (int l = 0; l < CommState::NLANE; l++) { cm->slab[l].release(); cm->gathered[l].release(); }
            cm->slab_bytes = slab_bytes;
        }
        DevBuf<uint8_t> &buf = cm->rank == 0 ? cm->gathered[q] : cm->slab[q];
        const size_t need = cm->rank == 0 ? slab_bytes * (size_t)cm->world : slab_bytes;
        if (!buf.p) HIP_TRY(buf.alloc(need));  // need > 0; slab padding is never assembled: no clearing needed
        out.rgba = buf.p;                      // rank 0: slab 0 of the gather buffer
        if (cm->rank == 0) {
            if (o.rgba8_device) {
                *frame_out = static_cast<uint8_t *>(o.rgba8_device);
            } else {
                HIP_TRY(s->out_rgba.reserve((size_t)W * H * 4));
                *frame_out = s->out_rgba.p;
            }
        }
    } else if (o.rgba8_device) {
        out.rgba = static_cast<uint8_t *>(o.rgba8_device);
    } else {
        HIP_TRY(s->out_rgba.reserve(npix * 4));
        out.rgba = s->out_rgba.p;
    }
    if (o.rgb32_device) {
        out.rgb = static_cast<float *>(o.rgb32_device);
    } else if (want_rgb) {
        HIP_TRY(s->out_rgb.reserve(npix * 3));
        out.rgb = s->out_rgb.p;
    }
    return RT_OK;
}

// Options "timeline" and "costmap" (persistent kernel): their buffers, cleared on the frame's stream.
rt_status frame_debug_buffers(rt_scene *s, const rt_render_opts &o, const SceneGPU &g, size_t npix, hipStream_t stream,
                              OutputGPU &out) {
    if (s->timeline_on) {
        const uint32_t blocks = s->cus * persistent_blocks_per_cu((o.flags & RT_RENDER_EXACT) != 0, s->fast_math, g);
        const size_t words = (size_t)blocks * 4 * TIMELINE_WORDS;
        HIP_TRY(s->timeline.reserve(words));
        HIP_TRY(hipMemsetAsync(s->timeline.p, 0, words * sizeof(unsigned long long), stream));
        out.timeline = s->timeline.p;
        s->timeline_waves = blocks * 4;
    }
    if (s->costmap_on && (o.flags & RT_RENDER_COUNT_WORK)) {
        HIP_TRY(s->costmap.reserve(npix));
        HIP_TRY(hipMemsetAsync(s->costmap.p, 0, npix * sizeof(uint32_t), stream));
        out.costmap = s->costmap.p;
        s->costmap_pixels = npix;
    }
    return RT_OK;
}

// The persistent grid of lane q's launch: `cap` workgroups fit on the GPU, `paths` camera paths are traced.
uint32_t persistent_grid(const rt_scene *s, int q, uint32_t cap, uint64_t paths) {
    uint32_t blocks = s->overlap && cap > 2 * s->reserve ? cap - s->reserve : cap;
    uint32_t pct = s->grid_pct;
    if (pct == 0) {
        bool partner = false;             // another lane's launch not finished yet (host query, ~1 us)
        for (int l = 0; s->overlap && l < rt_scene::NLANE && !partner; l++)
            partner = l != q && s->ln[l].r_done && hipEventQuery(s->ln[l].r_done) == hipErrorNotReady;
        // with a partner: half the GPU for up to 3 lanes, 1 / lanes + 12 % of it with more (4 lanes: 37 %, 8 lanes:
        // 24 %: the measured best for a whole frame on 4 lanes and for a rank's 1/2, 1/4 and 1/8 share once every
        // lane runs off the null stream: C2 0.173 -> 0.164 ms/frame, C2 1/8 share 0.041 -> 0.038, 1/4 0.059 ->
        // 0.052; profiles/r03_session2/share_grid_*.txt, lanes_new*.txt); alone: all of it
        pct = !partner ? 100u : (s->lanes <= 3 ? 50u : 100u / s->lanes + 12u);
        // a launch of >= BIG_LAUNCH_PATHS camera paths (C5: 4K x 4 traced spp = 33 M) keeps all of it: its own
        // tail is a small part of its span, and a half grid only stretches the span (C5 5.88 -> 5.43 ms/frame
        // with trees built once, 13.3 -> 11.2 with the per-frame rebuild; profiles/r04/c5_rebuild/)
        if (paths >= rt_scene::BIG_LAUNCH_PATHS) pct = 100u;
    }
    if (pct < 100) blocks = std::max<uint32_t>(8u, blocks * pct / 100u);
    return blocks;
}

// The counters of a synchronous frame into counters_host[0 .. CNT_NUM): lane q's block; with "overlap" +
// RT_RENDER_KEEP_COUNTERS the accumulated totals of every lane in the current epoch (as rt_scene_collect sums them),
// after every lane's launches finished.  Returns once the frame's stream has run.
rt_status frame_counters(rt_scene *s, uint32_t flags, int q, hipStream_t stream) {
    const bool sum_lanes = s->overlap && (flags & RT_RENDER_KEEP_COUNTERS);
    if (!sum_lanes)
        HIP_TRY(hipMemcpyAsync(s->counters_host, s->lane_counters(q), CNT_NUM * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, stream));
    RT_TRY(wait_stream(s, stream));
    if (sum_lanes) {
        unsigned long long sum[CNT_NUM];       // a lane 0 out of the epoch counts as little as any other
        RT_TRY(sum_lane_counters(s, sum));
        std::memcpy(s->counters_host, sum, sizeof sum);
    }
    return RT_OK;
}

// What this launch's prologue has done so far.  The prologue is the kernel in front of the trace (the schedule kernel,
// else the frame-copy kernel) that also performs the frame block's deferred upload, clears the lane's counter block
// and resets its queue heads: each of the three once per launch, by the first prologue kernel there is.
struct Prologue {
    unsigned long long *counters;   // the lane's counter block: only this lane's launches add here
    uint32_t *queue;                // the lane's queue heads (null: no persistent kernel)
    bool zero_lane;                 // the counter block is still to clear (the lane's first launch in the counter epoch)
    bool reset_queue = true;        // the queue heads are still to reset
    bool copied_here = false;       // this call enqueued the frame block's upload on `stream`
    // ... of this frame block: no event between the copy and the trace (each event record between two kernels
    // of a stream costs ~4.5 us of GPU idle: copy -> trace gap 10.6 -> 6.1 us, profiles/r02_gaps.txt); its
    // r_copied is the trace's completion event (the host waits on it only before reusing the staging buffer)
    int copied_block = -1, copied_stage = -1;
};

// What one prologue kernel takes on, struck off the list: the pending upload (frame_update with `defer`; consumed
// here and nowhere else), the counter block, the queue heads.
struct PrologueWork {
    uint8_t *dst = nullptr;
    const uint8_t *src = nullptr;
    size_t bytes = 0;
    unsigned long long *zero = nullptr;
    uint32_t *queue = nullptr;
};
PrologueWork take_prologue(rt_scene *s, Prologue &p) {
    PrologueWork w;
    if (s->pending_copy >= 0) {
        w.dst = s->blk[s->pending_copy].dev;
        w.src = s->stg[s->pending_stage].dev;
        w.bytes = s->frame_block;
        p.copied_here = true;
        p.copied_block = s->pending_copy;
        p.copied_stage = s->pending_stage;
        s->pending_copy = -1;
    }
    if (p.zero_lane) w.zero = p.counters;
    if (p.reset_queue) w.queue = p.queue;
    p.zero_lane = p.reset_queue = false;
    return w;
}

// Option "reorder" (schedule.hip; persistent kernel, 64-pixel claims): the lane's schedule step in front of its launch.
// The schedule kernel, when it runs, is the launch's prologue and resets the queue heads itself.
rt_status schedule_step(rt_scene *s, Lane &ln, OutputGPU &out, Prologue &pro, hipStream_t stream) {
    if (ln.unit_cost.n < 2 * (size_t)out.units) {         // [recorded costs | costs of the last launch (debug)]
        ln.unit_order.release();                          // sized with the costs, whatever it held
        HIP_TRY(ln.unit_cost.reserve(2 * (size_t)out.units));
        HIP_TRY(hipMemsetAsync(ln.unit_cost.p, 0, ln.unit_cost.n * sizeof(uint32_t), stream));
        HIP_TRY(ln.unit_order.reserve(4 * (size_t)out.units));   // <= 4 items per unit
        ln.valid = false;
    }
    const uint32_t sig[7] = {out.units, out.units_x, out.tile_w, out.tile_h, out.tile_rank, out.tile_count,
                             out.queue_parts};
    // the costs the lane's previous launch recorded are for the layout it had
    const bool layout_ok = ln.valid && std::memcmp(sig, ln.sig, sizeof sig) == 0;
    const SchedStep d = sched_step(layout_ok, s->reorder_period, ln.phase);
    ln.phase = d.phase;
    if (d.drop_order) ln.order_ok = false;
    if (d.run_sched) {
        const uint32_t rows = out.tile_count == 0 ? out.units / out.units_x : out.units;
        const uint32_t upr = out.tile_count == 0 ? out.units_x : 1u;
        const PrologueWork w = take_prologue(s, pro);
        HIP_TRY(launch_schedule(ln.unit_cost.p, ln.unit_cost.p + out.units, ln.unit_order.p, ln.queue, rows, upr, out.queue_parts,
                                d.do_order, s->split & 0xFFu, (s->split >> 8) & 0xFFu, s->merge, w.dst, w.src, w.bytes, w.zero,
                                stream));
        if (d.do_order) ln.order_ok = true;
    }
    std::memcpy(ln.sig, sig, sizeof sig);
    ln.valid = true;
    out.order = ln.order_ok ? ln.unit_order.p : nullptr;
    out.unit_cost = d.track ? ln.unit_cost.p : nullptr;
    return RT_OK;
}

// What the launch waits for on its stream before its prologue: the previous launch of its lane, and the caller's
// null-stream work.
rt_status lane_waits(rt_scene *s, int q, bool order_null, hipStream_t stream) {
    if (hipEvent_t prev = s->overlap ? s->ln[q].r_done : s->r_done) HIP_TRY(hipStreamWaitEvent(stream, prev, 0));
    // Device outputs and no stream: the trace runs on a non-blocking stream of the scene, which HIP does not order
    // with the caller's null-stream work, so it waits for what the caller enqueued there before the call (e.g. a fill
    // of the buffer), and — without "overlap" — the null stream waits for the frame (a read of it after the call).  The
    // reference draws into a surface it owns on its own stream (Renderer.cu:305-317), so a drop-in caller expects no
    // ordering of its own.  With "overlap" the frames run side by side on the scene's lanes; a null-stream wait per
    // frame would serialise them, so their device outputs are complete once rt_synchronize returns.
    // (A null stream with nothing pending needs no wait: one host query instead of a cross-queue wait, ~5 us of GPU
    // idle time per frame, profiles/r02_gaps.txt.)
    if (order_null && hipStreamQuery(nullptr) == hipErrorNotReady) RT_TRY(order_after_null_stream(s, stream));
    return RT_OK;
}

// The launch's prologue: the schedule step, the frame block's upload or the wait for it, the lane's resets.
rt_status frame_prologue(rt_scene *s, Lane &ln, OutputGPU &out, Prologue &pro, hipStream_t stream) {
    if (s->use_persistent && s->reorder && s->grab == 64u) RT_TRY(schedule_step(s, ln, out, pro, stream));
    const bool upload = s->pending_copy >= 0;
    const FrameBlock &blk = s->blk[s->active];
    // the frame block's upload: stream-ordered when this call enqueues it
    if (!upload && !pro.copied_here && !(s->gpu_tlas() && blk.chain == stream))   // else built on this stream
        HIP_TRY(hipStreamWaitEvent(stream, blk.r_copied, 0));
    // the frame block's upload (and the lane's counter / queue reset); GPU-built frames: one small kernel instead of
    // two fills
    if (upload || pro.zero_lane || (pro.reset_queue && pro.queue)) {
        const PrologueWork w = take_prologue(s, pro);
        HIP_TRY(launch_frame_copy(w.dst, w.src, w.bytes, w.zero, w.queue, stream));
    }
    return RT_OK;
}

// The trace, between the timing events of its ring slot.
rt_status launch_trace(rt_scene *s, int q, uint32_t flags, const SceneGPU &g, const CameraGPU &cam, const OutputGPU &out,
                       const Prologue &pro, hipStream_t stream, uint32_t *ring_slot) {
    const bool exact = (flags & RT_RENDER_EXACT) != 0;
    const bool count = (flags & RT_RENDER_COUNT_WORK) != 0;
    const TraceFlavour &kernels = trace_flavour(exact, s->fast_math);
    const uint32_t slot = s->ring_head;
    s->ring_head = (s->ring_head + 1) % rt_scene::RING;
    if (s->ring_pending < rt_scene::RING) s->ring_pending++;
    s->last_stream = stream;
    HIP_TRY(hipEventRecord(s->ring_start[slot], stream));
    if (s->use_persistent) {
        const uint32_t cap = s->cus * persistent_blocks_per_cu(exact, s->fast_math, g);
        const uint32_t blocks = persistent_grid(s, q, cap, (uint64_t)out.units * 64u * cam.sqrt_s * cam.sqrt_s);
        const uint32_t thr = s->threshold ? s->threshold : (cam.depth * cam.sqrt_s * cam.sqrt_s <= 2u ? 64u : 40u);
        HIP_TRY(kernels.render_persistent(g, cam, out, count, pro.counters, pro.queue, blocks, thr, pro.reset_queue, stream));
    } else {
        HIP_TRY(kernels.render(g, cam, out, count, pro.counters, stream));
    }
    HIP_TRY(hipEventRecord(s->ring_stop[slot], stream));
    *ring_slot = slot;
    return RT_OK;
}

// The launch's one completion event (see FrameBlock::r_used) and every purpose it completes.
rt_status complete_launch(rt_scene *s, int q, uint32_t slot, const Prologue &pro, uint8_t *frame_out, bool null_waits,
                          hipStream_t stream) {
    hipEvent_t done = s->ring_stop[slot];
    if (s->comm) {                             // after the gather + assemble; one event per launch, never one
        RT_TRY(comm_gather(s, q, frame_out, stream));
        HIP_TRY(hipEventRecord(s->ring_post[slot], stream));   // re-recorded by the lane's next frame (the
        done = s->ring_post[slot];                              // staging / block waits must see this launch)
    }
    s->blk[s->active].r_used = s->r_done = s->ln[q].r_done = done;
    if (pro.copied_block >= 0) s->blk[pro.copied_block].r_copied = s->stg[pro.copied_stage].r_staged = done;
    if (s->cur.ev_lane[q]) HIP_TRY(hipEventRecord(s->cur.ev_lane[q], stream));   // "blas_double": this set's reader
    if (null_waits) HIP_TRY(hipStreamWaitEvent(nullptr, done, 0));
    return RT_OK;
}

}  // namespace

namespace rtamd {

// The counters of every lane whose block belongs to the current epoch, summed (rt_scene_collect, frame_counters),
// after every launch of the scene finished; counters_host holds the lanes' blocks afterwards.
rt_status sum_lane_counters(rt_scene *s, unsigned long long *sum) {
    RT_TRY(drain(s));
    HIP_TRY(hipMemcpy(s->counters_host, s->counters, rt_scene::NLANE * CNT_NUM * sizeof(unsigned long long),
                      hipMemcpyDeviceToHost));
    std::fill(sum, sum + CNT_NUM, 0ull);
    for (int l = 0; l < rt_scene::NLANE; l++)
        if (s->ln[l].epoch == s->cnt_epoch)
            for (uint32_t k = 0; k < CNT_NUM; k++) sum[k] += s->counters_host[(size_t)l * CNT_NUM + k];
    return RT_OK;
}

// a caller buffer kernels on `device` may touch: device memory of that device, managed memory, or mapped host memory
bool device_accessible(const void *p, int device) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();               // an unregistered host pointer is an error of the query, not of the runtime
        return false;
    }
    if (a.type == hipMemoryTypeDevice) return a.device == device;
    if (a.type == hipMemoryTypeManaged) return true;
    if (a.type == hipMemoryTypeHost) return a.devicePointer != nullptr;
    return false;
}

// every non-null buffer of a call is device_accessible, or the call fails with `message`
rt_status all_accessible(std::initializer_list<const void *> bufs, int device, const std::string &message) {
    for (const void *p : bufs)
        if (p && !device_accessible(p, device)) return fail(RT_ERR_INVALID_ARGUMENT, message);
    return RT_OK;
}

}  // namespace rtamd

namespace {

// rt_query_rays and rt_query_camera from the validated call on (the scene's device is current): the dependency waits,
// the launch — launch(scene, the slot's band heads, stream) -> hipError_t — and the bookkeeping of one query.
template <class Launch>
rt_status enqueue_query(rt_scene *s, void *caller_stream, bool no_sync, Launch &&launch) {
    hipStream_t st = caller_stream ? static_cast<hipStream_t>(caller_stream) : s->stream;
    const uint32_t slot = s->query_next;       // advanced once the query is enqueued: a failed call takes no slot
    hipEvent_t done = s->ev_query[slot];
    FrameBlock &blk = s->blk[s->active];
    // What the launch waits for.  Its slot's previous query (head free; see ev_query) and the previous call's (queries
    // run in call order even with a frame's launch between them).  The frame block of the last
    // update, as a RT_RENDER_SKIP_UPDATE frame does, and a GPU BLAS build still running on the scene's stream.  And
    // every event this call replaces below — the block's r_used, r_done, the BLAS set's reader event: whoever waits on those
    // afterwards sees only this query, which runs on a caller stream and so implies nothing about the launches on the
    // lane streams they stood for.
    // An event that has already completed needs no wait (a host query, ~1 us, as wait_blas_built): whatever is enqueued
    // now runs after it, and each cross-stream wait in front of a kernel costs GPU idle time.  The
    // purposes often share one event (a frame's single completion event): each is waited on once.
    const int bl = s->last_lane;
    hipEvent_t prev_query = s->ev_query[(slot + rt_scene::NQUERY - 1) % rt_scene::NQUERY];
    hipEvent_t deps[] = {done, prev_query, blk.r_copied, blk.r_used, s->r_done, s->cur.ev_lane[bl]};
    for (size_t i = 0; i < sizeof deps / sizeof deps[0]; i++) {
        bool dup = !deps[i];
        for (size_t j = 0; j < i && !dup; j++) dup = deps[j] == deps[i];
        bool pending;
        if (!dup) RT_TRY(wait_if_pending(st, deps[i], &pending));
    }
    // the caller's null-stream work (rt_render)
    if (!caller_stream && hipStreamQuery(nullptr) == hipErrorNotReady) RT_TRY(order_after_null_stream(s, st));
    if (s->blas_build_seq != 0 && st != s->stream) RT_TRY(wait_blas_built(s, st));

    HIP_TRY(launch(scene_gpu(s), s->query_heads + (size_t)slot * QUERY_PARTS * QUEUE_STRIDE, st));
    HIP_TRY(hipEventRecord(done, st));
    s->query_next = (slot + 1) % rt_scene::NQUERY;
    s->query_live = true;
    blk.r_used = s->r_done = done;             // later uploads into the block, later BLAS rebuilds, rt_synchronize
    if (s->cur.ev_lane[bl]) HIP_TRY(hipEventRecord(s->cur.ev_lane[bl], st));   // "blas_double": this set's reader
    if (!caller_stream) HIP_TRY(hipStreamWaitEvent(nullptr, done, 0));
    if (no_sync) return RT_OK;
    return wait_event(s, done);
}

}  // namespace

extern "C" {

rt_status rt_render(rt_scene *s, uint64_t frame, const rt_render_opts *opts, uint8_t *rgba_host, float *rgb_host,
                    rt_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    rt_render_opts o{};
    RT_TRY(frame_options(s, opts, rgb_host, o));
    if ((o.flags & RT_RENDER_SKIP_UPDATE) && s->blas_dirty) return fail_blas_dirty();
    HIP_TRY(hipSetDevice(s->device));
    // the lanes, the stream, the frame update
    if (s->overlap_auto) RT_TRY(auto_lanes(s, o));
    hipStream_t stream = nullptr;
    RT_TRY(frame_stream(s, o, &stream));
    const bool lib_lane = !o.stream && s->overlap;
    double update_ms = 0.0;
    if (!(o.flags & RT_RENDER_SKIP_UPDATE)) {
        const auto u0 = std::chrono::steady_clock::now();
        RT_TRY(frame_update(s, frame, stream, /*defer=*/true));
        update_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - u0).count();
    }

    // Launches of one lane never overlap, whatever streams callers pass (queue heads, unit costs).
    // Without "overlap" every launch is lane 0.  With it, frames alternate lanes: a launch waits only
    // for the previous launch of its own lane (and, below, for its frame block), so the caller can run
    // consecutive frames concurrently on two streams.
    const int q = s->overlap ? (int)s->lane : 0;
    OutputGPU out{};
    size_t npix = 0;
    RT_TRY(frame_geometry(s, o, out, &npix));
    uint8_t *frame_out = nullptr;              // multi-GPU, rank 0: the assembled frame
    RT_TRY(frame_outputs(s, o, q, npix, rgb_host != nullptr, out, &frame_out));
    CameraGPU cam = s->cam;
    cam.frame_seed = o.frame_seed;
    const SceneGPU g = scene_gpu(s);
    if (s->use_persistent) {
        out.queue_parts = s->queue_parts;
        out.grab = s->grab;
        out.supertile = s->supertile;
        RT_TRY(frame_debug_buffers(s, o, g, npix, stream, out));
    }
    s->lane = s->overlap ? (s->lane + 1) % s->lanes : 0u;
    s->last_lane = q;
    // the waits, the prologue (schedule, upload, resets), the trace, its completion event
    const bool order_null = !o.stream && (o.rgba8_device || o.rgb32_device);
    RT_TRY(lane_waits(s, q, order_null, stream));
    Lane &ln = s->ln[q];
    if (!(o.flags & RT_RENDER_KEEP_COUNTERS)) s->cnt_epoch++;
    Prologue pro{s->lane_counters(q), s->use_persistent ? ln.queue : nullptr, /*zero_lane=*/ln.epoch != s->cnt_epoch};
    ln.epoch = s->cnt_epoch;
    RT_TRY(frame_prologue(s, ln, out, pro, stream));
    uint32_t slot = 0;
    RT_TRY(launch_trace(s, q, o.flags, g, cam, out, pro, stream, &slot));
    RT_TRY(complete_launch(s, q, slot, pro, frame_out, order_null && !lib_lane, stream));
    if (o.flags & RT_RENDER_NO_SYNC) {
        if (stats) { std::memset(stats, 0, sizeof *stats); stats->update_ms = update_ms; stats->update_wait_ms = s->update_wait_ms; }
        return RT_OK;
    }
    // a synchronous frame: its counters, its pixels, its statistics
    RT_TRY(frame_counters(s, o.flags, q, stream));
    s->ring_pending = 0;
    const CommState *cm = s->comm;
    if (rgba_host && cm && cm->rank == 0)
        HIP_TRY(hipMemcpy(rgba_host, frame_out, (size_t)s->width * s->height * 4, hipMemcpyDeviceToHost));
    else if (rgba_host && !cm) HIP_TRY(hipMemcpy(rgba_host, out.rgba, npix * 4, hipMemcpyDeviceToHost));
    if (rgb_host) HIP_TRY(hipMemcpy(rgb_host, out.rgb, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (stats) {
        float kms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&kms, s->ring_start[slot], s->ring_stop[slot]));
        fill_stats(stats, s->counters_host);
        stats->kernel_ms = kms;
        stats->update_ms = update_ms;
        stats->update_wait_ms = s->update_wait_ms;
        stats->frame_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if ((o.flags & RT_RENDER_COUNT_WORK) && s->counters_host[CNT_OVERFLOW] != 0)
        return fail(RT_ERR_UNSUPPORTED, "traversal stack overflow (tree deeper than 64 levels)");
    return RT_OK;
}

rt_status rt_assemble_tiles(rt_scene *s, const void *gathered, uint32_t slab_tiles, uint32_t tw, uint32_t th,
                            uint32_t tile_count, void *frame, void *stream) {
    if (!s || !gathered || !frame) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!s->cam_ok) return fail(RT_ERR_STATE, "rt_camera_set has not been called");
    if (tw == 0 || th == 0 || tile_count == 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad tile geometry");
    if (((uintptr_t)gathered | (uintptr_t)frame) & 3u) return fail(RT_ERR_INVALID_ARGUMENT, "RGBA8 buffers must be 4-byte aligned");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : s->stream;
    // caller buffers on the scene's stream: ordered with the null stream (rt_render), pending work there or not
    if (!stream) RT_TRY(order_after_null_stream(s, st));
    HIP_TRY(launch_assemble(gathered, slab_tiles, tw, th, tile_count, s->width, s->height, frame, st));
    if (!stream) {
        HIP_TRY(hipEventRecord(s->ev_caller, st));
        HIP_TRY(hipStreamWaitEvent(nullptr, s->ev_caller, 0));
    }
    return RT_OK;
}

rt_status rt_trace_rays(rt_scene *s, const float *rays, size_t n, uint32_t flags, rt_hit *hits) {
    if (!s || (n && (!rays || !hits))) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!s->built) return fail(RT_ERR_STATE, "rt_scene_build has not been called");
    if (n == 0) return RT_OK;
    if (n > 0xFFFFFFFFull) return fail(RT_ERR_INVALID_ARGUMENT, "too many rays");
    if (s->blas_dirty) return fail_blas_dirty();
    HIP_TRY(hipSetDevice(s->device));
    float *d_rays = nullptr;
    rt_hit *d_hits = nullptr;
    HIP_TRY(hipMalloc(&d_rays, n * 6 * sizeof(float)));
    hipError_t e = hipMalloc(&d_hits, n * sizeof(rt_hit));
    if (e != hipSuccess) { (void)hipFree(d_rays); return fail(RT_ERR_OUT_OF_MEMORY, "hipMalloc hits"); }
    const SceneGPU g = scene_gpu(s);
    e = hipMemcpyAsync(d_rays, rays, n * 6 * sizeof(float), hipMemcpyHostToDevice, s->stream);
    FrameBlock &blk = s->blk[s->active];
    if (e == hipSuccess) e = hipStreamWaitEvent(s->stream, blk.r_copied, 0);
    if (e == hipSuccess)
        e = trace_flavour((flags & RT_RENDER_EXACT) != 0, s->fast_math).trace_rays(g, d_rays, (uint32_t)n, d_hits, s->stream);
    if (e == hipSuccess) e = hipEventRecord(blk.ev_used, s->stream);
    if (e == hipSuccess) blk.r_used = s->r_done = blk.ev_used;
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e == hipSuccess) e = hipMemcpy(hits, d_hits, n * sizeof(rt_hit), hipMemcpyDeviceToHost);
    (void)hipFree(d_rays);
    (void)hipFree(d_hits);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, std::string("rt_trace_rays: ") + hipGetErrorString(e));
    return RT_OK;
}

rt_status rt_query_rays(rt_scene *s, const rt_ray_query *qy) {
    if (!s || !qy) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    const uint32_t known = RT_QUERY_EXACT | RT_QUERY_ANY_HIT | RT_QUERY_NO_SYNC;
    if (qy->reserved != 0 || (qy->flags & ~known)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_query_rays: reserved bits set");
    if (qy->ray_count > 0xFFFFFFFFull) return fail(RT_ERR_INVALID_ARGUMENT, "too many rays");
    const bool any = (qy->flags & RT_QUERY_ANY_HIT) != 0;
    if (any && (!qy->occluded_device || qy->hits_device || qy->t_device))
        return fail(RT_ERR_INVALID_ARGUMENT, "an any-hit query writes occluded_device only");
    if (!any && (qy->occluded_device || (!qy->hits_device && !qy->t_device)))
        return fail(RT_ERR_INVALID_ARGUMENT, "a closest query writes hits_device and / or t_device");
    if (qy->ray_count && !qy->rays_device) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!s->built) return fail(RT_ERR_STATE, "rt_scene_build has not been called");
    if (qy->ray_count == 0) return RT_OK;
    if (s->blas_dirty) return fail_blas_dirty();
    DeviceRestore restore;
    HIP_TRY(hipSetDevice(s->device));
    RT_TRY(all_accessible({qy->rays_device, qy->tmax_device, qy->hits_device, qy->t_device, qy->occluded_device}, s->device,
                          "rt_query_rays: a buffer is not accessible from the scene's device"));

    RayQueryGPU q{};
    q.rays = qy->rays_device; q.tmax = qy->tmax_device;
    q.n = (uint32_t)qy->ray_count;
    q.hits = qy->hits_device; q.t = qy->t_device; q.occluded = qy->occluded_device;
    const TraceFlavour &fl = trace_flavour((qy->flags & RT_QUERY_EXACT) != 0, s->fast_math);
    return enqueue_query(s, qy->stream, (qy->flags & RT_QUERY_NO_SYNC) != 0,
                         [&](const SceneGPU &g, uint32_t *head, hipStream_t st) {
                             q.head = head;
                             return fl.ray_query(g, q, any, s->cus, st);
                         });
}

rt_status rt_query_camera(rt_scene *s, const rt_camera_query *cq) {
    if (!s || !cq) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    const uint32_t known = RT_CAMERA_QUERY_EXACT | RT_CAMERA_QUERY_NO_SYNC | RT_CAMERA_QUERY_FIRST_SAMPLE;
    if (cq->reserved != 0 || (cq->flags & ~known)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_query_camera: reserved bits set");
    if (!cq->rays_device && !cq->t_device && !cq->hits_device && !cq->albedo_device)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_query_camera: no output buffer");
    if (!s->built) return fail(RT_ERR_STATE, "rt_scene_build has not been called");
    if (!s->cam_ok) return fail(RT_ERR_STATE, "rt_camera_set has not been called");
    // the rectangle inside the frame, without forming x0 + width
    if (cq->x0 > s->width || cq->width > s->width - cq->x0 || cq->y0 > s->height || cq->height > s->height - cq->y0)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_query_camera: the rectangle is not inside the camera's frame");
    // work items (the pixels; 64 per 8x8 block in the block-claim variant) and output elements are 32-bit indices
    const uint64_t blocks = (uint64_t)((cq->width + 7u) / 8u) * ((cq->height + 7u) / 8u);
    if (blocks * 64u > 0xFFFFFFFFull) return fail(RT_ERR_INVALID_ARGUMENT, "rt_query_camera: too many pixels");
    if (cq->width == 0 || cq->height == 0) return RT_OK;
    if (s->blas_dirty) return fail_blas_dirty();
    DeviceRestore restore;
    HIP_TRY(hipSetDevice(s->device));
    RT_TRY(all_accessible({cq->rays_device, cq->t_device, cq->hits_device, cq->albedo_device}, s->device,
                          "rt_query_camera: a buffer is not accessible from the scene's device"));

    RayQueryGPU q{};
    q.hits = cq->hits_device; q.t = cq->t_device;
    CameraQueryGPU c{};
    c.x0 = cq->x0; c.y0 = cq->y0; c.w = cq->width; c.h = cq->height;
    c.first_sample = (cq->flags & RT_CAMERA_QUERY_FIRST_SAMPLE) ? 1u : 0u;
    c.trace = (cq->t_device || cq->hits_device || cq->albedo_device) ? 1u : 0u;
    c.rays = cq->rays_device; c.albedo = cq->albedo_device;
    CameraGPU cam = s->cam;                    // the camera as of this call
    cam.frame_seed = cq->frame_seed ? cq->frame_seed : 0x5EEDull;      // as rt_render_opts.frame_seed
    const TraceFlavour &fl = trace_flavour((cq->flags & RT_CAMERA_QUERY_EXACT) != 0, s->fast_math);
    return enqueue_query(s, cq->stream, (cq->flags & RT_CAMERA_QUERY_NO_SYNC) != 0,
                         [&](const SceneGPU &g, uint32_t *head, hipStream_t st) {
                             q.head = head;
                             return fl.camera_query(g, cam, q, c, s->cus, st);
                         });
}

rt_status rt_box_test(int device, const float *boxes, const float *rays, const float *tmax, size_t n, uint32_t mode,
                      uint8_t *hit, float *te) {
    if (n && (!boxes || !rays || !tmax || !hit || !te)) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (mode > RT_BOX_QUAD_GREEDY) return fail(RT_ERR_INVALID_ARGUMENT, "mode must be an rt_box_mode");
    if (n > 0xFFFFFFFFull / 6) return fail(RT_ERR_INVALID_ARGUMENT, "too many boxes");
    if (n == 0) return RT_OK;
    RT_TRY(select_device(device));             // and it stays current
    const size_t fb = n * 6 * sizeof(float);
    char *d = nullptr;                          // boxes | rays | tmax | te | hit
    HIP_TRY(hipMalloc(&d, 2 * fb + 2 * n * sizeof(float) + n));
    float *db = reinterpret_cast<float *>(d), *dr = reinterpret_cast<float *>(d + fb);
    float *dt = reinterpret_cast<float *>(d + 2 * fb), *de = dt + n;
    uint8_t *dh = reinterpret_cast<uint8_t *>(de + n);
    hipError_t e = hipMemcpy(db, boxes, fb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dr, rays, fb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dt, tmax, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = mode == RT_BOX_REFERENCE ? launch_box_test_exact(db, dr, dt, (uint32_t)n, mode, dh, de, nullptr)
                                     : launch_box_test_fast(db, dr, dt, (uint32_t)n, mode, dh, de, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(hit, dh, n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(te, de, n * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, std::string("rt_box_test: ") + hipGetErrorString(e));
    return RT_OK;
}

}  // extern "C"
