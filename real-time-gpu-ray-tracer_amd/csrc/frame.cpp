// frame.cpp — the host half of a frame: instance matrices, the per-frame TLAS (host-built, or the kernels that build
// it), staging and upload of a frame block (frame_update), and the SceneGPU a launch of that block sees (scene_gpu).
#include "launch.hpp"
#include "scene.hpp"

namespace {

// Instance::updateTransformArguments (src/AS/Instance.cu:4-17)
hm::V3 cos3(const rt_xform &x) {
    hm::V3 c, s;
    hm::xform_cos_sin(x, c, s);
    return c;
}
hm::V3 sin3(const rt_xform &x) {
    hm::V3 c, s;
    hm::xform_cos_sin(x, c, s);
    return s;
}

void store_rows(float *dst, const hm::Mat &m) {   // rows 1..3, cols 1..4
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) dst[4 * i + j] = m.d[i + 1][j + 1];
}

}  // namespace

namespace rtamd {

void instance_update(InstState &in, const rt_xform &x) {
    in.x = x;
    in.fwd = hm::instance_forward(x);             // shared with rt_instance_motion_records (instance_motion.hpp)
    in.inv = hm::inverse(in.fwd);
    in.nrm = hm::transpose(in.inv);
    in.tbox = hm::transform_box(in.box, in.fwd);
    in.tcentroid = hm::apply_point(in.fwd, in.centroid);
}

// Host half of one frame: update callback, instance matrices, TLAS rebuild, staging, upload.
// RT_BUILD_LBVH: the host stages matrices and transformed instance boxes only; the BLAS roots are
// patched into the instance records and the TLAS is built by kernels on the scene's stream.
// `upload` (host-built trees): the stream the upload is enqueued on — rt_render passes the stream the
// trace will run on, so upload -> schedule -> trace stay in one queue (a wait on an event of another
// queue cost ~35 us per frame, measured).
// defer (rt_render): the copy itself is left to the next launch on `upload` (pending_copy).
rt_status frame_update(rt_scene *s, uint64_t frame, hipStream_t upload, bool defer) {
    const int b = s->active < 0 ? 0 : (s->active + 1) % rt_scene::NLANE;
    const auto w0 = std::chrono::steady_clock::now();
    const int si = s->stage_next % s->stage_depth;      // this frame's staging buffer
    s->stage_next = (si + 1) % s->stage_depth;
    Stage &stage = s->stg[si];
    FrameBlock &blk = s->blk[b];
    if (stage.r_staged) RT_TRY(wait_event(s, stage.r_staged));   // no longer read by a pending copy
    if (!stage.host) {
        // every buffer of the cycle at once, on the first frame that needs one: a pinned allocation inside a run of
        // pipelined frames stalls the host's submission (one per frame for the first stage_depth frames)
        for (int i = 0; i < s->stage_depth; i++) {
            Stage &n = s->stg[i];
            if (n.host) continue;
            HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&n.host), s->frame_block, hipHostMallocDefault));
            HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&n.dev), n.host, 0));
        }
    }
    s->update_wait_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    if (s->update) {                                  // Renderer.cu:269
        std::vector<rt_xform> xs(s->inst.size());
        for (size_t i = 0; i < xs.size(); i++) xs[i] = s->inst[i].x;
        s->update(s->update_user, xs.data(), xs.size(), frame);
        // matrices are a pure function of (local box, xform): only instances whose xform changed are
        // recomputed (the demo animates 5 of C2's 73 instances) — on the GPU for GPU-built frames
        for (size_t i = 0; i < xs.size(); i++)
            if (std::memcmp(&xs[i], &s->inst[i].x, sizeof(rt_xform)) != 0) {
                if (s->gpu_tlas()) { s->inst[i].x = xs[i]; s->inst_dirty[i] = rt_scene::ALL_BLOCKS; }
                else instance_update(s->inst[i], xs[i]);
            }
    }
    uint8_t *st = stage.host;
    InstHot *hot = reinterpret_cast<InstHot *>(st + s->off_hot);
    InstCold *cold = reinterpret_cast<InstCold *>(st + s->off_cold);
    if (s->gpu_tlas()) {
        RT_TRY(lbvh_sync_groups(s));                  // option "group": which records are TLAS items
        blk.by_slot = false;                  // until the slot-order copy below
        // records: the instances, then (LBVH, option "group") the groups as instances of their merged BLAS
        const size_t nrec = s->inst.size() + s->groups.size();
        // only the changed records cross PCIe: (index, shift, cos / sin of the angles, scale, local box, inactive)
        InstDelta *dl = reinterpret_cast<InstDelta *>(st + s->off_delta);
        uint32_t nd = 0;
        const uint16_t bit = (uint16_t)(1u << b);
        for (size_t i = 0; i < nrec; i++) {
            if (!(s->inst_dirty[i] & bit)) continue;
            s->inst_dirty[i] &= (uint16_t)~bit;
            const InstState &in = record_state(s, i);
            InstDelta &d = dl[nd++];
            std::memset(&d, 0, sizeof d);
            d.index = (uint32_t)i;
            const hm::V3 c = cos3(in.x), sn = sin3(in.x);
            for (int a = 0; a < 3; a++) {
                d.p.shift[a] = hm::of(in.x.shift)[a];
                d.p.cos[a] = c[a];
                d.p.sin[a] = sn[a];
                d.p.scale[a] = hm::of(in.x.scale)[a];
                d.p.centroid[a] = in.centroid[a];
            }
            in.box.store(d.p.box);
            d.p.pad[0] = record_inactive(s, i) ? 1.0f : 0.0f;
            d.p.pad[1] = dev_bounded_rec(s, i) ? 1.0f : 0.0f;   // RT_TRI_UPDATE_BOUNDS
        }
        uint8_t *fd = blk.dev;
        uint32_t live = 0;                              // records in this frame's TLAS
        for (size_t i = 0; i < nrec; i++) live += record_inactive(s, i) ? 0u : 1u;
        const bool small = s->tlas_small && live > 0 && live <= SMALL_TLAS_MAX;
        const uint32_t n = (uint32_t)nrec;
        // the one-workgroup TLAS path touches only block b's buffers, so it runs on the trace's own stream
        // (no cross-queue wait before the trace); the multi-kernel builder's scratch is shared: scene stream
        const hipStream_t cs = small ? upload : s->stream;
        if (s->blas_builder && (s->rebuild_blas || s->blas_dirty)) {    // GPU-built BLASes only (scene stream)
            RT_TRY(gpu_build_blas(s));
            if (!s->ev_blas_built) HIP_TRY(hipEventCreateWithFlags(&s->ev_blas_built, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(s->ev_blas_built, s->stream));
            s->blas_build_seq++;
        }
        // Every frame whose records / TLAS / trace run off the scene stream waits for the last BLAS build once per
        // stream, not only the frame that enqueued it: a build swaps cur (the roots, the primitive records) to the set
        // being written ("blas_double") or rewrites them in place, and a later frame on another lane stream that
        // builds nothing would otherwise read them mid-build (rt_scene_update_triangles once, a group break)
        if (cs != s->stream && s->blas_build_seq != 0) RT_TRY(wait_blas_built(s, cs));
        if (blk.r_used) HIP_TRY(hipStreamWaitEvent(cs, blk.r_used, 0));      // block b no longer read
        RT_TRY(wait_queries(s, cs));
        // Instance::updateTransformArguments for every record of block b, on the GPU, with its BLAS root
        // (instances.hip); the deltas are read from the pinned staging block directly
        HIP_TRY(launch_instance_update(reinterpret_cast<const InstDelta *>(stage.dev + s->off_delta), nd,
                                       s->inst_params.p + (size_t)b * n, n,
                                       reinterpret_cast<InstHot *>(fd + s->off_hot), reinterpret_cast<InstCold *>(fd + s->off_cold),
                                       reinterpret_cast<float *>(fd + s->off_tbox), reinterpret_cast<float4 *>(fd + s->off_tcent),
                                       s->inst_blas.p, s->cur.roots.p, s->blas_wide_refs.p, s->ib_cent.p, /*inf_inactive=*/!small, cs));
        blk.chain = cs;
        if (small) {
            // one workgroup: the LBVH TLAS over the live records, quads, slots, slot-ordered records (lbvh_tlas_small.hpp)
            SmallTlasArgs a{};
            a.n = n;
            a.hot = reinterpret_cast<const InstHot *>(fd + s->off_hot); a.cold = reinterpret_cast<const InstCold *>(fd + s->off_cold);
            a.tbox = reinterpret_cast<const float *>(fd + s->off_tbox); a.tcent = reinterpret_cast<const float4 *>(fd + s->off_tcent);
            a.pairs = reinterpret_cast<NodePair *>(fd + s->off_pairs); a.root = reinterpret_cast<TreeRoot *>(fd + s->off_root);
            a.root_wide = reinterpret_cast<TreeRoot *>(fd + s->off_root_wide);
            a.quads = reinterpret_cast<NodeQuad *>(fd + s->off_quads); a.slots = reinterpret_cast<uint32_t *>(fd + s->off_slots);
            a.hot_s = reinterpret_cast<InstHot *>(fd + s->off_hot_s); a.cold_s = reinterpret_cast<InstCold *>(fd + s->off_cold_s);
            a.pair_count = s->gpu_counts.p + 2 + b;
            a.leaf_cap = s->tlas_leaf;
            HIP_TRY(launch_tlas_small(a, cs));
            blk.by_slot = s->inst_by_slot;
            // the trace indexes the slot-ordered copy (live records) or, without "inst_by_slot", the record-order
            // array, whose TLAS slots hold record indices up to n - 1 (lds_scene copies instance_count records)
            blk.items = s->inst_by_slot ? live : n;
            HIP_TRY(hipEventRecord(blk.ev_copied, cs));
            blk.r_copied = stage.r_staged = blk.ev_copied;
            s->active = b;
            s->frame = frame;
            return RT_OK;
        }
        blk.items = n;
        HIP_TRY(s->tlas_builder->set_items(reinterpret_cast<const float *>(fd + s->off_tbox),
                                           reinterpret_cast<const float4 *>(fd + s->off_tcent)));
        HIP_TRY(s->tlas_builder->build(reinterpret_cast<NodePair *>(fd + s->off_pairs), reinterpret_cast<TreeRoot *>(fd + s->off_root),
                                       s->gpu_counts.p + 2 + b, s->stream));
        HIP_TRY(s->tlas_builder->collapse_wide(reinterpret_cast<const NodePair *>(fd + s->off_pairs),
                                               reinterpret_cast<const TreeRoot *>(fd + s->off_root),
                                               reinterpret_cast<NodeQuad *>(fd + s->off_quads),
                                               reinterpret_cast<TreeRoot *>(fd + s->off_root_wide), s->stream));
        HIP_TRY(s->tlas_builder->gather_items(reinterpret_cast<uint32_t *>(fd + s->off_slots), s->stream));
        if (s->inst_by_slot) {
            HIP_TRY(launch_instance_slot_order(reinterpret_cast<const uint32_t *>(fd + s->off_slots),
                                               reinterpret_cast<const InstHot *>(fd + s->off_hot),
                                               reinterpret_cast<const InstCold *>(fd + s->off_cold), n,
                                               reinterpret_cast<InstHot *>(fd + s->off_hot_s),
                                               reinterpret_cast<InstCold *>(fd + s->off_cold_s), s->stream));
            blk.by_slot = true;
        }
        HIP_TRY(hipEventRecord(blk.ev_copied, s->stream));
        blk.r_copied = stage.r_staged = blk.ev_copied;
        s->active = b;
        s->frame = frame;
        return RT_OK;
    }
    // TLAS::constructTLAS over transformed instance boxes (Renderer.cu:275, TLAS.cu:4-129)
    // option "group": a group still holding its transform is one item (n + g), else its members are
    std::vector<uint8_t> intact(s->groups.size(), 0);
    for (size_t g = 0; g < s->groups.size(); g++) intact[g] = group_intact(s, g);
    std::vector<BuildItem> items;
    items.reserve(s->inst.size() + s->groups.size());
    for (size_t i = 0; i < s->inst.size(); i++)
        if (!s->group_of[i] || !intact[s->group_of[i] - 1]) items.push_back({s->inst[i].tbox, s->inst[i].tcentroid, (uint32_t)i});
    for (size_t g = 0; g < s->groups.size(); g++)
        if (intact[g]) items.push_back({s->groups[g].st.tbox, s->groups[g].st.tcentroid, (uint32_t)(s->inst.size() + g)});
    // RT_BUILD_SAH builds an SAH TLAS (option "tlas_sah" 0: the reference's median split, TLAS.cu:4-129).  The TLAS
    // decides the order in which instances are visited, and with the parallelogram's q-centred box
    // (Parallelogram.cu:48-50) that order is visible: a ray that hits the parallelogram outside its box keeps the hit
    // only when the box is tested before a farther surface shrinks the range.  The reference's median trees test the
    // ground sphere first for the demo's view (a subtree holding it and anything above the camera contains the camera,
    // so its entry is t_min); an SAH TLAS isolates the ground at the root, and visited by entry t (the SAH scenes'
    // quad order) it tests the ground first too — in the reference's pair order it would not (303 of C2's pixels at
    // depth 1; profiles/r05/order/).
    s->tlas = s->build_mode == RT_BUILD_SAH && s->tlas_sah
                  ? build_sah_tree(std::move(items), s->tlas_leaf)
                  : build_median_tree(std::move(items),
                                      s->build_mode == RT_BUILD_SAH && s->tlas_median_leaf ? s->tlas_median_leaf : TLAS_LEAF_CAP,
                                      hm::tlas_axis_state(s->build_seed, frame));
    s->tlas_flat = flatten_tree(s->tlas, 0, 0, 0, false);
    s->tlas_wide = flatten_tree_wide(s->tlas, 0, 0, 0, false, s->quad_halves());

    TreeRoot root{};
    std::memcpy(root.box, s->tlas_flat.root_box, sizeof root.box);
    root.ref = s->tlas_flat.root_ref;
    root.height = s->tlas_flat.height;
    std::memcpy(st + s->off_root, &root, sizeof root);
    root.ref = s->tlas_wide.root_ref;
    root.height = s->tlas_wide.height;
    std::memcpy(st + s->off_root_wide, &root, sizeof root);
    std::memcpy(st + s->off_quads, s->tlas_wide.quads.data(), s->tlas_wide.quads.size() * sizeof(NodeQuad));
    std::memcpy(st + s->off_pairs, s->tlas_flat.pairs.data(), s->tlas_flat.pairs.size() * sizeof(NodePair));
    std::memcpy(st + s->off_slots, s->tlas.refs.data(), s->tlas.refs.size() * sizeof(uint32_t));
    // instance records in TLAS leaf-slot order (SceneGPU::inst_by_slot): record j = the instance in slot j
    const size_t nrec = s->inst_by_slot ? s->tlas.refs.size() : s->inst.size() + s->groups.size();
    blk.by_slot = s->inst_by_slot;
    blk.items = (uint32_t)nrec;
    for (size_t j = 0; j < nrec; j++) {
        const size_t id = s->inst_by_slot ? s->tlas.refs[j] : j;
        const InstState &in = id < s->inst.size() ? s->inst[id] : s->groups[id - s->inst.size()].st;
        const BlasHost &bl = s->blas[in.blas];
        store_rows(hot[j].inv, in.inv);
        std::memcpy(hot[j].root_box, bl.flat.root_box, sizeof hot[j].root_box);
        hot[j].root_ref = bl.flat.root_ref;
        hot[j].root_ref_wide = bl.wide.root_ref;
        store_rows(cold[j].fwd, in.fwd);
        store_rows(cold[j].nrm, in.nrm);
    }
    // Measured: the upload on a dedicated copy stream (the reference's copyStream, Renderer.cu:281-303)
    // went through an SDMA engine whose first use stalled a frame by ~7.6 ms; enqueued on the trace's
    // stream it is a ~4 us blit kernel between two traces.
    HIP_TRY(hipStreamWaitEvent(upload, blk.r_used, 0));            // the block free on device
    RT_TRY(wait_queries(s, upload));
    if (defer) {
        s->pending_copy = b;
        s->pending_stage = si;
    } else {
        HIP_TRY(hipMemcpyAsync(blk.dev, st, s->frame_block, hipMemcpyHostToDevice, upload));
        HIP_TRY(hipEventRecord(blk.ev_copied, upload));
        blk.r_copied = stage.r_staged = blk.ev_copied;
    }
    s->active = b;
    s->frame = frame;
    return RT_OK;
}

SceneGPU scene_gpu(const rt_scene *s) {
    SceneGPU g{};
    const FrameBlock &blk = s->blk[s->active];
    g.blas_pairs = s->cur.pairs.p;
    g.tlas_pairs = reinterpret_cast<const NodePair *>(blk.dev + s->off_pairs);
    g.tlas_root = reinterpret_cast<const TreeRoot *>(blk.dev + s->off_root);
    g.tlas_root_wide = reinterpret_cast<const TreeRoot *>(blk.dev + s->off_root_wide);
    g.tlas_quads = reinterpret_cast<const NodeQuad *>(blk.dev + s->off_quads);
    g.blas_quads = s->cur.quads.p;
    // quad trees (GPU-built: from collapse_wide): 1 = host SAH BLASes collapsed greedily, visited by entry t; 2 = two
    // binary levels per quad visited in the reference's order (GPU-built trees); 3 = the same with every box decision
    // inside the FAST slab's error margin re-taken with the reference's slab (the reference's own trees; GPU-built
    // trees with option "exact_decisions")
    g.wide = s->wide && s->cur.quads.p != nullptr
                 ? (s->quad_halves() ? ((s->build_mode == RT_BUILD_COMPAT_MEDIAN || s->exact_decisions) ? 3u : 2u) : 1u)
                 : 0u;
    g.tlas_slots = reinterpret_cast<const uint32_t *>(blk.dev + s->off_slots);
    const bool gpu_slots = s->gpu_tlas() && blk.by_slot;   // the slot-ordered copies of GPU-built frames
    g.inst_hot = reinterpret_cast<const InstHot *>(blk.dev + (gpu_slots ? s->off_hot_s : s->off_hot));
    g.inst_cold = reinterpret_cast<const InstCold *>(blk.dev + (gpu_slots ? s->off_cold_s : s->off_cold));
    g.inst_by_slot = blk.by_slot ? 1u : 0u;   // how frame block b's instance records were staged
    g.tri_hot = s->cur.tri_hot.p; g.tri_cold = s->raw_shading() ? nullptr : s->cur.tri_cold.p;
    g.raw_tris = s->raw_shading() ? s->raw_tris.p : nullptr;
    g.sph_hot = s->cur.sph_hot.p; g.sph_cold = s->cur.sph_cold.p;
    g.quad_hot = s->cur.quad_hot.p; g.quad_cold = s->cur.quad_cold.p;
    g.materials = s->materials.p;
    g.instance_count = blk.items;   // records the frame's TLAS holds (GPU-built, small path: the live ones)
    g.rough_count = (uint32_t)s->roughs.size();
    g.material_count = (uint32_t)(s->materials.n / 4);
    // fixed setting "lds_scene" (an option until round 5): the quads the frame's TLAS refs can index (host-built: this frame's quad count;
    // GPU-built: quad q is rooted at pair q, < n - 1) and, if they fit too, the instance hot records
    // then, in this order while they fit: sphere and parallelogram records (hot + cold), instance cold records
    g.lds_icold = g.lds_sph_hot = g.lds_sph_cold = g.lds_q_hot = g.lds_q_cold = LDS_NONE;
    if (s->lds_scene && g.wide) {
        const uint32_t n = g.instance_count;
        const uint32_t nq = s->gpu_tlas() ? (n > 1 ? n - 1 : 0) : (uint32_t)s->tlas_wide.quads.size();   // GPU: <= items - 1
        if (nq > 0 && nq * LDS_QUAD_F4 <= LDS_SCENE_F4) {
            g.lds_quads = nq;
            if (nq * LDS_QUAD_F4 + n * LDS_INST_F4 <= LDS_SCENE_F4) g.lds_insts = n;
        }
        uint32_t at = s->lds_scene >= 2 ? g.lds_quads * LDS_QUAD_F4 + g.lds_insts * LDS_INST_F4 : LDS_SCENE_F4;
        const uint32_t ns = (uint32_t)s->cur.sph_hot.n, nqd = (uint32_t)s->cur.quad_hot.n;
        if (ns > 0 && at + 2 * ns <= LDS_SCENE_F4) { g.lds_sph_hot = at; g.lds_sph_cold = at + ns; at += 2 * ns; }
        if (nqd > 0 && at + (LDS_QPRIM_F4 + 1) * nqd <= LDS_SCENE_F4) {
            g.lds_q_hot = at; g.lds_q_cold = at + LDS_QPRIM_F4 * nqd; at += (LDS_QPRIM_F4 + 1) * nqd;
        }
        if (g.lds_insts && at + n * LDS_ICOLD_F4 <= LDS_SCENE_F4) { g.lds_icold = at; at += n * LDS_ICOLD_F4; }
        // option "group": the top levels of the first group's BLAS in what is left (quads in level order)
        if (s->lds_scene >= 2 && s->lds_blas && g.lds_insts && !s->groups.empty() && !s->gpu_tlas()) {
            const BlasHost &bh = s->blas[s->groups[0].st.blas];
            const uint32_t room = (LDS_SCENE_F4 - std::min(at, LDS_SCENE_F4)) / LDS_QUAD_F4;
            const uint32_t nq_b = std::min<uint32_t>(room, (uint32_t)bh.wide.quads.size());
            if (nq_b > 0 && !(bh.wide.root_ref & REF_LEAF)) {
                g.lds_bq0 = bh.wide.root_ref & REF_INDEX_MASK;
                g.lds_bqn = nq_b;
                g.lds_bq_at = at;
                at += nq_b * LDS_QUAD_F4;
            }
        }
    }
    return g;
}

// RT_BUILD_LBVH + option "group": record i (instances, then groups) kept out of the GPU TLAS — a member of an
// intact group (the group is the TLAS item) or a broken group (its members are)
bool record_inactive(const rt_scene *s, size_t i) {
    if (s->build_mode != RT_BUILD_LBVH || s->groups.empty()) return false;
    if (i < s->inst.size()) return s->group_of[i] && s->lbvh_intact[s->group_of[i] - 1];
    return !s->lbvh_intact[i - s->inst.size()];
}
const InstState &record_state(const rt_scene *s, size_t i) {
    return i < s->inst.size() ? s->inst[i] : s->groups[i - s->inst.size()].st;
}
// a group is one TLAS item while it is valid (no rt_scene_update_instances on a member) and every member still
// has the group's transform (SAH: frame_update; LBVH: lbvh_sync_groups)
bool group_intact(const rt_scene *s, size_t g) {
    const InstGroup &G = s->groups[g];
    bool ok = G.valid;
    for (size_t k = 0; ok && k < G.members.size(); k++)
        ok = std::memcmp(&s->inst[G.members[k]].x, &G.st.x, sizeof(rt_xform)) == 0;
    return ok;
}

}  // namespace rtamd
