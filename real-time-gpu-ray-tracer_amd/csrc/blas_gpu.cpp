// blas_gpu.cpp — the BLASes of RT_BUILD_LBVH, built on the GPU: the builder's segments and their book-keeping for
// option "group", the build itself (at rt_scene_build, and from frame.cpp whenever a frame needs one: option
// "rebuild", a triangle update, a group that broke), in place or into a spare BLAS set.
#include "launch.hpp"
#include "scene.hpp"

namespace rtamd {

// RT_BUILD_LBVH: (re)configure the builder's segments for the current group states: the segments of the BLASes
// in use (item ranges re-tiled in BLAS order), the group member tables, the BLAS arrays sized for them, the
// record -> segment map.  Called at the build and when a group breaks or re-forms (the device is drained).
rt_status lbvh_segments(rt_scene *s) {
    std::vector<uint8_t> use(s->blas.size(), 1);
    for (size_t g = 0; g < s->groups.size(); g++) {
        if (s->lbvh_intact[g]) for (uint32_t m : s->groups[g].members) use[s->inst[m].blas] = 0;
        else use[s->groups[g].st.blas] = 0;
    }
    std::vector<LbvhSeg> segs;
    std::vector<uint32_t> members;
    s->seg_of_blas.assign(s->blas.size(), rt_scene::NONE);
    uint32_t item = 0;
    for (size_t b = 0; b < s->blas.size(); b++) {
        if (!use[b]) continue;
        LbvhSeg sg = s->lbvh_segs[b];
        sg.item_base = item;
        sg.node_base = item - (uint32_t)segs.size();
        if (!s->blas[b].members.empty()) {
            sg.member_base = (uint32_t)(members.size() / 2);
            sg.member_count = (uint32_t)s->blas[b].members.size();
            for (const auto &m : s->blas[b].members) { members.push_back(m[0]); members.push_back(m[2]); }
        }
        s->seg_of_blas[b] = (uint32_t)segs.size();
        segs.push_back(sg);
        item += sg.count;
    }
    if (!s->blas_builder) s->blas_builder = new LbvhBuilder();
    HIP_TRY(s->blas_builder->init(segs, s->stream));
    HIP_TRY(s->blas_builder->set_members(members, s->stream));
    RT_TRY(alloc_buf(s->cur.pairs, s->blas_builder->max_pairs()));
    RT_TRY(alloc_buf(s->cur.quads, s->blas_builder->max_pairs()));   // quad q = rooted at pair q
    RT_TRY(alloc_buf(s->cur.roots, segs.size()));
    const size_t n = s->inst.size() + s->groups.size();
    std::vector<uint32_t> ib(n);
    for (size_t i = 0; i < n; i++) {
        uint32_t sg = s->seg_of_blas[record_state(s, i).blas];
        if (sg == rt_scene::NONE && i < s->inst.size() && s->group_of[i]) sg = s->seg_of_blas[s->groups[s->group_of[i] - 1].st.blas];
        ib[i] = sg == rt_scene::NONE ? 0u : sg;            // an inactive record's root is never entered
    }
    RT_TRY(upload(s->inst_blas, ib));
    s->blas_dirty = true;
    return RT_OK;
}

// RT_BUILD_LBVH, per frame: a group that broke (a member moved, rt_scene_update_instances) or re-formed switches
// the BLASes built and the records in the TLAS (their inactive flags travel with the next instance deltas)
rt_status lbvh_sync_groups(rt_scene *s) {
    if (s->build_mode != RT_BUILD_LBVH || s->groups.empty()) return RT_OK;
    bool changed = false;
    std::vector<uint8_t> now(s->groups.size());
    for (size_t g = 0; g < s->groups.size(); g++) {
        now[g] = group_intact(s, g) ? 1 : 0;
        changed = changed || now[g] != s->lbvh_intact[g];
    }
    if (!changed) return RT_OK;
    RT_TRY(drain(s));
    for (size_t g = 0; g < s->groups.size(); g++) {
        if (now[g] == s->lbvh_intact[g]) continue;
        for (uint32_t m : s->groups[g].members) s->inst_dirty[m] = rt_scene::ALL_BLOCKS;
        s->inst_dirty[s->inst.size() + g] = rt_scene::ALL_BLOCKS;
    }
    s->lbvh_intact = now;
    for (rt_scene::BlasSet &sp : s->spare) sp.release();   // re-sized with the next double-buffered build
    return lbvh_segments(s);
}

// RT_BUILD_LBVH: rebuild every BLAS on the GPU (prep -> Morton -> sort -> Karras -> boxes -> pairs ->
// leaf-ordered primitive records), on the scene stream, after the last trace that read the set it writes.
rt_status gpu_build_blas(rt_scene *s) {
    const bool spare = s->blas_double && s->blas_builds > 0;
    rt_scene::BlasSet &to = spare ? s->spare[0] : s->cur;
    if (spare) {
        // into the spare set: wait only for the traces that read it (each lane's last one), then swap it in
        if (!to.sized_as(s->cur)) {
            RT_TRY(drain(s));
            to.release();
            HIP_TRY(to.alloc_like(s->cur));
        }
        for (int q = 0; q < rt_scene::NLANE; q++)      // created with the first set (gpu_setup_blas); never recorded: no wait
            HIP_TRY(hipStreamWaitEvent(s->stream, to.ev_lane[q], 0));
    } else {
        // in place: after every trace
        if (s->blas_builds && s->r_done) HIP_TRY(hipStreamWaitEvent(s->stream, s->r_done, 0));
        for (const Lane &l : s->ln)                    // "overlap": the other lane's trace may still be running
            if (s->blas_builds && l.r_done) HIP_TRY(hipStreamWaitEvent(s->stream, l.r_done, 0));
    }
    // ray queries on caller streams; a frame on the lane may also have re-recorded a query's reader event
    RT_TRY(wait_queries(s, s->stream));
    const RawPrimsGPU raw{s->raw_tris.p, s->raw_verts.p, s->raw_sph.p, s->raw_quad.p, (uint32_t)s->roughs.size()};
    const PrimOutGPU out{to.tri_hot.p, s->raw_shading() ? nullptr : to.tri_cold.p, to.sph_hot.p, to.sph_cold.p,
                         to.quad_hot.p, to.quad_cold.p};
    HIP_TRY(s->blas_builder->set_timing(s->timeline_on));      // option "timeline": stage events (debug_read)
    HIP_TRY(s->blas_builder->prep_blas_items(raw, s->stream, !out.tri_cold));
    HIP_TRY(s->blas_builder->build(to.pairs.p, to.roots.p, s->gpu_counts.p, s->stream, &raw, &out));   // + gather
    HIP_TRY(s->blas_builder->collapse_wide(to.pairs.p, to.roots.p, to.quads.p, nullptr, s->stream));
    if (spare) {
        std::swap(s->cur, to);
        // the set just retired (frame k read it) becomes the newest spare; the one read longest ago is written next
        std::rotate(s->spare, s->spare + 1, s->spare + (s->blas_sets - 1));
    }
    s->blas_dirty = false;
    s->blas_builds++;
    return RT_OK;
}

// RT_BUILD_LBVH: upload the raw primitives, allocate the leaf-ordered arrays, build every BLAS once.
rt_status gpu_setup_blas(rt_scene *s, const uint32_t *slot_count) {
    for (const LbvhSeg &g : s->lbvh_segs) {            // the host builds check the same materials
        if (g.ptype == RT_PRIM_TRIANGLE) RT_TRY(check_materials(s, s->tris.data() + g.prim_base, g.count));
        else if (g.ptype == RT_PRIM_SPHERE) RT_TRY(check_materials(s, s->spheres.data() + g.prim_base, g.count));
        else RT_TRY(check_materials(s, s->quads.data() + g.prim_base, g.count));
    }
    RT_TRY(upload(s->raw_tris, s->tris));
    RT_TRY(alloc_buf(s->raw_verts, 9 * s->tris.size()));
    HIP_TRY(extract_tri_verts(s->raw_tris.p, s->raw_verts.p, 0, s->tris.size(), s->stream));
    RT_TRY(upload(s->raw_sph, s->spheres));
    RT_TRY(upload(s->raw_quad, s->quads));
    rt_scene::BlasSet &c = s->cur;
    RT_TRY(alloc_buf(c.tri_hot, slot_count[RT_PRIM_TRIANGLE]));
    if (s->cold_eff) {
        RT_TRY(alloc_buf(c.tri_cold, slot_count[RT_PRIM_TRIANGLE]));
    } else {
        c.tri_cold.release();                           // raw_shading(): no TriCold records
    }
    RT_TRY(alloc_buf(c.sph_hot, slot_count[RT_PRIM_SPHERE]));
    RT_TRY(alloc_buf(c.sph_cold, slot_count[RT_PRIM_SPHERE]));
    RT_TRY(alloc_buf(c.quad_hot, slot_count[RT_PRIM_PARALLELOGRAM]));
    RT_TRY(alloc_buf(c.quad_cold, slot_count[RT_PRIM_PARALLELOGRAM]));
    delete s->blas_builder;
    s->blas_builder = nullptr;
    s->lbvh_intact.assign(s->groups.size(), 1);       // members start with the group's transform (frame 0 re-checks)
    for (rt_scene::BlasSet &sp : s->spare) sp.release();
    RT_TRY(lbvh_segments(s));
    RT_TRY(alloc_buf(s->gpu_counts, 2 + rt_scene::NLANE));
    for (int q = 0; q < rt_scene::NLANE; q++) {       // "blas_double": every trace records its lane's event from now on
        if (!c.ev_lane[q]) HIP_TRY(hipEventCreateWithFlags(&c.ev_lane[q], hipEventDisableTiming));
        for (rt_scene::BlasSet &sp : s->spare)
            if (!sp.ev_lane[q]) HIP_TRY(hipEventCreateWithFlags(&sp.ev_lane[q], hipEventDisableTiming));
    }
    s->blas_builds = 0;
    RT_TRY(gpu_build_blas(s));
    // one-time readback for introspection (rt_scene_get_info)
    uint32_t pairs = 0;
    std::vector<TreeRoot> roots(c.roots.n);
    RT_TRY(drain(s));
    HIP_TRY(hipMemcpy(&pairs, s->gpu_counts.p, sizeof pairs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(roots.data(), c.roots.p, roots.size() * sizeof(TreeRoot), hipMemcpyDeviceToHost));
    s->blas_pair_count = pairs;
    s->blas_leaf_count = pairs + roots.size();       // binary trees: leaves = interior nodes + 1
    for (const TreeRoot &r : roots) s->max_blas_height = std::max(s->max_blas_height, r.height);
    return RT_OK;
}

}  // namespace rtamd
