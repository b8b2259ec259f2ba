// build.cpp — the acceleration structures: rt_scene_build (instances, their BLASes, the option-"group" BLASes, the
// leaf-ordered primitive arrays, the frame blocks and per-lane resources), the GPU BLAS builds of RT_BUILD_LBVH and
// their segment book-keeping, and the geometry updates between frames.
#include "launch.hpp"
#include "scene.hpp"

namespace {

hm::Box prim_box(const rt_scene *s, uint32_t type, uint32_t i) {
    if (type == RT_PRIM_SPHERE) return hm::sphere_box(s->spheres[i]);
    if (type == RT_PRIM_PARALLELOGRAM) return hm::quad_box(s->quads[i]);
    return hm::tri_box(s->tris[i]);
}
hm::V3 prim_centroid(const rt_scene *s, uint32_t type, uint32_t i) {
    if (type == RT_PRIM_SPHERE) return hm::sphere_centroid(s->spheres[i]);
    if (type == RT_PRIM_PARALLELOGRAM) return hm::quad_centroid(s->quads[i]);
    return hm::tri_centroid(s->tris[i]);
}

// an instance's local bounds from its primitives: their union box and mean centroid
void bounds_from_prims(const rt_scene *s, InstState &in) {
    hm::Box bb = prim_box(s, in.ptype, in.pindex);
    double c[3] = {0, 0, 0};
    for (uint32_t k = 0; k < in.pcount; k++) {
        if (k) bb = hm::Box::merge(bb, prim_box(s, in.ptype, in.pindex + k));
        const hm::V3 pc = prim_centroid(s, in.ptype, in.pindex + k);
        for (int a = 0; a < 3; a++) c[a] += pc[a];
    }
    in.box = bb;
    in.centroid = hm::v3((float)(c[0] / in.pcount), (float)(c[1] / in.pcount), (float)(c[2] / in.pcount));
}

uint32_t material_slot(const rt_scene *s, uint32_t type, uint32_t index, bool &ok) {
    if (type == RT_MAT_ROUGH && index < s->roughs.size()) return index;
    if (type == RT_MAT_METAL && index < s->metals.size()) return (uint32_t)(s->roughs.size() + index) | MAT_METAL_BIT;
    ok = false;
    return 0;
}

}  // namespace

namespace rtamd {

size_t prim_len(const rt_scene *s, uint32_t type) {
    return type == RT_PRIM_SPHERE ? s->spheres.size() : (type == RT_PRIM_PARALLELOGRAM ? s->quads.size() : s->tris.size());
}

// RT_BUILD_LBVH: (re)configure the builder's segments for the current group states: the segments of the BLASes
// in use (item ranges re-tiled in BLAS order), the group member tables, the BLAS arrays sized for them, the
// record -> segment map.  Called at the build and when a group breaks or re-forms (the device is drained).
rt_status lbvh_segments(rt_scene *s) {
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    std::vector<uint8_t> use(s->blas.size(), 1);
    for (size_t g = 0; g < s->groups.size(); g++) {
        if (s->lbvh_intact[g]) for (uint32_t m : s->groups[g].members) use[s->inst[m].blas] = 0;
        else use[s->groups[g].st.blas] = 0;
    }
    std::vector<LbvhSeg> segs;
    std::vector<uint32_t> members;
    s->seg_of_blas.assign(s->blas.size(), NONE);
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
    RT_TRY(alloc_buf(s->blas_pairs, s->blas_builder->max_pairs()));
    RT_TRY(alloc_buf(s->blas_quads, s->blas_builder->max_pairs()));   // quad q = rooted at pair q
    RT_TRY(alloc_buf(s->blas_roots, segs.size()));
    const size_t n = s->inst.size() + s->groups.size();
    std::vector<uint32_t> ib(n);
    for (size_t i = 0; i < n; i++) {
        uint32_t sg = s->seg_of_blas[record_state(s, i).blas];
        if (sg == NONE && i < s->inst.size() && s->group_of[i]) sg = s->seg_of_blas[s->groups[s->group_of[i] - 1].st.blas];
        ib[i] = sg == NONE ? 0u : sg;                      // an inactive record's root is never entered
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
// leaf-ordered primitive records), on the scene stream, after the last trace that read them.
rt_status gpu_build_blas(rt_scene *s) {
    if (s->blas_double && s->blas_builds > 0) {
        // into the spare set: wait only for the traces that read it (each lane's last one), then swap it in
        rt_scene::BlasSet &sp = s->spare[0];
        if (sp.pairs.n != s->blas_pairs.n || sp.tri_hot.n != s->tri_hot.n || sp.sph_hot.n != s->sph_hot.n ||
            sp.quad_hot.n != s->quad_hot.n || sp.roots.n != s->blas_roots.n) {
            RT_TRY(drain(s));
            sp.release();
            RT_TRY(alloc_buf(sp.pairs, s->blas_pairs.n));
            RT_TRY(alloc_buf(sp.quads, s->blas_quads.n));
            RT_TRY(alloc_buf(sp.roots, s->blas_roots.n));
            RT_TRY(alloc_buf(sp.tri_hot, s->tri_hot.n));
            RT_TRY(alloc_buf(sp.tri_cold, s->tri_cold.n));
            RT_TRY(alloc_buf(sp.sph_hot, s->sph_hot.n));
            RT_TRY(alloc_buf(sp.sph_cold, s->sph_cold.n));
            RT_TRY(alloc_buf(sp.quad_hot, s->quad_hot.n));
            RT_TRY(alloc_buf(sp.quad_cold, s->quad_cold.n));
        }
        for (int q = 0; q < rt_scene::NLANE; q++)      // created with the first set (gpu_setup_blas); never recorded: no wait
            HIP_TRY(hipStreamWaitEvent(s->stream, sp.ev_lane[q], 0));
        RT_TRY(wait_queries(s, s->stream));            // a frame on the lane may have re-recorded a query's reader event
        const RawPrimsGPU raw{s->raw_tris.p, s->raw_verts.p, s->raw_sph.p, s->raw_quad.p, (uint32_t)s->roughs.size()};
        const PrimOutGPU out{sp.tri_hot.p, s->raw_shading() ? nullptr : sp.tri_cold.p, sp.sph_hot.p, sp.sph_cold.p,
                             sp.quad_hot.p, sp.quad_cold.p};
        HIP_TRY(s->blas_builder->set_timing(s->timeline_on));      // option "timeline": stage events (debug_read)
        HIP_TRY(s->blas_builder->prep_blas_items(raw, s->stream, !out.tri_cold));
        HIP_TRY(s->blas_builder->build(sp.pairs.p, sp.roots.p, s->gpu_counts.p, s->stream, &raw, &out));   // + gather
        HIP_TRY(s->blas_builder->collapse_wide(sp.pairs.p, sp.roots.p, sp.quads.p, nullptr, s->stream));
        std::swap(s->blas_pairs, sp.pairs); std::swap(s->blas_quads, sp.quads); std::swap(s->blas_roots, sp.roots);
        std::swap(s->tri_hot, sp.tri_hot); std::swap(s->tri_cold, sp.tri_cold);
        std::swap(s->sph_hot, sp.sph_hot); std::swap(s->sph_cold, sp.sph_cold);
        std::swap(s->quad_hot, sp.quad_hot); std::swap(s->quad_cold, sp.quad_cold);
        for (int q = 0; q < rt_scene::NLANE; q++) std::swap(s->ev_blas_lane[q], sp.ev_lane[q]);
        // the set just retired (frame k read it) becomes the newest spare; the one read longest ago is written next
        std::rotate(s->spare, s->spare + 1, s->spare + (s->blas_sets - 1));
        s->blas_dirty = false;
        s->blas_builds++;
        return RT_OK;
    }
    if (s->blas_builds && s->r_done) HIP_TRY(hipStreamWaitEvent(s->stream, s->r_done, 0));
    for (int q = 0; q < rt_scene::NLANE; q++)           // "overlap": the other lane's trace may still be running
        if (s->blas_builds && s->r_lane[q]) HIP_TRY(hipStreamWaitEvent(s->stream, s->r_lane[q], 0));
    RT_TRY(wait_queries(s, s->stream));                 // ray queries on caller streams
    const RawPrimsGPU raw{s->raw_tris.p, s->raw_verts.p, s->raw_sph.p, s->raw_quad.p, (uint32_t)s->roughs.size()};
    const PrimOutGPU out{s->tri_hot.p, s->raw_shading() ? nullptr : s->tri_cold.p, s->sph_hot.p, s->sph_cold.p,
                         s->quad_hot.p, s->quad_cold.p};
    HIP_TRY(s->blas_builder->set_timing(s->timeline_on));      // option "timeline": stage events (debug_read)
    HIP_TRY(s->blas_builder->prep_blas_items(raw, s->stream, !out.tri_cold));
    HIP_TRY(s->blas_builder->build(s->blas_pairs.p, s->blas_roots.p, s->gpu_counts.p, s->stream, &raw, &out));   // + gather
    HIP_TRY(s->blas_builder->collapse_wide(s->blas_pairs.p, s->blas_roots.p, s->blas_quads.p, nullptr, s->stream));
    s->blas_dirty = false;
    s->blas_builds++;
    return RT_OK;
}

// The host mirror `tris` after rt_scene_update_triangles_device: read raw_tris back once (a cold path: the device is
// drained).  Called before the mirror's geometry is read: prim_box / prim_centroid, the host builders, the upload
// of raw_tris by a second rt_scene_build.
rt_status refresh_tris_mirror(rt_scene *s) {
    if (!s->tris_host_stale) return RT_OK;
    RT_TRY(drain(s));
    HIP_TRY(hipMemcpy(s->tris.data(), s->raw_tris.p, s->tris.size() * sizeof(rt_triangle), hipMemcpyDeviceToHost));
    s->tris_host_stale = false;
    return RT_OK;
}

// RT_TRI_UPDATE_BOUNDS (inst_bounds.hip), at rt_scene_build: the static tables — an instance's primitives never
// change — the partial sums, and every record's local centroid as the host holds it.  No record is device-bounded.
rt_status setup_inst_bounds(rt_scene *s) {
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    const size_t n = s->inst.size() + s->groups.size();
    s->dev_bounded.assign(n, 0);
    s->ib_entry_of.assign(s->inst.size(), NONE);
    std::vector<InstBoundsEntry> table;
    std::vector<uint32_t> chunk_inst, multi, members;
    std::vector<uint2> groups;
    for (size_t i = 0; i < s->inst.size(); i++) {
        const InstState &in = s->inst[i];
        if (in.ptype != RT_PRIM_TRIANGLE) continue;
        s->ib_entry_of[i] = (uint32_t)table.size();
        const uint32_t nc = ib_chunks(in.pcount);
        if (nc > 1) multi.push_back((uint32_t)table.size());
        table.push_back(InstBoundsEntry{in.pindex, in.pcount, (uint32_t)chunk_inst.size(), (uint32_t)i});
        chunk_inst.insert(chunk_inst.end(), nc, (uint32_t)table.size() - 1);
    }
    for (const InstGroup &G : s->groups) {
        groups.push_back(make_uint2((uint32_t)members.size(), (uint32_t)G.members.size()));
        for (uint32_t m : G.members) members.push_back(s->ib_entry_of[m]);       // groups hold triangle instances only
    }
    RT_TRY(upload(s->ib_table, table));
    RT_TRY(upload(s->ib_chunk_inst, chunk_inst));
    RT_TRY(upload(s->ib_multi, multi));
    RT_TRY(upload(s->ib_groups, groups));
    RT_TRY(upload(s->ib_members, members));
    RT_TRY(alloc_buf(s->ib_partials, 3 * chunk_inst.size()));
    std::vector<float4> cent(n);
    for (size_t i = 0; i < n; i++) {
        const hm::V3 c = record_state(s, i).centroid;
        cent[i] = make_float4(c.x, c.y, c.z, 0.0f);
    }
    RT_TRY(upload(s->ib_cent, cent));
    if (s->ib_cent_stage) HIP_TRY(hipHostFree(s->ib_cent_stage));
    s->ib_cent_stage = nullptr;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&s->ib_cent_stage), (n ? n : 1) * sizeof(float4), hipHostMallocDefault));
    return RT_OK;
}

// RT_BUILD_LBVH: upload the raw primitives, allocate the leaf-ordered arrays, build every BLAS once.
rt_status gpu_setup_blas(rt_scene *s, const uint32_t *slot_count) {
    const std::vector<LbvhSeg> &segs = s->lbvh_segs;
    bool ok = true;                                  // the host builds check the same materials
    for (const LbvhSeg &g : segs)
        for (uint32_t k = 0; k < g.count; k++) {
            const uint32_t pi = g.prim_base + k;
            if (g.ptype == RT_PRIM_TRIANGLE) material_slot(s, s->tris[pi].material_type, s->tris[pi].material_index, ok);
            else if (g.ptype == RT_PRIM_SPHERE) material_slot(s, s->spheres[pi].material_type, s->spheres[pi].material_index, ok);
            else material_slot(s, s->quads[pi].material_type, s->quads[pi].material_index, ok);
        }
    if (!ok) return fail(RT_ERR_INVALID_ARGUMENT, "primitive references a material out of range");
    RT_TRY(upload(s->raw_tris, s->tris));
    RT_TRY(alloc_buf(s->raw_verts, 9 * s->tris.size()));
    HIP_TRY(extract_tri_verts(s->raw_tris.p, s->raw_verts.p, 0, s->tris.size(), s->stream));
    RT_TRY(upload(s->raw_sph, s->spheres));
    RT_TRY(upload(s->raw_quad, s->quads));
    RT_TRY(alloc_buf(s->tri_hot, slot_count[RT_PRIM_TRIANGLE]));
    if (s->cold_eff) {
        RT_TRY(alloc_buf(s->tri_cold, slot_count[RT_PRIM_TRIANGLE]));
    } else {
        s->tri_cold.release();                          // raw_shading(): no TriCold records
    }
    RT_TRY(alloc_buf(s->sph_hot, slot_count[RT_PRIM_SPHERE]));
    RT_TRY(alloc_buf(s->sph_cold, slot_count[RT_PRIM_SPHERE]));
    RT_TRY(alloc_buf(s->quad_hot, slot_count[RT_PRIM_PARALLELOGRAM]));
    RT_TRY(alloc_buf(s->quad_cold, slot_count[RT_PRIM_PARALLELOGRAM]));
    delete s->blas_builder;
    s->blas_builder = nullptr;
    s->lbvh_intact.assign(s->groups.size(), 1);       // members start with the group's transform (frame 0 re-checks)
    for (rt_scene::BlasSet &sp : s->spare) sp.release();
    RT_TRY(lbvh_segments(s));
    RT_TRY(alloc_buf(s->gpu_counts, 2 + rt_scene::NLANE));
    if (!s->ev_render_done) HIP_TRY(hipEventCreateWithFlags(&s->ev_render_done, hipEventDisableTiming));
    if (!s->r_done) s->r_done = s->ev_render_done;
    for (int q = 0; q < rt_scene::NLANE; q++) {       // "blas_double": every trace records its lane's event from now on
        if (!s->ev_blas_lane[q]) HIP_TRY(hipEventCreateWithFlags(&s->ev_blas_lane[q], hipEventDisableTiming));
        for (rt_scene::BlasSet &sp : s->spare)
            if (!sp.ev_lane[q]) HIP_TRY(hipEventCreateWithFlags(&sp.ev_lane[q], hipEventDisableTiming));
    }
    s->blas_builds = 0;
    RT_TRY(gpu_build_blas(s));
    // one-time readback for introspection (rt_scene_get_info)
    uint32_t pairs = 0;
    std::vector<TreeRoot> roots(s->blas_roots.n);
    RT_TRY(drain(s));
    HIP_TRY(hipMemcpy(&pairs, s->gpu_counts.p, sizeof pairs, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(roots.data(), s->blas_roots.p, roots.size() * sizeof(TreeRoot), hipMemcpyDeviceToHost));
    s->blas_pair_count = pairs;
    s->blas_leaf_count = pairs + roots.size();       // binary trees: leaves = interior nodes + 1
    for (const TreeRoot &r : roots) s->max_blas_height = std::max(s->max_blas_height, r.height);
    return RT_OK;
}

}  // namespace rtamd

// rt_scene_build's steps, in the order it runs them
namespace {

// where the next BLAS goes in the scene's arrays: its node pairs, its quads, its leaf slots per primitive type
struct BlasCursor {
    uint32_t pair = 0, quad = 0;
    uint32_t slot[3] = {0, 0, 0};
};

rt_status fail_leaf_slots() { return fail(RT_ERR_UNSUPPORTED, "too many primitives of one type (2^26 leaf slots)"); }

// A host-built BLAS over `count` primitives of bh.type (bh.tree): flattened at the cursor, which moves past it, and
// added to the scene.  Returns its index.
uint32_t add_host_blas(rt_scene *s, BlasHost &&bh, BlasCursor &at, uint32_t count, bool level_order) {
    bh.pair_base = at.pair;
    bh.slot_base = at.slot[bh.type];
    bh.flat = flatten_tree(bh.tree, at.pair, bh.slot_base, bh.type, true);
    bh.wide = flatten_tree_wide(bh.tree, at.quad, bh.slot_base, bh.type, true, s->quad_halves(), level_order);
    at.quad += (uint32_t)bh.wide.quads.size();
    s->max_blas_height = std::max(s->max_blas_height, bh.flat.height);
    at.pair += (uint32_t)bh.flat.pairs.size();
    at.slot[bh.type] += count;
    s->blas.push_back(std::move(bh));
    return (uint32_t)s->blas.size() - 1;
}

// buildBLASPinMem (RenderPin.cu:99-201): complete instances, one BLAS per unique (type, index).
// The reference's map stores the instance index instead of the BLAS index (RenderPin.cu:151);
// the BLAS index is stored here (identical whenever the reference's demo order is used).
rt_status build_instances(rt_scene *s, BlasCursor &at) {
    const rt_build_mode mode = s->build_mode;
    std::vector<std::pair<uint64_t, uint32_t>> seen;
    std::vector<LbvhSeg> &segs = s->lbvh_segs;  // RT_BUILD_LBVH: one tree per unique BLAS
    segs.clear();
    uint64_t item_total = 0;
    uint32_t *slot_base = at.slot;
    for (size_t i = 0; i < s->inst_desc.size(); i++) {
        const rt_instance_desc &id = s->inst_desc[i];
        InstState in{};
        in.ptype = id.primitive_type; in.pindex = id.primitive_index; in.pcount = id.primitive_count;
        if (in.pcount == 0) {
            in.pcount = 1;                                           // objectPrimitiveCount()
            in.box = prim_box(s, in.ptype, in.pindex);
            in.centroid = prim_centroid(s, in.ptype, in.pindex);
        } else if (id.has_local_bounds) {                            // VTKReader.cu:204-209
            in.box = hm::Box::from_ranges({id.local_bounds[0], id.local_bounds[1]}, {id.local_bounds[2], id.local_bounds[3]},
                                          {id.local_bounds[4], id.local_bounds[5]});
            in.centroid = hm::of(id.local_centroid);
        } else {                                                     // extension: union box, mean centroid
            bounds_from_prims(s, in);
        }
        const uint64_t key = ((uint64_t)in.ptype << 32) | in.pindex;
        bool dup = false;
        for (const auto &kv : seen)
            if (kv.first == key) { in.blas = kv.second; dup = true; break; }
        if (!dup) {
            in.blas = (uint32_t)s->blas.size();
            seen.push_back({key, in.blas});
            BlasHost bh;
            bh.type = in.ptype;
            if (mode == RT_BUILD_LBVH) {
                if ((uint64_t)slot_base[in.ptype] + in.pcount >= MAX_LEAF_SLOTS || item_total + in.pcount >= (1ull << 31))
                    return fail(RT_ERR_UNSUPPORTED, "too many primitives of one type (2^26 leaf slots)");
                bh.pair_base = 0;
                bh.slot_base = slot_base[in.ptype];
                segs.push_back(LbvhSeg{(uint32_t)item_total, in.pcount, slot_base[in.ptype], in.pindex, in.ptype,
                                       (uint32_t)(item_total - segs.size()), LBVH_BLAS_LEAF_CAP, 1u});
                item_total += in.pcount;
                slot_base[in.ptype] += in.pcount;
                s->blas.push_back(std::move(bh));
                s->inst.push_back(in);
                continue;
            }
            std::vector<BuildItem> items(in.pcount);
            for (uint32_t k = 0; k < in.pcount; k++)
                items[k] = {prim_box(s, in.ptype, in.pindex + k), prim_centroid(s, in.ptype, in.pindex + k), in.pindex + k};
            bh.tree = mode == RT_BUILD_SAH ? build_sah_tree(std::move(items), s->blas_leaf)
                                           : build_median_tree(std::move(items), BLAS_LEAF_CAP,
                                                               hm::blas_axis_state(s->build_seed, in.blas));
            if ((uint64_t)slot_base[in.ptype] + in.pcount >= MAX_LEAF_SLOTS) return fail_leaf_slots();
            add_host_blas(s, std::move(bh), at, in.pcount, /*level_order=*/false);
        }
        s->inst.push_back(in);
    }
    s->blas_own = s->blas.size();
    return RT_OK;
}

// Option "group": triangle instances with bit-identical transforms and a BLAS of their own share one merged BLAS
// (InstGroup), added behind the instances' own BLASes.
rt_status build_groups(rt_scene *s, BlasCursor &at) {
    const rt_build_mode mode = s->build_mode;
    std::vector<LbvhSeg> &segs = s->lbvh_segs;
    s->group_of.assign(s->inst.size(), 0u);
    if (s->group_inst && ((mode == RT_BUILD_SAH && !s->gpu_tlas()) || mode == RT_BUILD_LBVH)) {
        std::vector<uint32_t> users(s->blas.size(), 0u);
        for (const InstState &in : s->inst) users[in.blas]++;
        std::map<std::string, std::vector<uint32_t>> by_xform;
        for (size_t i = 0; i < s->inst.size(); i++) {
            const InstState &in = s->inst[i];
            if (in.ptype != RT_PRIM_TRIANGLE || users[in.blas] != 1) continue;
            const rt_xform &x = s->inst_desc[i].xform;
            by_xform[std::string(reinterpret_cast<const char *>(&x), sizeof x)].push_back((uint32_t)i);
        }
        for (auto &kv : by_xform) {
            if (kv.second.size() < 2) continue;
            InstGroup g;
            g.members = kv.second;
            std::vector<std::array<uint32_t, 3>> ranges;
            for (uint32_t i : g.members) ranges.push_back({s->inst[i].pindex, s->inst[i].pcount, i});
            std::sort(ranges.begin(), ranges.end());
            bool disjoint = true;          // every triangle of the group belongs to exactly one member
            for (size_t k = 1; k < ranges.size(); k++)
                disjoint = disjoint && ranges[k][0] >= ranges[k - 1][0] + ranges[k - 1][1];
            if (mode == RT_BUILD_LBVH) {
                // the group's LBVH segment is one contiguous primitive range and reuses its members' leaf slots:
                // their triangles back to back, their slot ranges too (the reference's VTK particles, C5)
                for (size_t k = 1; k < ranges.size() && disjoint; k++) {
                    const BlasHost &a = s->blas[s->inst[ranges[k - 1][2]].blas], &c = s->blas[s->inst[ranges[k][2]].blas];
                    disjoint = ranges[k][0] == ranges[k - 1][0] + ranges[k - 1][1] && c.slot_base == a.slot_base + ranges[k - 1][1];
                }
            }
            if (!disjoint) continue;
            const uint32_t gi = (uint32_t)s->groups.size();
            uint64_t total = 0;
            double c[3] = {0, 0, 0};
            BlasHost bh;
            bh.type = RT_PRIM_TRIANGLE;
            for (size_t k = 0; k < g.members.size(); k++) {
                const InstState &m = s->inst[g.members[k]];
                g.st.box = k ? hm::Box::merge(g.st.box, m.box) : m.box;
                for (int a = 0; a < 3; a++) c[a] += m.centroid[a];
                total += m.pcount;
                bh.members.push_back({m.pindex, m.pcount, g.members[k]});
                s->group_of[g.members[k]] = gi + 1;
            }
            if (mode != RT_BUILD_LBVH && (uint64_t)at.slot[RT_PRIM_TRIANGLE] + total >= MAX_LEAF_SLOTS)
                return fail_leaf_slots();
            g.st.ptype = RT_PRIM_TRIANGLE;
            g.st.pindex = 0;
            g.st.pcount = (uint32_t)total;
            g.st.centroid = hm::v3((float)(c[0] / g.members.size()), (float)(c[1] / g.members.size()),
                                   (float)(c[2] / g.members.size()));
            g.st.x = s->inst_desc[g.members[0]].xform;
            if (mode == RT_BUILD_LBVH) {
                // one more segment over the members' triangles, in their leaf slots (lbvh_segments builds either
                // it or the members' own segments); item / node bases are assigned there
                bh.slot_base = s->blas[s->inst[ranges[0][2]].blas].slot_base;
                bh.pair_base = 0;
                segs.push_back(LbvhSeg{0u, (uint32_t)total, bh.slot_base, ranges[0][0], RT_PRIM_TRIANGLE, 0u,
                                       LBVH_BLAS_LEAF_CAP, 1u, 0u, 0u});
                std::sort(bh.members.begin(), bh.members.end());
                g.st.blas = (uint32_t)s->blas.size();
                s->blas.push_back(std::move(bh));
                s->groups.push_back(std::move(g));
                continue;
            }
            std::vector<BuildItem> items;
            items.reserve(total);
            for (const auto &mr : bh.members)
                for (uint32_t k = 0; k < mr[1]; k++)
                    items.push_back({prim_box(s, RT_PRIM_TRIANGLE, mr[0] + k), prim_centroid(s, RT_PRIM_TRIANGLE, mr[0] + k), mr[0] + k});
            bh.tree = build_sah_tree(std::move(items), s->blas_leaf);
            std::sort(bh.members.begin(), bh.members.end());
            g.st.blas = add_host_blas(s, std::move(bh), at, (uint32_t)total, /*level_order=*/true);
            s->groups.push_back(std::move(g));
        }
    }
    return RT_OK;
}

// Host-built BLASes: the leaf-ordered primitive arrays and the node pairs / quads of every BLAS, uploaded.
rt_status upload_host_blases(rt_scene *s, const BlasCursor &at) {
    const uint32_t *slot_base = at.slot;
    std::vector<NodePair> pairs;
    pairs.reserve(at.pair);
    std::vector<NodeQuad> quads;
    quads.reserve(at.quad);
    std::vector<TriHot> th; std::vector<TriCold> tc;
    std::vector<SphereHot> sh; std::vector<PrimCold> sc;
    std::vector<QuadHot> qh; std::vector<PrimCold> qc;
    th.reserve(slot_base[2]); tc.reserve(slot_base[2]);
    bool mat_ok = true;
    s->blas_leaf_count = 0;
    for (const BlasHost &bh : s->blas) {
        pairs.insert(pairs.end(), bh.flat.pairs.begin(), bh.flat.pairs.end());
        quads.insert(quads.end(), bh.wide.quads.begin(), bh.wide.quads.end());
        s->blas_leaf_count += bh.flat.leaves;
        for (uint32_t pi : bh.tree.refs) {
            if (bh.type == RT_PRIM_TRIANGLE) {
                const rt_triangle &t = s->tris[pi];
                const hm::TriDerived dv = hm::tri_derive(t);
                TriHot h{};
                TriCold c{};
                for (int a = 0; a < 3; a++) {
                    h.v0[a] = hm::of(t.vertex[0])[a]; h.e1[a] = dv.e1[a]; h.e2[a] = dv.e2[a];
                    c.n0[a] = dv.n[0][a]; c.n1[a] = dv.n[1][a]; c.n2[a] = dv.n[2][a];
                }
                c.material = material_slot(s, t.material_type, t.material_index, mat_ok);
                c.orig_index = pi;
                if (!bh.members.empty()) {        // a group's BLAS: the caller instance holding triangle pi, + 1
                    auto it = std::upper_bound(bh.members.begin(), bh.members.end(), std::array<uint32_t, 3>{pi, ~0u, ~0u});
                    c.pad = (*(it - 1))[2] + 1u;
                }
                th.push_back(h); tc.push_back(c);
            } else if (bh.type == RT_PRIM_SPHERE) {
                const rt_sphere &sp = s->spheres[pi];
                sh.push_back(SphereHot{{sp.center.x, sp.center.y, sp.center.z}, sp.radius});
                sc.push_back(PrimCold{material_slot(s, sp.material_type, sp.material_index, mat_ok), pi, 0, 0});
            } else {
                const rt_parallelogram &p = s->quads[pi];
                const hm::QuadDerived dv = hm::quad_derive(p);
                QuadHot q{};
                for (int a = 0; a < 3; a++) {
                    q.n[a] = dv.n[a]; q.q[a] = hm::of(p.q)[a]; q.u[a] = hm::of(p.u)[a]; q.v[a] = hm::of(p.v)[a];
                    q.nx[a] = dv.nx[a];
                }
                q.d = dv.d; q.den = dv.den;
                qh.push_back(q);
                qc.push_back(PrimCold{material_slot(s, p.material_type, p.material_index, mat_ok), pi, 0, 0});
            }
        }
    }
    if (!mat_ok) return fail(RT_ERR_INVALID_ARGUMENT, "primitive references a material out of range");
    s->blas_pair_count = pairs.size();

    RT_TRY(upload(s->blas_pairs, pairs));
    RT_TRY(upload(s->blas_quads, quads));
    RT_TRY(upload(s->tri_hot, th));
    RT_TRY(upload(s->tri_cold, tc));
    RT_TRY(upload(s->sph_hot, sh));
    RT_TRY(upload(s->sph_cold, sc));
    RT_TRY(upload(s->quad_hot, qh));
    RT_TRY(upload(s->quad_cold, qc));
    return RT_OK;
}

// per-frame double buffers (sized for every instance and every group as a TLAS item): the frame block's layout
void layout_frame_block(rt_scene *s) {
    const size_t n = s->inst.size() + s->groups.size();
    s->off_root = 0;
    s->off_pairs = 64;
    s->off_slots = align16(s->off_pairs + n * sizeof(NodePair));
    s->off_hot = align16(s->off_slots + n * sizeof(uint32_t));
    s->off_cold = align16(s->off_hot + n * sizeof(InstHot));
    s->off_tbox = align16(s->off_cold + n * sizeof(InstCold));
    s->off_tcent = align16(s->off_tbox + n * 6 * sizeof(float));
    s->off_root_wide = 32;                                         // second half of the root's 64 B
    s->off_quads = (s->off_tcent + n * 4 * sizeof(float) + 127) & ~size_t(127);
    s->off_delta = align16(s->off_quads + n * sizeof(NodeQuad));   // <= n - 1 quads
    s->frame_block = s->off_delta + (s->gpu_tlas() ? n * sizeof(InstDelta) : 0);
    if (s->gpu_tlas()) {       // GPU-built TLAS: the instance records again, in TLAS leaf-slot order
        s->off_hot_s = align16(s->frame_block);
        s->off_cold_s = align16(s->off_hot_s + n * sizeof(InstHot));
        s->frame_block = s->off_cold_s + n * sizeof(InstCold);
    }
}

// GPU-built TLAS: the side tables its kernels read, the per-block instance parameters, the TLAS builder
rt_status setup_gpu_tlas(rt_scene *s) {
    const size_t n = s->inst.size() + s->groups.size();
    if (s->gpu_tlas() && s->build_mode == RT_BUILD_SAH) {
        // host-built BLASes under the GPU TLAS: their roots (box, pair ref, quad ref) and the instance map
        std::vector<TreeRoot> roots(s->blas.size());
        std::vector<uint32_t> wide_refs(s->blas.size()), ib(n);
        for (size_t b = 0; b < s->blas.size(); b++) {
            std::memcpy(roots[b].box, s->blas[b].flat.root_box, sizeof roots[b].box);
            roots[b].ref = s->blas[b].flat.root_ref;
            roots[b].height = s->blas[b].flat.height;
            wide_refs[b] = s->blas[b].wide.root_ref;
        }
        for (size_t i = 0; i < s->inst.size(); i++) ib[i] = s->inst[i].blas;
        RT_TRY(upload(s->blas_roots, roots));
        RT_TRY(upload(s->blas_wide_refs, wide_refs));
        RT_TRY(upload(s->inst_blas, ib));
        RT_TRY(alloc_buf(s->gpu_counts, 2 + rt_scene::NLANE));
    }
    if (s->gpu_tlas()) {
        RT_TRY(alloc_buf(s->inst_params, n * rt_scene::NLANE));   // one copy per frame block
        s->inst_dirty.assign(n, rt_scene::ALL_BLOCKS);              // each block's first frame uploads every record
        delete s->tlas_builder;
        s->tlas_builder = new LbvhBuilder();
        const std::vector<LbvhSeg> tseg{LbvhSeg{0u, (uint32_t)n, 0u, 0u, 0u, 0u, s->tlas_leaf, 0u}};
        HIP_TRY(s->tlas_builder->init(tseg, s->stream));
    }
    return RT_OK;
}

// The frame blocks and what every lane and launch needs: staging reset, events, counters, queue heads, query slots.
// Everything that survives a rebuild is created once.
rt_status setup_frame_resources(rt_scene *s) {
    for (int i = 0; i < rt_scene::NSTAGE; i++) {
        if (s->staging[i]) { (void)hipHostFree(s->staging[i]); s->staging[i] = nullptr; }   // frame_update allocates
        s->staging_dev[i] = nullptr;
        s->r_staged[i] = nullptr;
    }
    s->stage_next = 0;
    for (int b = 0; b < rt_scene::NLANE; b++) {
        if (s->frame_dev[b]) { (void)hipFree(s->frame_dev[b]); s->frame_dev[b] = nullptr; }
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->frame_dev[b]), s->frame_block));
        if (!s->ev_copied[b]) HIP_TRY(hipEventCreateWithFlags(&s->ev_copied[b], hipEventDisableTiming));
        if (!s->ev_used[b]) HIP_TRY(hipEventCreateWithFlags(&s->ev_used[b], hipEventDisableTiming));
        if (!s->r_copied[b]) s->r_copied[b] = s->ev_copied[b];
        if (!s->r_used[b]) s->r_used[b] = s->ev_used[b];
    }
    for (uint32_t i = 0; i < rt_scene::RING; i++) {
        if (!s->ring_start[i]) HIP_TRY(hipEventCreate(&s->ring_start[i]));
        if (!s->ring_stop[i]) HIP_TRY(hipEventCreate(&s->ring_stop[i]));
        if (!s->ring_post[i]) HIP_TRY(hipEventCreateWithFlags(&s->ring_post[i], hipEventDisableTiming));
    }
    if (!s->counters) {
        HIP_TRY(hipMalloc(&s->counters, rt_scene::NLANE * CNT_NUM * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(s->counters, 0, rt_scene::NLANE * CNT_NUM * sizeof(unsigned long long)));
    }
    for (int q = 0; q < rt_scene::NLANE; q++) {
        if (!s->queue[q]) {   // band heads, then (option "reorder") band item counts, one 128 B line each
            HIP_TRY(hipMalloc(&s->queue[q], QUEUE_WORDS * sizeof(uint32_t)));
            HIP_TRY(hipMemset(s->queue[q], 0, QUEUE_WORDS * sizeof(uint32_t)));
        }
        if (!s->ev_lane_done[q]) HIP_TRY(hipEventCreateWithFlags(&s->ev_lane_done[q], hipEventDisableTiming));
        if (!s->r_lane[q]) s->r_lane[q] = s->ev_lane_done[q];
    }
    {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, s->device));
        s->cus = (uint32_t)prop.multiProcessorCount;
        if (const char *k = std::getenv("RTAMD_KERNEL")) s->use_persistent = std::string(k) != "grid";
        if (const char *t = std::getenv("RTAMD_THRESHOLD")) {
            const long v = std::strtol(t, nullptr, 10);
            if (v >= 1 && v <= 64) s->threshold = (uint32_t)v;
        }
    }
    if (!s->query_heads) {
        HIP_TRY(hipMalloc(&s->query_heads, rt_scene::NQUERY * QUERY_PARTS * QUEUE_STRIDE * sizeof(uint32_t)));
        HIP_TRY(hipMemset(s->query_heads, 0, rt_scene::NQUERY * QUERY_PARTS * QUEUE_STRIDE * sizeof(uint32_t)));
        for (hipEvent_t &e : s->ev_query) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (!s->counters_host)
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&s->counters_host), rt_scene::NLANE * CNT_NUM * sizeof(unsigned long long),
                              hipHostMallocDefault));
    return RT_OK;
}

bool tri_range_overlaps(const InstState &in, uint64_t first, uint64_t count) {
    return in.ptype == RT_PRIM_TRIANGLE && (uint64_t)in.pindex + in.pcount > first && in.pindex < first + count;
}

// RT_TRI_UPDATE_BOUNDS: the host changed the local centroids of `records` (sorted): their entries of the device array,
// which a group's mean reads, on the scene stream — through the pinned stage, after the record chains of the frames
// already enqueued (a chain may still read the device-written value of a record the host just took back)
rt_status refresh_dev_centroids(rt_scene *s, const std::vector<uint32_t> &records) {
    if (records.empty() || !s->ib_cent.p) return RT_OK;
    RT_TRY(wait_record_chains(s, s->stream));
    for (size_t k = 0; k < records.size();) {
        size_t e = k;
        while (e + 1 < records.size() && records[e + 1] == records[e] + 1) e++;
        for (size_t j = k; j <= e; j++) {
            const hm::V3 c = record_state(s, records[j]).centroid;
            s->ib_cent_stage[records[j]] = make_float4(c.x, c.y, c.z, 0.0f);
        }
        HIP_TRY(hipMemcpyAsync(s->ib_cent.p + records[k], s->ib_cent_stage + records[k], (e - k + 1) * sizeof(float4),
                               hipMemcpyHostToDevice, s->stream));
        k = e + 1;
    }
    return RT_OK;
}

// an instance's bounds as rt_scene_update_triangles derives them from the (current) host mirror
void host_bounds(rt_scene *s, InstState &in) {
    bounds_from_prims(s, in);
    if (in.pcount == 1) in.centroid = prim_centroid(s, in.ptype, in.pindex);   // not the mean of one: keeps a -0
}

// What rt_scene_update_triangles and rt_scene_update_triangles_device check alike: the scene's state, its build mode
// and the range, overflow-safe.
rt_status tri_update_check(const rt_scene *s, uint64_t first, uint64_t count) {
    if (!s->built) return fail(RT_ERR_STATE, "rt_scene_build has not been called");
    if (s->build_mode != RT_BUILD_LBVH) return fail(RT_ERR_UNSUPPORTED, "triangle updates need RT_BUILD_LBVH");
    if (first > s->tris.size() || count > s->tris.size() - first) return fail(RT_ERR_INVALID_ARGUMENT, "triangle range out of bounds");
    return RT_OK;
}

// ... and what both order their write into raw_tris behind.  No drain: the write goes on the scene stream, behind its
// pending BLAS builds (the next build, which the frame update enqueues after it, reads the new triangles); with
// raw_shading() traces read raw_tris at their hits too, so it also waits for every lane's last trace (and the last
// synchronous one)
rt_status tri_update_waits(rt_scene *s) {
    if (!s->raw_shading()) return RT_OK;
    if (s->r_done) HIP_TRY(hipStreamWaitEvent(s->stream, s->r_done, 0));
    for (int q = 0; q < rt_scene::NLANE; q++)
        if (s->r_lane[q]) HIP_TRY(hipStreamWaitEvent(s->stream, s->r_lane[q], 0));
    return wait_queries(s, s->stream);               // a query's records read raw_tris too (finalize, RAW 1)
}

}  // namespace

extern "C" {

rt_status rt_scene_build(rt_scene *s, rt_build_mode mode, uint64_t seed) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "null scene");
    if (mode != RT_BUILD_COMPAT_MEDIAN && mode != RT_BUILD_SAH && mode != RT_BUILD_LBVH)
        return fail(RT_ERR_UNSUPPORTED, "unsupported build mode");
    HIP_TRY(hipSetDevice(s->device));
    if (s->built) RT_TRY(drain(s));              // a rebuild frees buffers earlier frames may still read
    RT_TRY(refresh_tris_mirror(s));              // ... and builds from the triangles a device update wrote
    s->build_seed = seed;
    s->build_mode = mode;
    s->cold_eff = s->cold_records == 1 || (s->cold_records < 0 && !s->rebuild_blas);
    s->inst.clear();
    s->blas.clear();
    s->groups.clear();
    s->group_of.clear();
    s->max_blas_height = 0;
    for (bool &v : s->block_by_slot) v = false;    // a rebuild may change the mode: no block is slot-ordered yet

    BlasCursor at;
    RT_TRY(build_instances(s, at));
    RT_TRY(build_groups(s, at));
    if (!s->stream) {
        // the scene stream (uploads, GPU BLAS builds) at normal priority: the highest measured neutral (round 3)
        HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    }
    if (!s->ev_render_done) HIP_TRY(hipEventCreateWithFlags(&s->ev_render_done, hipEventDisableTiming));
    if (!s->r_done) s->r_done = s->ev_render_done;
    for (bool &v : s->sched_valid) v = false;
    if (mode == RT_BUILD_LBVH) RT_TRY(gpu_setup_blas(s, at.slot));
    else RT_TRY(upload_host_blases(s, at));
    std::vector<float> mats;
    for (const auto &r : s->roughs) { mats.push_back(r.albedo.x); mats.push_back(r.albedo.y); mats.push_back(r.albedo.z); mats.push_back(0.0f); }
    for (const auto &m : s->metals) { mats.push_back(m.albedo.x); mats.push_back(m.albedo.y); mats.push_back(m.albedo.z); mats.push_back(m.fuzz); }
    RT_TRY(upload(s->materials, mats));
    layout_frame_block(s);
    RT_TRY(setup_gpu_tlas(s));
    s->dev_bounded.clear();                      // the descriptions' or the host-derived bounds again
    if (mode == RT_BUILD_LBVH) RT_TRY(setup_inst_bounds(s));
    RT_TRY(setup_frame_resources(s));
    s->active = -1;

    // initial transforms, then the frame-0 update + TLAS (Renderer.cu:110-111, 148-150)
    for (size_t i = 0; i < s->inst.size(); i++) instance_update(s->inst[i], s->inst_desc[i].xform);
    for (InstGroup &g : s->groups) instance_update(g.st, g.st.x);
    s->built = true;
    return frame_update(s, 0, s->stream);
}

rt_status rt_scene_update_triangles(rt_scene *s, size_t first, size_t count, const rt_triangle *tris) {
    if (!s || (count && !tris)) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    RT_TRY(tri_update_check(s, first, count));
    if (count == 0) return RT_OK;
    bool ok = true;
    for (size_t k = 0; k < count; k++) material_slot(s, tris[k].material_type, tris[k].material_index, ok);
    if (!ok) return fail(RT_ERR_INVALID_ARGUMENT, "triangle references a material out of range");
    HIP_TRY(hipSetDevice(s->device));
    if (s->ev_raw_staged) RT_TRY(wait_event(s, s->ev_raw_staged));      // the previous staged copy is done
    else HIP_TRY(hipEventCreateWithFlags(&s->ev_raw_staged, hipEventDisableTiming));
    if (count > s->raw_stage_cap) {
        if (s->raw_stage) HIP_TRY(hipHostFree(s->raw_stage));
        s->raw_stage = nullptr;
        s->raw_stage_cap = 0;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&s->raw_stage), count * sizeof(rt_triangle), hipHostMallocDefault));
        s->raw_stage_cap = count;
    }
    std::memcpy(s->raw_stage, tris, count * sizeof(rt_triangle));
    std::memcpy(s->tris.data() + first, tris, count * sizeof(rt_triangle));
    RT_TRY(tri_update_waits(s));
    HIP_TRY(hipMemcpyAsync(s->raw_tris.p + first, s->raw_stage, count * sizeof(rt_triangle), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(extract_tri_verts(s->raw_tris.p, s->raw_verts.p, first, count, s->stream));
    HIP_TRY(hipEventRecord(s->ev_raw_staged, s->stream));
    // instance boxes derived from the triangles (RenderPin.cu:124-139); VTK-style bounds stay as given.  A
    // device-bounded instance in the range, or in a group with a member in the range, comes back to the host: its
    // bounds from the mirror, read back first (RT_TRI_UPDATE_BOUNDS)
    const size_t ni = s->inst.size();
    std::vector<uint8_t> back(s->dev_bounded.empty() ? 0 : ni, 0);
    for (size_t g = 0; g < s->groups.size() && !back.empty(); g++) {
        const InstGroup &G = s->groups[g];
        if (!s->dev_bounded[ni + g]) continue;
        bool touched = false;
        for (uint32_t m : G.members) touched = touched || tri_range_overlaps(s->inst[m], first, count);
        if (!touched) continue;
        for (uint32_t m : G.members) back[m] = s->dev_bounded[m];
        s->dev_bounded[ni + g] = 0;
    }
    std::vector<uint32_t> changed;                     // group members whose centroid the host changed
    for (size_t i = 0; i < s->inst.size(); i++) {
        InstState &in = s->inst[i];
        const rt_instance_desc &id = s->inst_desc[i];
        const bool in_range = tri_range_overlaps(in, first, count);
        const bool take_back = !back.empty() && (back[i] || (s->dev_bounded[i] && in_range));
        if (!take_back && (!in_range || id.has_local_bounds)) continue;
        RT_TRY(refresh_tris_mirror(s));     // after a device update: raw_tris, this call's copy included, read back once
        host_bounds(s, in);
        instance_update(in, in.x);
        if (take_back) s->dev_bounded[i] = 0;
        if (s->gpu_tlas()) s->inst_dirty[i] = rt_scene::ALL_BLOCKS;     // the GPU copies of its local box
        if (s->group_of[i]) changed.push_back((uint32_t)i);
    }
    for (size_t g = 0; g < s->groups.size(); g++) {   // option "group" (LBVH): the union of the members' boxes
        InstGroup &G = s->groups[g];
        if (!s->dev_bounded.empty() && s->dev_bounded[ni + g]) continue;       // the device's, untouched by this range
        double c[3] = {0, 0, 0};
        for (size_t k = 0; k < G.members.size(); k++) {
            const InstState &m = s->inst[G.members[k]];
            G.st.box = k ? hm::Box::merge(G.st.box, m.box) : m.box;
            for (int a = 0; a < 3; a++) c[a] += m.centroid[a];
        }
        G.st.centroid = hm::v3((float)(c[0] / G.members.size()), (float)(c[1] / G.members.size()), (float)(c[2] / G.members.size()));
        if (s->gpu_tlas()) s->inst_dirty[s->inst.size() + g] = rt_scene::ALL_BLOCKS;
    }
    RT_TRY(refresh_dev_centroids(s, changed));
    s->blas_dirty = true;
    return RT_OK;
}

rt_status rt_scene_update_triangles_device(rt_scene *s, const rt_triangle_update *u) {
    if (!s || !u) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (u->reserved != 0 || (u->flags & ~(uint32_t)(RT_TRI_UPDATE_NO_SYNC | RT_TRI_UPDATE_BOUNDS)))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_update_triangles_device: reserved bits set");
    if (u->count && !u->vertices_device) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    RT_TRY(tri_update_check(s, u->first, u->count));
    if (u->count == 0) return RT_OK;
    DeviceRestore restore;
    HIP_TRY(hipSetDevice(s->device));
    if (!device_accessible(u->vertices_device, s->device) || (u->normals_device && !device_accessible(u->normals_device, s->device)))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_update_triangles_device: a buffer is not accessible from the scene's device");
    const bool bounds = (u->flags & RT_TRI_UPDATE_BOUNDS) != 0;
    // instance bounds derived from the triangles (rt_scene_update_triangles recomputes them on the host) cannot
    // follow vertices the host never sees, unless the device derives them (RT_TRI_UPDATE_BOUNDS)
    for (size_t i = 0; i < s->inst.size() && !bounds; i++) {
        const InstState &in = s->inst[i];
        if (in.ptype != RT_PRIM_TRIANGLE || s->inst_desc[i].has_local_bounds) continue;
        if ((uint64_t)in.pindex + in.pcount <= u->first || in.pindex >= u->first + u->count) continue;
        return fail(RT_ERR_UNSUPPORTED, "rt_scene_update_triangles_device: instance " + std::to_string(i) +
                                            " derives its bounds from triangles in the range (has_local_bounds == 0)");
    }
    // a device-bounded instance's box is its BLAS's root: the BLAS must hold exactly the instance's triangles (instances
    // with one first primitive share a BLAS whatever their counts)
    for (size_t i = 0; i < s->inst.size() && bounds; i++) {
        const InstState &in = s->inst[i];
        if (!tri_range_overlaps(in, u->first, u->count) || s->lbvh_segs[in.blas].count == in.pcount) continue;
        return fail(RT_ERR_UNSUPPORTED, "rt_scene_update_triangles_device: instance " + std::to_string(i) +
                                            " shares the BLAS of an instance with another primitive count");
    }
    if (!s->ev_tri_update) HIP_TRY(hipEventCreateWithFlags(&s->ev_tri_update, hipEventDisableTiming));
    // scene stream after the caller's (the buffers' producer), the kernel where the host path's copy sits, the
    // caller's stream after the kernel (the buffers are free again in its order)
    hipStream_t from = static_cast<hipStream_t>(u->stream);
    if (from || hipStreamQuery(nullptr) == hipErrorNotReady) RT_TRY(order_after_stream(s, from, s->stream));
    RT_TRY(tri_update_waits(s));
    HIP_TRY(launch_tri_update(s->raw_tris.p, s->raw_verts.p, u->vertices_device, u->normals_device, u->first, u->count, s->stream));
    HIP_TRY(hipEventRecord(s->ev_tri_update, s->stream));
    HIP_TRY(hipStreamWaitEvent(from, s->ev_tri_update, 0));
    if (bounds) {
        // every triangle instance the range overlaps, and its group, is device-bounded from the next frame update on:
        // that update rebuilds the BLASes (their roots are the boxes) behind these kernels on the scene stream, and
        // every record chain waits for that build.  The centroid array is shared by all frame blocks, so the kernels
        // wait for the chains already enqueued; nothing here waits for a trace or for the device to drain
        const size_t ni = s->inst.size();
        for (size_t i = 0; i < ni; i++) {
            if (!tri_range_overlaps(s->inst[i], u->first, u->count)) continue;
            if (!s->dev_bounded[i]) { s->dev_bounded[i] = 1; s->inst_dirty[i] = rt_scene::ALL_BLOCKS; }
            if (!s->group_of[i]) continue;
            const size_t gr = ni + s->group_of[i] - 1;             // its group's record
            if (!s->dev_bounded[gr]) { s->dev_bounded[gr] = 1; s->inst_dirty[gr] = rt_scene::ALL_BLOCKS; }
        }
        RT_TRY(wait_record_chains(s, s->stream));
        const InstBoundsGPU ib{s->ib_table.p, s->ib_chunk_inst.p, s->ib_multi.p, s->ib_groups.p, s->ib_members.p,
                               (uint32_t)s->ib_chunk_inst.n, (uint32_t)s->ib_multi.n, (uint32_t)s->ib_groups.n, (uint32_t)ni,
                               s->ib_partials.p, s->ib_cent.p};
        HIP_TRY(launch_inst_bounds(ib, s->raw_verts.p, u->first, u->count, s->stream));
    }
    s->tris_host_stale = true;
    s->blas_dirty = true;
    if (u->flags & RT_TRI_UPDATE_NO_SYNC) return RT_OK;
    return wait_event(s, s->ev_tri_update);
}

rt_status rt_scene_update_instances(rt_scene *s, size_t first, size_t count, const rt_instance_desc *d) {
    if (!s || (count && !d)) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!s->built) return fail(RT_ERR_STATE, "rt_scene_build has not been called");
    if (first > s->inst.size() || count > s->inst.size() - first) return fail(RT_ERR_INVALID_ARGUMENT, "instance range out of bounds");
    for (size_t k = 0; k < count; k++) {
        const rt_instance_desc &o = s->inst_desc[first + k], &n = d[k];
        if (o.primitive_type != n.primitive_type || o.primitive_index != n.primitive_index ||
            o.primitive_count != n.primitive_count)
            return fail(RT_ERR_INVALID_ARGUMENT, "an instance update may not change its primitives (type / index / count)");
    }
    for (size_t k = 0; k < count; k++) {
        const size_t i = first + k;
        s->inst_desc[i] = d[k];
        InstState &in = s->inst[i];
        if (d[k].has_local_bounds) {                                          // VTKReader.cu:204-209
            in.box = hm::Box::from_ranges({d[k].local_bounds[0], d[k].local_bounds[1]}, {d[k].local_bounds[2], d[k].local_bounds[3]},
                                          {d[k].local_bounds[4], d[k].local_bounds[5]});
            in.centroid = hm::of(d[k].local_centroid);
        } else if (!s->dev_bounded.empty() && s->dev_bounded[i]) {            // back from the device: the mirror, read back
            RT_TRY(refresh_tris_mirror(s));
            host_bounds(s, in);
        }
        if (!s->dev_bounded.empty()) s->dev_bounded[i] = 0;                   // RT_TRI_UPDATE_BOUNDS ends here
        instance_update(in, d[k].xform);
        if (s->gpu_tlas()) s->inst_dirty[i] = rt_scene::ALL_BLOCKS;
        // option "group": the group's box and transform were taken at the build; its members go back to
        // their own TLAS items for good
        if (s->group_of[i]) s->groups[s->group_of[i] - 1].valid = false;
    }
    return RT_OK;
}

}  // extern "C"
