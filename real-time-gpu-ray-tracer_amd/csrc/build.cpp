// build.cpp — rt_scene_build and its steps (instances, their BLASes, the option-"group" BLASes, the host-built BLASes'
// leaf-ordered primitive arrays, the materials, the frame blocks and per-lane resources), and the primitives' bounds
// and material slots as every builder and update reads them (blas_gpu.cpp: the GPU BLAS builds; update.cpp: the updates).
#include "scene.hpp"

namespace rtamd {

size_t prim_len(const rt_scene *s, uint32_t type) {
    return type == RT_PRIM_SPHERE ? s->spheres.size() : (type == RT_PRIM_PARALLELOGRAM ? s->quads.size() : s->tris.size());
}
hm::Box prim_box(const rt_scene *s, uint32_t type, uint32_t i) {
    return type == RT_PRIM_SPHERE ? hm::sphere_box(s->spheres[i])
                                  : (type == RT_PRIM_PARALLELOGRAM ? hm::quad_box(s->quads[i]) : hm::tri_box(s->tris[i]));
}
hm::V3 prim_centroid(const rt_scene *s, uint32_t type, uint32_t i) {
    return type == RT_PRIM_SPHERE ? hm::sphere_centroid(s->spheres[i])
                                  : (type == RT_PRIM_PARALLELOGRAM ? hm::quad_centroid(s->quads[i]) : hm::tri_centroid(s->tris[i]));
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

// ... as its description gives them (has_local_bounds; VTKReader.cu:204-209)
void bounds_from_desc(const rt_instance_desc &d, InstState &in) {
    in.box = hm::Box::from_ranges({d.local_bounds[0], d.local_bounds[1]}, {d.local_bounds[2], d.local_bounds[3]},
                                  {d.local_bounds[4], d.local_bounds[5]});
    in.centroid = hm::of(d.local_centroid);
}

// a group's local bounds from its members': their union box and mean centroid, in member order
void group_bounds(const rt_scene *s, InstGroup &G) {
    double c[3] = {0, 0, 0};
    for (size_t k = 0; k < G.members.size(); k++) {
        const InstState &m = s->inst[G.members[k]];
        G.st.box = k ? hm::Box::merge(G.st.box, m.box) : m.box;
        for (int a = 0; a < 3; a++) c[a] += m.centroid[a];
    }
    G.st.centroid = hm::v3((float)(c[0] / G.members.size()), (float)(c[1] / G.members.size()), (float)(c[2] / G.members.size()));
}

uint32_t material_slot(const rt_scene *s, uint32_t type, uint32_t index, bool &ok) {
    if (type == RT_MAT_ROUGH && index < s->roughs.size()) return index;
    if (type == RT_MAT_METAL && index < s->metals.size()) return (uint32_t)(s->roughs.size() + index) | MAT_METAL_BIT;
    ok = false;
    return 0;
}

rt_status check_materials(bool ok, const char *what) {
    return ok ? RT_OK : fail(RT_ERR_INVALID_ARGUMENT, std::string(what) + " references a material out of range");
}

}  // namespace rtamd

// rt_scene_build's steps, in the order it runs them
namespace {

// where the next BLAS goes in the scene's arrays: its node pairs, its quads, its leaf slots per primitive type
struct BlasCursor {
    uint32_t pair = 0, quad = 0, slot[3] = {0, 0, 0};
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
        } else if (id.has_local_bounds) {
            bounds_from_desc(id, in);
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
                    return fail_leaf_slots();
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
            BlasHost bh;
            bh.type = RT_PRIM_TRIANGLE;
            group_bounds(s, g);
            for (size_t k = 0; k < g.members.size(); k++) {
                const InstState &m = s->inst[g.members[k]];
                total += m.pcount;
                bh.members.push_back({m.pindex, m.pcount, g.members[k]});
                s->group_of[g.members[k]] = gi + 1;
            }
            if (mode != RT_BUILD_LBVH && (uint64_t)at.slot[RT_PRIM_TRIANGLE] + total >= MAX_LEAF_SLOTS)
                return fail_leaf_slots();
            g.st.ptype = RT_PRIM_TRIANGLE;
            g.st.pindex = 0;
            g.st.pcount = (uint32_t)total;
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
    std::vector<NodePair> pairs; std::vector<NodeQuad> quads;
    pairs.reserve(at.pair); quads.reserve(at.quad);
    std::vector<TriHot> th; std::vector<TriCold> tc;
    std::vector<SphereHot> sh; std::vector<PrimCold> sc;
    std::vector<QuadHot> qh; std::vector<PrimCold> qc;
    th.reserve(at.slot[RT_PRIM_TRIANGLE]); tc.reserve(at.slot[RT_PRIM_TRIANGLE]);
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
    RT_TRY(check_materials(mat_ok));
    s->blas_pair_count = pairs.size();

    RT_TRY(upload(s->cur.pairs, pairs));
    RT_TRY(upload(s->cur.quads, quads));
    RT_TRY(upload(s->cur.tri_hot, th));
    RT_TRY(upload(s->cur.tri_cold, tc));
    RT_TRY(upload(s->cur.sph_hot, sh));
    RT_TRY(upload(s->cur.sph_cold, sc));
    RT_TRY(upload(s->cur.quad_hot, qh));
    RT_TRY(upload(s->cur.quad_cold, qc));
    return RT_OK;
}

// the materials: four floats each (albedo, fuzz), the rough ones first (material_slot)
rt_status upload_materials(rt_scene *s) {
    std::vector<float> mats;
    for (const auto &r : s->roughs) { mats.push_back(r.albedo.x); mats.push_back(r.albedo.y); mats.push_back(r.albedo.z); mats.push_back(0.0f); }
    for (const auto &m : s->metals) { mats.push_back(m.albedo.x); mats.push_back(m.albedo.y); mats.push_back(m.albedo.z); mats.push_back(m.fuzz); }
    return upload(s->materials, mats);
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
        RT_TRY(upload(s->cur.roots, roots));
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
    for (Stage &st : s->stg) st.release();         // frame_update allocates
    s->stage_next = 0;
    for (FrameBlock &b : s->blk) HIP_TRY(b.alloc(s->frame_block));
    for (uint32_t i = 0; i < rt_scene::RING; i++) {
        if (!s->ring_start[i]) HIP_TRY(hipEventCreate(&s->ring_start[i]));
        if (!s->ring_stop[i]) HIP_TRY(hipEventCreate(&s->ring_stop[i]));
        if (!s->ring_post[i]) HIP_TRY(hipEventCreateWithFlags(&s->ring_post[i], hipEventDisableTiming));
    }
    if (!s->counters) {
        HIP_TRY(hipMalloc(&s->counters, rt_scene::NLANE * CNT_NUM * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(s->counters, 0, rt_scene::NLANE * CNT_NUM * sizeof(unsigned long long)));
    }
    for (Lane &l : s->ln) HIP_TRY(l.create());
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
    s->inst.clear(); s->blas.clear();
    s->groups.clear(); s->group_of.clear();
    s->max_blas_height = 0;
    for (FrameBlock &b : s->blk) b.by_slot = false;   // a rebuild may change the mode: no block is slot-ordered yet
    BlasCursor at;
    RT_TRY(build_instances(s, at));
    RT_TRY(build_groups(s, at));
    // the scene stream (uploads, GPU BLAS builds) at normal priority: the highest measured neutral (round 3)
    if (!s->stream) HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    s->forget_schedules();
    if (mode == RT_BUILD_LBVH) RT_TRY(gpu_setup_blas(s, at.slot));
    else RT_TRY(upload_host_blases(s, at));
    RT_TRY(upload_materials(s));
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

}  // extern "C"
