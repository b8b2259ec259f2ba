// debug.cpp — introspection: the debug read-backs (rt_scene_debug_read) and the tree exports the tests compare
// with the oracle's trees.
#include "scene.hpp"

namespace {

void export_tree(const Tree &t, float *boxes, uint32_t *ci) {
    for (size_t i = 0; i < t.nodes.size(); i++) {
        if (boxes) t.nodes[i].box.store(boxes + 6 * i);
        if (ci) { ci[2 * i] = t.nodes[i].count; ci[2 * i + 1] = t.nodes[i].index; }
    }
}

// Reference node form (BLASNode/TLASNode arrays, children adjacent, DFS leaf order) of a tree held in
// the node-pair layout: used to export GPU-built trees.
Tree tree_from_pairs(const TreeRoot &root, const std::vector<NodePair> &pairs, uint32_t slot_base,
                     const std::vector<uint32_t> &item_of_slot) {
    Tree t;
    if (root.ref == 0xFFFFFFFFu) return t;
    auto box_of = [](const float *b) { return hm::Box{{{b[0], b[1]}, {b[2], b[3]}, {b[4], b[5]}}}; };
    struct Work { uint32_t ref; hm::Box box; uint32_t node; };
    std::vector<Work> todo{{root.ref, box_of(root.box), 0u}};
    t.nodes.push_back(TreeNode{});
    while (!todo.empty()) {
        const Work w = todo.back();
        todo.pop_back();
        t.nodes[w.node].box = w.box;
        if (w.ref & REF_LEAF) {
            const uint32_t start = ref_leaf_start(w.ref) - slot_base, cnt = ref_leaf_count(w.ref);
            t.nodes[w.node].count = cnt;
            t.nodes[w.node].index = (uint32_t)t.refs.size();
            for (uint32_t k = 0; k < cnt; k++) t.refs.push_back(item_of_slot[start + k]);
            continue;
        }
        const NodePair &P = pairs[w.ref & REF_INDEX_MASK];
        const uint32_t left = (uint32_t)t.nodes.size();
        t.nodes.resize(left + 2);
        t.nodes[w.node].count = 0;
        t.nodes[w.node].index = left;
        todo.push_back({P.ref1, box_of(P.c1), left + 1});
        todo.push_back({P.ref0, box_of(P.c0), left});
    }
    return t;
}

// Node pairs the last GPU BLAS build wrote.  rt_scene::blas_pair_count is read back once, at rt_scene_build; a rebuild
// after rt_scene_update_triangles keeps another number of interior nodes, and a reader that copied the older count
// would miss pairs the roots refer to.  Host-built BLASes (a GPU TLAS over SAH trees) keep their one count.
rt_status gpu_blas_pairs(const rt_scene *s, size_t &count) {
    count = s->blas_pair_count;
    if (s->build_mode != RT_BUILD_LBVH || !s->blas_builder) return RT_OK;
    uint32_t n = 0;
    HIP_TRY(hipMemcpy(&n, s->gpu_counts.p, sizeof n, hipMemcpyDeviceToHost));
    count = std::min<size_t>(n, s->cur.pairs.n);
    return RT_OK;
}

}  // namespace

extern "C" {

rt_status rt_scene_debug_read(rt_scene *s, const char *name, void *dst, size_t capacity, size_t *bytes) {
    if (!s || !name || !bytes || (!dst && capacity)) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    *bytes = 0;
    const std::string k(name);
    const void *src = nullptr;
    size_t size = 0;
    if (k == "rebuild_stages") {
        // option "timeline" and RT_BUILD_LBVH: the last BLAS build's items, interior nodes, node pairs written, items
        // in large trees (> 2048 items), large trees, then the duration in ms of each LbvhBuilder stage
        // (LbvhBuilder::STAGE_NAMES), as float64 (waits for the build)
        if (!s->blas_builder) return fail(RT_ERR_STATE, "no GPU BLAS build (RT_BUILD_LBVH)");
        constexpr int NS = LbvhBuilder::STAGES;
        *bytes = (5 + NS) * sizeof(double);
        if (!capacity) return RT_OK;
        if (capacity < *bytes) return fail(RT_ERR_INVALID_ARGUMENT, "buffer too small");
        HIP_TRY(hipSetDevice(s->device));
        float ms[NS];
        const hipError_t e = s->blas_builder->stage_ms(ms);
        if (e != hipSuccess) return fail(RT_ERR_STATE, "no timed BLAS build: set option \"timeline\" before the frame");
        uint32_t pairs = 0;
        HIP_TRY(hipMemcpy(&pairs, s->gpu_counts.p, sizeof pairs, hipMemcpyDeviceToHost));
        double v[5 + NS];
        v[0] = s->blas_builder->items();
        v[1] = s->blas_builder->max_pairs();
        v[2] = pairs;
        v[3] = s->blas_builder->large_items();
        v[4] = s->blas_builder->large_trees();
        for (int j = 0; j < NS; j++) v[5 + j] = ms[j];
        std::memcpy(dst, v, sizeof v);
        return RT_OK;
    }
    if (k == "timeline") {
        src = s->timeline.p;
        size = (size_t)s->timeline_waves * TIMELINE_WORDS * sizeof(uint64_t);
    } else if (k == "costmap") {
        src = s->costmap.p;
        size = s->costmap_pixels * sizeof(uint32_t);
    } else if (k == "launch_times") {
        // the trace launches not yet collected (rt_scene_collect), oldest first: (start, stop) in ms relative to
        // the first one's start, as float pairs — how lanes' launches interleave (scripts/lane_timeline.py)
        HIP_TRY(hipSetDevice(s->device));
        RT_TRY(drain(s));
        const uint32_t n = s->ring_pending;
        *bytes = (size_t)n * 2 * sizeof(float);
        if (capacity) {
            if (capacity < *bytes) return fail(RT_ERR_INVALID_ARGUMENT, "buffer too small");
            float *o = static_cast<float *>(dst);
            const uint32_t first = (s->ring_head + rt_scene::RING - n) % rt_scene::RING;
            for (uint32_t j = 0; j < n; j++) {
                const uint32_t slot = (first + j) % rt_scene::RING;
                HIP_TRY(hipEventElapsedTime(&o[2 * j], s->ring_start[first], s->ring_start[slot]));
                HIP_TRY(hipEventElapsedTime(&o[2 * j + 1], s->ring_start[first], s->ring_stop[slot]));
            }
        }
        return RT_OK;
    } else if (k == "instances") {
        // GPU-built frames: the instance records the GPU computed for the current frame, in instance order,
        // 45 floats each: inverse, forward, inverse-transpose rows 1-3 (12 each), transformed box, centroid
        if (!s->built || !s->gpu_tlas()) return fail(RT_ERR_UNSUPPORTED, "instance records are computed on the GPU for RT_BUILD_LBVH only");
        HIP_TRY(hipSetDevice(s->device));
        RT_TRY(drain(s));
        const size_t n = s->inst.size();
        *bytes = n * 45 * sizeof(float);
        if (capacity) {
            const uint8_t *fd = s->blk[s->active].dev;
            std::vector<InstHot> hot;
            std::vector<InstCold> cold;
            std::vector<float> tbox, tcent;
            HIP_TRY(read_back(hot, reinterpret_cast<const InstHot *>(fd + s->off_hot), n));
            HIP_TRY(read_back(cold, reinterpret_cast<const InstCold *>(fd + s->off_cold), n));
            HIP_TRY(read_back(tbox, reinterpret_cast<const float *>(fd + s->off_tbox), 6 * n));
            HIP_TRY(read_back(tcent, reinterpret_cast<const float *>(fd + s->off_tcent), 4 * n));
            std::vector<float> outv(n * 45);
            for (size_t i = 0; i < n; i++) {
                float *o = outv.data() + 45 * i;
                std::memcpy(o, hot[i].inv, 12 * sizeof(float));
                std::memcpy(o + 12, cold[i].fwd, 12 * sizeof(float));
                std::memcpy(o + 24, cold[i].nrm, 12 * sizeof(float));
                std::memcpy(o + 36, tbox.data() + 6 * i, 6 * sizeof(float));
                std::memcpy(o + 42, tcent.data() + 4 * i, 3 * sizeof(float));
            }
            std::memcpy(dst, outv.data(), std::min(capacity, *bytes));
        }
        return RT_OK;
    } else if (k == "blas_pairs" || k == "blas_quads" || k == "blas_roots") {
        // RT_BUILD_LBVH: the forest as built on the GPU (NodePair / NodeQuad / TreeRoot records, layout.hpp)
        if (!s->built || !s->gpu_tlas()) return fail(RT_ERR_UNSUPPORTED, "raw BLAS records are exported for RT_BUILD_LBVH only");
        HIP_TRY(hipSetDevice(s->device));
        RT_TRY(drain(s));
        const void *from = k == "blas_pairs" ? (const void *)s->cur.pairs.p
                                             : (k == "blas_quads" ? (const void *)s->cur.quads.p : (const void *)s->cur.roots.p);
        size_t pair_count = 0;
        RT_TRY(gpu_blas_pairs(s, pair_count));
        *bytes = k == "blas_roots" ? s->cur.roots.n * sizeof(TreeRoot)
                                   : pair_count * (k == "blas_pairs" ? sizeof(NodePair) : sizeof(NodeQuad));
        if (capacity && *bytes) HIP_TRY(hipMemcpy(dst, from, std::min(capacity, *bytes), hipMemcpyDeviceToHost));
        return RT_OK;
    } else if (k == "leaf_prims") {
        // caller triangle index of every leaf-ordered triangle slot (TriCold::orig_index): BLAS b owns
        // the slots [slot_base, slot_base + count) of its primitives, in leaf order
        HIP_TRY(hipSetDevice(s->device));
        RT_TRY(drain(s));
        const bool raw = s->raw_shading();             // the index rides in TriHot::pad0 (option "cold_records" 0)
        const size_t n = s->cur.tri_hot.n;
        *bytes = n * sizeof(uint32_t);
        if (capacity && n) {
            const size_t m = std::min(capacity / sizeof(uint32_t), n);
            const uint8_t *src0 = raw ? reinterpret_cast<const uint8_t *>(s->cur.tri_hot.p) + offsetof(TriHot, pad0)
                                      : reinterpret_cast<const uint8_t *>(s->cur.tri_cold.p) + offsetof(TriCold, orig_index);
            HIP_TRY(hipMemcpy2D(dst, sizeof(uint32_t), src0, raw ? sizeof(TriHot) : sizeof(TriCold), sizeof(uint32_t), m,
                                hipMemcpyDeviceToHost));
        }
        return RT_OK;
    } else if (k == "unit_cost" || k == "unit_order") {
        const Lane &l = s->ln[s->last_lane];
        const size_t units = l.sig[0];
        src = k == "unit_cost" ? l.unit_cost.p + units : l.unit_order.p;
        size = l.valid ? units * (k == "unit_cost" ? 1 : 4) * sizeof(uint32_t) : 0;
    } else {
        return fail(RT_ERR_INVALID_ARGUMENT, "unknown debug buffer " + k);
    }
    if (!src || size == 0) return fail(RT_ERR_STATE, "debug buffer " + k + " not recorded (set the option first)");
    HIP_TRY(hipSetDevice(s->device));
    RT_TRY(drain(s));
    if (capacity) HIP_TRY(hipMemcpy(dst, src, capacity < size ? capacity : size, hipMemcpyDeviceToHost));
    *bytes = size;
    return RT_OK;
}

rt_status rt_scene_export_blas(const rt_scene *s, uint32_t b, float *boxes, uint32_t *ci, uint32_t *refs,
                               uint32_t *n_nodes, uint32_t *n_prims) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "null scene");
    if (!s->built || b >= s->blas.size()) return fail(RT_ERR_INVALID_ARGUMENT, "no such BLAS");
    Tree gpu_tree;
    if (s->build_mode == RT_BUILD_LBVH) {
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipStreamSynchronize(s->stream));
        std::vector<NodePair> pairs;
        std::vector<TreeRoot> roots;
        if (s->seg_of_blas[b] == 0xFFFFFFFFu)
            return fail(RT_ERR_STATE, "this BLAS is not built: its instance group is one BLAS (option \"group\")");
        size_t pair_count = 0;
        RT_TRY(gpu_blas_pairs(s, pair_count));
        HIP_TRY(read_back(pairs, s->cur.pairs.p, pair_count));
        HIP_TRY(read_back(roots, s->cur.roots.p, s->cur.roots.n));
        const uint32_t type = s->blas[b].type;
        std::vector<uint32_t> orig;
        if (type == RT_PRIM_TRIANGLE && s->raw_shading()) {
            std::vector<TriHot> h;
            HIP_TRY(read_back(h, s->cur.tri_hot.p, s->cur.tri_hot.n));
            for (const TriHot &x : h) {
                uint32_t v;
                std::memcpy(&v, &x.pad0, sizeof v);
                orig.push_back(v);
            }
        } else if (type == RT_PRIM_TRIANGLE) {
            std::vector<TriCold> c;
            HIP_TRY(read_back(c, s->cur.tri_cold.p, s->cur.tri_cold.n));
            for (const TriCold &x : c) orig.push_back(x.orig_index);
        } else {
            std::vector<PrimCold> c;
            HIP_TRY(read_back(c, type == RT_PRIM_SPHERE ? s->cur.sph_cold.p : s->cur.quad_cold.p,
                              type == RT_PRIM_SPHERE ? s->cur.sph_cold.n : s->cur.quad_cold.n));
            for (const PrimCold &x : c) orig.push_back(x.orig_index);
        }
        gpu_tree = tree_from_pairs(roots[s->seg_of_blas[b]], pairs, 0, orig);
    }
    const Tree &t = s->build_mode == RT_BUILD_LBVH ? gpu_tree : s->blas[b].tree;
    if (n_nodes) *n_nodes = (uint32_t)t.nodes.size();
    if (n_prims) *n_prims = (uint32_t)t.refs.size();
    export_tree(t, boxes, ci);
    if (refs) std::memcpy(refs, t.refs.data(), t.refs.size() * sizeof(uint32_t));
    return RT_OK;
}

rt_status rt_scene_export_tlas(const rt_scene *s, float *boxes, uint32_t *ci, uint32_t *refs, uint32_t *n_nodes,
                               uint32_t *n_refs) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "null scene");
    if (!s->built) return fail(RT_ERR_STATE, "rt_scene_build has not been called");
    Tree gpu_tree;
    if (s->gpu_tlas()) {
        HIP_TRY(hipSetDevice(s->device));
        RT_TRY(wait_frame_block(const_cast<rt_scene *>(s)));   // the frame's TLAS may have been built on a lane stream
        const uint8_t *fd = s->blk[s->active].dev;
        TreeRoot root{};
        std::vector<NodePair> pairs;
        std::vector<uint32_t> slots;
        HIP_TRY(hipMemcpy(&root, fd + s->off_root, sizeof root, hipMemcpyDeviceToHost));
        const size_t nrec = s->inst.size() + s->groups.size();
        HIP_TRY(read_back(pairs, reinterpret_cast<const NodePair *>(fd + s->off_pairs), nrec));
        HIP_TRY(read_back(slots, reinterpret_cast<const uint32_t *>(fd + s->off_slots), nrec));
        gpu_tree = tree_from_pairs(root, pairs, 0, slots);
    }
    const Tree &t = s->gpu_tlas() ? gpu_tree : s->tlas;
    if (n_nodes) *n_nodes = (uint32_t)t.nodes.size();
    if (n_refs) *n_refs = (uint32_t)t.refs.size();
    export_tree(t, boxes, ci);
    if (refs) std::memcpy(refs, t.refs.data(), t.refs.size() * sizeof(uint32_t));
    return RT_OK;
}

}  // extern "C"
