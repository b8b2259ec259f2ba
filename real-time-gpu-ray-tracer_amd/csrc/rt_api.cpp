// rt_api.cpp — the C ABI (include/rt.h): scene lifecycle, camera, options, statistics.
//
// Mirrors the reference's host orchestration (src/Global/Renderer.cu, RenderPin.cu,
// RenderGlob.cu) without windowing: commit geometry/materials, configure instances, build the
// acceleration structures, configure the camera, then per frame update instances, rebuild the
// TLAS on the host, upload it on a stream that is ordered against the previous frame's kernel
// through events (Renderer.cu:236-317), and launch the trace kernel.  Errors return rt_status
// with a thread-local message instead of exit() (Global.cu:34-41).
//
// Where the rest of the host side lives:
//   scene.hpp       struct rt_scene (RING, NLANE, every default with its measurement) and the internal interface
//   launch.hpp      the kernel launchers and the EXACT / FAST / fast_math table
//   scene_sync.cpp  ~rt_scene, drain and the other waits, order_after_null_stream
//   frame.cpp       frame_update (the host half of a frame), scene_gpu
//   build.cpp       rt_scene_build and its steps; the primitives' bounds and material slots
//   blas_gpu.cpp    the GPU BLAS builds of RT_BUILD_LBVH and their segments
//   update.cpp      rt_scene_update_triangles / _triangles_device / _instances, the device-bounds state
//   render.cpp      rt_render with auto_lanes and order_null, rt_assemble_tiles, rt_trace_rays, rt_query_rays, rt_query_camera,
//                   rt_box_test
//   filters.cpp     the calls that take no scene: rt_denoise (denoise.hip), rt_accumulate / _moments (accumulate.hip),
//                   rt_denoise_guided (guided.hip); select_device
//   scene_comm.cpp  the RCCL attach / detach / abort path and a frame's gather
//   debug.cpp       rt_scene_debug_read, rt_scene_export_blas / _tlas
#include "scene.hpp"

namespace {
thread_local std::string g_error;
}  // namespace

void rtamd_set_error(const std::string &msg) { g_error = msg; }   // error.hpp

namespace rtamd {

uint32_t tiles_for_rank(uint32_t w, uint32_t h, uint32_t tw, uint32_t th, uint32_t rank, uint32_t count) {
    if (tw == 0 || th == 0 || count == 0) return 0;
    const uint32_t total = ((w + tw - 1) / tw) * ((h + th - 1) / th);
    return rank < total ? (total - rank + count - 1) / count : 0;
}

void fill_stats(rt_stats *st, const unsigned long long *c) {
    std::memset(st, 0, sizeof *st);
    st->rays = c[CNT_RAYS];
    st->pixels = c[CNT_PIXELS];
    st->aabb_tests = 2ull * c[CNT_PAIRS];
    st->triangle_tests = c[CNT_TRI];
    st->sphere_quad_tests = c[CNT_SPHQUAD];
    st->quad_tests = c[CNT_QUAD];
    st->instance_visits = c[CNT_INST];
    st->hits = c[CNT_HITS];
}

// The camera rt_camera_set hands the kernels, from the caller's description: RendererImpl::calculateCameraProperties
// (src/Global/RenderPin.cu:73-95).  rt_camera_reprojection derives its rows from the same floats.
static void derive_camera(const rt_camera_input *c, uint32_t w, uint32_t h, CameraGPU &g) {
    using namespace hm;
    const V3 center = of(c->center), target = of(c->target), up = of(c->up);
    const float fd = distance(center, target);
    const float theta = c->fov * PI / 180.0f;
    const float vw = 2.0f * std::tan(theta / 2.0f) * fd;
    const float vh = vw / ((float)w * 1.0f / (float)h);
    const V3 W = unit(target - center);
    const V3 U = unit(cross(W, up));
    const V3 V = unit(cross(U, W));
    const V3 vx = U * vw, vy = V * vh;
    const V3 dx = vx / (float)w, dy = vy / (float)h;
    const V3 vorg = center + W * fd - vx * 0.5f - vy * 0.5f;
    const V3 po = vorg + dx * 0.5f + dy * 0.5f;
    for (int a = 0; a < 3; a++) {
        g.pixel_origin[a] = po[a]; g.dx[a] = dx[a]; g.dy[a] = dy[a]; g.center[a] = center[a];
        g.cu[a] = U[a]; g.cv[a] = V[a]; g.background[a] = of(c->background)[a];
    }
    g.focus_radius = c->focus_disk_radius;
    g.sqrt_s = (uint32_t)std::sqrt((double)c->sample_count);            // RenderPin.cu:93
    g.recip_sqrt = 1.0f / (float)g.sqrt_s;                              // RenderPin.cu:94
    g.depth = c->ray_trace_depth;
    g.width = w; g.height = h;
    g.pitch = (w + 15u) / 16u * 16u;                                    // 16x16 blocks (SDL_OpenGLWindow.cu:119-122)
}

}  // namespace rtamd

extern "C" {

uint32_t rt_abi_version(void) { return RT_ABI_VERSION; }

const char *rt_last_error(void) { return g_error.c_str(); }

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

rt_status rt_scene_create(const rt_scene_desc *d, int device, rt_scene **out) {
    if (!d || !out) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (d->instance_count == 0) return fail(RT_ERR_INVALID_ARGUMENT, "scene has no instances");
    if ((d->sphere_count && !d->spheres) || (d->parallelogram_count && !d->parallelograms) ||
        (d->triangle_count && !d->triangles) || (d->rough_count && !d->roughs) || (d->metal_count && !d->metals) ||
        !d->instances)
        return fail(RT_ERR_INVALID_ARGUMENT, "count without array");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RT_ERR_DEVICE, "no HIP device present");
    if (device < 0 || device >= ndev) return fail(RT_ERR_INVALID_ARGUMENT, "device index out of range");
    auto *s = new (std::nothrow) rt_scene();
    if (!s) return fail(RT_ERR_OUT_OF_MEMORY, "host allocation failed");
    s->device = device;
    s->spheres.assign(d->spheres, d->spheres + d->sphere_count);
    s->quads.assign(d->parallelograms, d->parallelograms + d->parallelogram_count);
    s->tris.assign(d->triangles, d->triangles + d->triangle_count);
    s->roughs.assign(d->roughs, d->roughs + d->rough_count);
    s->metals.assign(d->metals, d->metals + d->metal_count);
    s->inst_desc.assign(d->instances, d->instances + d->instance_count);
    s->update = d->update;
    s->update_user = d->update_user;
    // validate instance map (RenderPin.cu:119-172 would read out of bounds instead)
    for (const auto &id : s->inst_desc) {
        if (id.primitive_type > RT_PRIM_TRIANGLE) { delete s; return fail(RT_ERR_INVALID_ARGUMENT, "bad primitive type"); }
        const size_t len = prim_len(s, id.primitive_type);
        const size_t cnt = id.primitive_count ? id.primitive_count : 1;
        if ((size_t)id.primitive_index + cnt > len) { delete s; return fail(RT_ERR_INVALID_ARGUMENT, "instance primitive range out of bounds"); }
    }
    *out = s;
    return RT_OK;
}

rt_status rt_camera_set(rt_scene *s, const rt_camera_input *c, uint32_t w, uint32_t h) {
    if (!s || !c) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (w == 0 || h == 0 || w > 32768 || h > 32768) return fail(RT_ERR_INVALID_ARGUMENT, "bad framebuffer size");
    if (c->sample_count == 0) return fail(RT_ERR_INVALID_ARGUMENT, "sample_count must be >= 1");
    derive_camera(c, w, h, s->cam);
    s->width = w; s->height = h;
    s->cam_ok = true;
    return RT_OK;
}

rt_status rt_camera_reprojection(const rt_camera_input *c, uint32_t w, uint32_t h, rt_reprojection *out) {
    if (!c || !out) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (w == 0 || h == 0 || w > 32768 || h > 32768) return fail(RT_ERR_INVALID_ARGUMENT, "bad framebuffer size");
    CameraGPU g{};
    derive_camera(c, w, h, g);
    // x = center + s (p0 + fx dx + fy dy) solved for (fx, fy, 1 / s) by Cramer's rule, in double on the camera's floats
    double dx[3], dy[3], p0[3];
    for (int a = 0; a < 3; a++) { dx[a] = g.dx[a]; dy[a] = g.dy[a]; p0[a] = (double)g.pixel_origin[a] - (double)g.center[a]; }
    auto cross3 = [](const double *a, const double *b, double *r) {
        r[0] = a[1] * b[2] - a[2] * b[1]; r[1] = a[2] * b[0] - a[0] * b[2]; r[2] = a[0] * b[1] - a[1] * b[0];
    };
    double rx[3], ry[3], rw[3];
    cross3(dy, p0, rx);
    cross3(p0, dx, ry);
    cross3(dx, dy, rw);
    const double det = dx[0] * rx[0] + dx[1] * rx[1] + dx[2] * rx[2];
    rt_reprojection r;
    bool finite = true;
    for (int a = 0; a < 3; a++) {
        r.centre[a] = g.center[a];
        r.rx[a] = (float)(rx[a] / det); r.ry[a] = (float)(ry[a] / det); r.rw[a] = (float)(rw[a] / det);
        finite = finite && std::isfinite(r.centre[a]) && std::isfinite(r.rx[a]) && std::isfinite(r.ry[a]) && std::isfinite(r.rw[a]);
    }
    if (!finite) return fail(RT_ERR_INVALID_ARGUMENT, "rt_camera_reprojection: the camera is degenerate (non-finite rows)");
    *out = r;
    return RT_OK;
}

rt_status rt_scene_update(rt_scene *s, uint64_t frame) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "null scene");
    if (!s->built) return fail(RT_ERR_STATE, "rt_scene_build has not been called");
    HIP_TRY(hipSetDevice(s->device));
    return frame_update(s, frame, s->stream);
}

uint32_t rt_tiles_for_rank(const rt_scene *s, uint32_t tw, uint32_t th, uint32_t rank, uint32_t count) {
    if (!s || !s->cam_ok) return 0;
    return tiles_for_rank(s->width, s->height, tw, th, rank, count);
}

uint32_t rt_slab_tiles(uint32_t w, uint32_t h, uint32_t tw, uint32_t th, uint32_t count) {
    if (w == 0 || h == 0 || tw == 0 || th == 0 || count == 0) return 0;
    return slab_tile_count(w, h, tw, th, count);
}

rt_status rt_tile_pixels(uint32_t w, uint32_t h, uint32_t tw, uint32_t th, uint32_t rank, uint32_t count, uint64_t first,
                         uint64_t n, int32_t *xy) {
    if ((n && !xy) || w == 0 || h == 0 || tw == 0 || th == 0 || count == 0 || rank >= count)
        return fail(RT_ERR_INVALID_ARGUMENT, "bad tile geometry");
    for (uint64_t i = 0; i < n; i++) {
        uint32_t x = 0, y = 0;
        const bool in = tile_pixel(w, h, tw, th, rank, count, first + i, x, y);
        xy[2 * i] = in ? (int32_t)x : -1;
        xy[2 * i + 1] = in ? (int32_t)y : -1;
    }
    return RT_OK;
}

// The caller-facing options (include/rt.h, 19 keys).  Round 6 removed the tuning switches whose only use was an A/B
// study (their measured defaults are fixed now: refill threshold, leaf_early, queue bands, claim size, supertile walk,
// merge / split claim items, reorder period, reserved slots, LDS scene levels, instance-record order, leaf sizes) and
// the measured-negative or neutral ones with their code (variant, nt_store, cost_max, tlas_classes, wide_merge,
// scene_priority): DESIGN.md §4 keeps their measurements.
rt_status rt_scene_set_option(rt_scene *s, const char *key, int64_t value) {
    if (!s || !key) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    const std::string k(key);
    const auto boolean = [&](const char *name) -> rt_status {
        if (value != 0 && value != 1) return fail(RT_ERR_INVALID_ARGUMENT, std::string(name) + " must be 0 or 1");
        return RT_OK;
    };
    if (k == "kernel") {
        RT_TRY(boolean("kernel"));
        s->use_persistent = value == 1;
    } else if (k == "fast_math") {
        RT_TRY(boolean("fast_math"));
        s->fast_math = value == 1;
    } else if (k == "stage_depth") {
        // pinned staging buffers the host cycles through: it stages frame k once frame k - depth's trace is done
        if (value < 2 || value > rt_scene::NSTAGE) return fail(RT_ERR_INVALID_ARGUMENT, "stage_depth must be in 2..64");
        RT_TRY(drain(s));
        s->stage_depth = (int)value;
        s->stage_next = 0;
        s->stage_depth_set = true;
    } else if (k == "rebuild") {
        RT_TRY(boolean("rebuild"));
        if (value == 1 && s->built && s->build_mode != RT_BUILD_LBVH)
            return fail(RT_ERR_UNSUPPORTED, "per-frame BLAS rebuild needs RT_BUILD_LBVH");
        s->rebuild_blas = value == 1;
    } else if (k == "timeline") {
        RT_TRY(boolean("timeline"));
        s->timeline_on = value == 1;
    } else if (k == "costmap") {
        RT_TRY(boolean("costmap"));
        s->costmap_on = value == 1;
    } else if (k == "cold_records") {
        if (value < -1 || value > 1) return fail(RT_ERR_INVALID_ARGUMENT, "cold_records must be -1, 0 or 1");
        if (s->built) return fail(RT_ERR_STATE, "cold_records must be set before rt_scene_build");
        s->cold_records = (int)value;
    } else if (k == "blas_sets") {
        if (value < 2 || value > (int64_t)rt_scene::MAX_BLAS_SETS)
            return fail(RT_ERR_INVALID_ARGUMENT, "blas_sets must be in 2..8");
        RT_TRY(drain(s));
        s->blas_sets = (uint32_t)value;
    } else if (k == "blas_double") {
        RT_TRY(boolean("blas_double"));
        s->blas_double = value == 1;
    } else if (k == "grid_pct") {
        if (value < 0 || value > 100) return fail(RT_ERR_INVALID_ARGUMENT, "grid_pct must be in 0..100 (0 = auto)");
        s->grid_pct = (uint32_t)value;
    } else if (k == "wide") {
        RT_TRY(boolean("wide"));
        s->wide = value == 1;
    } else if (k == "exact_decisions") {
        RT_TRY(boolean("exact_decisions"));
        s->exact_decisions = value == 1;
    } else if (k == "tlas_small") {
        RT_TRY(boolean("tlas_small"));
        s->tlas_small = value == 1;
    } else if (k == "gpu_tlas") {
        RT_TRY(boolean("gpu_tlas"));
        if (s->built) return fail(RT_ERR_UNSUPPORTED, "gpu_tlas is set before rt_scene_build");
        s->gpu_tlas_sah = value == 1;
    } else if (k == "group") {
        RT_TRY(boolean("group"));
        s->group_inst = value == 1;                   // next rt_scene_build
    } else if (k == "lane_priority") {
        RT_TRY(boolean("lane_priority"));
        RT_TRY(drain(s));
        for (Lane &l : s->ln) {
            if (!l.st) continue;
            // nothing may keep a handle to a destroyed lane stream: drain() waits on last_stream, rt_render and
            // wait_record_chains compare each frame block's chain stream (FrameBlock::chain) with the frame's stream
            if (s->last_stream == l.st) s->last_stream = nullptr;
            for (FrameBlock &b : s->blk)
                if (b.chain == l.st) b.chain = nullptr;
            l.destroy_stream();                                         // recreated at the next frame
        }
        s->lane_priority = value == 1;
    } else if (k == "tlas_sah") {
        RT_TRY(boolean("tlas_sah"));
        s->tlas_sah = value == 1;                 // next frame's TLAS
    } else if (k == "overlap") {
        if (value < -1 || value > rt_scene::NLANE) return fail(RT_ERR_INVALID_ARGUMENT, "overlap must be -1 (auto) or 0..8 lanes");
        RT_TRY(drain(s));
        s->overlap_auto = value == -1;
        s->lanes = value < 1 ? (value == -1 ? 4u : 1u) : (uint32_t)value;      // auto: resolved per frame (auto_lanes)
        s->overlap = s->lanes > 1;
        s->lane = 0;
    } else if (k == "reorder") {
        RT_TRY(boolean("reorder"));
        if (s->reorder != (value == 1)) s->forget_schedules();
        s->reorder = value == 1;
    } else {
        return fail(RT_ERR_INVALID_ARGUMENT, "unknown option " + k);
    }
    return RT_OK;
}

rt_status rt_scene_collect(rt_scene *s, rt_stats *acc, float *kernel_ms, uint32_t capacity, uint32_t *count) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "null scene");
    if (!s->built) return fail(RT_ERR_STATE, "rt_scene_build has not been called");
    HIP_TRY(hipSetDevice(s->device));
    unsigned long long sum[CNT_NUM];
    RT_TRY(sum_lane_counters(s, sum));
    if (acc) fill_stats(acc, sum);
    // collected: the next KEEP_COUNTERS frames accumulate from zero (every block is clear and current)
    HIP_TRY(hipMemset(s->counters, 0, rt_scene::NLANE * CNT_NUM * sizeof(unsigned long long)));
    for (Lane &l : s->ln) l.epoch = s->cnt_epoch;
    const uint32_t n = s->ring_pending;
    uint32_t written = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t slot = (s->ring_head + rt_scene::RING - n + k) % rt_scene::RING;
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, s->ring_start[slot], s->ring_stop[slot]));
        if (kernel_ms && written < capacity) kernel_ms[written] = ms;
        written++;
    }
    if (count) *count = written < capacity ? written : capacity;
    s->ring_pending = 0;
    return RT_OK;
}

rt_status rt_synchronize(rt_scene *s) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "null scene");
    HIP_TRY(hipSetDevice(s->device));
    RT_TRY(drain(s));
    if (s->r_done) RT_TRY(wait_event(s, s->r_done));
    return RT_OK;
}

void rt_scene_destroy(rt_scene *s) { delete s; }

rt_status rt_scene_get_info(const rt_scene *s, rt_scene_info *info) {
    if (!s || !info) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    std::memset(info, 0, sizeof *info);
    info->blas_count = s->blas_own;     // per-instance BLASes (the groups' merged ones are not counted)
    info->overlap_lanes = s->lanes;
    info->stage_depth = (uint32_t)s->stage_depth;
    info->blas_node_pairs = s->blas_pair_count;
    info->blas_leaves = s->blas_leaf_count;
    info->tlas_node_pairs = s->tlas_flat.pairs.size();
    if (s->gpu_tlas() && s->built) {                 // GPU-built TLAS: read the last frame's count / root
        HIP_TRY(hipSetDevice(s->device));
        RT_TRY(wait_frame_block(const_cast<rt_scene *>(s)));   // the frame's TLAS may have been built on a lane stream
        uint32_t np = 0;
        TreeRoot root{};
        HIP_TRY(hipMemcpy(&np, s->gpu_counts.p + 2 + s->active, sizeof np, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&root, s->blk[s->active].dev + s->off_root, sizeof root, hipMemcpyDeviceToHost));
        info->tlas_node_pairs = np;
        info->tlas_height = root.height;
    }
    // the live set's roots have never been counted (the spares' are); nor inst_blas, gpu_counts, the ib_* tables
    info->device_bytes = s->cur.bytes() - s->cur.roots.bytes() +
                         s->materials.n * sizeof(float) + 2 * s->frame_block + s->out_rgba.n + s->out_rgb.n * sizeof(float) +
                         s->raw_tris.n * sizeof(rt_triangle) + s->raw_sph.n * sizeof(rt_sphere) +
                         s->raw_quad.n * sizeof(rt_parallelogram) + s->raw_verts.n * sizeof(float);
    for (const auto &sp : s->spare) info->device_bytes += sp.bytes();   // per-frame rebuilds ("blas_sets")
    if (s->blas_builder) info->device_bytes += s->blas_builder->workspace_bytes();   // incl. the staged TriHot records
    if (s->tlas_builder) info->device_bytes += s->tlas_builder->workspace_bytes();
    info->width = s->width; info->height = s->height;
    info->sqrt_sample_count = s->cam.sqrt_s;
    info->ray_trace_depth = s->cam.depth;
    if (!s->gpu_tlas()) info->tlas_height = s->tlas_flat.height;
    info->blas_height_max = s->max_blas_height;
    return RT_OK;
}

// updateInstance (src/Global/Main.cu:6-42)
void rt_demo_update(void *user, rt_xform *x, size_t n, uint64_t frame) {
    (void)user;
    const float ic[3] = {0.0f, 2.0f, 0.0f};
    const float radius = 2.0f, speed = 0.02f;
    const float angle = (float)frame * speed;
    const float c1[3] = {ic[0] + radius * std::cos(angle) * 1.5f, ic[1] + radius * std::sin(angle) * std::cos(angle),
                         ic[2] + radius * std::sin(angle) * 1.5f};
    const float c2[3] = {-c1[0], c1[1], -c1[2]};
    const float c3[3] = {-c1[0], c1[1] + 5.0f, c1[2]};
    const float rot = (float)frame * 0.4f;
    const rt_xform t[5] = {
        {{0.0f, -1000.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}},
        {{c1[0], c1[1], c1[2]}, {0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}},
        {{-5.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}},
        {{c2[0], c2[1], c2[2]}, {rot, rot, rot}, {3.0f, 3.0f, 3.0f}},
        {{c3[0], c3[1], c3[2]}, {0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}},
    };
    for (size_t i = 0; i < n && i < 5; i++) x[i] = t[i];
}

}  // extern "C"
