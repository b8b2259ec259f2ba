// scene.hpp — the scene's state (struct rt_scene) and the internal interface between the host files: the error and
// wait discipline (scene_sync.cpp), the host half of a frame (frame.cpp), the acceleration-structure builds (build.cpp,
// blas_gpu.cpp), the geometry updates (update.cpp), the RCCL path (scene_comm.cpp); render.cpp, debug.cpp and
// rt_api.cpp only call into them, and filters.cpp, whose calls take no scene, uses the error discipline alone.  What the scene keeps per overlap lane, per frame block and per staging buffer is
// declared once each (Lane, FrameBlock, Stage), with the members that create, reset and release it.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "../../include/rt.h"
#include "bvh_build.hpp"
#include "comm.hpp"
#include "devbuf.hpp"
#include "error.hpp"
#include "host_math.hpp"
#include "inst_bounds_map.hpp"
#include "layout.hpp"
#include "lbvh.hpp"

namespace rtamd {

inline rt_status fail(rt_status s, const std::string &msg) {
    rtamd_set_error(msg);
    return s;
}

#define RT_TRY(expr)                                                                               \
    do {                                                                                           \
        const rt_status st_ = (expr);                                                              \
        if (st_ != RT_OK) return st_;                                                              \
    } while (0)

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_DEVICE,          \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                       \
    } while (0)

constexpr uint32_t BLAS_LEAF_CAP = 4;   // BLAS.cuh:17
constexpr uint32_t TLAS_LEAF_CAP = 2;   // TLAS.cuh:22
constexpr uint32_t SAH_LEAF_CAP = 4;    // RT_BUILD_SAH: <= 4 items per leaf (2-bit count in a leaf ref)
constexpr uint32_t LBVH_BLAS_LEAF_CAP = 4;
// GPU TLAS leaves hold up to fixed setting "tlas_leaf" (an option until round 5) instances (default 1, as the SAH TLAS: a leaf's
// instances are entered without their own box test; 2 = the reference's TLAS leaf size, TLAS.cuh:22)

struct InstState {
    uint32_t ptype, pindex, pcount, blas;
    hm::Box box;
    hm::V3 centroid;
    hm::Mat fwd, inv, nrm;
    hm::Box tbox;
    hm::V3 tcentroid;
    rt_xform x;
};

struct BlasHost {
    uint32_t type;
    Tree tree;
    FlatTree flat;
    FlatWide wide;                 // quad form (option "wide"; host-built modes)
    uint32_t pair_base, slot_base;
    // a group's merged BLAS (option "group"): the members' triangle ranges {first, count, instance}
    std::vector<std::array<uint32_t, 3>> members;
};

// Option "group" (RT_BUILD_SAH, host-built TLAS): triangle instances whose transforms are bit-identical
// (the reference's VTK particles all carry one fixed transform, VTKReader.cu:204-215) share one instance
// space, so one SAH BLAS over all their triangles replaces their overlapping instance boxes in the TLAS.
// A frame uses the group while every member still has the group's transform (and its triangles and
// bounds were not replaced since the build); otherwise that frame's TLAS takes the members one by one.
struct InstGroup {
    InstState st;                  // the group as one instance: the shared transform, the union of the boxes
    std::vector<uint32_t> members;
    bool valid = true;
};

// Overlap lanes, and as many frame blocks: frame blocks cycle through NLANE buffers, so "overlap" lanes never wait on
// each other's block.  Round 6 measured 12 and 16 lanes: 1/8 shares equal or slower (C2 0.0384-0.0388 ms/frame at 8,
// 0.0394-0.0420 at 12, 0.0385-0.0392 at 16; C4 0.0465-0.0472 at 8, 0.0483-0.0499 at 16), the whole frame equal at 6
// and 8 (profiles/r06/lanes/)
constexpr int NLANE = 8;

// One overlap lane.  Option "overlap" = L lanes: consecutive frames cycle through L lanes (queue heads, unit costs,
// schedule), so frame k+1's persistent launch fills the CUs frame k's tail leaves idle when the caller cycles L
// streams; with L <= 1 every frame uses lane 0 and launches of one scene are serialised.  Launches of one lane never
// overlap, whatever streams callers pass.  The lane's block of the device counters is rt_scene::lane_counters(q).
struct Lane {
    // "overlap" frames rendered without a caller stream (opts.stream NULL) run on lane streams the scene owns, created
    // on first use (frame_stream, render.cpp)
    hipStream_t st = nullptr;
    // persistent megakernel: band heads, then (option "reorder") band item counts, one 128 B line each
    uint32_t *queue = nullptr;
    hipEvent_t r_done = nullptr;        // last trace launch of the lane finished (FrameBlock::r_used; null: none yet)
    uint64_t epoch = 0;                 // the counter epoch (rt_scene::cnt_epoch) the lane's counter block belongs to
    DevBuf<uint32_t> unit_cost, unit_order;   // option "reorder" (schedule.hip)
    uint32_t sig[7] = {};               // launch layout the recorded costs belong to
    uint32_t phase = 0;                 // fixed setting "reorder_period" (sched_phase.hpp)
    bool order_ok = false;              // unit_order holds an order for that layout
    bool valid = false;                 // sig and the costs are a launch's (not after a build or a change of "reorder")
    hipError_t create() {               // what survives a rebuild, created once
        if (queue) return hipSuccess;
        const hipError_t e = hipMalloc(&queue, QUEUE_WORDS * sizeof(uint32_t));
        return e == hipSuccess ? hipMemset(queue, 0, QUEUE_WORDS * sizeof(uint32_t)) : e;
    }
    void reset() { r_done = nullptr; }  // every launch was seen complete, or given up (abort_comm)
    void destroy_stream() { if (st) (void)hipStreamDestroy(st); st = nullptr; }   // recreated at the next frame
    void release() { unit_cost.release(); unit_order.release(); if (queue) (void)hipFree(queue); queue = nullptr; }
};

// One frame block: per-frame data in HBM (rt_scene::frame_block bytes, laid out by the off_* offsets).
// r_copied / r_used are what the waits use: the event last recorded for each purpose.  A trace launch records one
// event after it (its ring_stop timing event, or one event after a multi-GPU gather) and points every purpose
// it completes at that event (r_copied, r_used, Stage::r_staged, Lane::r_done, rt_scene::r_done) — each event record
// between two kernels of a stream costs ~5 us of GPU idle time (profiles/r02_gaps.txt), and a launch completed four
// purposes with four records.
struct FrameBlock {
    uint8_t *dev = nullptr;             // HBM
    hipEvent_t ev_copied = nullptr;     // frame block uploaded / built
    hipEvent_t ev_used = nullptr;       // last kernel reading dev finished
    hipEvent_t r_copied = nullptr, r_used = nullptr;   // never null once allocated (reset)
    hipStream_t chain = nullptr;        // a GPU-built frame's records / TLAS were built on this stream
    uint32_t items = 0;                 // TLAS items (= instance records when staged by slot)
    bool by_slot = false;               // staged in slot order
    hipError_t alloc(size_t bytes) {    // the block anew; the events are created once and survive a rebuild
        if (dev) { (void)hipFree(dev); dev = nullptr; }
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&dev), bytes);
        if (e == hipSuccess && !ev_copied) e = hipEventCreateWithFlags(&ev_copied, hipEventDisableTiming);
        if (e == hipSuccess && !ev_used) e = hipEventCreateWithFlags(&ev_used, hipEventDisableTiming);
        if (e == hipSuccess && !r_copied) r_copied = ev_copied;
        if (e == hipSuccess && !r_used) r_used = ev_used;
        return e;
    }
    void reset() { r_copied = ev_copied; r_used = ev_used; }   // the block's own events: no launch to wait for
    void release() {
        if (dev) (void)hipFree(dev);
        if (ev_copied) (void)hipEventDestroy(ev_copied);
        if (ev_used) (void)hipEventDestroy(ev_used);
    }
};

// One pinned host staging buffer of the per-frame upload, allocated on first use (frame_update).
struct Stage {
    uint8_t *host = nullptr;
    uint8_t *dev = nullptr;             // the same, as a device-visible pointer
    hipEvent_t r_staged = nullptr;      // host no longer read (null: never used, or drained)
    void reset() { r_staged = nullptr; }
    void release() { if (host) (void)hipHostFree(host); host = dev = nullptr; r_staged = nullptr; }
};

// rt_scene_attach_comm: this scene is rank `rank` of a `world`-rank frame.  One communicator
// per overlap lane at attach time (split from the first), so the lanes' gathers on different streams do not
// share one; lane q uses comm[q % ncomm] if "overlap" is raised after the attach (every rank issues the same
// lane sequence, so a shared communicator still sees its operations in one order on every rank).
struct CommState {
    static constexpr int NLANE = rtamd::NLANE;
    int rank = 0, world = 1;
    int ncomm = 1;
    uint32_t timeout_ms = 0;               // rt_comm_set_timeout: 0 = no deadline (async errors still polled)
    uint32_t tile_w = 64, tile_h = 64;
    ncclComm_t comm[NLANE] = {};
    size_t slab_bytes = 0;                 // one rank's slab (largest tile count), RGBA8
    DevBuf<uint8_t> slab[NLANE];           // ranks > 0: this rank's traced tiles
    DevBuf<uint8_t> gathered[NLANE];       // rank 0: world slabs; its own tiles are traced into slab 0
};

inline size_t align16(size_t x) { return (x + 15) & ~size_t(15); }

}  // namespace rtamd

using namespace rtamd;   // rt_scene is the C ABI's (global) type; this header is internal to the host files

struct rt_scene {
    int device = 0;
    // caller data (copied, Renderer.cu:31-39)
    std::vector<rt_sphere> spheres;
    std::vector<rt_parallelogram> quads;
    std::vector<rt_triangle> tris;
    std::vector<rt_rough> roughs;
    std::vector<rt_metal> metals;
    std::vector<rt_instance_desc> inst_desc;
    rt_update_fn update = nullptr;
    void *update_user = nullptr;

    std::vector<InstState> inst;
    std::vector<BlasHost> blas;
    size_t blas_own = 0;            // per-instance BLASes; the groups' merged BLASes follow them in `blas`
    std::vector<InstGroup> groups;  // option "group": TLAS item n + g is group g
    std::vector<uint32_t> group_of; // per instance: its group + 1 (0: none)
    bool group_inst = true;         // option "group" (set before the build)
    bool lds_blas = true;           // fixed setting "lds_blas" (an option until round 5): with "lds_scene" 2, a group BLAS's top levels in LDS
    static constexpr int NLANE = rtamd::NLANE;   // lanes, and frame blocks: one block per lane
    Tree tlas;
    FlatTree tlas_flat;
    FlatWide tlas_wide;
    uint64_t build_seed = 0;
    rt_build_mode build_mode = RT_BUILD_COMPAT_MEDIAN;
    bool built = false;
    uint64_t frame = 0;

    // HBM: static scene data.  A BLAS set: the node pairs, quads and roots of every BLAS and the leaf-ordered primitive
    // records, with each lane's last trace that read them (RT_BUILD_LBVH rebuilds, below).  Every DevBuf is named in
    // each_buf(), which release(), bytes() and alloc_like() walk.
    struct BlasSet {
        DevBuf<NodePair> pairs;
        DevBuf<NodeQuad> quads;         // option "wide"
        DevBuf<TreeRoot> roots;         // per segment the builder holds (seg_of_blas)
        DevBuf<TriHot> tri_hot; DevBuf<TriCold> tri_cold; DevBuf<SphereHot> sph_hot; DevBuf<PrimCold> sph_cold;
        DevBuf<QuadHot> quad_hot; DevBuf<PrimCold> quad_cold;
        hipEvent_t ev_lane[NLANE] = {};    // one per lane: its last trace of this set
        template <typename Self, typename F>
        static void each_buf(Self &b, F f) {
            f(b.pairs); f(b.quads); f(b.roots); f(b.tri_hot); f(b.tri_cold); f(b.sph_hot); f(b.sph_cold); f(b.quad_hot); f(b.quad_cold);
        }
        void release() { each_buf(*this, [](auto &b) { b.release(); }); }
        size_t bytes() const {
            size_t n = 0;
            each_buf(*this, [&](const auto &b) { n += b.bytes(); });
            return n;
        }
        // every buffer allocated anew for o's element counts (DevBuf::alloc: one element where o holds none, as a
        // released tri_cold)
        hipError_t alloc_like(const BlasSet &o) {
            std::vector<size_t> n;
            each_buf(o, [&](const auto &b) { n.push_back(b.n); });
            hipError_t e = hipSuccess;
            size_t k = 0;
            each_buf(*this, [&](auto &b) { if (e == hipSuccess) e = b.alloc(n[k++]); });
            return e;
        }
        // what a spare set is re-sized by: the counts a change of the segments or of the scene's primitives moves
        bool sized_as(const BlasSet &o) const {
            return pairs.n == o.pairs.n && tri_hot.n == o.tri_hot.n && sph_hot.n == o.sph_hot.n && quad_hot.n == o.quad_hot.n &&
                   roots.n == o.roots.n;
        }
    };
    BlasSet cur;                    // the set the traces read
    bool wide = true;               // FAST persistent kernel traverses the quad trees (host-built modes)
    bool exact_decisions = false;   // option "exact_decisions": GPU-built trees take the exact-decision traversal (mode 3)
    uint32_t lds_scene = 2;         // quad-tree kernel: 1 = TLAS quads (+ instance hot records) in LDS when they
                                    // fit, 2 = also sphere / parallelogram records and instance cold records
    // option "grid_pct": the persistent grid as a percentage of the resident capacity; 0 = auto: 50 when
    // another lane's launch is still in flight ("overlap"), so two lanes' launches are resident side by
    // side instead of the next one filling only the slots the previous one's tail frees (C2, 3 lanes:
    // 0.252 -> 0.229 ms/frame; a C2 1/8 share 0.115 -> 0.084; C3 1.64 -> 1.59,
    // profiles/r02_sweep_grid2.jsonl), else 100 (a frame alone on the GPU takes all of it)
    uint32_t grid_pct = 0;
    static constexpr uint64_t BIG_LAUNCH_PATHS = 16ull << 20;
    // option "cold_records" (RT_BUILD_LBVH, set before rt_scene_build; default 0): 1 = the BLAS builds write TriCold
    // records (normals, material, caller index) as the host builders do; 0 = they write TriHot only, with the caller's
    // triangle index and group member in its pads, and a hit reads normals and material from the caller's triangle
    // (SceneGPU::raw_tris) — a C5 rebuild's leaf-ordered gather then moves about half the bytes
    // -1 (auto, default): 1 when the BLASes are built once (option "rebuild" 0 at rt_scene_build: a hit's normals and
    // material are then one dependent HBM round trip nearer — C5 static 4.97 -> 4.80 ms/frame, C2-LBVH -1 %), 0 when
    // they are rebuilt every frame (the rebuild's gather moves half the bytes: C5 8.36 against 8.52;
    // profiles/r05/cold_records/)
    int cold_records = -1;
    bool cold_eff = false;          // the build's choice (rt_scene_build)
    bool raw_shading() const { return build_mode == RT_BUILD_LBVH && !cold_eff; }
    DevBuf<float> materials;
    uint64_t blas_pair_count = 0, blas_leaf_count = 0;

    // per-frame data, double-buffered:
    //   [tlas root | tlas pairs | tlas slots | inst hot | inst cold | tlas item boxes | tlas item centroids]
    // (the root and the item arrays are used by GPU-built TLASes only)
    size_t frame_block = 0, off_root = 0, off_pairs = 0, off_slots = 0, off_hot = 0, off_cold = 0, off_tbox = 0,
           off_tcent = 0, off_root_wide = 0, off_quads = 0, off_delta = 0, off_hot_s = 0, off_cold_s = 0;
    FrameBlock blk[NLANE];
    // GPU-built frames: per-instance parameters resident in HBM (instances.hip), one copy per frame block
    // (block b's at inst_params.p + b * records), so frames of different lanes update their records
    // concurrently; the host stages a delta (InstDelta at off_delta) only for the records whose transform
    // or local box changed since block b was last written: inst_dirty bit b (ALL_BLOCKS: every block)
    DevBuf<InstParams> inst_params;
    std::vector<uint16_t> inst_dirty;
    static constexpr uint16_t ALL_BLOCKS = 0xFFFF;
    static_assert(NLANE <= 16, "inst_dirty holds one bit per frame block");
    hipEvent_t ev_blas_built = nullptr;           // the last GPU BLAS build on the scene stream finished
    hipEvent_t ev_caller = nullptr;               // rt_render with device outputs and no stream: the null stream's
                                                  // work before the call (the trace writes the caller's buffers after it)
    uint64_t blas_build_seq = 0;                  // BLAS builds recorded on ev_blas_built so far
    uint64_t blas_build_done = 0;                 // ... of which the host has seen the last one complete
    // pinned host staging, cycled independently of the frame blocks and twice as deep: a frame's staging is
    // reusable once its upload ran, which rt_render can only tell by the trace's completion event (a record
    // right after the copy kernel would idle the GPU ~5 us) — with one staging per block, the host waited for
    // frame k-8's whole trace before it could stage frame k (8 lanes of 1/8-frame shares: 0.12 ms lane gaps)
    // option "stage_depth" (default 2 x NLANE): buffers in the cycle, allocated on first use
    static constexpr int NSTAGE = 64;
    int stage_depth = 16;
    Stage stg[NSTAGE];
    int stage_next = 0;
    int pending_copy = -1, pending_stage = -1;    // rt_render: block (and its staging) whose upload the next launch performs
    hipEvent_t r_done = nullptr;                  // last trace launch or query finished (as FrameBlock::r_used; null: none yet)
    int active = -1;                              // the frame block of the last frame update
    // rt_query_rays: NQUERY slots, taken in turn, of QUERY_PARTS work-queue heads (a 128 B line each) and one completion event.
    // A call's stream first waits on its slot's event — the query that used the slot NQUERY calls ago — so a head is
    // never shared by two queries in flight — and on the previous call's, so queries run in call order.  A frame launch
    // may replace r_used / r_done without having waited for a query on a caller stream, so everything that must see
    // every query — drain, the destructor, uploads into a frame block, BLAS rebuilds, rt_scene_update_triangles' copy
    // into raw_tris — waits on these events
    // themselves (wait_queries), not only on the r_* pointers a query sets.
    static constexpr uint32_t NQUERY = 8;
    uint32_t *query_heads = nullptr;              // NQUERY x QUERY_PARTS x QUEUE_STRIDE words, allocated with the first build
    hipEvent_t ev_query[NQUERY] = {};
    uint32_t query_next = 0;
    bool query_live = false;                      // a query was enqueued since every ev_query was last seen complete

    hipStream_t stream = nullptr;
    // per-frame kernel timing ring for pipelined frames (rt_scene_collect)
    static constexpr uint32_t RING = 256;
    hipEvent_t ring_start[RING] = {}, ring_stop[RING] = {};
    hipEvent_t ring_post[RING] = {};     // multi-GPU frames: the launch's completion event after its gather
    uint32_t ring_head = 0, ring_pending = 0;
    hipStream_t last_stream = nullptr;
    // persistent megakernel: work-queue head (Lane::queue), grid size (#CUs x resident blocks), refill threshold
    Lane ln[NLANE];
    bool overlap = false;           // option "overlap": more than one lane in use
    uint32_t blas_leaf = SAH_LEAF_CAP;   // fixed setting "blas_leaf" (an option until round 5): RT_BUILD_SAH BLAS leaf size (1..4), next rt_scene_build
    uint32_t tlas_leaf = 1;   // fixed setting "tlas_leaf" (an option until round 5): RT_BUILD_SAH per-frame SAH TLAS leaf size (1..4; 1 measured best)
    uint32_t tlas_median_leaf = 0;   // fixed setting "tlas_median_leaf" (an option until round 5): RT_BUILD_SAH median TLAS leaf size (0 = the reference's 2)
    bool tlas_sah = true;     // option "tlas_sah": RT_BUILD_SAH builds its per-frame TLAS with SAH (0: the median split)
    bool inst_by_slot = true;       // fixed setting "inst_by_slot" (an option until round 5): host-built TLAS stages instance records in slot order
    uint32_t lanes = 1;
    // fixed setting "reserve" (an option until round 5): with overlapped lanes the persistent grid leaves this many workgroup slots free (two
    // per XCD at 16), so the next lanes' schedule / upload kernels and GPU TLAS builds run beside a launch
    // that holds the rest of the GPU instead of waiting for its drain (C2, 3 lanes: 16 -> 0.260-0.261,
    // 8 -> 0.261-0.265, 0 -> 0.268-0.272 ms/frame; profiles/r02_sweep_lanes.jsonl)
    uint32_t reserve = 16;
    uint32_t lane = 0;              // lane of the next rt_render (overlap)
    int last_lane = 0;              // lane of the last rt_render
    // "overlap" frames rendered without a caller stream (opts.stream NULL) run on lane streams the scene owns
    // (Lane::st); with option "overlap" -1 (overlap_auto) the scene also picks the lane count and the staging depth
    // per frame kind (auto_lanes: the settings bench.py measured best), so a drop-in caller passes no
    // streams at all
    bool overlap_auto = false;
    // fixed setting "leaf_early" (an option until round 5) (OutputGPU::leaf_early): -1 = auto, 0 for paths of <= 2 segments (depth x samples; C2, C4),
    // else LEAF_EARLY_AUTO (C3 1.54 -> 1.25, C5 5.79 -> 4.97 ms/frame; C2 0.181 -> 0.185 with it,
    // profiles/r05/leaf_early/)
    int leaf_early = -1;
    static constexpr uint32_t LEAF_EARLY_AUTO = 12;
    // option "lane_priority": the scene's own lane streams at the device's highest priority (default 1): HIP gives them
    // hardware queues of their own, so 4 lanes run side by side at the default GPU_MAX_HW_QUEUES (4) — C2 0.256 ->
    // 0.180 ms/frame, C3 2.15 -> 1.54, a 1/8 share 0.064 -> 0.046 — as at 12 queues (profiles/r05/lanes/)
    bool lane_priority = true;
    bool stage_depth_set = false;   // option "stage_depth" given explicitly (auto lanes leave it alone)
    uint32_t cus = 0;
    // fixed setting "threshold" (an option until round 5) (lanes waiting before a wave leaves traversal to shade and refill); 0 = auto: 64 when
    // a pixel's path has at most two segments (depth x samples <= 2: the wave then shades and refills all its
    // lanes at once), else 40 (C2 0.194 -> 0.184 ms/frame, serialised 0.35 -> 0.33 ms; C3 at 64 would lose
    // 23 %, 40 ties 32; profiles/r02_sweep_thr2.jsonl)
    uint32_t threshold = 0;
    // option "fast_math": FAST frames with hardware reciprocal / rsq and FMA contraction instead of the reference's
    // correctly rounded arithmetic (C2 -7 %, C3 -9 % per pipelined frame; 0.008-0.09 % of pixels then differ from the
    // oracle even on its own trees); default 0: bit-identical to the oracle on the reference's trees
    bool fast_math = false;
    double update_wait_ms = 0.0;    // last frame_update: time blocked on ev_copied (GPU progress)
    bool use_persistent = true;
    uint32_t queue_parts = 8;       // one band per XCD (measured with "reorder": 8 beat 4, 2 and 1 on C2)
    uint32_t grab = 64;             // pixels per queue claim
    // fixed setting "merge" (an option until round 5): two adjacent units below this cost level share one claim item (128 pixels): 6 (sky, about
    // 4 steps per pixel) measured C2 0.203 -> 0.199 ms/frame; 8 or 10 (also the ground) put 128-pixel items at
    // the end of the order and lengthen the tail (profiles/r02_sweep_merge.jsonl)
    uint32_t merge = 6;
    uint32_t supertile = 16;        // band walk order: st x st-unit supertiles (measured: 16 beats rows, 8 and 32)
    uint32_t max_blas_height = 0;
    bool timeline_on = false;
    bool costmap_on = false;
    // option "reorder" (schedule.hip): longest-first claim order from the previous launch's unit costs
    bool reorder = true;
    // heavy-unit pieces: class level for halves | quarters << 8 (0xFF = never); measured (C2 / C3 / C4
    // shares, profiles/r02_sweep_period*.jsonl): quarters from level 12 and no halves
    uint32_t split = 12u | 12u << 8;
    // fixed setting "reorder_period" (an option until round 5) K: a lane records unit costs on one launch in K and rebuilds its order on
    // the next; the launches between reuse the order (the heaviest regions move little between frames)
    uint32_t reorder_period = 8;        // measured: 8 (C2 0.242 ms/step) beats 1 (0.265) with 3 lanes
    void forget_schedules() { for (Lane &l : ln) l.valid = false; }   // every lane's next launch starts a new layout
    DevBuf<uint32_t> costmap;
    size_t costmap_pixels = 0;
    DevBuf<unsigned long long> timeline;
    uint32_t timeline_waves = 0;    // waves of the last launch that recorded a timeline
    // device counters, one CNT_NUM block per lane: a launch only adds to its own lane's block, so resetting
    // or reading it never races with another lane's launch still in flight (rt_scene_collect sums the lanes)
    unsigned long long *counters = nullptr;       // HBM NLANE x CNT_NUM
    unsigned long long *counters_host = nullptr;  // pinned NLANE x CNT_NUM
    unsigned long long *lane_counters(int q) const { return counters + (size_t)q * CNT_NUM; }
    // a frame without RT_RENDER_KEEP_COUNTERS starts a new epoch; a lane's block is cleared by the first launch
    // of that lane in the epoch (no waiting on the other lanes: Lane::epoch), and rt_scene_collect sums only blocks
    // of the current epoch
    uint64_t cnt_epoch = 0;

    // camera
    bool cam_ok = false;
    CameraGPU cam{};
    uint32_t width = 0, height = 0;

    // scene-owned outputs
    DevBuf<uint8_t> out_rgba;
    DevBuf<float> out_rgb;

    // RT_BUILD_LBVH: GPU builders and the raw caller primitives they read
    LbvhBuilder *blas_builder = nullptr, *tlas_builder = nullptr;
    DevBuf<rt_triangle> raw_tris;
    DevBuf<float> raw_verts;            // 9 floats per triangle (extract_tri_verts): the builder's reads
    // rt_scene_update_triangles: the new triangles are staged in pinned memory and copied on the scene stream,
    // behind the BLAS builds that read raw_tris (the only readers) and without waiting for any trace
    rt_triangle *raw_stage = nullptr;
    size_t raw_stage_cap = 0;
    hipEvent_t ev_raw_staged = nullptr;            // the last staged copy finished (raw_stage reusable)
    // rt_scene_update_triangles_device: its kernel's completion (the caller's stream waits on it; the scene stream
    // orders everything else), and whether `tris` still mirrors raw_tris: the kernel's vertices and normals never
    // reach the host, so whoever reads the mirror's geometry first calls refresh_tris_mirror (update.cpp)
    hipEvent_t ev_tri_update = nullptr;
    bool tris_host_stale = false;
    // RT_TRI_UPDATE_BOUNDS (inst_bounds.hip): per record (instances, then groups) whether the device holds its local
    // bounds — the box is its BLAS root's, the centroid dev_cent's — until the host takes them back
    // (rt_scene_update_instances, a host rt_scene_update_triangles on it, rt_scene_build); the host's InstState::box /
    // centroid of such a record are stale.  The static tables of the build (InstBoundsGPU, launch.hpp); ib_cent holds
    // every record's local centroid, the host-bounded ones' uploaded at the build and whenever the host changes one
    // that a group's mean reads (refresh_dev_centroids, through the pinned ib_cent_stage, slot = record)
    std::vector<uint8_t> dev_bounded;   // empty outside RT_BUILD_LBVH (dev_bounded_rec)
    static constexpr uint32_t NONE = 0xFFFFFFFFu;   // ib_entry_of, seg_of_blas: no entry
    std::vector<uint32_t> ib_entry_of;  // instance -> entry of ib_table (NONE: not a triangle instance)
    DevBuf<InstBoundsEntry> ib_table;
    DevBuf<uint32_t> ib_chunk_inst, ib_multi, ib_members;
    DevBuf<uint2> ib_groups;
    DevBuf<double> ib_partials;
    DevBuf<float4> ib_cent;
    float4 *ib_cent_stage = nullptr;
    DevBuf<rt_sphere> raw_sph;
    DevBuf<rt_parallelogram> raw_quad;
    DevBuf<uint32_t> inst_blas;         // instance record (instances, then groups) -> segment
    // RT_BUILD_LBVH + option "group": every unique BLAS's segment (index = BLAS index; the groups' merged BLASes
    // follow the own ones), BLAS -> segment the builder currently holds (NONE: not built), and per group whether
    // it was intact at that setup.  A group's BLAS and its members' BLASes share one leaf-slot range, and only
    // one of them is built: the group's while it is intact, the members' once it breaks (lbvh_segments)
    std::vector<LbvhSeg> lbvh_segs;
    std::vector<uint32_t> seg_of_blas;
    std::vector<uint8_t> lbvh_intact;
    DevBuf<uint32_t> gpu_counts;        // [0] BLAS pairs written, [1] unused, [2 + b] TLAS pairs of frame block b
    bool rebuild_blas = false;          // option "rebuild": rebuild every BLAS each frame
    bool blas_dirty = false;            // rt_scene_update_triangles since the last BLAS build
    // RT_BUILD_LBVH rebuilds (option "blas_double", default on): a rebuild writes a spare BLAS set and swaps it
    // in, so frame k+1's rebuild runs while frame k's trace still reads the other set (C5: the rebuild no
    // longer waits for every lane's trace).  cur.ev_lane[q]: lane q's last trace of the current set.
    // Option "blas_sets" = 3 (default; 2 = one spare): two spare sets in rotation, so frame k+1's rebuild waits only
    // for frame k-2's trace and three traces stay in flight beside it (spare[0] = the set read longest ago, the next
    // one written; C5 with the rebuild 11.18 -> 10.85 ms/frame, profiles/r04/c5_rebuild/).
    static constexpr uint32_t MAX_BLAS_SETS = 8;
    BlasSet spare[MAX_BLAS_SETS - 1];   // spare[0]: the set read longest ago (written next) .. spare[sets - 2]: the newest
    uint32_t blas_sets = 3;
    bool blas_double = true;
    uint64_t blas_builds = 0;
    bool gpu_tlas_sah = false;          // option "gpu_tlas" (set before the build): RT_BUILD_SAH BLASes, per-frame TLAS on the GPU
    // option "tlas_small": GPU-built frames with at most SMALL_TLAS_MAX records in the TLAS build it in one workgroup
    // (lbvh_tlas_small.hpp tlas_small_kernel) instead of the ~17-launch chain
    bool tlas_small = true;
    DevBuf<uint32_t> blas_wide_refs;    // host-built BLASes under a GPU TLAS: quad root ref per BLAS
    // instance records + TLAS built by kernels each frame: RT_BUILD_LBVH, or RT_BUILD_SAH with "gpu_tlas"
    bool gpu_tlas() const { return build_mode == RT_BUILD_LBVH || (gpu_tlas_sah && build_mode == RT_BUILD_SAH); }
    // quads of two binary levels visited in the reference's order (layout.hpp NodeQuad): the reference's own trees and
    // GPU-built ones; host SAH trees keep the greedy collapse visited by entry t
    bool quad_halves() const { return build_mode != RT_BUILD_SAH; }

    CommState *comm = nullptr;             // multi-GPU frame (rt_scene_attach_comm)
    uint32_t comm_timeout_ms = 0;          // rt_comm_set_timeout (kept across attach / detach)
    void release_comm();                   // scene_comm.cpp
    // A failed frame (peer error or deadline): abort every communicator so the gather kernels in flight
    // return, and drop the communicator state.  The slabs are not freed: kernels of the aborted frames may
    // still reference them, and hipFree would wait for those (a bounded leak instead of a hang).
    void abort_comm();

    ~rt_scene();                           // scene_sync.cpp
};

namespace rtamd {

// the caller's current device, put back on every return path of a call that switches to the scene's
struct DeviceRestore {
    int prev = -1;
    DeviceRestore() { if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); } }
    ~DeviceRestore() { if (prev >= 0) (void)hipSetDevice(prev); }
};

template <typename T>
rt_status upload(DevBuf<T> &buf, const std::vector<T> &v) {
    buf.release();
    const size_t n = v.empty() ? 1 : v.size();
    HIP_TRY(hipMalloc(&buf.p, n * sizeof(T)));
    buf.n = v.size();
    if (!v.empty()) HIP_TRY(hipMemcpy(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return RT_OK;
}

template <typename T>
rt_status alloc_buf(DevBuf<T> &buf, size_t n) {
    buf.release();
    HIP_TRY(hipMalloc(&buf.p, (n ? n : 1) * sizeof(T)));
    buf.n = n;
    return RT_OK;
}

template <typename T>
hipError_t read_back(std::vector<T> &v, const T *src, size_t n) {
    v.resize(n);
    return n ? hipMemcpy(v.data(), src, n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
}

// scene_sync.cpp: wait for a stream / an event of the scene (bounded polls with a communicator attached)
rt_status comm_poll(rt_scene *s, hipStream_t st, hipEvent_t ev);
rt_status wait_stream(rt_scene *s, hipStream_t st);
rt_status wait_event(rt_scene *s, hipEvent_t ev);
rt_status drain(rt_scene *s);
rt_status wait_if_pending(hipStream_t st, hipEvent_t ev, bool *pending);
rt_status wait_queries(rt_scene *s, hipStream_t st);
rt_status wait_blas_built(rt_scene *s, hipStream_t st);
rt_status wait_frame_block(rt_scene *s);
rt_status order_after_stream(rt_scene *s, hipStream_t from, hipStream_t st);
rt_status order_after_null_stream(rt_scene *s, hipStream_t st);
rt_status wait_record_chains(rt_scene *s, hipStream_t st);

// frame.cpp
void instance_update(InstState &in, const rt_xform &x);
rt_status frame_update(rt_scene *s, uint64_t frame, hipStream_t upload, bool defer = false);
SceneGPU scene_gpu(const rt_scene *s);
bool record_inactive(const rt_scene *s, size_t i);
const InstState &record_state(const rt_scene *s, size_t i);
bool group_intact(const rt_scene *s, size_t g);

// build.cpp: rt_scene_build; the primitives' bounds and materials as every builder reads them
size_t prim_len(const rt_scene *s, uint32_t type);
hm::Box prim_box(const rt_scene *s, uint32_t type, uint32_t i);
hm::V3 prim_centroid(const rt_scene *s, uint32_t type, uint32_t i);
void bounds_from_prims(const rt_scene *s, InstState &in);
void bounds_from_desc(const rt_instance_desc &d, InstState &in);
void group_bounds(const rt_scene *s, InstGroup &G);
uint32_t material_slot(const rt_scene *s, uint32_t type, uint32_t index, bool &ok);
rt_status check_materials(bool ok, const char *what = "primitive");   // `ok` as material_slot left it
template <typename T>
rt_status check_materials(const rt_scene *s, const T *prims, size_t count, const char *what = "primitive") {
    bool ok = true;
    for (size_t k = 0; k < count; k++) material_slot(s, prims[k].material_type, prims[k].material_index, ok);
    return check_materials(ok, what);
}
// blas_gpu.cpp: the RT_BUILD_LBVH BLASes, built on the GPU
rt_status lbvh_segments(rt_scene *s);
rt_status lbvh_sync_groups(rt_scene *s);
rt_status gpu_build_blas(rt_scene *s);
rt_status gpu_setup_blas(rt_scene *s, const uint32_t *slot_count);
// update.cpp: the geometry updates between frames
rt_status refresh_tris_mirror(rt_scene *s);
rt_status setup_inst_bounds(rt_scene *s);
inline bool dev_bounded_rec(const rt_scene *s, size_t record) { return !s->dev_bounded.empty() && s->dev_bounded[record]; }

// scene_comm.cpp: a multi-GPU frame's gather to rank 0 and its assembly there, on the trace's stream
rt_status comm_gather(rt_scene *s, int q, uint8_t *frame_out, hipStream_t stream);

// rt_api.cpp, render.cpp, filters.cpp
uint32_t tiles_for_rank(uint32_t w, uint32_t h, uint32_t tw, uint32_t th, uint32_t rank, uint32_t count);
void fill_stats(rt_stats *st, const unsigned long long *c);
rt_status sum_lane_counters(rt_scene *s, unsigned long long *sum);
bool device_accessible(const void *p, int device);
rt_status all_accessible(std::initializer_list<const void *> bufs, int device, const std::string &message);
rt_status select_device(int device);

}  // namespace rtamd
