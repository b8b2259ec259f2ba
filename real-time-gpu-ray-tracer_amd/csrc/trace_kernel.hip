// trace_kernel.hip — the hot path on gfx950: camera ray -> two-level BVH traversal
// (TLAS -> instance -> BLAS) -> sphere / parallelogram / Moller-Trumbore intersection ->
// Rough/Metal scatter loop -> average -> gamma-2 quantise -> framebuffer write.
//
// Restates the reference kernel `render` (src/Global/Kernel.cu:105-147) and its device
// callees: rayColor (Kernel.cu:6-103), TLAS::hit (src/AS/TLAS.cu:131-201), Instance::hit
// (src/AS/Instance.cu:19-50), BLAS::hit (src/AS/BLAS.cu:119-206), BoundingBox::hit
// (src/AS/BoundingBox.cu:34-72), Sphere/Parallelogram/Triangle::hit (src/Geometry/*.cu),
// Rough/Metal::scatter (include/Material/*.cuh), Color3::castToUchar4 (Color3.cuh:99-114).
//
// This file is compiled three times:
//   RT_EXACT=1, -ffp-contract=off : every float operation in the reference's order with IEEE
//       division, the reference's binary trees and visit order — bit-faithful to the oracle on identical
//       trees, equal work counters (parity mode);
//   RT_EXACT=0 RT_FAST_IEEE=1, -ffp-contract=off (default): the persistent quad-tree kernel with
//       reciprocal-direction slab tests (one explicit FMA per plane, a cull only) and the reference's
//       arithmetic everywhere a value reaches a hit or a pixel — on the reference's trees its frames are
//       bit-identical to the oracle's;
//   RT_EXACT=0 RT_FAST_IEEE=0, -ffp-contract=fast (option "fast_math"): also reciprocal determinant /
//       division, v_rsq, FMA-contracted transforms (parity within the measured tolerance).
//
// Traversal keeps the reference's visit order exactly: node pairs test both children of an
// interior node (BLAS.cu:180-202), the near child (smaller entry t; ties -> left) is visited
// next and the far child is pushed with its entry t; a popped entry is culled iff its entry t
// >= the current tmax, which is exactly when the reference's re-test of the popped node box
// (BLAS.cu:145) fails.  TLAS leaves with two instances push a non-cullable "resume" entry, as
// the reference loops over a leaf's instances without re-testing the leaf box (TLAS.cu:157-173).
//
// This file holds the flavour macros and knobs, the kernels and their launchers.  The device functions are in
// headers included once below, inside namespace rtamd::RT_SUFFIX(dev), in this order:
//   vecmath.hpp     f3 and its operations, rcp / fdiv / unit per flavour, the pinned RNG, xf_point / xf_vector
//   box.hpp         RayP / prep, the reference's slab, the FAST conservative slabs and their exact re-takes (slab,
//                   slab4, quad_decide), XD_* / XBOX
//   primitives.hpp  tri_test, sphere_test, quad_test
//   stack.hpp       the per-lane LDS / scratch paged stack
//   traverse.hpp    Trav and the traversal state machine (trav_step; spec_round over binary pairs or quads), the LDS
//                   scene region, the diagnostic build's phase stamps
//   shade.hpp       finalize, ray_color, camera_ray, map_item, write_pixel, counter and unit-cost flushes
//   ray_query.hpp   (at the end, inside namespace rtamd) rt_query_rays' kernel and launcher
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "launch.hpp"
#include "layout.hpp"
#include "../../include/rt.h"

#ifndef RT_EXACT
#error "compile with -DRT_EXACT=0 or 1"
#endif

// RT_FAST_IEEE (FAST builds): 1 = the reference's correctly rounded division and 1/sqrt everywhere except the box
// tests' reciprocal slabs, compiled without FMA contraction (the default FAST kernel: on the reference's own trees
// its frames are bit-identical to the oracle's); 0 = hardware v_rcp / v_rsq and FMA contraction
// (option "fast_math": ~8 % faster on C2 / C3, and ~0.01-0.09 % of pixels differ, measured)
#ifndef RT_FAST_IEEE
#define RT_FAST_IEEE 1
#endif
#if RT_EXACT
#define RT_SUFFIX(n) n##_exact
#elif RT_FAST_IEEE
#define RT_SUFFIX(n) n##_fast
#else
#define RT_SUFFIX(n) n##_fastmath
#endif

namespace rtamd {
namespace RT_SUFFIX(dev) {

constexpr float FZERO = 1e-6f;          // FLOAT_ZERO_VALUE (Global.cuh:147)
constexpr float TMIN = 0.001f;          // Kernel.cu:66
constexpr int BLOCK = 256;              // 4 waves; each wave owns one 8x8 pixel unit
#ifndef RT_LDS_DEPTH
#define RT_LDS_DEPTH 16
#endif
#ifndef RT_LDS_MATERIALS
#define RT_LDS_MATERIALS 64              // the scene region ("lds_scene") needs the rest of the 52 KB
#endif
constexpr int LDS_DEPTH = RT_LDS_DEPTH;         // per-lane stack entries kept in LDS
constexpr int LDS_MATERIALS = RT_LDS_MATERIALS; // persistent kernel: material table in LDS up to this many slots
constexpr int SPILL_DEPTH = 64 - LDS_DEPTH;   // overflow entries in scratch (max depth 64 = reference)
static_assert(LDS_DEPTH % 4 == 0, "half-pages move as 16 B pieces");
#ifndef RT_CHAIN_ROOT_LEAF
#define RT_CHAIN_ROOT_LEAF 1            // quad trees: an entered instance whose BLAS root is a leaf (a sphere, a
                                        // parallelogram, a small mesh) has it tested in the same leaf round
#endif
#ifndef TRI_AHEAD
#define TRI_AHEAD 4                     // triangle records of a leaf requested before the first test (all 4 of a
                                        // full leaf: C2 serialised -2..-7 %, C3 -0.6 %; profiles/r02_ab_tri_ahead.jsonl)
#endif

#include "vecmath.hpp"
#include "box.hpp"
#include "primitives.hpp"
#include "stack.hpp"
#include "traverse.hpp"
#include "shade.hpp"

template <bool COUNT>
__global__ __launch_bounds__(BLOCK) void render_kernel(SceneGPU sc, CameraGPU cam, OutputGPU out,
                                                       unsigned long long *counters) {
    __shared__ unsigned long long lds_stack[LDS_DEPTH][BLOCK];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const uint32_t wunit = blockIdx.x * (BLOCK / 64) + (tid >> 6);
    if (wunit >= out.units) return;                       // wave-uniform

    // 8x8 pixel unit -> pixel + output index
    uint32_t px, py, oi;
    if (out.tile_count == 0) {
        const uint32_t ux = wunit % out.units_x, uy = wunit / out.units_x;
        px = ux * 8 + (lane & 7); py = uy * 8 + (lane >> 3);
        oi = py * cam.width + px;
    } else {
        const uint32_t upr = out.tile_w / 8, upt = upr * (out.tile_h / 8);
        const uint32_t k = wunit / upt, r = wunit % upt;
        const uint32_t t = out.tile_rank + k * out.tile_count;
        const uint32_t lx = (r % upr) * 8 + (lane & 7), ly = (r / upr) * 8 + (lane >> 3);
        px = (t % out.tiles_x) * out.tile_w + lx;
        py = (t / out.tiles_x) * out.tile_h + ly;
        oi = k * out.tile_w * out.tile_h + ly * out.tile_w + lx;
    }
    const bool valid = px < cam.width && py < cam.height;

    Trav T;
    T.stk.lds = (LdsU2 *)&lds_stack[0][tid];
    alignas(16) SEnt spill[SPILL_DEPTH];
    LaneCount cnt = {};
    uint32_t rays = 0;

    if (valid) {
        const uint32_t pixel = cam.pitch * py + px;                            // Kernel.cu:109
        Rng rng;
        rng.init((uint64_t)pixel ^ cam.frame_seed, pixel);                      // Kernel.cu:114
        f3 result = mk(0.0f, 0.0f, 0.0f);
        // (not camera_ray(): that one is never contracted; this follows the build, as the reference's kernel does)
        const f3 po = ld3(cam.pixel_origin), dx = ld3(cam.dx), dy = ld3(cam.dy), cc = ld3(cam.center);
        for (uint32_t si = 0; si < cam.sqrt_s; si++) {
            for (uint32_t sj = 0; sj < cam.sqrt_s; sj++) {                      // Kernel.cu:119-139
                const float ox = (((float)sj + rng.uniform()) * cam.recip_sqrt) - 0.5f;
                const float oy = (((float)si + rng.uniform()) * cam.recip_sqrt) - 0.5f;
                const f3 sp = add(add(po, scl(dx, (float)px + ox)), scl(dy, (float)py + oy));
                f3 origin = cc;
                if (cam.focus_radius > 0.0f) {
                    const f3 dv = random_plane_vector(rng, cam.focus_radius);
                    origin = add(add(cc, scl(ld3(cam.cu), dv.x)), scl(ld3(cam.cv), dv.y));
                }
                const f3 dir = unit(sub(sp, origin));
                result = add(result, ray_color<COUNT>(sc, cam, origin, dir, rng, T, spill, cnt, rays));
            }
        }
        result = scl(result, cam.recip_sqrt * cam.recip_sqrt);                  // Kernel.cu:143
        // (write_pixel()'s code, inline: calling it here changed this kernel's code in every flavour)
        if (out.rgb) {
            out.rgb[3 * (size_t)oi + 0] = result.x;
            out.rgb[3 * (size_t)oi + 1] = result.y;
            out.rgb[3 * (size_t)oi + 2] = result.z;
        }
        // Color3::castToUchar4, gamma 2 (Color3.cuh:99-114)
        const float cr = fminf(fmaxf(sqrtf(result.x), 0.0f), 0.999f);
        const float cg = fminf(fmaxf(sqrtf(result.y), 0.0f), 0.999f);
        const float cb = fminf(fmaxf(sqrtf(result.z), 0.0f), 0.999f);
        const uint32_t packed = (uint32_t)(uint8_t)(256.0f * cr) | ((uint32_t)(uint8_t)(256.0f * cg) << 8) |
                                ((uint32_t)(uint8_t)(256.0f * cb) << 16) | (255u << 24);
        reinterpret_cast<uint32_t *>(out.rgba)[oi] = packed;
    }

    const uint32_t wr = wave_sum(rays);
    const uint32_t wp = wave_sum(valid ? 1u : 0u);
    flush_counts<COUNT>(counters, cnt, lane);
    if (lane == 0) {
        atomicAdd(&counters[CNT_RAYS], (unsigned long long)wr);
        atomicAdd(&counters[CNT_PIXELS], (unsigned long long)wp);
    }
}

// ---- persistent-wave megakernel ------------------------------------------------------------
// One launch of (#CUs x resident blocks) workgroups.  Each lane owns one pixel at a time and runs its
// whole path (samples x bounces) as a sequence of ray segments; a segment is traversed step by
// step (trav_step).  A wave keeps stepping while most lanes are traversing; when `threshold` lanes
// have finished their segment (or are idle), the wave leaves the traversal loop and shades those
// lanes together (scatter -> next segment, or next sample, or pixel write + a new pixel from the
// work queue).  Lanes are refilled from a per-wave pool of 64 consecutive work items claimed with
// one atomic per pool (ballot-compacted lane refill).  Each pixel's RNG stream
// is consumed in exactly the reference order, so the image equals the grid kernel's bit for bit — but
// under fast_math, where the grid kernel's inline camera-ray code is FMA-contracted and camera_ray() is
// not, so the two kernels may start a path from rays one rounding apart.
template <bool COUNT, int WIDE, int RAW>
__device__ __forceinline__ void render_persistent_body(const SceneGPU &sc, const CameraGPU &cam, const OutputGPU &out,
                                                       uint32_t *queue, uint32_t threshold, unsigned long long *counters) {
    __shared__ unsigned long long lds_stack[LDS_DEPTH][BLOCK];
    __shared__ float4 lds_mat[LDS_MATERIALS];     // the scene's materials (shading reads them per hit)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const bool mat_lds = sc.material_count <= LDS_MATERIALS;
    if (mat_lds && tid < (int)sc.material_count) lds_mat[tid] = reinterpret_cast<const float4 *>(sc.materials)[tid];
#if !RT_EXACT
    if constexpr (WIDE) lds_scene_fill(sc);
#endif
    __syncthreads();                              // once, before any wave leaves for the queue
    const TreeRoot root = uniform_root<WIDE != 0>(sc);

    Trav T;
    T.stk.lds = (LdsU2 *)&lds_stack[0][tid];
    T.tracing = false;
    T.found = false;
    alignas(16) SEnt spill[SPILL_DEPTH];
    LaneCount cnt = {};
    uint32_t rays = 0, pixels = 0;

    bool has = false;                  // lane owns a pixel
    uint32_t px_steps = 0;             // traversal steps spent on the lane's pixel (COUNT cost map, reorder)
    uint32_t item = 0, sample = 0, depth = 0;
    Rng rng;
    rng.s = 0;
    f3 acc = mk(0.0f, 0.0f, 0.0f), thr = mk(1.0f, 1.0f, 1.0f);
    uint32_t pool_next = 0, pool_end = 0;     // wave-uniform
    uint32_t limit = 0, limit_part = ~0u;     // wave-uniform: claim positions in band `limit_part`
    bool exhausted = false;                   // wave-uniform
    const uint32_t S2 = cam.sqrt_s * cam.sqrt_s;
    // Work queue: the frame's units are split into `parts` bands; a wave drains the band of its own
    // XCD first (primary rays of one band share geometry in that XCD's L2), then steals from the others.
    const uint32_t parts = out.queue_parts;
    const uint32_t xcc = xcc_id();
    uint32_t part = xcc % parts, tried = 0;
    const uint32_t grab = out.grab;                 // claim size (pixels)
    const bool track = out.unit_cost != nullptr;    // record unit costs for the next launch's order
    uint32_t pend_unit = 0, pend_cost = 0;          // the lane's unflushed unit cost (flushed before a claim)
    unsigned long long t_start = 0, t_exhaust = 0;
    uint32_t n_rounds = 0, n_shades = 0, n_grabs = 0;      // wave-uniform (timeline)
    PhaseCycles pc = {};
    if (out.timeline) t_start = __builtin_amdgcn_s_memrealtime();

    for (;;) {
        // ---- refill idle lanes from the wave's pool / the global queue
        DIAG_T(t_refill);
        uint64_t need = __ballot(!has);
        while (need && !exhausted) {
            if (RT_DIAG) pc.refill_iters++;
            const uint32_t n_need = __popcll(need);
            if (pool_next >= pool_end) {
                // bands: whole unit rows in frame mode (so a band can be walked in supertiles)
                const uint32_t rows = out.tile_count == 0 ? out.units / out.units_x : out.units;
                const uint32_t upr = out.tile_count == 0 ? out.units_x : 1u;
                const uint32_t p_begin = (rows * part / parts) * upr * 64u;
                const uint32_t p_end = (rows * (part + 1) / parts) * upr * 64u;
                // ordered walk (schedule.hip): one item per claim, a whole unit or a 1/2, 1/4 of a heavy
                // one; the band's item count sits next to its head.  Screen walk: `grab` pixels per claim.
                const uint32_t step = out.order ? 1u : grab;
                if (part != limit_part) {          // the band's item count: read once per band, off the head's line
                    limit_part = part;
                    limit = out.order ? __builtin_amdgcn_readfirstlane(queue[(QUEUE_MAX_PARTS + part) * QUEUE_STRIDE])
                                      : p_end - p_begin;
                }
                if (track) {                         // completes under the claim's wait
                    unit_cost_add(out.unit_cost, pend_cost != 0, pend_unit, pend_cost);
                    pend_cost = 0;
                }
                uint32_t b = 0;
                if (lane == 0) b = atomicAdd(queue + part * QUEUE_STRIDE, step);
                b = __builtin_amdgcn_readfirstlane(__shfl(b, 0, 64));
                n_grabs++;
                if (b >= limit) {
                    // the band is dry: try the next one.  `tried` counts failures over the wave's life, so a
                    // wave retires after `parts` failed claims even if a band it left still has items: it frees
                    // its slot for the next lane's launch (a scan of every band's head instead, stealing until
                    // the last item, measured 45 % slower on C2: profiles/r02_ab_exit_scan.jsonl)
                    if (++tried >= parts) {
                        exhausted = true;
                        if (out.timeline) t_exhaust = __builtin_amdgcn_s_memrealtime();
                        break;
                    }
                    part = part + 1 == parts ? 0 : part + 1;
                    continue;
                }
                if (out.order) {
                    const uint32_t it = out.order[4u * (p_begin >> 6) + b];
                    // log2 pieces 3: two adjacent light units (schedule setting "merge"), 128 pixels
                    const uint32_t ls = it & 3u, len = ls == 3u ? 128u : 64u >> ls;
                    pool_next = (it >> 4) * 64u + (ls == 3u ? 0u : ((it >> 2) & 3u) * len);
                    pool_end = pool_next + len;
                } else {
                    b += p_begin;
                    pool_next = b;
                    pool_end = min(b + grab, p_end);
                }
                if (!out.order && out.supertile && out.tile_count == 0 && grab == 64u) {
                    // walk the band in st x st-unit supertiles (row-major supertiles, row-major units
                    // inside): the units in flight form a compact screen region, not a full-width strip
                    const uint32_t W = out.units_x, st = out.supertile;
                    const uint32_t r0 = p_begin / (64u * W), Hb = (p_end - p_begin) / (64u * W);
                    const uint32_t j = (b - p_begin) >> 6;
                    const uint32_t sr = j / (W * st);
                    const uint32_t h = min(st, Hb - sr * st);
                    const uint32_t k = j - sr * W * st;
                    const uint32_t sc = k / (st * h);
                    const uint32_t w = min(st, W - sc * st);
                    const uint32_t m = k - sc * st * h;
                    const uint32_t u = (r0 + sr * st + m / w) * W + sc * st + m % w;
                    pool_next = u * 64u;
                    pool_end = pool_next + 64u;
                }
            }
            const uint32_t take = min(n_need, pool_end - pool_next);
            const uint32_t rank = __popcll(need & ((1ull << lane) - 1ull));
            DIAG_T(t_lanes);
            if (!has && rank < take) {
                uint32_t px, py, oi;
                item = pool_next + rank;
                if (map_item(out, cam, item, px, py, oi)) {
                    has = true;
                    const uint32_t pixel = cam.pitch * py + px;                    // Kernel.cu:109
                    rng.init((uint64_t)pixel ^ cam.frame_seed, pixel);              // Kernel.cu:114
                    acc = mk(0.0f, 0.0f, 0.0f);
                    thr = mk(1.0f, 1.0f, 1.0f);
                    sample = 0; depth = 0;
                    px_steps = 0;
                    f3 o, d;
                    camera_ray(cam, px, py, 0, rng, o, d);
                    trav_init<XBOX(WIDE)>(T, root, o, d);
                    pixels++;
                }
            }
            DIAG_ADD(pc.claim, t_lanes);
            pool_next += take;
            need = __ballot(!has);          // lanes handed an out-of-frame item (edge units) retry
        }
        DIAG_ADD(pc.refill, t_refill);
        if (!__any(has)) {
            if (exhausted) break;
            continue;
        }
        // ---- traverse while enough lanes are busy
        for (;;) {
            const uint64_t tr = __ballot(T.tracing);
            if (tr == 0) break;
            const uint64_t want = __ballot(!T.tracing && (has || !exhausted));
            if ((uint32_t)__popcll(want) >= threshold) break;
            spec_round<COUNT, WIDE>(T, sc, spill, cnt, pc, px_steps, COUNT || track, out.leaf_early);
            n_rounds++;
        }
        // ---- shade lanes whose segment finished (rayColor body, Kernel.cu:64-100)
        n_shades++;
        DIAG_T(t_shade);
        bool fin = false;                    // lane wrote its pixel in this step
        if (RT_DIAG) pc.lanes_shade += (unsigned long long)__popcll(__ballot(has && !T.tracing));
        if (has && !T.tracing) {
            rays++;
            bool path_done;
            f3 no = T.wr.o, nd = T.wr.d;                                     // next segment
            if (T.found) {
                if (COUNT) cnt.hits++;
                if (RT_DIAG) pc.hits++;
                const uint32_t material = hit_material<WIDE != 0, RAW>(sc, T.hit);
                const uint32_t mi = material & ~MAT_METAL_BIT;
                if (depth + 1 >= cam.depth && !(material & MAT_METAL_BIT)) {
                    // A path's last segment on a rough surface (Rough.cuh:14-29 never absorbs): only the albedo
                    // reaches the pixel, so the surface is not reconstructed.  The scatter draws are consumed while
                    // the pixel has samples left — they see the RNG stream they would have — and skipped after
                    // the last one, whose stream nobody reads.
                    if (RT_DIAG) pc.hits_last_rough++;
                    const float4 m = mat_lds ? lds_mat[mi] : reinterpret_cast<const float4 *>(sc.materials)[mi];
                    if (sample + 1 < S2) (void)random_space_vector(rng);
                    thr = mul(thr, mk(m.x, m.y, m.z));
                    depth++;
                    path_done = true;
                } else {
                    const Surface s = finalize<WIDE != 0, RAW>(sc, T.wr.o, T.wr.d, T.hit);
                    DIAG_WAIT_VM();
                    DIAG_T(t_hit);
                    const float4 m = mat_lds ? lds_mat[mi] : reinterpret_cast<const float4 *>(sc.materials)[mi];
                    bool absorbed = false;
                    if (!(s.material & MAT_METAL_BIT)) {                     // Rough.cuh:14-29
                        nd = add(s.n, random_space_vector(rng));
                        if (f_eq(dot(nd, nd), FZERO * FZERO)) nd = s.n;
                    } else {                                                 // Metal.cuh:15-32
                        nd = unit(sub(T.wr.d, scl(s.n, 2.0f * dot(T.wr.d, s.n))));
                        if (m.w > 0.0f) nd = add(nd, scl(random_space_vector(rng), m.w));
                        absorbed = !(dot(nd, s.n) > 0.0f);
                    }
                    DIAG_ADD(pc.hit, t_hit);
                    if (absorbed) {
                        path_done = true;                                    // throughput (Kernel.cu:85-87)
                    } else {
                        thr = mul(thr, mk(m.x, m.y, m.z));
                        no = s.p;
                        depth++;
                        path_done = depth >= cam.depth;                      // throughput on exhaustion
                    }
                }
            } else {
                thr = mul(thr, ld3(cam.background));
                path_done = true;
            }
            if (path_done) {
                acc = add(acc, thr);                                         // Kernel.cu:138
                sample++;
                uint32_t px, py, oi;
                map_item(out, cam, item, px, py, oi);
                if (sample < S2) {
                    thr = mk(1.0f, 1.0f, 1.0f);
                    depth = 0;
                    camera_ray(cam, px, py, sample, rng, no, nd);
                } else {
                    write_pixel(out, oi, scl(acc, cam.recip_sqrt * cam.recip_sqrt));   // Kernel.cu:143-146
                    if (COUNT && out.costmap) out.costmap[oi] = px_steps;
                    has = false;
                    fin = true;
                }
            }
            if (has) trav_init<XBOX(WIDE)>(T, root, no, nd);
        }
        if (track && fin) {
            const uint32_t u = item >> 6;
            if (u != pend_unit) {
                if (pend_cost) unit_cost_flush(out.unit_cost, pend_unit, pend_cost);
                pend_unit = u;
                pend_cost = 0;
            }
            pend_cost = pend_cost + px_steps + 1u;
        }
        DIAG_ADD(pc.shade, t_shade);
    }

    if (track && pend_cost) unit_cost_flush(out.unit_cost, pend_unit, pend_cost);
    const uint32_t wr = wave_sum(rays);
    const uint32_t wp = wave_sum(pixels);
    flush_counts<COUNT>(counters, cnt, lane);
    if (lane == 0) {
        atomicAdd(&counters[CNT_RAYS], (unsigned long long)wr);
        atomicAdd(&counters[CNT_PIXELS], (unsigned long long)wp);
        if (out.timeline) {
            // the wave's index from its stack window address (threadIdx.x kept live to here was spilled)
            const uint32_t wv = (uint32_t)((const unsigned long long *)T.stk.lds - &lds_stack[0][0]) >> 6;
            unsigned long long *w = out.timeline + (unsigned long long)TIMELINE_WORDS * (blockIdx.x * (BLOCK / 64) + wv);
            w[0] = t_start;
            w[1] = __builtin_amdgcn_s_memrealtime();
            w[2] = ((unsigned long long)hw_id() << 32) | xcc;
            w[3] = wp;
            w[4] = t_exhaust;
            w[5] = n_rounds;
            w[6] = n_shades;
            w[7] = n_grabs;
            w[8] = pc.refill;
            w[9] = pc.interior;
            w[10] = pc.leaf;
            w[11] = pc.shade;
            w[12] = pc.iters;
            w[13] = pc.refill_iters;
            w[14] = pc.claim;
            w[15] = pc.hit;
            w[16] = pc.lanes_interior;
            w[17] = pc.lanes_leaf_tlas;
            w[18] = pc.lanes_leaf_blas;
            w[19] = pc.lanes_shade;
            w[20] = pc.lanes_postpone;
            w[21] = pc.iters_idle;
        }
    }
    if (RT_DIAG && out.timeline) {     // per-lane counts: summed over the wave
        const uint32_t wv = (uint32_t)((const unsigned long long *)T.stk.lds - &lds_stack[0][0]) >> 6;
        unsigned long long *w = out.timeline + (unsigned long long)TIMELINE_WORDS * (blockIdx.x * (BLOCK / 64) + wv);
        atomicAdd(&w[22], pc.hits);
        atomicAdd(&w[23], pc.hits_last_rough);
    }
}

// Register budget variants: WPE = minimum waves per SIMD the compiler must allow (0 = its choice).
template <bool COUNT, int WPE, int WIDE = 0, int RAW = 2>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(WPE > 0 ? WPE : 1)))
void render_persistent_kernel(SceneGPU sc, CameraGPU cam, OutputGPU out, uint32_t *queue, uint32_t threshold,
                              unsigned long long *counters) {
    render_persistent_body<COUNT, WIDE, RAW>(sc, cam, out, queue, threshold, counters);
}

__global__ __launch_bounds__(BLOCK) void trace_rays_kernel(SceneGPU sc, const float *rays, uint32_t n, rt_hit *hits) {
    __shared__ unsigned long long lds_stack[LDS_DEPTH][BLOCK];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    Trav T;
    T.stk.lds = (LdsU2 *)&lds_stack[0][threadIdx.x];
    alignas(16) SEnt spill[SPILL_DEPTH];
    LaneCount cnt = {};
    const f3 o = mk(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
    const f3 d = mk(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    Hit h;
    rt_hit r;
    // (ray_query_kernel fills the same record: one shared function changed both kernels' code in every flavour)
    if (trace<false, XD_ALL>(sc, o, d, h, T, spill, cnt)) {
        const Surface s = finalize(sc, o, d, h);
        r.t = h.t; r.instance = s.member ? s.member - 1u : (sc.inst_by_slot ? sc.tlas_slots[h.inst] : h.inst);
        r.primitive_type = h.ptype; r.primitive_index = s.orig;
        r.point.x = s.p.x; r.point.y = s.p.y; r.point.z = s.p.z;
        r.normal.x = s.n.x; r.normal.y = s.n.y; r.normal.z = s.n.z;
        const bool metal = (s.material & MAT_METAL_BIT) != 0;
        r.material_type = metal ? RT_MAT_METAL : RT_MAT_ROUGH;
        r.material_index = (s.material & ~MAT_METAL_BIT) - (metal ? sc.rough_count : 0u);
    } else {
        r.t = __builtin_huge_valf(); r.instance = 0xFFFFFFFFu; r.primitive_type = 0; r.primitive_index = 0;
        r.point.x = r.point.y = r.point.z = 0.0f; r.normal.x = r.normal.y = r.normal.z = 0.0f;
        r.material_type = 0; r.material_index = 0;
    }
    hits[i] = r;
}


// rt_box_test (parity tests, not a render path): the box decisions the kernels take, on caller boxes and rays, one
// thread per (box, ray, tmax) with tmin = 0.001.  Mode 0 (EXACT build): BoundingBox::hit (BoundingBox.cu:34-72).  FAST
// build: 1 the single-box conservative cull (slab<XD_CULL>: instance and root boxes of modes 1 / 2), 2 the same with
// marginal decisions re-taken exactly (slab<XD_ALL>: binary pairs, instance and root boxes of mode 3), 3 a quad slot in
// pair order with exact decisions (quad_decide<true, XD_ALL>: mode 3), 4 a quad slot's conservative cull
// (quad_decide<false, XD_CULL>: modes 1 / 2).  Modes 3 / 4 put the box in slot 0 of a quad whose slot 1 is
// its empty partner (a leaf child's) and whose slots 2 / 3 hold a box behind the ray's origin.
__global__ __launch_bounds__(BLOCK) void box_test_kernel(const float *boxes, const float *rays, const float *tmaxs, uint32_t n,
                                                         uint32_t mode, uint8_t *hit, float *te) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    float b[6];
    for (int c = 0; c < 6; c++) b[c] = boxes[6 * (size_t)i + c];
    RayP r;
    r.o = mk(rays[6 * (size_t)i], rays[6 * (size_t)i + 1], rays[6 * (size_t)i + 2]);
    r.d = mk(rays[6 * (size_t)i + 3], rays[6 * (size_t)i + 4], rays[6 * (size_t)i + 5]);
    const float tmax = tmaxs[i];
    float e = 0.0f;
    bool h = false;
#if RT_EXACT
    (void)mode;
    h = slab_ref(b, r.o, r.d, TMIN, tmax, e);
#else
    if (mode == 1 || mode == 2) {
        if (mode == 2) { prep<XD_ALL>(r); h = slab<XD_ALL>(b, r, TMIN, tmax, e); }
        else { prep<XD_CULL>(r); h = slab<XD_CULL>(b, r, TMIN, tmax, e); }
    } else {
        float4 Q[8];
        float bb[6];       // behind the origin: around o - d, half-width |d_a| / 2 per axis (exit t = -0.5 on every axis)
        const float p3[3] = {r.o.x - r.d.x, r.o.y - r.d.y, r.o.z - r.d.z}, d3[3] = {r.d.x, r.d.y, r.d.z};
        for (int a = 0; a < 3; a++) {
            const float w = 0.5f * fabsf(d3[a]);
            bb[2 * a] = p3[a] - w; bb[2 * a + 1] = p3[a] + w;
        }
        for (int c = 0; c < 6; c++) {
            float *q = reinterpret_cast<float *>(&Q[c]);
            q[0] = b[c]; q[1] = b[c]; q[2] = bb[c]; q[3] = bb[c];
        }
        uint4 R = make_uint4(0u, REF_EMPTY, 0u, REF_EMPTY);
        reinterpret_cast<uint4 *>(Q)[6] = R;
        Q[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float t[4], pa, pb;
        bool hq[4];
        if (mode == 3) {
            prep<XD_ALL>(r);
            quad_decide<true, XD_ALL>(Q, Q[0], Q[1], Q[2], Q[3], Q[4], Q[5], R, r, tmax, t, hq, pa, pb);
        } else {
            prep<XD_CULL>(r);
            quad_decide<false, XD_CULL>(Q, Q[0], Q[1], Q[2], Q[3], Q[4], Q[5], R, r, tmax, t, hq, pa, pb);
        }
        h = hq[0];
        e = t[0];
    }
#endif
    hit[i] = h ? 1 : 0;
    te[i] = h ? e : __builtin_huge_valf();
}
}  // namespace dev

hipError_t RT_SUFFIX(launch_render)(const SceneGPU &sc, const CameraGPU &cam, const OutputGPU &out, bool count,
                                    unsigned long long *counters, hipStream_t stream) {
    using namespace RT_SUFFIX(dev);
    const uint32_t waves_per_block = BLOCK / 64;
    const dim3 grid((out.units + waves_per_block - 1) / waves_per_block);
    if (grid.x == 0) return hipSuccess;
    if (count) hipLaunchKernelGGL(render_kernel<true>, grid, dim3(BLOCK), 0, stream, sc, cam, out, counters);
    else hipLaunchKernelGGL(render_kernel<false>, grid, dim3(BLOCK), 0, stream, sc, cam, out, counters);
    return hipGetLastError();
}

namespace {
template <int WPE, int WIDE = 0, int RAW = 2>
hipError_t launch_persistent_wpe(const SceneGPU &sc, const CameraGPU &cam, const OutputGPU &out, bool count,
                                 unsigned long long *counters, uint32_t *queue, uint32_t blocks_per_cu_cus,
                                 uint32_t threshold, hipStream_t stream) {
    using namespace RT_SUFFIX(dev);
    const uint32_t need = (out.units + (BLOCK / 64) - 1) / (BLOCK / 64);
    const dim3 grid(blocks_per_cu_cus < need ? blocks_per_cu_cus : need);
    if (count)
        hipLaunchKernelGGL((render_persistent_kernel<true, WPE, WIDE, RAW>), grid, dim3(BLOCK), 0, stream, sc, cam, out, queue, threshold, counters);
    else
        hipLaunchKernelGGL((render_persistent_kernel<false, WPE, WIDE, RAW>), grid, dim3(BLOCK), 0, stream, sc, cam, out, queue, threshold, counters);
    return hipGetLastError();
}
template <int WPE, int WIDE = 0, int RAW = 2>
uint32_t blocks_per_cu_wpe() {
    using namespace RT_SUFFIX(dev);
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_persistent_kernel<false, WPE, WIDE, RAW>, BLOCK, 0) != hipSuccess) return 1;
    return n > 0 ? (uint32_t)n : 1u;
}
#if RT_EXACT
constexpr int HAS_WIDE = 0;           // EXACT keeps the reference's binary trees and visit order
#else
constexpr int HAS_WIDE = 1;
#endif
}  // namespace

// One instance per scene kind: traversal mode W (SceneGPU::wide, XBOX) and where a hit triangle's shading data lives
// (finalize's RAW: GPU-built trees without cold records).  Quad trees hold 3 waves per SIMD (WPE 3); binary pairs take
// the compiler's budget (WPE 0).  (Round 5's option "variant" 4 — at least 4 waves per SIMD — was 12 % slower: removed.)
#define RT_DISPATCH_INSTANCE(wide, raw, CALL)                                                  \
    do {                                                                                       \
        if ((wide) && HAS_WIDE) {                                                              \
            if ((raw) && (wide) == 3) return CALL(3, 3 * HAS_WIDE, 1);                         \
            if (raw) return CALL(3, 2 * HAS_WIDE, 1);                                          \
            if ((wide) == 3) return CALL(3, 3 * HAS_WIDE, 0);                                  \
            if ((wide) == 2) return CALL(3, 2 * HAS_WIDE, 0);                                  \
            return CALL(3, HAS_WIDE, 0);                                                       \
        }                                                                                      \
        return CALL(0, 0, 2);                                                                  \
    } while (0)

hipError_t RT_SUFFIX(launch_render_persistent)(const SceneGPU &sc, const CameraGPU &cam, const OutputGPU &out, bool count,
                                               unsigned long long *counters, uint32_t *queue, uint32_t blocks,
                                               uint32_t threshold, bool reset_queue, hipStream_t stream) {
    if (out.units == 0) return hipSuccess;
    if (reset_queue) {       // else the schedule kernel (schedule.hip) just reset the heads
        const hipError_t e = hipMemsetAsync(queue, 0, QUEUE_MAX_PARTS * QUEUE_STRIDE * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
    }
#define RT_LAUNCH(WPE, W, RAW) launch_persistent_wpe<WPE, W, RAW>(sc, cam, out, count, counters, queue, blocks, threshold, stream)
    RT_DISPATCH_INSTANCE(sc.wide, sc.raw_tris != nullptr, RT_LAUNCH);
#undef RT_LAUNCH
}

// the occupancy of the instance launch_render_persistent runs for (wide, raw): the persistent grid is sized from it
uint32_t RT_SUFFIX(persistent_blocks_per_cu)(uint32_t wide, bool raw) {
#define RT_OCC(WPE, W, RAW) blocks_per_cu_wpe<WPE, W, RAW>()
    RT_DISPATCH_INSTANCE(wide, raw, RT_OCC);
#undef RT_OCC
}
hipError_t RT_SUFFIX(launch_trace_rays)(const SceneGPU &sc, const float *rays, uint32_t n, rt_hit *hits,
                                        hipStream_t stream) {
    using namespace RT_SUFFIX(dev);
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(trace_rays_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, sc, rays, n, hits);
    return hipGetLastError();
}

hipError_t RT_SUFFIX(launch_box_test)(const float *boxes, const float *rays, const float *tmax, uint32_t n, uint32_t mode,
                                      uint8_t *hit, float *te, hipStream_t stream) {
    using namespace RT_SUFFIX(dev);
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(box_test_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, boxes, rays, tmax, n, mode, hit, te);
    return hipGetLastError();
}

#include "ray_query.hpp"

}  // namespace rtamd
