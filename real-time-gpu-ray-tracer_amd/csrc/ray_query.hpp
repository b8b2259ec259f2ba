// ray_query.hpp — rt_query_rays: closest-hit and occlusion queries for rays the caller holds in device memory.
// Included by trace_kernel.hip inside namespace rtamd, after the render kernels: compiled into all three flavours.
//
// ray_query_kernel is the render kernel's traversal without its shading: persistent waves (the grid is what stays
// resident, or fewer when the query is small), the scene region in LDS for quad trees, speculative while-while rounds
// (spec_round), and idle lanes refilled by ballot rank.  Rays are claimed in chunks of 64 consecutive indices.  The
// chunks are split into QUERY_PARTS contiguous bands, each with its own atomic head (RayQueryGPU::head, one 128 B line
// per band, zeroed on the call's stream before the launch): a wave drains the band of its XCD first and then steals
// from the others, and retires after QUERY_PARTS failed claims — every band it has seen dry stays dry.  (One head for
// the whole call saturates: 256 CUs ran at 55-68 claims/us whatever the rays, profiles/ray_query/README.md.)  No wave
// waits for another: the claim loop is bounded by the chunk
// count, the traversal by the trees.
//
// A ray's range is [TMIN, tmax[i]] with the reference's in_range semantics: the traversal starts with T.tmax =
// tmax[i] instead of +inf (trav_init's tmax argument), so every box and primitive test sees the caller's bound exactly
// as it sees the closest hit so far.  !(tmax > TMIN), NaN included, is a miss without traversal.
//
// Closest, tmax that grows: Range::inRange is closed with a 1e-6 window (Range.cuh:33-43), so a primitive up to 1e-6
// BEYOND the closest hit so far is accepted and becomes the new tmax: the range's upper end does not only shrink, and
// spec_round's argument that a decision taken ahead of a postponed leaf is made good by its re-test (traverse.hpp,
// above pop_next) needs that it does.  Where a box has a corner on a vertex several triangles share, its entry t
// equals the hit's t and "entry t < tmax" depends on the moment it is asked: a pop ahead of the leaf that raises tmax
// drops a node for good, and an entry pushed ahead of a leaf passes its re-test only because a later leaf raised tmax
// (DESIGN §3.3).  While no leaf phase leaves a lane's tmax larger than it found it, every such decision was taken with
// a tmax no smaller than the reference's and re-tested with one no larger, and the argument holds.  So a lane watches
// its tmax from round to round (a round runs at most one BLAS leaf per lane), and a ray whose tmax grew is traced
// again before it retires, by trav_step: every decision where the reference takes it, as rt_trace_rays.  That takes two
// surfaces within 1e-6 of each other, the farther tested later: about every other ray through a shared edge or vertex
// (tests/test_gpu_prim_edges.py), hardly any ray of a frame.
//
// ANY (occlusion): a lane stops after the first round in which it accepted a hit.  The any-hit traversal is a prefix
// of the closest traversal of the same instance, so occluded == (the closest query finds a hit).
//
// rt_query_camera: the same loop with a second ray source (CameraRays).  A refilled lane is handed a pixel of the
// caller's rectangle instead of a ray index and builds the pixel's camera ray in registers (query_camera_ray); at
// retirement it writes, next to t / hits, the ray and the hit material's albedo where asked.  A chunk of 64 is 64
// consecutive pixels of the rectangle, row-major (camera_item, below, has the 8x8 alternative).  Closest hit only.

namespace RT_SUFFIX(dev) {

// Lanes idle before a wave leaves traversal to retire and refill.  Swept over {16, 32, 40, 64} on incoherent rays (C2
// ambient-occlusion rays, closest-t): 0.216 / 0.221 / 0.220 / 0.191 ms (profiles/ray_query/threshold_sweep.json).
// Retiring a ray is a store, not a shade, so leaving early buys nothing: 64 — a wave refills once all its rays are
// done, and the early-leave test compiles away.  (-DRT_QUERY_THRESHOLD=n builds a variant for another sweep.)
#ifndef RT_QUERY_THRESHOLD
#define RT_QUERY_THRESHOLD 64
#endif
constexpr uint32_t QUERY_THRESHOLD = RT_QUERY_THRESHOLD;
static_assert(QUERY_THRESHOLD >= 1 && QUERY_THRESHOLD <= 64, "lanes of one wave");

// ---- the ray sources of the query loop
// BufferRays: ray q.rays[idx] with the range [TMIN, q.tmax[idx]] (rt_query_rays).
// CameraRays: work item -> pixel of the rectangle -> its camera ray over [TMIN, +inf) (rt_query_camera).
struct BufferRays { static constexpr bool CAMERA = false; };
struct CameraRays {
    static constexpr bool CAMERA = true;
    const CameraGPU &cam;
    const CameraQueryGPU &cq;
};

// The claim unit.  A chunk is 64 consecutive pixels of the rectangle in row-major order, as a buffer query's chunk is 64
// consecutive rays.  The alternative, a chunk = an 8x8 pixel block as the frame kernel's units are (blocks on the
// rectangle's right and top edges partial: the refill retries lanes handed an item outside it), measured slower on
// C2's 1080p primary rays: 0.162-0.175 ms against 0.152-0.153 ms, t only, and the buffer query orders the two the
// same way (profiles/camera_query/README.md).  -DRT_CAMERA_QUERY_BLOCKS=1 builds the 8x8 variant.
#ifndef RT_CAMERA_QUERY_BLOCKS
#define RT_CAMERA_QUERY_BLOCKS 0
#endif

// work item -> pixel (i, j) of the rectangle; false: outside it (8x8 blocks only)
__device__ __forceinline__ bool camera_item(const CameraQueryGPU &cq, uint32_t item, uint32_t &i, uint32_t &j) {
#if !RT_CAMERA_QUERY_BLOCKS
    j = item / cq.w; i = item - j * cq.w;
    return true;                                   // items are the rectangle's pixels: every item < w h is one
#else
    const uint32_t blk = item >> 6, l = item & 63u;          // blk is wave-uniform: a pool never leaves its chunk
    const uint32_t by = blk / cq.blocks_x, bx = blk - by * cq.blocks_x;
    i = bx * 8u + (l & 7u); j = by * 8u + (l >> 3);
    return i < cq.w && j < cq.h;
#endif
}

// a * b rounded on its own in every flavour.  Under -ffp-contract=fast (option "fast_math") the backend fuses any
// multiply with the add that follows it, `#pragma clang fp contract(off)` or not; it does not look through a
// canonicalize, which on a product is the identity and compiles to nothing.
__device__ __forceinline__ float mul_rn(float a, float b) { return __builtin_canonicalizef(a * b); }

// The camera ray of pixel (px, py).  FIRST: camera_ray(cam, px, py, 0, rng) after the render kernels' RNG init
// (trace_kernel.hip: pixel = pitch * py + px, rng.init(pixel ^ frame_seed, pixel)) — the ray rt_render starts the
// pixel's first path with.  Otherwise the ray through the pixel's centre: camera_ray() with ox = oy = 0, no RNG, no
// focus disk.  camera_ray()'s operations in its order, spelled out so that no flavour contracts or approximates any of
// them (under fast_math camera_ray() itself is contracted and its unit() is v_rsq): the reference's ray bit for bit
// in all three flavours, and camera_ray()'s own in EXACT and FAST (tests/test_gpu_camera_query.py holds it against
// the frame).
template <bool FIRST>
__device__ __forceinline__ void query_camera_ray(const CameraGPU &cam, uint32_t px, uint32_t py, f3 &o, f3 &d) {
    float fx = (float)px, fy = (float)py;
    o = ld3(cam.center);
    if (FIRST) {
        const uint32_t pixel = cam.pitch * py + px;                            // Kernel.cu:109
        Rng rng;
        rng.init((uint64_t)pixel ^ cam.frame_seed, pixel);                      // Kernel.cu:114
        const float u0 = rng.uniform();
        const float u1 = rng.uniform();
        fx = fx + (mul_rn(u0, cam.recip_sqrt) - 0.5f);                          // sample 0: cell (0, 0), 0.0f + u = u
        fy = fy + (mul_rn(u1, cam.recip_sqrt) - 0.5f);
        if (cam.focus_radius > 0.0f) {                                         // random_plane_vector (Vec3.cu:29-36)
            float x, y;
            do {
                x = -1.0f + mul_rn(2.0f, rng.uniform());
                y = -1.0f + mul_rn(2.0f, rng.uniform());
            } while (mul_rn(x, x) + mul_rn(y, y) > mul_rn(cam.focus_radius, cam.focus_radius));
            o.x = (o.x + mul_rn(cam.cu[0], x)) + mul_rn(cam.cv[0], y);
            o.y = (o.y + mul_rn(cam.cu[1], x)) + mul_rn(cam.cv[1], y);
            o.z = (o.z + mul_rn(cam.cu[2], x)) + mul_rn(cam.cv[2], y);
        }
    }
    const float vx = ((cam.pixel_origin[0] + mul_rn(cam.dx[0], fx)) + mul_rn(cam.dy[0], fy)) - o.x;
    const float vy = ((cam.pixel_origin[1] + mul_rn(cam.dx[1], fx)) + mul_rn(cam.dy[1], fy)) - o.y;
    const float vz = ((cam.pixel_origin[2] + mul_rn(cam.dx[2], fx)) + mul_rn(cam.dy[2], fy)) - o.z;
    float l2 = 0.0f;
    l2 += mul_rn(vx, vx); l2 += mul_rn(vy, vy); l2 += mul_rn(vz, vz);
    const float f = 1.0f / sqrtf(l2);                                          // Vec3.cuh:129-137
    d = mk(vx * f, vy * f, vz * f);
}

// The loop of both kernels.  (A device function, not a template parameter of ray_query_kernel: the camera source's
// kernel arguments then stay out of the buffer kernels, whose code is the parent's: profiles/camera_query/.)
template <int ANY, int WIDE, int RAW, class SRC>
__device__ __forceinline__ void ray_query_body(const SceneGPU &sc, const RayQueryGPU &q, const SRC &src) {
    static_assert(!(ANY && SRC::CAMERA), "camera queries are closest-hit");
    __shared__ unsigned long long lds_stack[LDS_DEPTH][BLOCK];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
#if !RT_EXACT
    if constexpr (WIDE != 0) lds_scene_fill(sc);
#endif
    __syncthreads();                              // once, before any wave leaves for the queue
    const TreeRoot root = uniform_root<WIDE != 0>(sc);

    Trav T;
    T.stk.lds = (LdsU2 *)&lds_stack[0][tid];
    T.tracing = false;
    T.found = false;
    alignas(16) SEnt spill[SPILL_DEPTH];
    LaneCount cnt = {};
    PhaseCycles pc = {};
    uint32_t steps = 0;

    bool has = false;                  // lane owns a ray
    uint32_t idx = 0;                  // its index (< q.n whenever has)
    float seen = 0.0f;                 // its tmax after the last round
    bool grew = false;                 // a leaf phase raised it: the ray is traced again in the reference's order
    uint32_t pool_next = 0, pool_end = 0;     // wave-uniform: the claimed chunk's unassigned rays
    bool exhausted = false;                   // wave-uniform
    const uint32_t chunks = (q.n >> 6) + ((q.n & 63u) ? 1u : 0u);     // <= 2^26
    uint32_t part = xcc_id() % QUERY_PARTS, tried = 0;                // wave-uniform: the band claimed from

    for (;;) {
        // ---- refill idle lanes from the wave's chunk / the head
        uint64_t need = __ballot(!has);
        while (need && !exhausted) {
            if (pool_next >= pool_end) {
                const uint32_t c0 = chunks * part / QUERY_PARTS, c1 = chunks * (part + 1u) / QUERY_PARTS;
                uint32_t b = 0;
                if (lane == 0) b = atomicAdd(q.head + part * QUEUE_STRIDE, 1u);
                b = __builtin_amdgcn_readfirstlane(b);
                if (b >= c1 - c0) {                                   // the band is dry: the next one
                    if (++tried >= QUERY_PARTS) {
                        exhausted = true;
                        break;
                    }
                    part = part + 1u == QUERY_PARTS ? 0u : part + 1u;
                    continue;
                }
                pool_next = (c0 + b) << 6;                            // chunk c0 + b < chunks, so < q.n
                pool_end = pool_next + min(64u, q.n - pool_next);     // <= q.n: the last chunk may be partial
            }
            const uint32_t take = min((uint32_t)__popcll(need), pool_end - pool_next);
            const uint32_t rank = __popcll(need & ((1ull << lane) - 1ull));
            if constexpr (SRC::CAMERA) {
                uint32_t i, j;
                if (!has && rank < take && camera_item(src.cq, pool_next + rank, i, j)) {
                    has = true;
                    idx = j * src.cq.w + i;                           // < w h <= 2^32 - 1 (the frame's pixels)
                    f3 o, d;
                    if (src.cq.first_sample) query_camera_ray<true>(src.cam, src.cq.x0 + i, src.cq.y0 + j, o, d);
                    else query_camera_ray<false>(src.cam, src.cq.x0 + i, src.cq.y0 + j, o, d);
                    seen = __builtin_huge_valf();
                    grew = false;
                    if (src.cq.trace) {
                        trav_init<XBOX(WIDE)>(T, root, o, d);
                    } else {                                          // rays only: retired as generated
                        T.wr.o = o; T.wr.d = d;
                        T.tracing = false;
                        T.found = false;
                    }
                }
            } else if (!has && rank < take) {
                has = true;
                idx = pool_next + rank;
                const float *r = q.rays + 6 * (size_t)idx;
                const f3 o = mk(r[0], r[1], r[2]);
                const f3 d = mk(r[3], r[4], r[5]);
                const float tmax = q.tmax ? q.tmax[idx] : __builtin_huge_valf();
                seen = tmax;
                grew = false;
                if (tmax > TMIN) {
                    trav_init<XBOX(WIDE)>(T, root, o, d, tmax);
                } else {                                              // empty range (NaN included): a miss
                    T.tracing = false;
                    T.found = false;
                }
            }
            pool_next += take;
            need = __ballot(!has);                // (camera: lanes handed an item outside the rectangle retry)
        }
        if (!__any(has)) break;                   // only when exhausted: the loop above fills every lane otherwise
        // ---- traverse while enough lanes are busy
        for (;;) {
            if (__ballot(T.tracing) == 0) break;
            if constexpr (QUERY_THRESHOLD < 64) {
                const uint64_t want = __ballot(!T.tracing && (has || !exhausted));
                if ((uint32_t)__popcll(want) >= QUERY_THRESHOLD) break;
            }
            spec_round<false, WIDE>(T, sc, spill, cnt, pc, steps, false, 0u);
            if (!ANY) {
                grew = grew || T.tmax > seen;
                seen = T.tmax;
            }
            if (ANY && T.tracing && T.found) {    // occlusion: the first accepted hit ends the ray
                T.tracing = false;
                T.cur = REF_NONE;
                T.pleaf = REF_NONE;
                T.stk.clear();
            }
        }
        // ---- retire the lanes whose ray finished
        if (!ANY && has && !T.tracing && grew) {      // (grew: the range was not empty, the ray was traversed)
            const f3 o = T.wr.o, d = T.wr.d;
            if constexpr (SRC::CAMERA) trav_init<XD_ALL>(T, *sc.tlas_root, o, d);
            else trav_init<XD_ALL>(T, *sc.tlas_root, o, d, q.tmax ? q.tmax[idx] : __builtin_huge_valf());
            while (T.tracing) trav_step<false, XD_ALL>(T, sc, spill, cnt);
        }
        if (has && !T.tracing) {
            if (ANY) {
                q.occluded[idx] = T.found ? 1 : 0;
            } else {
                if (q.t) q.t[idx] = T.found ? T.hit.t : __builtin_huge_valf();
                if (q.hits) {                     // the record rt_trace_rays writes (trace_rays_kernel: keep the two alike)
                    rt_hit r;
                    if (T.found) {
                        const Hit h = T.hit;
                        const Surface s = finalize<WIDE != 0, RAW>(sc, T.wr.o, T.wr.d, h);
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
                    q.hits[idx] = r;
                }
                if constexpr (SRC::CAMERA) {      // plain stores, like the records above
                    if (src.cq.rays) {
                        float *r = src.cq.rays + 6 * (size_t)idx;
                        r[0] = T.wr.o.x; r[1] = T.wr.o.y; r[2] = T.wr.o.z;
                        r[3] = T.wr.d.x; r[4] = T.wr.d.y; r[5] = T.wr.d.z;
                    }
                    if (src.cq.albedo) {          // the hit's material slot (rough or metal); the background on a miss
                        f3 a = ld3(src.cam.background);
                        if (T.found) {
                            const uint32_t mi = hit_material<WIDE != 0, RAW>(sc, T.hit) & ~MAT_METAL_BIT;
                            const float4 m = reinterpret_cast<const float4 *>(sc.materials)[mi];
                            a = mk(m.x, m.y, m.z);
                        }
                        float *c = src.cq.albedo + 3 * (size_t)idx;
                        c[0] = a.x; c[1] = a.y; c[2] = a.z;
                    }
                }
            }
            has = false;
        }
    }
}

template <int ANY, int WPE, int WIDE, int RAW>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(WPE > 0 ? WPE : 1)))
void ray_query_kernel(SceneGPU sc, RayQueryGPU q) {
    ray_query_body<ANY, WIDE, RAW>(sc, q, BufferRays{});
}

// rt_query_camera: closest hit only
template <int WPE, int WIDE, int RAW>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(WPE > 0 ? WPE : 1)))
void camera_query_kernel(SceneGPU sc, RayQueryGPU q, CameraGPU cam, CameraQueryGPU cq) {
    ray_query_body<0, WIDE, RAW>(sc, q, CameraRays{cam, cq});
}

}  // namespace dev

namespace {
template <int WPE, int WIDE, int RAW>
hipError_t launch_ray_query_wpe(const SceneGPU &sc, const RayQueryGPU &q, bool any_hit, uint32_t cus, hipStream_t stream) {
    using namespace RT_SUFFIX(dev);
    // the grid: what stays resident, or one wave per chunk of 64 rays when that is fewer (65 rays: one block)
    // (asked once per instance and mode: a property of the kernel's registers and LDS, the same on every device)
    static std::atomic<int> cached[2];           // zero-initialised; threads that race store the same value
    int per_cu = cached[any_hit ? 1 : 0].load(std::memory_order_relaxed);
    if (per_cu == 0) {
        const hipError_t oe = any_hit
            ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ray_query_kernel<1, WPE, WIDE, RAW>, BLOCK, 0)
            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ray_query_kernel<0, WPE, WIDE, RAW>, BLOCK, 0);
        if (oe != hipSuccess || per_cu < 1) per_cu = 1;
        cached[any_hit ? 1 : 0].store(per_cu, std::memory_order_relaxed);
    }
    const uint32_t chunks = (q.n >> 6) + ((q.n & 63u) ? 1u : 0u);
    const uint32_t need = (chunks + (BLOCK / 64) - 1) / (BLOCK / 64);
    const uint32_t cap = (cus ? cus : 1u) * (uint32_t)per_cu;
    const dim3 grid(cap < need ? cap : need);
    if (any_hit)
        hipLaunchKernelGGL((ray_query_kernel<1, WPE, WIDE, RAW>), grid, dim3(BLOCK), 0, stream, sc, q);
    else
        hipLaunchKernelGGL((ray_query_kernel<0, WPE, WIDE, RAW>), grid, dim3(BLOCK), 0, stream, sc, q);
    return hipGetLastError();
}
}  // namespace

namespace {
template <int WPE, int WIDE, int RAW>
hipError_t launch_camera_query_wpe(const SceneGPU &sc, const RayQueryGPU &q, const CameraGPU &cam, const CameraQueryGPU &cq,
                                   uint32_t cus, hipStream_t stream) {
    using namespace RT_SUFFIX(dev);
    static std::atomic<int> cached;              // as launch_ray_query_wpe
    int per_cu = cached.load(std::memory_order_relaxed);
    if (per_cu == 0) {
        const hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, camera_query_kernel<WPE, WIDE, RAW>, BLOCK, 0);
        if (oe != hipSuccess || per_cu < 1) per_cu = 1;
        cached.store(per_cu, std::memory_order_relaxed);
    }
    const uint32_t chunks = (q.n >> 6) + ((q.n & 63u) ? 1u : 0u);
    const uint32_t need = (chunks + (BLOCK / 64) - 1) / (BLOCK / 64);
    const uint32_t cap = (cus ? cus : 1u) * (uint32_t)per_cu;
    const dim3 grid(cap < need ? cap : need);
    hipLaunchKernelGGL((camera_query_kernel<WPE, WIDE, RAW>), grid, dim3(BLOCK), 0, stream, sc, q, cam, cq);
    return hipGetLastError();
}
}  // namespace

// rt_query_camera's launch: the rectangle of cq (x0, y0, w, h; w h > 0, inside cam's frame) on the instance of the
// scene's kind.  q carries t, hits and the band heads (zeroed here, as below); the item count and the block grid are
// set here, where the claim unit is known.
hipError_t RT_SUFFIX(launch_camera_query)(const SceneGPU &sc, const CameraGPU &cam, RayQueryGPU q, CameraQueryGPU cq,
                                          uint32_t cus, hipStream_t stream) {
    cq.blocks_x = (cq.w + 7u) / 8u;
#if !RT_CAMERA_QUERY_BLOCKS
    q.n = cq.w * cq.h;
#else
    q.n = cq.blocks_x * ((cq.h + 7u) / 8u) * 64u;         // the caller keeps it below 2^32
#endif
    if (q.n == 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(q.head, 0, QUERY_PARTS * QUEUE_STRIDE * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
#define RT_QUERY(WPE, W, RAW) launch_camera_query_wpe<WPE, W, RAW>(sc, q, cam, cq, cus, stream)
    RT_DISPATCH_INSTANCE(sc.wide, sc.raw_tris != nullptr, RT_QUERY);
#undef RT_QUERY
}

// One instance per scene kind, as launch_render_persistent: EXACT runs the binary pairs, FAST / fastmath the scene's
// (wide, raw) instance.  The band heads at q.head are zeroed on `stream` first: the caller provisions heads no other
// query in flight uses.
hipError_t RT_SUFFIX(launch_ray_query)(const SceneGPU &sc, const RayQueryGPU &q, bool any_hit, uint32_t cus,
                                       hipStream_t stream) {
    if (q.n == 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(q.head, 0, QUERY_PARTS * QUEUE_STRIDE * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
#define RT_QUERY(WPE, W, RAW) launch_ray_query_wpe<WPE, W, RAW>(sc, q, any_hit, cus, stream)
    RT_DISPATCH_INSTANCE(sc.wide, sc.raw_tris != nullptr, RT_QUERY);
#undef RT_QUERY
}
