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

template <int ANY, int WPE, int WIDE, int RAW>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(WPE > 0 ? WPE : 1)))
void ray_query_kernel(SceneGPU sc, RayQueryGPU q) {
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
            if (!has && rank < take) {
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
            need = __ballot(!has);
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
            trav_init<XD_ALL>(T, *sc.tlas_root, o, d, q.tmax ? q.tmax[idx] : __builtin_huge_valf());
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
            }
            has = false;
        }
    }
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
