// shade.hpp — what happens to a finished traversal: hit finalisation, the grid kernel's path loop, camera rays, the
// work-item -> pixel map, the pixel write, and the wave-level counter / unit-cost bookkeeping.
// Includable only from trace_kernel.hip, once, inside namespace rtamd::RT_SUFFIX(dev), after traverse.hpp.

// Record fields the shading needs (HitRecord, BasicTypes.cuh:19-31), world space.
struct Surface { f3 p, n; uint32_t material; uint32_t orig; uint32_t member; };   // member: group BLAS (option "group"): instance + 1

// Recompute the hit point / normal of the closest hit exactly as the primitive hit function and
// Instance::hit (Instance.cu:41-45) would have stored them.
// RAW: where a hit triangle's normals / material / caller index come from — 0 its TriCold record, 1 the caller's
// triangle (SceneGPU::raw_tris, GPU-built BLASes without cold records), 2 whichever the scene has (a runtime branch).
// The persistent kernel is instantiated per scene kind (0 / 1): with the branch inlined, host-built scenes' kernel
// lost 2 VGPRs to spills and ~1 % per frame (profiles/r04/cold_records/).
template <bool LDSS = false, int RAW = 2>
__device__ __forceinline__ Surface finalize(const SceneGPU &sc, const f3 &wo, const f3 &wd, const Hit &h) {
#if !RT_EXACT
    const InstCold IC = LDSS ? lds_or_global(sc.lds_icold, sc.inst_cold, h.inst) : sc.inst_cold[h.inst];
#else
    const InstCold &IC = sc.inst_cold[h.inst];
#endif
    f3 lo, ld;
#if !RT_EXACT
    if (LDSS) {
        const InstRec I = load_inst<true>(sc, h.inst);
        // (spec_leaf_phase unpacks the record the same way: a shared helper changed the diagnostic FAST build's code)
        const float inv[12] = {I.i0.x, I.i0.y, I.i0.z, I.i0.w, I.i1.x, I.i1.y, I.i1.z, I.i1.w,
                               I.i2.x, I.i2.y, I.i2.z, I.i2.w};
        lo = xf_point(inv, wo); ld = xf_vector(inv, wd);
    } else
#endif
    {
        const InstHot &I = sc.inst_hot[h.inst];
        lo = xf_point(I.inv, wo); ld = xf_vector(I.inv, wd);
    }
    const f3 p = add(lo, scl(ld, h.t));                                        // Ray::at (Ray.cuh:18-20)
    f3 n;
    Surface s;
    if (h.ptype == RT_PRIM_TRIANGLE) {                                         // Triangle.cu:40-42
        f3 n0, n1, n2;
        if (RAW == 1 || (RAW == 2 && sc.raw_tris)) {   // GPU-built BLAS without cold records (layout.hpp SceneGPU)
            const TriHot &H = sc.tri_hot[h.slot];
            s.orig = __float_as_uint(H.pad0);
            s.member = __float_as_uint(H.pad1);
            const rt_triangle &R = sc.raw_tris[s.orig];
            if (R.has_normals) {
                n0 = mk(R.normal[0].x, R.normal[0].y, R.normal[0].z);
                n1 = mk(R.normal[1].x, R.normal[1].y, R.normal[1].z);
                n2 = mk(R.normal[2].x, R.normal[2].y, R.normal[2].z);
            } else {
                n0 = tri_face_normal(ld3(H.e1), ld3(H.e2)); n1 = n0; n2 = n0;
            }
            s.material = R.material_type == RT_MAT_ROUGH ? R.material_index
                                                         : ((sc.rough_count + R.material_index) | MAT_METAL_BIT);
        } else {
            const TriCold &T = sc.tri_cold[h.slot];
            n0 = ld3(T.n0); n1 = ld3(T.n1); n2 = ld3(T.n2);
            s.material = T.material; s.orig = T.orig_index; s.member = T.pad;
        }
        const f3 nn = unit(add(add(scl(n0, (1.0f - h.u) - h.v), scl(n1, h.u)), scl(n2, h.v)));
        n = dot(ld, nn) < 0.0f ? nn : neg(nn);
    } else if (h.ptype == RT_PRIM_SPHERE) {                                    // Sphere.cu:37-39
#if !RT_EXACT
        const SphereHot S = LDSS ? lds_or_global(sc.lds_sph_hot, sc.sph_hot, h.slot) : sc.sph_hot[h.slot];
        const PrimCold C = LDSS ? lds_or_global(sc.lds_sph_cold, sc.sph_cold, h.slot) : sc.sph_cold[h.slot];
#else
        const SphereHot &S = sc.sph_hot[h.slot];
        const PrimCold &C = sc.sph_cold[h.slot];
#endif
        const f3 outward = unit(sub(p, ld3(S.center)));
        n = dot(ld, outward) < 0.0f ? outward : neg(outward);
        s.material = C.material; s.orig = C.orig_index; s.member = 0u;
    } else {                                                                   // Parallelogram.cu:42-43
#if !RT_EXACT
        const float4 qn4 = LDSS && sc.lds_q_hot != LDS_NONE ? lds_scene[sc.lds_q_hot + times<LDS_QPRIM_F4>(h.slot)]
                                                              : reinterpret_cast<const float4 *>(sc.quad_hot + h.slot)[0];
        const PrimCold C = LDSS ? lds_or_global(sc.lds_q_cold, sc.quad_cold, h.slot) : sc.quad_cold[h.slot];
        const f3 qn = mk(qn4.x, qn4.y, qn4.z);
#else
        const QuadHot &Q = sc.quad_hot[h.slot];
        const PrimCold &C = sc.quad_cold[h.slot];
        const f3 qn = ld3(Q.n);
#endif
        n = dot(ld, qn) < 0.0f ? qn : neg(qn);
        s.material = C.material; s.orig = C.orig_index; s.member = 0u;
    }
    s.p = xf_point(IC.fwd, p);
    s.n = unit(xf_vector(IC.nrm, n));
    return s;
}

// The closest hit's material word alone (Surface::material), from the records finalize takes it from: what a path's
// last segment needs of a rough surface, whose point, normal and scattered direction nobody reads.
template <bool LDSS = false, int RAW = 2>
__device__ __forceinline__ uint32_t hit_material(const SceneGPU &sc, const Hit &h) {
    if (h.ptype == RT_PRIM_TRIANGLE) {
        if (RAW == 1 || (RAW == 2 && sc.raw_tris)) {
            const rt_triangle &R = sc.raw_tris[__float_as_uint(sc.tri_hot[h.slot].pad0)];
            return R.material_type == RT_MAT_ROUGH ? R.material_index : ((sc.rough_count + R.material_index) | MAT_METAL_BIT);
        }
        return sc.tri_cold[h.slot].material;
    }
#if !RT_EXACT
    if (LDSS) {
        if (h.ptype == RT_PRIM_SPHERE) return lds_or_global(sc.lds_sph_cold, sc.sph_cold, h.slot).material;
        return lds_or_global(sc.lds_q_cold, sc.quad_cold, h.slot).material;
    }
#endif
    return (h.ptype == RT_PRIM_SPHERE ? sc.sph_cold : sc.quad_cold)[h.slot].material;
}

template <bool COUNT>
__device__ f3 ray_color(const SceneGPU &sc, const CameraGPU &cam, f3 o, f3 d, Rng &rng, Trav &T, SEnt *spill,
                        LaneCount &cnt, uint32_t &rays) {                      // Kernel.cu:6-103
    f3 result = mk(1.0f, 1.0f, 1.0f);
    for (uint32_t depth = 0; depth < cam.depth; depth++) {
        Hit h;
        rays++;
        if (trace<COUNT, XD_ALL>(sc, o, d, h, T, spill, cnt)) {
            if (COUNT) cnt.hits++;
            const Surface s = finalize(sc, o, d, h);
            const float4 m = reinterpret_cast<const float4 *>(sc.materials)[s.material & ~MAT_METAL_BIT];
            const f3 albedo = mk(m.x, m.y, m.z);
            f3 out;
            if (!(s.material & MAT_METAL_BIT)) {                               // Rough.cuh:14-29
                out = add(s.n, random_space_vector(rng));
                if (f_eq(dot(out, out), FZERO * FZERO)) out = s.n;
            } else {                                                           // Metal.cuh:15-32
                out = unit(sub(d, scl(s.n, 2.0f * dot(d, s.n))));
                if (m.w > 0.0f) out = add(out, scl(random_space_vector(rng), m.w));
                if (!(dot(out, s.n) > 0.0f)) return result;                    // absorbed: throughput (Kernel.cu:85-87)
            }
            o = s.p; d = out;
            result = mul(result, albedo);
        } else {
            result = mul(result, ld3(cam.background));
            break;
        }
    }
    return result;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// a wave's work counters into rt_counters: one atomic per wave per counter
template <bool COUNT>
__device__ __forceinline__ void flush_counts(unsigned long long *counters, const LaneCount &cnt, int lane) {
    if (COUNT) {
        const uint32_t a = wave_sum(cnt.pairs), b = wave_sum(cnt.tri), c = wave_sum(cnt.sq), d = wave_sum(cnt.inst),
                       e = wave_sum(cnt.overflow), f = wave_sum(cnt.quad), g = wave_sum(cnt.hits);
        if (lane == 0) {
            atomicAdd(&counters[CNT_PAIRS], (unsigned long long)a);
            atomicAdd(&counters[CNT_TRI], (unsigned long long)b);
            atomicAdd(&counters[CNT_SPHQUAD], (unsigned long long)c);
            atomicAdd(&counters[CNT_INST], (unsigned long long)d);
            atomicAdd(&counters[CNT_OVERFLOW], (unsigned long long)e);
            atomicAdd(&counters[CNT_QUAD], (unsigned long long)f);
            atomicAdd(&counters[CNT_HITS], (unsigned long long)g);
        }
    }
}

// XCD (XCC) of the executing wave, 0..7, and the raw HW_ID register (CU / SE / SIMD of the wave).
__device__ __forceinline__ uint32_t xcc_id() {
    uint32_t v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(v));
    return v;
}
__device__ __forceinline__ uint32_t hw_id() {
    uint32_t v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(v));
    return v;
}

// work item of the persistent kernel's queue -> pixel (px, py) and output index oi; false: outside the frame
__device__ __forceinline__ bool map_item(const OutputGPU &out, const CameraGPU &cam, uint32_t item,
                                         uint32_t &px, uint32_t &py, uint32_t &oi) {
    // multiply-shift divisions (FastDiv, host-precomputed): this runs per refilled lane and per sample
    const uint32_t wunit = item >> 6, l = item & 63u;
    if (out.tile_count == 0) {
        const uint32_t uy = out.div_units_x.div(wunit), ux = wunit - uy * out.units_x;
        px = ux * 8 + (l & 7); py = uy * 8 + (l >> 3);
        oi = py * cam.width + px;
    } else {
        const uint32_t k = out.div_upt.div(wunit), r = wunit - k * out.div_upt.d;
        const uint32_t t = out.tile_rank + k * out.tile_count;
        const uint32_t ry = out.div_upr.div(r), rx = r - ry * out.div_upr.d;
        const uint32_t lx = rx * 8 + (l & 7), ly = ry * 8 + (l >> 3);
        const uint32_t ty = out.div_tiles_x.div(t), tx = t - ty * out.tiles_x;
        px = tx * out.tile_w + lx;
        py = ty * out.tile_h + ly;
        oi = k * out.tile_w * out.tile_h + ly * out.tile_w + lx;
    }
    return px < cam.width && py < cam.height;
}

// Camera ray of sample `sample` of pixel (px, py) (Kernel.cu:119-135), consuming the pixel's RNG.
// Evaluated without FMA contraction in both builds, so FAST and EXACT start every path from the same
// camera ray.  (The grid kernel's own camera-ray code in render_kernel is not a copy of this: it follows its build's
// contraction, so under fast_math its rays may differ in the last bit.)
__device__ __forceinline__ void camera_ray(const CameraGPU &cam, uint32_t px, uint32_t py, uint32_t sample, Rng &rng,
                                           f3 &o, f3 &d) {
#pragma clang fp contract(off)
    const uint32_t si = sample / cam.sqrt_s, sj = sample % cam.sqrt_s;
    const float ox = (((float)sj + rng.uniform()) * cam.recip_sqrt) - 0.5f;
    const float oy = (((float)si + rng.uniform()) * cam.recip_sqrt) - 0.5f;
    const f3 sp = add(add(ld3(cam.pixel_origin), scl(ld3(cam.dx), (float)px + ox)), scl(ld3(cam.dy), (float)py + oy));
    o = ld3(cam.center);
    if (cam.focus_radius > 0.0f) {
        const f3 dv = random_plane_vector(rng, cam.focus_radius);
        o = add(add(o, scl(ld3(cam.cu), dv.x)), scl(ld3(cam.cv), dv.y));
    }
    d = unit(sub(sp, o));
}

// the persistent kernel's pixel write (render_kernel has the same code inline: calling this there changed its code)
__device__ __forceinline__ void write_pixel(const OutputGPU &out, uint32_t oi, f3 result) {
    if (out.rgb) {
        out.rgb[3 * (size_t)oi + 0] = result.x;
        out.rgb[3 * (size_t)oi + 1] = result.y;
        out.rgb[3 * (size_t)oi + 2] = result.z;
    }
    const float cr = fminf(fmaxf(sqrtf(result.x), 0.0f), 0.999f);       // Color3::castToUchar4, gamma 2 (Color3.cuh:99-114)
    const float cg = fminf(fmaxf(sqrtf(result.y), 0.0f), 0.999f);
    const float cb = fminf(fmaxf(sqrtf(result.z), 0.0f), 0.999f);
    const uint32_t packed = (uint32_t)(uint8_t)(256.0f * cr) | ((uint32_t)(uint8_t)(256.0f * cg) << 8) |
                            ((uint32_t)(uint8_t)(256.0f * cb) << 16) | (255u << 24);
    reinterpret_cast<uint32_t *>(out.rgba)[oi] = packed;
}

// Option "reorder": a unit's cost for the next launch's claim order (schedule.hip) is the traversal
// work of its 64 pixels (interior steps + leaf phases + 1 per pixel).  A wave's lanes refill from
// the unit it claimed, so a unit's total work is the time it holds a wave; units over the particle
// cluster hold one for up to ~0.4 ms against ~20 us for a sky unit (C2, measured), and the launch
// ends with whichever wave claimed the last heavy units.
// A lane keeps one pending (unit, cost) sum and flushes it with a no-return atomic just before the
// wave's next claim atomic, whose returned value the wave waits for anyway, so the flush adds no wait of
// its own (vector memory counters retire in order: a returning atomic's wait also covers the stores and
// atomics issued before it).  A lane that finishes a pixel of another unit before that flushes its old
// sum at once.  Measured: per-shade-step atomics made each next node load wait for their memory-side
// completion (~11 % of C2 throughput, profiles/r02_ab_unit_cost.jsonl).
// a unit's recorded cost is the sum over its paths (round 3's "cost_max", 64 x its longest path, ordered C2 slower)
__device__ __forceinline__ void unit_cost_flush(uint32_t *cost, uint32_t unit, uint32_t c) { atomicAdd(cost + unit, c); }
// the pending sums of the lanes in `fin`: one atomic per distinct unit
__device__ __forceinline__ void unit_cost_add(uint32_t *cost, bool fin, uint32_t unit, uint32_t c) {
    uint64_t m = __ballot(fin);
    while (m) {
        const uint32_t first = (uint32_t)__builtin_ctzll(m);
        const uint32_t u = __shfl(unit, (int)first, 64);
        const bool mine = fin && unit == u;
        const uint32_t x = wave_sum(mine ? c : 0u);
        if ((threadIdx.x & 63u) == first) unit_cost_flush(cost, u, x);
        m &= ~(uint64_t)__ballot(mine);
    }
}
