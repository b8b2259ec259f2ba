// box.hpp — box decisions: the reference's slab, the FAST kernels' conservative reciprocal slabs and their exact re-takes.
// Includable only from trace_kernel.hip, once, inside namespace rtamd::RT_SUFFIX(dev), after vecmath.hpp.
//
// Conservative slabs (FAST; the contract tests/test_gpu_box.py pins, not a build option): the interval [lo, hi] a box
// test computes with reciprocal-FMA planes is widened by a bound on its distance from the reference's (mn - q) / d
// interval before the lo < hi test (and a popped entry's lo before its lo < tmax re-test), so a FAST cull never rejects
// a box the reference's slab accepts — but for a parallel axis (|d| < 1e-6) whose origin lies exactly on a face of the
// slab, which planes cannot widen (the reference keeps q == min / max, BoundingBox.cu:47; the FAST planes there are the
// rounding residual of o / d): the exact-decision instances (XD_ALL, XBOX) re-take every box test of a ray with a
// parallel axis with the reference's slab; the others keep the exception.  Entries keep the unwidened lo, so children
// are still ordered by it.
//
// Exact re-takes (FAST; tests/test_gpu_parity_full.py, not a build option): box decisions that lie inside the slabs'
// error margin (and every box test of a ray with a parallel axis) are re-taken with the reference's division slab, as
// are the pair-order comparisons of two entry t's inside the margin: on the reference's trees the traversal takes the
// reference's decisions.
//
// The persistent kernel's traversal modes (SceneGPU::wide): 0 binary node pairs, 1 greedy quads by entry t (host SAH
// trees), 2 two-level quads in pair order (GPU-built trees), 3 the same with exact decisions (the reference's trees, and
// GPU-built trees with option "exact_decisions").
// Exact-decision level of a traversal instance (template argument XB):
//   XD_CULL: conservative culls only (modes 1 and 2).  One documented exception to "a FAST cull never rejects a box the
//            reference keeps": a ray with a parallel axis (|d| < 1e-6) whose origin lies exactly on a face of that
//            axis's slab (the reference keeps q == min / max, BoundingBox.cu:47; reciprocal planes cannot represent it;
//            tests/test_gpu_box.py pins the misses to exactly that case).  Re-taking such rays' decisions in modes 1 / 2
//            (round 6) cost C2 4.4 % and C3 2.5 % per frame through register pressure alone;
//   XD_ALL : every decision inside the slabs' error margin, every box test of a ray with a parallel axis and (pair
//            order) every comparison of two entry t's inside the margin re-taken with the reference's slab: the traversal
//            takes the reference's decisions; and every leaf that is hit gets the reference's entry t (slab_ref_near), so
//            that its re-test at the pop is the reference's too (traverse.hpp, pop_keep).  The binary pairs and mode 3 —
//            FAST then equals EXACT on the same trees (tests/test_gpu_parity_full.py: the reference's trees, and C5's
//            benched LBVH trees with "exact_decisions"; tests/test_gpu_xform_edges.py: surfaces 1e-6 apart).
//            For mode 2 by default it cost C5 +34 % per frame (sibling boxes' entry t's often tie exactly:
//            profiles/r06/exact_decisions/).
constexpr int XD_CULL = 0, XD_ALL = 2;
#define XBOX(W) (((W) == 0 || (W) == 3) ? XD_ALL : XD_CULL)

// ---- rays ---------------------------------------------------------------------------
struct RayP {
    f3 o, d;
#if !RT_EXACT
    f3 inv, oinv;      // 1/d and o/d for one-FMA slab planes
    float pad;         // the absolute part of a plane distance's error bound: 2^-22 max |o/d| over the non-parallel
                       // axes; negative (sign bit set) when an axis is parallel (|d| < 1e-6)
#endif
};
template <int XB = XD_CULL>
__device__ __forceinline__ void prep(RayP &r) {
#if !RT_EXACT
    // |d| < 1e-6 (the reference's parallel-axis threshold, BoundingBox.cu:44-50) -> +-1e-20: the plane distances
    // of that axis are +-1e20 * (face - o), so the axis rejects the box exactly when o lies outside the slab and
    // constrains nothing otherwise — the reference's parallel branch, with finite reciprocals (never 0 * inf)
    const auto nz = [](float x) { return fabsf(x) < FZERO ? copysignf(1e-20f, x) : x; };
    r.inv = mk(rcp(nz(r.d.x)), rcp(nz(r.d.y)), rcp(nz(r.d.z)));
    r.oinv = mk(r.o.x * r.inv.x, r.o.y * r.inv.y, r.o.z * r.inv.z);
    {   // fmaf(b, inv, -oinv) differs from (b - o) / d by <= 2^-24 |o / d| (oinv's rounding) + ~2^-21.7 |t| (the
        // reciprocal's 1 ulp, the fma's and the reference's roundings); parallel axes only decide inside / outside
        const float px = fabsf(r.d.x) < FZERO ? 0.0f : fabsf(r.oinv.x);
        const float py = fabsf(r.d.y) < FZERO ? 0.0f : fabsf(r.oinv.y);
        const float pz = fabsf(r.d.z) < FZERO ? 0.0f : fabsf(r.oinv.z);
        const float pad = 0x1p-22f * fmaxf(px, fmaxf(py, pz));
        r.pad = pad;
        if (XB != XD_CULL) {   // the exact-decision instances re-take every box test of a ray with a parallel axis
            const bool par = fabsf(r.d.x) < FZERO || fabsf(r.d.y) < FZERO || fabsf(r.d.z) < FZERO;
            r.pad = par ? -pad : pad;
        }
    }
#else
    (void)r;
#endif
}

// BoundingBox::hit (BoundingBox.cu:34-72), reference arithmetic.  b = {xmin,xmax,ymin,ymax,zmin,zmax}
__device__ __forceinline__ bool slab_ref(const float *b, const f3 &o, const f3 &d, float tmin, float tmax, float &te) {
    float cmin = tmin, cmax = tmax;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float q = comp(o, a), dd = comp(d, a), mn = b[2 * a], mx = b[2 * a + 1];
        if (fabsf(dd) < FZERO) {
            if (q < mn || q > mx) return false;
            continue;
        }
        const float t1 = fdiv(mn - q, dd);
        const float t2 = fdiv(mx - q, dd);
        if (t1 < t2) {
            if (t1 > cmin) cmin = t1;
            if (t2 < cmax) cmax = t2;
        } else {
            if (t2 > cmin) cmin = t2;
            if (t1 < cmax) cmax = t1;
        }
        if (cmin >= cmax) return false;
    }
    te = cmin;
    return true;
}

#if !RT_EXACT
// The reference's slab as one out-of-line copy for the FAST kernels' rare exact re-tests (inlined at every box test it
// would add its divisions to the hot loop's code and registers).  Returns the entry t, or NaN for a miss.
struct BoxArgs { float b[6]; f3 o, d; float tmax; };
__device__ __attribute__((noinline)) float slab_ref_entry(BoxArgs a) {
    float te = 0.0f;
    return slab_ref(a.b, a.o, a.d, TMIN, a.tmax, te) ? te : __builtin_nanf("");
}
// The entry t of the reference's slab alone (cur.min after the three axes, BoundingBox.cu:34-72), for a box the
// reference accepts.  Per axis min(t1, t2) is the nearer plane's distance, and which plane that is follows from the
// sign of d: IEEE subtraction and division are monotone, so t1 <= t2 for d > 0 and t2 <= t1 for d < 0 (equal values
// where they tie).  A parallel axis leaves cur.min alone.  Three divisions instead of the slab's six.
__device__ __forceinline__ float slab_ref_near(const float *b, const f3 &o, const f3 &d) {
    float cmin = TMIN;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float dd = comp(d, a);
        if (fabsf(dd) < FZERO) continue;
        const float t = fdiv((dd > 0.0f ? b[2 * a] : b[2 * a + 1]) - comp(o, a), dd);
        if (t > cmin) cmin = t;
    }
    return cmin;
}
// A FAST box decision: each end of the interval [lo, hi] (hi includes tmax) is within |pad| + 2^-20 |t| of the
// reference's (lo, hi >= TMIN > 0 wherever lo < hi can hold), so the widened test cons_lo(lo) < cons_hi(hi) keeps every
// box the reference's slab accepts (a cull is never wrong), and hi - lo > box_margin is an accept the reference shares;
// in between, the XB instances re-take the decision with the reference's slab
__device__ __forceinline__ float cons_lo(float lo, float pad) { return fmaf(lo, 1.0f - 0x1p-20f, -fabsf(pad)); }
__device__ __forceinline__ float cons_hi(float hi, float pad) { return fmaf(hi, 1.0f + 0x1p-20f, fabsf(pad)); }
__device__ __forceinline__ float box_margin(float lo, float hi, float pad) { return fmaf(lo + hi, 0x1p-20f, 2.0f * fabsf(pad)); }
__device__ __forceinline__ bool ray_parallel(const RayP &r) { return __builtin_signbit(r.pad) != 0; }
#endif
// XB: decisions inside the margin re-taken with the reference's slab (the quad instance for the reference's own trees
// and the binary-pair one, where the traversal then takes exactly the reference's decisions)
template <int XB = XD_CULL>
__device__ __forceinline__ bool slab(const float *b, const RayP &r, float tmin, float tmax, float &te) {
#if RT_EXACT
    return slab_ref(b, r.o, r.d, tmin, tmax, te);
#else
    const float tx1 = fmaf(b[0], r.inv.x, -r.oinv.x), tx2 = fmaf(b[1], r.inv.x, -r.oinv.x);
    const float ty1 = fmaf(b[2], r.inv.y, -r.oinv.y), ty2 = fmaf(b[3], r.inv.y, -r.oinv.y);
    const float tz1 = fmaf(b[4], r.inv.z, -r.oinv.z), tz2 = fmaf(b[5], r.inv.z, -r.oinv.z);
    const float lo = fmaxf(fmaxf(tmin, fminf(tx1, tx2)), fmaxf(fminf(ty1, ty2), fminf(tz1, tz2)));
    const float hi = fminf(fminf(tmax, fmaxf(tx1, tx2)), fminf(fmaxf(ty1, ty2), fmaxf(tz1, tz2)));
    te = lo;
    bool h = cons_lo(lo, r.pad) < cons_hi(hi, r.pad);
    if ((XB == XD_ALL && h && !(hi - lo > box_margin(lo, hi, r.pad))) || (XB != XD_CULL && ray_parallel(r))) {
        // rare: the reference's decision
        BoxArgs a;
        for (int c = 0; c < 6; c++) a.b[c] = b[c];
        a.o = r.o; a.d = r.d; a.tmax = tmax;
        const float e = slab_ref_entry(a);            // (tmin is TMIN at every call site)
        h = e == e;
        if (h) te = e;
    }
    return h;
#endif
}

#if !RT_EXACT
// one axis of the 4 slot slab tests; pa / pb: that axis's contribution to the entry t of the halves' boxes (a
// half's box is the union of its two slots' boxes, and the plane distances are monotone in the bound, so its near
// plane is the nearer of its slots' near planes)
template <bool PAIR>
__device__ __forceinline__ void slab4(const float4 &lo, const float4 &hi, float inv, float oinv, float4 &tn, float4 &tf,
                                      float &pa, float &pb) {
    const float a0 = fmaf(lo.x, inv, -oinv), b0 = fmaf(hi.x, inv, -oinv);
    const float a1 = fmaf(lo.y, inv, -oinv), b1 = fmaf(hi.y, inv, -oinv);
    const float a2 = fmaf(lo.z, inv, -oinv), b2 = fmaf(hi.z, inv, -oinv);
    const float a3 = fmaf(lo.w, inv, -oinv), b3 = fmaf(hi.w, inv, -oinv);
    const float n0 = fminf(a0, b0), n1 = fminf(a1, b1), n2 = fminf(a2, b2), n3 = fminf(a3, b3);
    tn = make_float4(fmaxf(tn.x, n0), fmaxf(tn.y, n1), fmaxf(tn.z, n2), fmaxf(tn.w, n3));
    tf = make_float4(fminf(tf.x, fmaxf(a0, b0)), fminf(tf.y, fmaxf(a1, b1)), fminf(tf.z, fmaxf(a2, b2)), fminf(tf.w, fmaxf(a3, b3)));
    if (PAIR) {
        pa = fmaxf(pa, fminf(n0, n1));
        pb = fmaxf(pb, fminf(n2, n3));
    }
}
__device__ __forceinline__ float comp4(const float4 &v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w)); }
// The hit decisions and entry t's of a quad's 4 slots (and, PAIR, of its two halves' boxes) for ray r with the current
// tmax: FAST reciprocal slabs, conservative; XB: decisions inside the error margin re-taken with the reference's
// division slab on the node's bounds re-read from Q.  Shared by the traversal step and the box-test entry point the
// parity tests call (rt_box_test, RT_BOX_QUAD_*).
template <bool PAIR, int XB>
__device__ __forceinline__ void quad_decide(const float4 *Q, const float4 &lx, const float4 &hx, const float4 &ly,
                                            const float4 &hy, const float4 &lz, const float4 &hz, const uint4 &R,
                                            const RayP &r, float tmax, float (&t)[4], bool (&h)[4], float &pa, float &pb) {
    bool und[4] = {false, false, false, false};   // und: hit decision inside the error margin
    // XD_ALL: whether an entry t is TMIN for certain — every entry plane below TMIN by more than the error bound, so the
    // reference's is TMIN too.  Two such entries compare equal in both slabs (the ray starts inside both boxes: most
    // nodes around a bounce origin), so their order needs no re-take.
    bool low[4] = {false, false, false, false}, low_a = false, low_b = false;
    const float t0 = XB == XD_ALL ? -__builtin_huge_valf() : TMIN;
    pa = t0; pb = t0;                                // entry t of the two halves' boxes
    {
        float4 tn = make_float4(t0, t0, t0, t0), tf = make_float4(tmax, tmax, tmax, tmax);
        slab4<PAIR>(lx, hx, r.inv.x, r.oinv.x, tn, tf, pa, pb);
        slab4<PAIR>(ly, hy, r.inv.y, r.oinv.y, tn, tf, pa, pb);
        slab4<PAIR>(lz, hz, r.inv.z, r.oinv.z, tn, tf, pa, pb);
        if (XB == XD_ALL) {
            const auto below = [&](float v) { return fmaf(fabsf(v), 0x1p-19f, v + 2.0f * fabsf(r.pad)) < TMIN; };
            low[0] = below(tn.x); low[1] = below(tn.y); low[2] = below(tn.z); low[3] = below(tn.w);
            low_a = below(pa); low_b = below(pb);
            tn = make_float4(fmaxf(tn.x, TMIN), fmaxf(tn.y, TMIN), fmaxf(tn.z, TMIN), fmaxf(tn.w, TMIN));
            pa = fmaxf(pa, TMIN); pb = fmaxf(pb, TMIN);
        }
        t[0] = tn.x; t[1] = tn.y; t[2] = tn.z; t[3] = tn.w;
        h[0] = cons_lo(tn.x, r.pad) < cons_hi(tf.x, r.pad); h[1] = cons_lo(tn.y, r.pad) < cons_hi(tf.y, r.pad);
        h[2] = cons_lo(tn.z, r.pad) < cons_hi(tf.z, r.pad); h[3] = cons_lo(tn.w, r.pad) < cons_hi(tf.w, r.pad);
        if (XB == XD_ALL) {
            und[0] = !(tf.x - tn.x > box_margin(tn.x, tf.x, r.pad)); und[1] = !(tf.y - tn.y > box_margin(tn.y, tf.y, r.pad));
            und[2] = !(tf.z - tn.z > box_margin(tn.z, tf.z, r.pad)); und[3] = !(tf.w - tn.w > box_margin(tn.w, tf.w, r.pad));
        }
    }
    // an empty slot repeats its sibling's box (the half's union stays exact) and is never accepted
    h[1] = h[1] && R.y != REF_EMPTY;
    h[3] = h[3] && R.w != REF_EMPTY;
    if (XB != XD_CULL) {   // Rare: a hit decision inside the error margin, a ray with a parallel axis, or (pair order) two entry t's the order
        // compares inside the margin — then the boxes involved (a ray with a parallel axis: every box of the node) are
        // re-tested with the reference's slab (a half's box: the union of its slots' boxes), on the node's bounds read
        // again (keeping the 24 bounds live through the step would cost registers on the hot path), one box per
        // iteration so that one copy of the division slab serves all six.  Boxes of the mask m: bit k = slot k, bits 4 / 5
        // = the halves.  Re-taking only the two entries a close comparison involves (round 6) instead of all six boxes
        // took C5 with exact decisions from 13.6 to 11.9 ms per serialised launch.
        const auto close = [&](float a, float b) { return fabsf(a - b) <= box_margin(a, b, r.pad); };
        uint32_t m = ray_parallel(r) ? (PAIR ? 0x3Fu : 0xFu) : 0u;
        if (XB == XD_ALL)
            m |= (h[0] && und[0] ? 1u : 0u) | (h[1] && und[1] ? 2u : 0u) | (h[2] && und[2] ? 4u : 0u) | (h[3] && und[3] ? 8u : 0u);
        if (PAIR && XB == XD_ALL)
            m |= (h[0] && h[1] && !(low[0] && low[1]) && close(t[0], t[1]) ? 0x3u : 0u) |
                 (h[2] && h[3] && !(low[2] && low[3]) && close(t[2], t[3]) ? 0xCu : 0u) |
                 ((h[0] || h[1]) && (h[2] || h[3]) && !(low_a && low_b) && close(pa, pb) ? 0x30u : 0u);
        if (m) {
            const float4 L[6] = {Q[0], Q[1], Q[2], Q[3], Q[4], Q[5]};
#pragma unroll 1
            for (; m; m &= m - 1u) {
                const int j = __builtin_ctz(m);
                const int k0 = j < 4 ? j : 2 * (j - 4), k1 = j < 4 ? j : k0 + 1;     // a slot, or a half's two slots
                float b[6];
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    const float u = comp4(L[c], k0), v = comp4(L[c], k1);
                    b[c] = (c & 1) ? fmaxf(u, v) : fminf(u, v);
                }
                BoxArgs ba;
                for (int c = 0; c < 6; c++) ba.b[c] = b[c];
                ba.o = r.o; ba.d = r.d; ba.tmax = tmax;
                const float te = slab_ref_entry(ba);
                const bool hh = te == te;
                if (j < 4) {
                    const uint32_t rk = j == 0 ? R.x : (j == 1 ? R.y : (j == 2 ? R.z : R.w));
                    const bool live = rk != REF_EMPTY;
                    const bool hk = hh && live;
                    h[0] = j == 0 ? hk : h[0]; h[1] = j == 1 ? hk : h[1]; h[2] = j == 2 ? hk : h[2]; h[3] = j == 3 ? hk : h[3];
                    if (hk) { t[0] = j == 0 ? te : t[0]; t[1] = j == 1 ? te : t[1]; t[2] = j == 2 ? te : t[2]; t[3] = j == 3 ? te : t[3]; }
                } else if (hh) {
                    pa = j == 4 ? te : pa;
                    pb = j == 5 ? te : pb;
                }
            }
        }
        if (XB == XD_ALL) {    // a leaf that is hit carries the reference's entry t to its re-test at the pop (pop_keep)
            uint32_t lm = (h[0] && (R.x & REF_LEAF) ? 1u : 0u) | (h[1] && (R.y & REF_LEAF) ? 2u : 0u) |
                          (h[2] && (R.z & REF_LEAF) ? 4u : 0u) | (h[3] && (R.w & REF_LEAF) ? 8u : 0u);
#pragma unroll 1
            for (; lm; lm &= lm - 1u) {
                const int j = __builtin_ctz(lm);
                float b[6];
#pragma unroll
                for (int c = 0; c < 6; c++) b[c] = comp4(Q[c], j);
                const float te = slab_ref_near(b, r.o, r.d);
                t[0] = j == 0 ? te : t[0]; t[1] = j == 1 ? te : t[1]; t[2] = j == 2 ? te : t[2]; t[3] = j == 3 ? te : t[3];
            }
        }
    }
}
#endif
