// traverse.hpp — the resumable traversal state machine: binary pairs (trav_step), the speculative while-while rounds
// (spec_round) over binary pairs or quads, and the LDS scene region the quad-tree kernels read.
// Includable only from trace_kernel.hip, once, inside namespace rtamd::RT_SUFFIX(dev), after box.hpp, primitives.hpp
// and stack.hpp.

// ---- closest hit -----------------------------------------------------------------------
struct Hit {
    float t;
    uint32_t inst;     // instance index
    uint32_t ptype;    // primitive type
    uint32_t slot;     // leaf-ordered slot in the type's array
    float u, v;
};

// Resumable per-lane traversal state: TLAS::hit (TLAS.cu:131-201) as a state machine so that a
// persistent wave can interleave traversal steps with shading / ray regeneration of other lanes.
// (REF_NONE: stack.hpp)
struct Trav {
    RayP wr, lr;           // world-space ray, instance-space ray of cur_inst
    float tmax;            // currentRange.max
    uint32_t cur;          // node to process next (REF_NONE: stack exhausted)
    float curT;            // entry t of cur (speculative traversal re-checks it)
    uint32_t pleaf;        // postponed leaf (speculative traversal), REF_NONE if none
    uint32_t cur_inst;
    Hit hit;
    bool found;
    bool tracing;
    Stack stk;
};

// A popped entry (or the speculative successor) survives its re-test: the reference re-runs the box test with the
// current tmax, which accepts it iff its entry t < tmax (the exit side passed at the push and tmax only shrinks).
// FAST (conservative slabs): the entry is widened by its ray's bound first (a BLAS entry belongs to the current
// instance's ray).  An interior node kept that the reference culls costs box tests only: its children's entries are
// not below its own, and their tests see the same tmax.  A leaf kept that the reference culls is entered without
// another box test, and a primitive in it within 1e-6 beyond tmax (Range.cuh:33-43) replaces the hit.  So the
// exact-decision instances (XD_ALL) give every leaf the reference's own entry t where it is hit (pair_test,
// quad_decide) and compare that one as the reference does.
template <int XB = XD_CULL>
__device__ __forceinline__ bool pop_keep(const Trav &T, float tn, uint32_t ref) {
#if !RT_EXACT
    if (XB == XD_ALL && (ref & REF_LEAF)) return tn < T.tmax;
    return cons_lo(tn, (ref & REF_BLAS) ? T.lr.pad : T.wr.pad) < T.tmax;
#else
    (void)ref;
    return tn < T.tmax;
#endif
}

// R: this frame's TLAS root (the persistent kernel holds it in SGPRs, loaded once per wave).  tmax: currentRange.max at
// the start — +inf for a path segment, the caller's bound for a ray with the range [TMIN, tmax] (ray_query.hpp)
template <int XB = XD_CULL>
__device__ __forceinline__ void trav_init(Trav &T, const TreeRoot &R, const f3 &o, const f3 &d,
                                          float tmax = __builtin_huge_valf()) {
    T.wr.o = o; T.wr.d = d; prep<XB>(T.wr);
    T.lr = T.wr;
    T.tmax = tmax;
    T.found = false;
    T.stk.clear();
    T.cur = R.ref;
    T.cur_inst = 0;
    T.pleaf = REF_NONE;
    float te = 0.0f;
    T.tracing = slab<XB>(R.box, T.wr, TMIN, T.tmax, te);                 // root pop test (TLAS.cu:150)
    T.curT = te;
}

// The frame's TLAS root as wave-uniform values (SGPRs): read once per wave instead of per ray.
template <bool WIDE>
__device__ __forceinline__ TreeRoot uniform_root(const SceneGPU &sc) {
    const float4 *p = reinterpret_cast<const float4 *>(WIDE ? sc.tlas_root_wide : sc.tlas_root);
    const float4 a = p[0], b = p[1];
    auto u = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    TreeRoot R;
    R.box[0] = u(a.x); R.box[1] = u(a.y); R.box[2] = u(a.z); R.box[3] = u(a.w);
    R.box[4] = u(b.x); R.box[5] = u(b.y);
    R.ref = (uint32_t)__builtin_amdgcn_readfirstlane(__float_as_int(b.z));
    R.height = 0;
    return R;
}

// An interior node pair (TLAS.cu:175-197 / BLAS.cu:178-202): both children's boxes tested against the ray of the
// node's level with the current tmax.  h / e: hit and entry t (written only on a hit in the EXACT build) of the left (0)
// and right (1) child.  Returns the node's refs: .x the left child, .y the right.  (Returning hits and entries in a
// struct instead compiles to other EXACT code; the out-parameters keep the inline code's.)
template <bool COUNT, int XB>
__device__ __forceinline__ uint4 pair_test(const Trav &T, const SceneGPU &sc, uint32_t cur, LaneCount &cnt,
                                           bool &h0, bool &h1, float &e0, float &e1) {
    const bool blas = (cur & REF_BLAS) != 0;
    const NodePair *P = (blas ? sc.blas_pairs : sc.tlas_pairs) + (cur & REF_INDEX_MASK);
    const float4 *P4 = reinterpret_cast<const float4 *>(P);
    const float4 A = P4[0], B = P4[1], Cc = P4[2];
    const uint4 D = reinterpret_cast<const uint4 *>(P)[3];
    const float b0[6] = {A.x, A.y, A.z, A.w, B.x, B.y};
    const float b1[6] = {B.z, B.w, Cc.x, Cc.y, Cc.z, Cc.w};
    if (COUNT) cnt.pairs++;
    const RayP &r = blas ? T.lr : T.wr;
    h0 = slab<XB>(b0, r, TMIN, T.tmax, e0);
    h1 = slab<XB>(b1, r, TMIN, T.tmax, e1);
#if !RT_EXACT
    if (XB == XD_ALL) {   // a leaf that is hit carries the reference's entry t to its re-test at the pop (pop_keep)
        // ... and where both children are hit, both entries: the callers order them by e0 > e1, which must compare two
        // values of one kind (siblings often share their near plane, and then tie in the reference)
        const bool l0 = h0 && (D.x & REF_LEAF), l1 = h1 && (D.y & REF_LEAF);
        if (l0 || (l1 && h0)) e0 = slab_ref_near(b0, r.o, r.d);
        if (l1 || (l0 && h1)) e1 = slab_ref_near(b1, r.o, r.d);
    }
#endif
    return D;
}

// A primitive test accepted a hit: it becomes the closest so far and shrinks the range (BLAS.cu:160-172)
__device__ __forceinline__ void accept(Trav &T, float t, uint32_t type, uint32_t slot, float u, float v) {
    T.found = true; T.tmax = t;
    T.hit.t = t; T.hit.inst = T.cur_inst; T.hit.ptype = type; T.hit.slot = slot; T.hit.u = u; T.hit.v = v;
}

// Instance::hit's entry (Instance.cu:26-27): the world ray into the local space of T.cur_inst (inv: its inverse
// transform's 12 floats; d' not renormalised), then the BLAS root's pop test on its box.  te: the root's entry t
template <int XB>
__device__ __forceinline__ bool enter_instance(Trav &T, const float *inv, const float *root_box, float &te) {
    T.lr.o = xf_point(inv, T.wr.o);
    T.lr.d = xf_vector(inv, T.wr.d);
    prep<XB>(T.lr);
    return slab<XB>(root_box, T.lr, TMIN, T.tmax, te);
}

// Process T.cur (one node pair, one TLAS leaf instance or one BLAS leaf), then choose the next node:
// the near child, or a popped entry surviving the re-test; clears T.tracing when the stack is dry.
// XB (FAST builds): box decisions inside the slab error margin re-taken with the reference's slab (rt_trace_rays and
// the grid kernel: the binary pairs in the reference's order, so their decisions are the reference's)
template <bool COUNT, int XB = XD_CULL>
__device__ __forceinline__ void trav_step(Trav &T, const SceneGPU &sc, SEnt *spill, LaneCount &cnt) {
    const uint32_t cur = T.cur;
    if (!(cur & REF_LEAF)) {
        float e0 = 0.0f, e1 = 0.0f;
        bool h0, h1;
        const uint4 D = pair_test<COUNT, XB>(T, sc, cur, cnt, h0, h1, e0, e1);
        if (h0 && h1) {
            // reference: tLeft > tRight -> push left then right (right popped first)
            const bool right_near = e0 > e1;
            stack_push(T.stk, spill, right_near ? D.x : D.y, right_near ? e0 : e1, cnt);
            T.cur = right_near ? D.y : D.x;
            return;
        }
        if (h0) { T.cur = D.x; return; }
        if (h1) { T.cur = D.y; return; }
    } else if (!(cur & REF_BLAS)) {
        // TLAS leaf: its instances in order (TLAS.cu:157-173)
        const uint32_t start = ref_leaf_start(cur), count = ref_leaf_count(cur);
        if (count > 1) stack_push(T.stk, spill, make_leaf_ref(start + 1, count - 1, 0, false), -__builtin_huge_valf(), cnt);
        T.cur_inst = sc.inst_by_slot ? start : sc.tlas_slots[start];
        const InstHot &I = sc.inst_hot[T.cur_inst];
        if (COUNT) cnt.inst++;
        float te;
        if (enter_instance<XB>(T, I.inv, I.root_box, te)) { T.cur = I.root_ref; return; }
    } else {
        // BLAS leaf: primitives in leaf order (BLAS.cu:153-176; spec_leaf_phase has the loop per type)
        const uint32_t start = ref_leaf_start(cur), count = ref_leaf_count(cur), type = ref_leaf_type(cur);
        for (uint32_t k = 0; k < count; k++) {
            const uint32_t slot = start + k;
            float t = 0.0f, u = 0.0f, v = 0.0f;
            bool h;
            if (type == RT_PRIM_TRIANGLE) {
                if (COUNT) cnt.tri++;
                h = tri_test(sc.tri_hot[slot], T.lr, TMIN, T.tmax, t, u, v);
            } else if (type == RT_PRIM_SPHERE) {
                if (COUNT) cnt.sq++;
                h = sphere_test(sc.sph_hot[slot], T.lr, TMIN, T.tmax, t);
            } else {
                if (COUNT) { cnt.sq++; cnt.quad++; }
                h = quad_test(sc.quad_hot[slot], T.lr, TMIN, T.tmax, t, u, v);
            }
            if (h) accept(T, t, type, slot, u, v);
        }
    }
    // pop until an entry survives the re-test (entry t < tmax)
    while (!T.stk.empty()) {
        const SEnt e = stack_pop(T.stk, spill);
        if (pop_keep<XB>(T, __uint_as_float(e.tn), e.ref)) { T.cur = e.ref; return; }
    }
    T.tracing = false;
}

// ---- speculative while-while traversal (Aila & Laine 2009), reference-order preserving ----------
// Phase 1 (interior loop): every lane walks interior node pairs; the first leaf a lane reaches is
// postponed (pleaf) and the lane keeps walking (speculatively) until it meets a second leaf; the
// wave leaves the loop once every traversing lane holds a postponed leaf.  Phase 2 processes the
// postponed leaves together.  The reference processes a leaf before the nodes that follow it, with
// the tmax the leaf produced.  Speculative steps used the older (larger) tmax, so:
//   * the postponed leaf itself passed its test with the current tmax (no leaf ran in between);
//   * entries pushed speculatively are re-tested at pop (entry t < tmax), as always;
//   * the node the lane stopped at (cur) is re-tested after the leaf: every node reached below a node
//     N has entry t >= N's entry t (child boxes lie inside parent boxes and the slab entry is
//     monotone in the box bounds), so cur fails its re-test whenever the reference would have culled
//     N or any node on the way.
// Hence leaves are processed in the reference order with the reference's tmax: same hits, same
// primitive tests, same instance visits (only extra node-pair tests are speculative).
// A leaf is postponed where it appears in cur — in the iteration whose node step produced it, and at the end of
// the leaf phase when the re-tested successor is one — not in an iteration of its own: no leaf runs between the two
// places, so tmax, every pop_keep decision and the lane's operations and their order are the same, and a lane
// takes one interior iteration less per leaf.
template <int XB>
__device__ __forceinline__ void pop_next(Trav &T, const SEnt *spill) {
    while (!T.stk.empty()) {
        const SEnt e = stack_pop(T.stk, spill);
        const float tn = __uint_as_float(e.tn);
        if (pop_keep<XB>(T, tn, e.ref)) { T.cur = e.ref; T.curT = tn; return; }
    }
    T.cur = REF_NONE;
}
// The leaf in cur (a real ref: REF_NONE carries the leaf bit too) waits in pleaf for the leaf phase; the lane goes on
// with the next entry.  T.tracing stays set while pleaf is, whatever cur becomes.
template <int XB>
__device__ __forceinline__ void postpone_leaf(Trav &T, const SEnt *spill) {
    T.pleaf = T.cur;
    pop_next<XB>(T, spill);
}

// k * N for a record of N dwordx4 (N <= 8) as shifts and adds, ahead of a dependent load: v_mul_lo_u32 and
// v_mad_u64_u32 issue at a quarter of the rate.  The optimiser folds a plain (k << 3) - k back into the multiply, so
// the shifted value passes through an empty asm.
template <uint32_t N>
__device__ __forceinline__ uint32_t times(uint32_t k) {
    static_assert(N >= 1 && N <= 8, "a small record size");
    if constexpr ((N & (N - 1)) == 0) {
        return k * N;
    } else if constexpr (N == 6) {
        return times<3>(k) << 1;
    } else {
        uint32_t s = k << (N == 3 ? 1 : (N == 5 ? 2 : 3));
        asm("" : "+v"(s));
        return N == 7 ? s - k : s + k;
    }
}

// One interior-loop step of a lane whose cur is an interior node.
#if !RT_EXACT
// Quad node (option "wide", layout.hpp NodeQuad): 4 slab tests on SoA bounds; the hit slots are visited
//   PAIR (quads of two binary levels: the reference's trees, GPU-built trees): in the reference's order — the two
//     halves (binary children) by their boxes' entry t, then the slots of a half by theirs, the nearer first and the
//     left one on ties (BLAS.cu:186-202, TLAS.cu:182-197) — so the closest hit is the reference's, ties included;
//   else (host SAH trees, collapsed greedily): by entry t, nearest first (measured against the oracle: DESIGN §3.4).
// The first is visited next and the others pushed last-first, each with its own entry t for the pop re-test (a
// half's box holds its slots' boxes, so its re-test passes whenever one of theirs does).
// Option "lds_scene" (SceneGPU::lds_quads / lds_insts): the frame's TLAS quads and instance hot records,
// copied into LDS by every workgroup of the persistent quad-tree kernel at its start.  On C2 an average
// ray visits ~1.6 quads (mostly TLAS) and enters ~1 instance, so most of its dependent loads are these.
__shared__ float4 lds_scene[LDS_SCENE_F4];

struct InstRec { float4 i0, i1, i2, box01, box2ref; };   // InstHot as 5 dwordx4 (inv rows, root box, refs)
template <bool LDSS>
__device__ __forceinline__ InstRec load_inst(const SceneGPU &sc, uint32_t i) {
    InstRec r;
    if (LDSS && sc.lds_insts) {
        const float4 *p = lds_scene + sc.lds_quads * LDS_QUAD_F4 + times<LDS_INST_F4>(i);
        r.i0 = p[0]; r.i1 = p[1]; r.i2 = p[2]; r.box01 = p[3]; r.box2ref = p[4];
    } else {
        static_assert(sizeof(InstHot) == LDS_INST_F4 * 16, "InstHot is LDS_INST_F4 dwordx4");
        const float4 *p = reinterpret_cast<const float4 *>(sc.inst_hot) + times<LDS_INST_F4>(i);     // (i < 2^26)
        r.i0 = p[0]; r.i1 = p[1]; r.i2 = p[2]; r.box01 = p[3]; r.box2ref = p[4];
    }
    return r;
}
// the workgroup's copy (before the kernel's first barrier)
__device__ __forceinline__ void lds_scene_fill(const SceneGPU &sc) {
    const uint32_t nq = sc.lds_quads * LDS_QUAD_F4, ni = sc.lds_insts * LDS_INST_F4;
    const float4 *q = reinterpret_cast<const float4 *>(sc.tlas_quads);
    for (uint32_t i = threadIdx.x; i < nq; i += BLOCK) {
        const uint32_t k = i / LDS_QUAD_F4, j = i - k * LDS_QUAD_F4;
        lds_scene[i] = q[k * 8 + j];
    }
    const float4 *h = reinterpret_cast<const float4 *>(sc.inst_hot);
    for (uint32_t i = threadIdx.x; i < ni; i += BLOCK) lds_scene[nq + i] = h[i];
    const auto copy = [](uint32_t at, const void *src, uint32_t n4) {
        if (at == LDS_NONE) return;
        const float4 *p = reinterpret_cast<const float4 *>(src);
        for (uint32_t i = threadIdx.x; i < n4; i += BLOCK) lds_scene[at + i] = p[i];
    };
    copy(sc.lds_icold, sc.inst_cold, sc.instance_count * LDS_ICOLD_F4);
    copy(sc.lds_sph_hot, sc.sph_hot, sc.lds_sph_cold - sc.lds_sph_hot);
    copy(sc.lds_sph_cold, sc.sph_cold, sc.lds_sph_cold - sc.lds_sph_hot);
    copy(sc.lds_q_hot, sc.quad_hot, (sc.lds_q_cold - sc.lds_q_hot));
    copy(sc.lds_q_cold, sc.quad_cold, (sc.lds_q_cold - sc.lds_q_hot) / LDS_QPRIM_F4);
    const float4 *bq = reinterpret_cast<const float4 *>(sc.blas_quads + sc.lds_bq0);   // a group BLAS's top levels
    for (uint32_t i = threadIdx.x; i < sc.lds_bqn * LDS_QUAD_F4; i += BLOCK) {
        const uint32_t k = i / LDS_QUAD_F4, j = i - k * LDS_QUAD_F4;
        lds_scene[sc.lds_bq_at + i] = bq[k * 8 + j];
    }
}
// record k of an array that may be resident in the LDS scene region (at = its dwordx4 offset, LDS_NONE = HBM)
template <typename R>
__device__ __forceinline__ R lds_or_global(uint32_t at, const R *g, uint32_t k) {
    constexpr uint32_t N4 = sizeof(R) / 16;
    R r;
    float4 *d = reinterpret_cast<float4 *>(&r);
    if (at != LDS_NONE) {
#pragma unroll
        for (uint32_t j = 0; j < N4; j++) d[j] = lds_scene[at + times<N4>(k) + j];
    } else {
        const float4 *p = reinterpret_cast<const float4 *>(g) + times<N4>(k);     // (k < 2^26: an instance or a slot)
#pragma unroll
        for (uint32_t j = 0; j < N4; j++) d[j] = p[j];
    }
    return r;
}

__device__ __forceinline__ void cswap(float &ta, uint32_t &ra, float &tb, uint32_t &rb) {
    const bool sw = tb < ta;
    const float t = sw ? tb : ta, u = sw ? ta : tb;
    const uint32_t r = sw ? rb : ra, q = sw ? ra : rb;
    ta = t; tb = u; ra = r; rb = q;
}

template <bool COUNT, bool PAIR, int XB>
__device__ __forceinline__ void wide_interior_step(Trav &T, const SceneGPU &sc, SEnt *spill, LaneCount &cnt) {
    const uint32_t cur = T.cur;
    const bool blas = (cur & REF_BLAS) != 0;
    float4 lx, hx, ly, hy, lz, hz;
    uint4 R;
    // one code path: a generic pointer into the LDS scene region or HBM (flat loads serve both), chosen once as a
    // base and a byte offset (an LDS record is LDS_QUAD_F4 dwordx4 and its index small; a NodeQuad in HBM is 128 B)
    const float4 *Q;
    {
        const uint32_t qi = cur & REF_INDEX_MASK, qb = qi - sc.lds_bq0;
        const bool in_lds = blas ? qb < sc.lds_bqn : sc.lds_quads != 0;
        const uint32_t at = (blas ? sc.lds_bq_at : 0u) + times<LDS_QUAD_F4>(blas ? qb : qi);
        const char *base = in_lds ? reinterpret_cast<const char *>(static_cast<const float4 *>(lds_scene))
                                  : reinterpret_cast<const char *>(blas ? sc.blas_quads : sc.tlas_quads);
        const uint64_t off = in_lds ? (uint64_t)(at << 4) : (uint64_t)qi << 7;
        Q = reinterpret_cast<const float4 *>(base + off);
        lx = Q[0]; hx = Q[1]; ly = Q[2]; hy = Q[3]; lz = Q[4]; hz = Q[5];
        R = reinterpret_cast<const uint4 *>(Q)[6];
    }
    // the child refs are needed only when a child is hit, so the compiler would issue their load after the slab
    // tests: a second dependent memory round trip per step.  Pinning them here keeps all 7 dwordx4 loads of the
    // node in one round trip.
    asm volatile("" ::"v"(R.x), "v"(R.y), "v"(R.z), "v"(R.w));
    if (COUNT) cnt.pairs += 2;                       // 4 child boxes = 2 node-pair equivalents
    const RayP &r = blas ? T.lr : T.wr;
    float t[4];
    bool h[4];
    float pa, pb;                                    // entry t of the two halves' boxes
    quad_decide<PAIR, XB>(Q, lx, hx, ly, hy, lz, hz, R, r, T.tmax, t, h, pa, pb);
    const float inf = __builtin_huge_valf();
    if (!PAIR) {
        float t0 = h[0] ? t[0] : inf, t1 = h[1] ? t[1] : inf, t2 = h[2] ? t[2] : inf, t3 = h[3] ? t[3] : inf;
        uint32_t r0 = R.x, r1 = R.y, r2 = R.z, r3 = R.w;
        const uint32_t nh = (uint32_t)h[0] + (uint32_t)h[1] + (uint32_t)h[2] + (uint32_t)h[3];
        if (nh == 0) { pop_next<XB>(T, spill); return; }
        // sort the 4 (t, ref) ascending; misses (t = inf) sink to the end
        cswap(t0, r0, t1, r1); cswap(t2, r2, t3, r3); cswap(t0, r0, t2, r2); cswap(t1, r1, t3, r3); cswap(t1, r1, t2, r2);
        // the 1..3 far hits go to the three LDS slots above the top without branching on their count (farthest
        // first; the slots past the new top are free space), after one page-out check
        if (nh > 1) {
            if (T.stk.sp > LDS_DEPTH - 3) stack_page_out(T.stk, spill, cnt);
            SEnt a, b, c;
            a.ref = nh == 4 ? r3 : (nh == 3 ? r2 : r1);
            a.tn = __float_as_uint(nh == 4 ? t3 : (nh == 3 ? t2 : t1));
            b.ref = nh == 4 ? r2 : r1;
            b.tn = __float_as_uint(nh == 4 ? t2 : t1);
            c.ref = r1;
            c.tn = __float_as_uint(t1);
            stack_push3(T.stk, a, b, c, nh - 1u);
        }
        T.cur = r0;
        T.curT = t0;
        return;
    }
    const uint32_t na = (uint32_t)h[0] + (uint32_t)h[1], nb = (uint32_t)h[2] + (uint32_t)h[3];
    if (na + nb == 0) { pop_next<XB>(T, spill); return; }
    // The reference's visit order (BLAS.cu:186-202: push far, visit near, the right child first iff tLeft > tRight):
    // inside each half its two slots, then the halves by their boxes' entry t.  A missed slot counts as t = +inf, so
    // it is second in its half, and a half without hits goes second; the hits then come first in each half.
    const float u0 = h[0] ? t[0] : inf, u1 = h[1] ? t[1] : inf, u2 = h[2] ? t[2] : inf, u3 = h[3] ? t[3] : inf;
    const bool sa = u0 > u1, sb = u2 > u3;
    const float a0t = sa ? u1 : u0, a1t = sa ? u0 : u1, b0t = sb ? u3 : u2, b1t = sb ? u2 : u3;
    const uint32_t a0r = sa ? R.y : R.x, a1r = sa ? R.x : R.y, b0r = sb ? R.w : R.z, b1r = sb ? R.z : R.w;
    const bool sr = na == 0 || (nb != 0 && pa > pb);                 // the right half first
    const float n0t = sr ? b0t : a0t, n1t = sr ? b1t : a1t, f0t = sr ? a0t : b0t, f1t = sr ? a1t : b1t;
    const uint32_t n0r = sr ? b0r : a0r, n1r = sr ? b1r : a1r, f0r = sr ? a0r : b0r, f1r = sr ? a1r : b1r;
    const uint32_t nn = sr ? nb : na, nf = sr ? na : nb;             // hits in the near / far half (nn >= 1)
    // the near half's first hit is visited next; the rest go to the three LDS slots above the top, deepest first
    // (far half's second, its first, the near half's second), without branching on their count, after one
    // page-out check
    const uint32_t npush = nn - 1u + nf;
    if (npush > 0) {
        if (T.stk.sp > LDS_DEPTH - 3) stack_page_out(T.stk, spill, cnt);
        SEnt a, b, c;
        a.ref = nf == 2 ? f1r : (nf == 1 ? f0r : n1r);
        a.tn = __float_as_uint(nf == 2 ? f1t : (nf == 1 ? f0t : n1t));
        b.ref = nf == 2 ? f0r : n1r;
        b.tn = __float_as_uint(nf == 2 ? f0t : n1t);
        c.ref = n1r;
        c.tn = __float_as_uint(n1t);
        stack_push3(T.stk, a, b, c, npush);
    }
    T.cur = n0r;
    T.curT = n0t;
}
#endif

template <bool COUNT, int WIDE = 0>
__device__ __forceinline__ void spec_interior_step(Trav &T, const SceneGPU &sc, SEnt *spill, LaneCount &cnt) {
    const uint32_t cur = T.cur;
#if !RT_EXACT
    if (WIDE) {
        wide_interior_step<COUNT, (WIDE >= 2), XBOX(WIDE)>(T, sc, spill, cnt);
        return;
    }
#endif
    float e0 = 0.0f, e1 = 0.0f;
    bool h0, h1;
    const uint4 D = pair_test<COUNT, XBOX(WIDE)>(T, sc, cur, cnt, h0, h1, e0, e1);
    if (h0 && h1) {
        const bool right_near = e0 > e1;          // TLAS.cu:185-192 ordering
        stack_push(T.stk, spill, right_near ? D.x : D.y, right_near ? e0 : e1, cnt);
        T.cur = right_near ? D.y : D.x;
        T.curT = right_near ? e1 : e0;
        return;
    }
    if (h0 || h1) {
        T.cur = h0 ? D.x : D.y;
        T.curT = h0 ? e0 : e1;
        return;
    }
    pop_next<XBOX(WIDE)>(T, spill);
}

// Process the postponed leaf, then resume at cur (re-tested) — TLAS.cu:157-173 / BLAS.cu:153-176.
// a sphere / parallelogram record: from the LDS scene region in the quad-tree kernel when resident
#if RT_EXACT
#define WIDE_LDS_REC(at, arr, k) (arr)[k]
#else
#define WIDE_LDS_REC(at, arr, k) (WIDE ? lds_or_global((at), (arr), (k)) : (arr)[k])
#endif
// FAST quad trees (RT_CHAIN_ROOT_LEAF): when the entered instance's BLAS root is itself a leaf, its
// primitives are tested in this same round, as BLAS::hit tests a leaf root right after the root box
// (BLAS.cu:140-176) — the speculative successor waits on the stack as before and is popped (re-tested)
// after the tests.  A segment against the demo's spheres / parallelogram then takes one round, not two.
// Returns 1 when a root leaf was chained (it counts as a step of its own in the unit costs, so the
// claim order's cost classes keep the scale they were tuned on).
template <bool COUNT, int WIDE = 0>
__device__ __forceinline__ uint32_t spec_leaf_phase(Trav &T, const SceneGPU &sc, SEnt *spill, LaneCount &cnt) {
    uint32_t leaf = T.pleaf;
    bool chained = false;
    T.pleaf = REF_NONE;
    if (!(leaf & REF_BLAS)) {
        // TLAS leaf: enter the first instance's BLAS; the speculative successor and the leaf's
        // remaining instances wait on the stack (popped in reference order).
        const uint32_t start = ref_leaf_start(leaf), count = ref_leaf_count(leaf);
        if (T.cur != REF_NONE) stack_push(T.stk, spill, T.cur, T.curT, cnt);
        if (count > 1) stack_push(T.stk, spill, make_leaf_ref(start + 1, count - 1, 0, false), -__builtin_huge_valf(), cnt);
        T.cur_inst = sc.inst_by_slot ? start : sc.tlas_slots[start];
        if (COUNT) cnt.inst++;
        float te = 0.0f;
#if !RT_EXACT
        if (WIDE) {
            const InstRec I = load_inst<true>(sc, T.cur_inst);
            // all 5 dwordx4 of the record in one round trip (the root ref is used only when the root box is hit,
            // so its load would otherwise be issued after the slab test)
            asm volatile("" ::"v"(I.i2.x), "v"(I.i2.y), "v"(I.i2.z), "v"(I.i2.w), "v"(I.box2ref.w));
            const float inv[12] = {I.i0.x, I.i0.y, I.i0.z, I.i0.w, I.i1.x, I.i1.y, I.i1.z, I.i1.w,
                                   I.i2.x, I.i2.y, I.i2.z, I.i2.w};              // (as finalize does)
            const float box[6] = {I.box01.x, I.box01.y, I.box01.z, I.box01.w, I.box2ref.x, I.box2ref.y};
            if (enter_instance<XBOX(WIDE)>(T, inv, box, te)) {
                T.cur = __float_as_uint(I.box2ref.w);
                T.curT = te;
                if (RT_CHAIN_ROOT_LEAF && (T.cur & REF_LEAF)) { leaf = T.cur; chained = true; }
            } else {
                pop_next<XBOX(WIDE)>(T, spill);
            }
        } else
#endif
        {
            const InstHot &I = sc.inst_hot[T.cur_inst];
            if (enter_instance<XBOX(WIDE)>(T, I.inv, I.root_box, te)) { T.cur = WIDE ? I.root_ref_wide : I.root_ref; T.curT = te; }
            else pop_next<XBOX(WIDE)>(T, spill);
        }
    }
    if (leaf & REF_BLAS) {                  // the postponed BLAS leaf, or (chained) the entered BLAS's root leaf
        const uint32_t start = ref_leaf_start(leaf), count = ref_leaf_count(leaf), type = ref_leaf_type(leaf);
        if (type == RT_PRIM_TRIANGLE) {
            // every triangle record of the leaf is requested before the first test: one memory round
            // trip per leaf instead of one per triangle (tests still run in leaf order, BLAS.cu:153-176)
            for (uint32_t k0 = 0; k0 < count; k0 += TRI_AHEAD) {
                TriHot H[TRI_AHEAD];           // 3 x 12 B loads per triangle (the pad words stay unread)
                // unconditional loads (slots past the leaf's last triangle re-read that one): a load under
                // `k0 + k < count` would be issued only after the previous triangles' loads were waited for
#pragma unroll
                for (uint32_t k = 0; k < TRI_AHEAD; k++) {
                    static_assert(sizeof(TriHot) == 48 && offsetof(TriHot, v0) == 0, "TriHot is 3 dwordx4, v0 first");
                    const float *src = reinterpret_cast<const float *>(sc.tri_hot) +
                                       (times<3>(start + min(k0 + k, count - 1u)) << 2);   // (slot < 2^26)
                    const float3 a = *reinterpret_cast<const float3 *>(src);
                    const float3 b = *reinterpret_cast<const float3 *>(src + 4);
                    const float3 c = *reinterpret_cast<const float3 *>(src + 8);
                    H[k].v0[0] = a.x; H[k].v0[1] = a.y; H[k].v0[2] = a.z;
                    H[k].e1[0] = b.x; H[k].e1[1] = b.y; H[k].e1[2] = b.z;
                    H[k].e2[0] = c.x; H[k].e2[1] = c.y; H[k].e2[2] = c.z;
                }
#pragma unroll
                for (uint32_t k = 0; k < TRI_AHEAD; k++) {
                    if (k0 + k >= count) break;
                    float t = 0.0f, u = 0.0f, v = 0.0f;
                    if (COUNT) cnt.tri++;
                    if (tri_test(H[k], T.lr, TMIN, T.tmax, t, u, v)) accept(T, t, type, start + k0 + k, u, v);
                }
            }
        } else {
            // (trav_step has this loop with the triangles in it: sharing the body changed every flavour's code)
            for (uint32_t k = 0; k < count; k++) {
                const uint32_t slot = start + k;
                float t = 0.0f, u = 0.0f, v = 0.0f;
                bool h;
                if (type == RT_PRIM_SPHERE) {
                    if (COUNT) cnt.sq++;
                    h = sphere_test(WIDE_LDS_REC(sc.lds_sph_hot, sc.sph_hot, slot), T.lr, TMIN, T.tmax, t);
                } else {
                    if (COUNT) { cnt.sq++; cnt.quad++; }
                    h = quad_test(WIDE_LDS_REC(sc.lds_q_hot, sc.quad_hot, slot), T.lr, TMIN, T.tmax, t, u, v);
                }
                if (h) accept(T, t, type, slot, u, v);
            }
        }
        if (chained) pop_next<XBOX(WIDE)>(T, spill);                       // the root leaf is done
        else if (T.cur != REF_NONE && !pop_keep<XBOX(WIDE)>(T, T.curT, T.cur))     // re-test the successor
            pop_next<XBOX(WIDE)>(T, spill);
    }
    if (T.cur == REF_NONE) T.tracing = false;
    return chained ? 1u : 0u;
}

#ifndef RT_DIAG
#define RT_DIAG 0
#endif
// Diagnostic builds (make diag -> librtamd_diag.so): wave-uniform cycle stamps per phase.
// claim / hit (diagnostic builds): cycles giving idle lanes their pixels (map, RNG, camera ray, traversal
// init) and sampling scatter directions after the hit records arrived
struct PhaseCycles {
    unsigned long long refill, interior, leaf, shade, iters, refill_iters, claim, hit;
    // lane occupancy (diagnostic builds): lanes stepping per interior iteration, lanes holding a TLAS / BLAS leaf per
    // leaf phase, lanes shaded per shade step (sums; the timeline divides by iters / rounds / shades)
    unsigned long long lanes_interior, lanes_leaf_tlas, lanes_leaf_blas, lanes_shade;
    // lanes_postpone: leaves postponed in the interior loop (lane sums); iters_idle: interior iterations in which no
    // lane took a node step;
    // hits / hits_last_rough: shaded hits, and those on a path's last segment with a rough material (albedo only)
    unsigned long long lanes_postpone, iters_idle, hits, hits_last_rough;
};
__device__ __forceinline__ unsigned long long stamp() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}
#if RT_DIAG
#define DIAG_WAIT_VM() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define DIAG_T(var) const unsigned long long var = stamp()
#define DIAG_ADD(acc, t0) (acc) += stamp() - (t0)
#else
#define DIAG_WAIT_VM() (void)0
#define DIAG_T(var) (void)0
#define DIAG_ADD(acc, t0) (void)0
#endif

// One round: interior loop until every traversing lane holds a leaf, then the leaf phase.
// An iteration of the interior loop: a lane whose cur is an interior node takes its step; then a lane without a
// postponed leaf whose cur is a leaf — the one the step just produced, or a segment's first node — postpones it and
// goes on with the next entry.  Likewise after the leaf phase, when the successor that survived its re-test (or the
// entered BLAS's root) is a leaf.
// steps (when `track`): the lane's node steps + postponements + leaf phases, the pixel's cost for the work order
// leaf_early (setting "leaf_early"): the interior loop also ends once no more than this many lanes are still looking
// for a leaf while some hold one; the lanes without a leaf skip the leaf phase and go on descending next round
template <bool COUNT, int WIDE = 0>
__device__ __forceinline__ void spec_round(Trav &T, const SceneGPU &sc, SEnt *spill, LaneCount &cnt,
                                           PhaseCycles &pc, uint32_t &steps, bool track, uint32_t leaf_early) {
    DIAG_T(t0);
    // The loop's exit tests stand ahead of the loop and at the end of its body, not in the middle of `for (;;)`: with
    // the breaks inside, the compiler carries the lane's state (cur, curT, the stack's top and counts) through the body
    // in a second set of registers and moves it back every iteration (about 14 v_mov_b32 per iteration of the
    // benched instantiation); with the tests at the end it updates the state in place.
    const auto more = [&]() -> bool {
        if (T.tracing && T.pleaf == REF_NONE && T.cur == REF_NONE) T.tracing = false;   // done, no leaf left
        const uint64_t looking = __ballot(T.tracing && T.pleaf == REF_NONE);
        if (!looking) return false;
        return !(leaf_early && (uint32_t)__popcll(looking) <= leaf_early && __any(T.tracing && T.pleaf != REF_NONE));
    };
    for (bool go = more(); go; go = more()) {
        const bool active = T.tracing && T.cur != REF_NONE && (!(T.cur & REF_LEAF) || T.pleaf == REF_NONE);
        const bool node = active && !(T.cur & REF_LEAF);
        if (RT_DIAG) {
            pc.lanes_interior += (unsigned long long)__popcll(__ballot(active));
            if (!__ballot(node)) pc.iters_idle++;
        }
        if (node) {
            spec_interior_step<COUNT, WIDE>(T, sc, spill, cnt);
            if (track) steps++;
        }
        const bool leaf = active && T.pleaf == REF_NONE && (T.cur & REF_LEAF) && T.cur != REF_NONE;
        if (RT_DIAG) pc.lanes_postpone += (unsigned long long)__popcll(__ballot(leaf));
        if (leaf) {
            postpone_leaf<XBOX(WIDE)>(T, spill);
            if (track) steps++;
        }
        if (RT_DIAG) pc.iters++;
    }
    DIAG_ADD(pc.interior, t0);
    if (RT_DIAG) {
        pc.lanes_leaf_tlas += (unsigned long long)__popcll(__ballot(T.tracing && T.pleaf != REF_NONE && !(T.pleaf & REF_BLAS)));
        pc.lanes_leaf_blas += (unsigned long long)__popcll(__ballot(T.tracing && T.pleaf != REF_NONE && (T.pleaf & REF_BLAS)));
    }
    DIAG_T(t1);
    if (T.tracing && T.pleaf != REF_NONE) {
        const uint32_t chained = spec_leaf_phase<COUNT, WIDE>(T, sc, spill, cnt);
        if (track) steps += 1u + chained;
        if (T.tracing && (T.cur & REF_LEAF) && T.cur != REF_NONE) {     // (the leaf phase cleared tracing on REF_NONE)
            postpone_leaf<XBOX(WIDE)>(T, spill);
            if (track) steps++;
        }
    }
    DIAG_ADD(pc.leaf, t1);
}

template <bool COUNT, int XB = XD_CULL>
__device__ __forceinline__ bool trace(const SceneGPU &sc, const f3 &o, const f3 &d, Hit &hit, Trav &T, SEnt *spill,
                                      LaneCount &cnt) {
    trav_init<XB>(T, *sc.tlas_root, o, d);
    while (T.tracing) trav_step<COUNT, XB>(T, sc, spill, cnt);
    hit = T.hit;
    return T.found;
}
