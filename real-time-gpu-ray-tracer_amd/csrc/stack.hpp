// stack.hpp — the per-lane traversal stack: a top entry held in registers above an LDS window paged to scratch by
// half-pages.
// Includable only from trace_kernel.hip, once, inside namespace rtamd::RT_SUFFIX(dev) (BLOCK, LDS_DEPTH and
// SPILL_DEPTH are defined there).

// a lane's work counters (rt_counters); the stack counts its own overflows
struct LaneCount { uint32_t pairs, tri, sq, quad, inst, hits, overflow; };

// Per-lane traversal stack: a window of LDS_DEPTH entries in LDS (layout [depth][BLOCK]: a wave's
// 64 lanes touch 64 consecutive u64 at any depth -> bank-conflict-free ds_*_b64) backed by a
// scratch array.  When the window fills, its bottom half is paged out to
// scratch, and when it empties the most recent half-page is paged back in.  Median-split trees stay
// within 16 entries up to ~1k instances x 1k triangles, but GPU-built (LBVH) trees over clustered
// centroids are chains and page on nearly every ray: tests/test_gpu_deep_stack.py pins every paging
// site on trees 29 and 10 + 29 levels deep.  Capacity LDS_DEPTH + SPILL_DEPTH = 64 entries, the
// reference's stack size (BLAS.cu:129, TLAS.cu:138), plus the held one.
//
// The newest entry is held in two VGPRs (top_ref / top_tn) and goes to LDS only when another is pushed on top of
// it: an entry popped before the next push (the postponed leaf's successor, the far child of a short ray) never
// makes the ds_write -> ds_read -> s_waitcnt round trip.  Logical order, bottom to top: scratch pages, the LDS
// window, the held entry; tests/test_gpu_stack_top.py walks the held entry over every paging site.
constexpr uint32_t REF_NONE = 0xFFFFFFFFu;   // leaf bit + primitive type 3: never a real ref (Trav::cur: stack exhausted)

struct SEnt { uint32_t ref; uint32_t tn; };   // node ref, entry t (float bits)
// LDS entries are stored packed as u64 (low = ref, high = entry t bits)
typedef __attribute__((address_space(3))) unsigned long long LdsU2;
__device__ __forceinline__ unsigned long long pack(SEnt e) { return (unsigned long long)e.ref | ((unsigned long long)e.tn << 32); }
__device__ __forceinline__ SEnt unpack(unsigned long long v) { SEnt e; e.ref = (uint32_t)v; e.tn = (uint32_t)(v >> 32); return e; }
constexpr int HALF = LDS_DEPTH / 2;

struct Stack {
    LdsU2 *lds;            // &lds_stack[0][tid]; entry k at lds[k * BLOCK]
    int sp;                // entries in the LDS window
    int spilled;           // entries paged out to scratch
    uint32_t top_ref;      // the held (newest) entry's ref, REF_NONE: none held
    uint32_t top_tn;       // its entry t bits
    __device__ __forceinline__ bool held() const { return top_ref != REF_NONE; }
    __device__ __forceinline__ bool empty() const { return !held() && sp == 0 && spilled == 0; }
    __device__ __forceinline__ void clear() { sp = 0; spilled = 0; top_ref = REF_NONE; }
};

// A half-page (HALF entries = 64 B, 16 B-aligned: pages start at multiples of HALF) moves as 16 B pieces; a
// page-in requests all four before the first LDS write.  (A contiguous row per thread in HBM instead of
// lane-swizzled scratch measured 3 % slower with the same WRITE_SIZE: paging is not the write excess)
__device__ __forceinline__ void spill_store(SEnt *dst, const Stack &stk) {
    uint4 *d = reinterpret_cast<uint4 *>(__builtin_assume_aligned(dst, 16));
#pragma unroll
    for (int k = 0; k < HALF; k += 2) {
        const unsigned long long a = stk.lds[k * BLOCK], b = stk.lds[(k + 1) * BLOCK];
        d[k / 2] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
    }
}
__device__ __forceinline__ void spill_load(const SEnt *src, Stack &stk) {
    const uint4 *p = reinterpret_cast<const uint4 *>(__builtin_assume_aligned(src, 16));
#pragma unroll
    for (int k = 0; k < HALF; k += 2) {
        const uint4 v = p[k / 2];
        stk.lds[k * BLOCK] = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
        stk.lds[(k + 1) * BLOCK] = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
    }
}
// Page the bottom half of the LDS window out: when it is full (stack_push), or when fewer than 3 slots are free (the
// quad step's three-entry push: sp > HALF; slots >= sp are free space, moved along harmlessly).  The held entry stays
// where it is: paging moves the LDS window only.
__device__ __forceinline__ void stack_page_out(Stack &stk, SEnt *spill, LaneCount &c) {   // sp > HALF
    if (stk.spilled + HALF > SPILL_DEPTH) {        // deeper than the reference's 64 entries
        c.overflow++;
        stk.spilled = SPILL_DEPTH - HALF;          // the last half-page in scratch is overwritten (result flagged)
    }
    spill_store(spill + stk.spilled, stk);
#pragma unroll
    for (int k = 0; k < HALF; k++) stk.lds[k * BLOCK] = stk.lds[(k + HALF) * BLOCK];   // slots >= sp: don't care
    stk.sp -= HALF;
    stk.spilled += HALF;
}
__device__ __forceinline__ void stack_page_in(Stack &stk, const SEnt *spill) {
    stk.spilled -= HALF;
    spill_load(spill + stk.spilled, stk);
    stk.sp = HALF;
}
// (ref is a real ref, never REF_NONE)
__device__ __forceinline__ void stack_push(Stack &stk, SEnt *spill, uint32_t ref, float tn, LaneCount &c) {
    if (stk.held()) {                              // the held entry makes room: down into the LDS window
        if (stk.sp == LDS_DEPTH) stack_page_out(stk, spill, c);
        SEnt e;
        e.ref = stk.top_ref;
        e.tn = stk.top_tn;
        stk.lds[stk.sp * BLOCK] = pack(e);
        stk.sp++;
    }
    stk.top_ref = ref;
    stk.top_tn = __float_as_uint(tn);
}
__device__ __forceinline__ SEnt stack_pop(Stack &stk, const SEnt *spill) {   // precondition: !empty()
    if (stk.held()) {                              // no LDS access, no wait
        SEnt e;
        e.ref = stk.top_ref;
        e.tn = stk.top_tn;
        stk.top_ref = REF_NONE;
        return e;
    }
    if (stk.sp == 0) stack_page_in(stk, spill);
    --stk.sp;
    return unpack(stk.lds[stk.sp * BLOCK]);
}
// The quad step's push of n = 1..3 entries (a the oldest; those past n are don't-cares): the newest becomes the held
// entry, the previously held one (if any) and the n - 1 older ones go to the LDS slots above the top, oldest first —
// three unconditional stores, without branching on n or on the hold (a slot past the new top is free space, and a
// lane's stores to one slot land in program order).  The caller has made room (stack_page_out when
// sp > LDS_DEPTH - 3): the stores touch slots sp .. sp + 2 and sp grows by at most 3.
__device__ __forceinline__ void stack_push3(Stack &stk, SEnt a, SEnt b, SEnt c, uint32_t n) {
    const int h = stk.held() ? 1 : 0;
    SEnt t;
    t.ref = stk.top_ref;
    t.tn = stk.top_tn;
    stk.lds[stk.sp * BLOCK] = pack(t);
    stk.lds[(stk.sp + h) * BLOCK] = pack(a);
    stk.lds[(stk.sp + h + 1) * BLOCK] = pack(b);
    stk.sp += h + (int)n - 1;
    stk.top_ref = n == 3u ? c.ref : (n == 2u ? b.ref : a.ref);
    stk.top_tn = n == 3u ? c.tn : (n == 2u ? b.tn : a.tn);
}
