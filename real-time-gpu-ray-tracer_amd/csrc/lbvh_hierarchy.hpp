// lbvh_hierarchy.hpp — from sorted Morton codes to the binary radix tree with its node boxes (lbvh.hip maps the
// headers).  Three builders, by tree size: Karras' per-node searches (karras_kernel) with a single-workgroup climb
// for the boxes (bottom_up_local_kernel) for trees of <= LOCAL_MAX items; Apetrei's bottom-up climb, which finds the
// hierarchy and the boxes together, for larger ones: per chunk in LDS (hierarchy_chunk_kernel), then device-wide
// (hierarchy_top_kernel).  All three write the same arrays: child, range, nbox, height, kept, at Karras node indices.
#pragma once
#include "lbvh_sort.hpp"

namespace rtamd::lbvh {

// δ of Karras 2012 for two sorted positions a != b holding codes ka, kb: the length of the common prefix of the codes,
// and of the positions behind equal codes (so no two δ along a tree are equal)
__device__ __forceinline__ int code_delta(uint32_t ka, uint32_t kb, uint32_t a, uint32_t b) {
    if (ka != kb) return __clz(ka ^ kb);
    return 32 + __clz(a ^ b);
}

// Karras 2012, one thread per interior node.  Local indices are positions inside the segment.  The sorted codes
// within KWIN positions of the workgroup's own are staged in LDS first: nearly every node's searches stay inside
// that window (a range of <= KWIN / 2 items), so a search step is an LDS read, not a dependent global load.
// (tlas_small_kernel runs the same per-node search over its LDS keys; as one function the two kernels' code changes.)
constexpr int KWIN = 256;
__global__ __launch_bounds__(BLOCK) void karras_kernel(const LbvhSeg *segs, const uint32_t *seg_of, const uint32_t *keys,
                                                       uint32_t n, uint32_t *child, uint32_t *parent, uint32_t *parent_leaf,
                                                       uint32_t *range, uint32_t *flag, const uint32_t *vals, RawPrimsGPU raw,
                                                       PrimOutGPU out, const uint32_t *item_member, const TriHot *stage,
                                                       uint32_t gather, uint32_t small_only) {
    __shared__ uint32_t skey[BLOCK + 2 * KWIN];
    if (small_only) {               // trees of > LOCAL_MAX items: hierarchy_chunk_kernel (block-uniform exit)
        const uint32_t p0 = blockIdx.x * BLOCK, p1 = min(p0 + BLOCK, n) - 1u;
        const uint32_t s0 = seg_of[p0];
        if (s0 == seg_of[p1] && segs[s0].count > LOCAL_MAX) return;
    }
    const int64_t w0 = (int64_t)blockIdx.x * BLOCK - KWIN;       // position of skey[0]
    for (int k = threadIdx.x; k < BLOCK + 2 * KWIN; k += BLOCK) {
        const int64_t q = w0 + k;
        skey[k] = (q >= 0 && q < (int64_t)n) ? keys[q] : 0u;
    }
    __syncthreads();
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const LbvhSeg S = segs[seg_of[p]];
    if (small_only && S.count > LOCAL_MAX) return;
    // fused BLAS gather (build() with raw / out): item p's leaf-ordered record; its loads overlap the searches below
    if (gather) gather_item(S, p, vals, raw, out, item_member, stage);
    const int m = (int)S.count;
    const int i = (int)(p - S.item_base);
    if (m == 1) { parent_leaf[p] = NONE; return; }
    if (i >= m - 1) return;
    const auto key = [&](int a) -> uint32_t {                    // code at segment position a (0 <= a < m)
        const int64_t pos = (int64_t)S.item_base + a, o = pos - w0;
        return (o >= 0 && o < BLOCK + 2 * KWIN) ? skey[o] : keys[pos];
    };
    const uint32_t ki = key(i);
    auto delta = [&](int a, int b) -> int {                      // a == i throughout
        if (b < 0 || b >= m) return -1;
        return code_delta(ki, key(b), (uint32_t)a, (uint32_t)b);
    };
    const int d = (delta(i, i + 1) - delta(i, i - 1)) >= 0 ? 1 : -1;
    const int dmin = delta(i, i - d);
    int lmax = 2;
    while (delta(i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1)
        if (delta(i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = delta(i, j);
    int s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + (d < 0 ? -1 : 0);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const uint32_t g = S.node_base + (uint32_t)i;
    uint32_t c0, c1;
    if (lo == gamma) { c0 = LEAF_BIT | (S.item_base + (uint32_t)gamma); parent_leaf[S.item_base + gamma] = g; }
    else { c0 = S.node_base + (uint32_t)gamma; parent[c0] = g; }
    if (hi == gamma + 1) { c1 = LEAF_BIT | (S.item_base + (uint32_t)gamma + 1); parent_leaf[S.item_base + gamma + 1] = g; }
    else { c1 = S.node_base + (uint32_t)gamma + 1; parent[c1] = g; }
    child[2 * g] = c0;
    child[2 * g + 1] = c1;
    range[2 * g] = S.item_base + (uint32_t)lo;
    range[2 * g + 1] = S.item_base + (uint32_t)hi;
    flag[g] = 0;
    if (i == 0) parent[g] = NONE;
}

// ---- bottom-up box union -------------------------------------------------------------------------
// Each leaf climbs; the second thread to reach a node finishes it (union of the two child boxes,
// height) and climbs on.  Trees of <= LOCAL_MAX items (every particle BLAS, small TLASes) are
// finished by one workgroup with node boxes and arrival counters in LDS, so the hand-off between
// the two arriving threads is a workgroup-scope one.  Larger trees end in a device-wide pass
// (hierarchy_top_kernel), where the two threads may sit on different XCDs (per-XCD L2s are not
// coherent): the finished node is published with write-through (sc1) stores, drained (s_waitcnt
// vmcnt(0)) before the arrival's agent-scope atomic, and the second arriver reads it with sc1
// loads — no __threadfence() (an L2 writeback + invalidate per step, MI355X_MICROARCH.md § visibility).
__device__ __forceinline__ void union_children(const uint32_t *child, uint32_t g, const uint32_t *vals, const float *item_box,
                                               float *b, uint32_t &h, const float *node_box_lds, const uint32_t *height_lds,
                                               uint32_t node_base) {
    h = 0;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const uint32_t ch = child[2 * g + c];
        float cb[6];
        uint32_t chh = 0;
        if (ch & LEAF_BIT) {
            const float2 *src = reinterpret_cast<const float2 *>(item_box + 6 * (size_t)vals[ch & ~LEAF_BIT]);
#pragma unroll
            for (int k = 0; k < 3; k++) { const float2 v = src[k]; cb[2 * k] = v.x; cb[2 * k + 1] = v.y; }
        } else {
            const uint32_t l = ch - node_base;
#pragma unroll
            for (int k = 0; k < 6; k++) cb[k] = node_box_lds[6 * l + k];
            chh = height_lds[l];
        }
        if (c == 0) {
#pragma unroll
            for (int k = 0; k < 6; k++) b[k] = cb[k];
        } else {
            merge_into(b, cb);
        }
        h = chh > h ? chh : h;
    }
}

__global__ __launch_bounds__(BLOCK) void bottom_up_local_kernel(const LbvhSeg *segs, const uint32_t *vals, const float *item_box,
                                                                const uint32_t *child, const uint32_t *parent,
                                                                const uint32_t *parent_leaf, const uint32_t *range,
                                                                float *nbox, uint32_t *height, uint32_t *kept) {
    __shared__ float sbox[(LOCAL_MAX - 1) * 6];
    __shared__ uint32_t sheight[LOCAL_MAX - 1];
    __shared__ uint32_t sflag[LOCAL_MAX - 1];
    const LbvhSeg S = segs[blockIdx.x];
    if (S.count < 2 || S.count > LOCAL_MAX) return;                    // block-uniform
    const uint32_t m = S.count, ni = m - 1;
    for (uint32_t k = threadIdx.x; k < ni; k += BLOCK) sflag[k] = 0;
    __syncthreads();
    for (uint32_t li = threadIdx.x; li < m; li += BLOCK) {
        uint32_t g = parent_leaf[S.item_base + li];
        while (g != NONE) {
            const uint32_t l = g - S.node_base;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (atomicAdd(&sflag[l], 1u) == 0u) break;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            float b[6];
            uint32_t h;
            union_children(child, g, vals, item_box, b, h, sbox, sheight, S.node_base);
            const uint32_t size = range[2 * g + 1] - range[2 * g] + 1u;
#pragma unroll
            for (int k = 0; k < 6; k++) sbox[6 * l + k] = b[k];
            sheight[l] = size > S.leaf_cap ? h + 1u : 0u;
            g = parent[g];
        }
    }
    __syncthreads();
    for (uint32_t l = threadIdx.x; l < ni; l += BLOCK) {
        const uint32_t g = S.node_base + l;
#pragma unroll
        for (int k = 0; k < 6; k++) nbox[6 * (size_t)g + k] = sbox[6 * l + k];
        height[g] = sheight[l];
        kept[g] = (range[2 * g + 1] - range[2 * g] + 1u) > S.leaf_cap ? 1u : 0u;
    }
}

// Large trees (> LOCAL_MAX items, e.g. C5's 10 M-triangle group BLAS): hierarchy_chunk_kernel / hierarchy_top_kernel
// below.  (One device-wide pass over all 10 M nodes took 1.7 ms per C5 rebuild: every level an agent-scope round trip;
// rounds 3-5 ran karras_kernel over them and then a chunk climb over its parent arrays: 0.42 + 0.47 ms per C5 rebuild
// against 0.78 for the two kernels below, gather included, profiles/r06/hierarchy/.)
#ifndef LBVH_CHUNK
#define LBVH_CHUNK 1024                         // 2048-item chunks (~150 KB of LDS, one workgroup per CU): 2.33 against
#endif                                          // 2.17 ms per C5 rebuild (round 6, Karras chunks); 512: equal, 256: +0.27 ms
#ifndef LBVH_TOP_BLOCKS
#define LBVH_TOP_BLOCKS 4096                    // hierarchy_top_kernel's grid (its gather wants the waves; 256: +0.2 ms)
#endif
constexpr uint32_t CHUNK = LBVH_CHUNK;         // sorted items per workgroup
constexpr uint32_t CHUNK_THREADS = CHUNK < 1024 ? CHUNK : 1024;   // the chunk kernel's workgroup: CHUNK / CHUNK_THREADS items per thread
constexpr uint32_t CHUNK_PER = CHUNK / CHUNK_THREADS;
static_assert(CHUNK % CHUNK_THREADS == 0, "whole items per thread");

// ---- large trees without the Karras pass: hierarchy and boxes in one bottom-up climb ------------------------------
// Apetrei, "Fast and Simple Agglomerative LBVH Construction" (CGVC 2014): over the sorted codes, a finished node
// [l, r] is its parent's LEFT child iff l == 0 or (r != m - 1 and δ(r, r + 1) > δ(l - 1, l)) — the parent takes the
// neighbour sharing the longer prefix (δ as karras_kernel's: code prefix, then the position's, so no two adjacent δ
// are equal) — and the parent's split lies at r (left child) or l - 1 (right child).  That is the same binary radix
// tree Karras' per-node searches build, and the Karras index of every node follows from it locally: a left child's
// index is its last position, a right child's its first (the root's is 0), and the children of the node split at γ
// are Karras nodes / leaves γ and γ + 1.  So each leaf climbs, the second arrival at a split finishes the parent
// (range, children, box, height) and writes it at its Karras index: the arrays karras_kernel + a climb over its parent
// arrays produce, bit for bit, without the searches, the parent arrays or a second pass over the chunk (tests/test_gpu_lbvh.py
// compares every node with the restatement).  Arrival bits per split: 1 / 2 = the left / right child arrived, 4 / 8 =
// that child is a leaf.
struct SegKeys {                // the top pass's view of one tree's sorted codes (the chunk pass stages δ in LDS)
    const uint32_t *keys;       // sorted codes (global)
    uint32_t base;              // the segment's first sorted position
    int m;                      // the segment's items
};
__device__ __forceinline__ uint32_t seg_key(const SegKeys &K, int a) { return K.keys[(size_t)K.base + a]; }
__device__ __forceinline__ int seg_delta(const SegKeys &K, int a, int b) {      // 0 <= a < m
    if (b < 0 || b >= K.m) return -1;
    return code_delta(seg_key(K, a), seg_key(K, b), (uint32_t)a, (uint32_t)b);
}
__device__ __forceinline__ bool left_child(const SegKeys &K, int l, int r) {
    return l == 0 || (r != K.m - 1 && seg_delta(K, r, r + 1) > seg_delta(K, l - 1, l));
}

// Chunk pass: one workgroup per CHUNK sorted positions finishes every node whose range lies inside the chunk (LDS
// arrivals, node records at their Karras index in LDS), and also writes the chunk's leaf-ordered primitive records
// (karras_kernel's fused gather).  A climb whose parent split has a child outside the chunk, and every split that got
// only one of its arrivals here, go to the top pass as (split, bits) arrivals.
__global__ __launch_bounds__(CHUNK_THREADS) void hierarchy_chunk_kernel(const LbvhSeg *segs, const uint32_t *seg_of,
                                                                        const uint32_t *keys, const uint32_t *vals,
                                                                        const float *item_box, uint32_t n, uint32_t *child,
                                                                        uint32_t *range, float *nbox, uint32_t *height,
                                                                        uint32_t *kept, uint32_t *frontier) {
    __shared__ int sdel[CHUNK + 1];             // δ(q, q + 1) for positions q = lo - 1 .. lo + CHUNK - 1 (-1 across trees)
    __shared__ float sleaf[CHUNK * 6];          // the chunk's item boxes, in sorted order
    __shared__ float sbox[CHUNK * 6];           // node boxes, at the node's Karras index
    __shared__ uint32_t sheight[CHUNK];
    __shared__ uint2 srl[CHUNK];                // node range (segment-local first, last); x = NONE: not finished here
    __shared__ uint32_t ssplit[CHUNK];          // node split (segment-local)
    __shared__ uint32_t sarr[CHUNK];            // arrival bits per split position
    constexpr uint32_t FRONT_LDS = 256;         // this chunk's arrivals for the top pass (more go direct)
    __shared__ uint2 sfront[FRONT_LDS];
    __shared__ uint32_t sfront_n, sfront_at;
    const uint32_t lo = blockIdx.x * CHUNK;
    if (threadIdx.x == 0) sfront_n = 0;
    // an arrival for the top pass: into this chunk's LDS list while it has room, else straight into the global one
    const auto front_push = [&](uint32_t P, uint32_t bits) {
        const uint32_t k = atomicAdd(&sfront_n, 1u);
        if (k < FRONT_LDS) sfront[k] = make_uint2(P, bits);
        else {
            const uint32_t at = atomicAdd(frontier, 1u);
            frontier[1 + 2 * at] = P;
            frontier[2 + 2 * at] = bits;
        }
    };
    // the parent rule compares only adjacent δ's: each is computed once here (seg_delta's value) instead of from four
    // staged codes per climb step
    for (uint32_t k = threadIdx.x; k < CHUNK + 1; k += CHUNK_THREADS) {
        const int64_t q = (int64_t)lo - 1 + k;
        int d = -1;
        if (q >= 0 && q + 1 < (int64_t)n) {
            const uint32_t s0 = seg_of[q];
            if (s0 == seg_of[q + 1]) {
                const uint32_t ka = keys[q], kb = keys[q + 1], a = (uint32_t)q - segs[s0].item_base;
                d = code_delta(ka, kb, a, a + 1u);
            }
        }
        sdel[k] = d;
    }
    bool big[CHUNK_PER];
    LbvhSeg S[CHUNK_PER];
#pragma unroll
    for (uint32_t j = 0; j < CHUNK_PER; j++) {
        const uint32_t l = threadIdx.x + j * CHUNK_THREADS, p = lo + l;
        sarr[l] = 0;
        srl[l].x = NONE;
        const uint32_t seg = p < n ? seg_of[p] : NONE;
        big[j] = seg != NONE && segs[seg].count > LOCAL_MAX;   // else karras_kernel + bottom_up_local_kernel
        if (big[j]) {
            S[j] = segs[seg];
            const float2 *src = reinterpret_cast<const float2 *>(item_box + 6 * (size_t)vals[p]);
#pragma unroll
            for (int k = 0; k < 3; k++) { const float2 v = src[k]; sleaf[6 * l + 2 * k] = v.x; sleaf[6 * l + 2 * k + 1] = v.y; }
        }
    }
    __syncthreads();
    for (uint32_t j = 0; j < CHUNK_PER; j++) {
        if (!big[j]) continue;
        const uint32_t p = lo + threadIdx.x + j * CHUNK_THREADS;
        const LbvhSeg &Sj = S[j];
        const int m = (int)Sj.count;
        const int off = (int)((int64_t)Sj.item_base - (int64_t)lo + 1);   // sdel[off + i] = δ(i, i + 1), segment-local i
        const auto left_child_local = [&](int l, int r) {
            return l == 0 || (r != m - 1 && sdel[off + r] > sdel[off + l - 1]);
        };
        int l = (int)(p - Sj.item_base), r = l;
        bool leaf = true, left = left_child_local(l, r);
        for (;;) {
            const int gam = left ? r : l - 1;
            const uint32_t P = Sj.item_base + (uint32_t)gam;       // the split: children at positions P, P + 1
            const uint32_t bits = (left ? 1u : 2u) | (leaf ? (left ? 4u : 8u) : 0u);
            if (P < lo || P + 1 >= lo + CHUNK) {                 // a child outside the chunk: the top pass's
                front_push(P, bits);
                break;
            }
            const uint32_t sl = P - lo, sr = sl + 1;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            const uint32_t old = atomicOr(&sarr[sl], bits);
            if (old == 0u) break;                                 // first arrival: the sibling finishes the parent
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const uint32_t a = old | bits;
            const int lL = (a & 4u) ? gam : (int)srl[sl].x;
            const int rR = (a & 8u) ? gam + 1 : (int)srl[sr].y;
            const float *c0 = (a & 4u) ? sleaf + 6 * sl : sbox + 6 * sl;
            const float *c1 = (a & 8u) ? sleaf + 6 * sr : sbox + 6 * sr;
            float b[6], t[6];
#pragma unroll
            for (int k = 0; k < 6; k++) { b[k] = c0[k]; t[k] = c1[k]; }
            merge_into(b, t);                                     // union_children's order
            const uint32_t h0 = (a & 4u) ? 0u : sheight[sl], h1 = (a & 8u) ? 0u : sheight[sr];
            const uint32_t h = h0 > h1 ? h0 : h1;
            const bool root = lL == 0 && rR == m - 1;
            const bool nleft = !root && left_child_local(lL, rR);
            const uint32_t slot = Sj.item_base + (uint32_t)(root ? 0 : (nleft ? rR : lL)) - lo;
            const uint32_t size = (uint32_t)(rR - lL) + 1u;
#pragma unroll
            for (int k = 0; k < 6; k++) sbox[6 * slot + k] = b[k];
            sheight[slot] = size > Sj.leaf_cap ? h + 1u : 0u;
            ssplit[slot] = (uint32_t)gam;
            srl[slot] = make_uint2((uint32_t)lL, (uint32_t)rR);
            if (root) break;
            l = lL; r = rR; leaf = false; left = nleft;
        }
    }
    __syncthreads();
    // splits that got one arrival here: the other child finishes in the top pass
#pragma unroll
    for (uint32_t j = 0; j < CHUNK_PER; j++) {
        const uint32_t l = threadIdx.x + j * CHUNK_THREADS;
        const uint32_t a = sarr[l];
        if (a != 0u && (a & 3u) != 3u) front_push(lo + l, a);
    }
    __syncthreads();
    const uint32_t nf = sfront_n < FRONT_LDS ? sfront_n : FRONT_LDS;   // one global reservation per chunk
    if (threadIdx.x == 0 && nf) sfront_at = atomicAdd(frontier, nf);
    __syncthreads();
    if (threadIdx.x < nf) {
        frontier[1 + 2 * (sfront_at + threadIdx.x)] = sfront[threadIdx.x].x;
        frontier[2 + 2 * (sfront_at + threadIdx.x)] = sfront[threadIdx.x].y;
    }
#pragma unroll
    for (uint32_t j = 0; j < CHUNK_PER; j++) {
        const uint32_t l = threadIdx.x + j * CHUNK_THREADS, p = lo + l;
        const uint2 rl = srl[l];
        if (big[j] && rl.x != NONE) {                         // the node at this Karras position finished here
            const LbvhSeg &Sj = S[j];
            const uint32_t g = Sj.node_base + (p - Sj.item_base), gam = ssplit[l];
            child[2 * g] = rl.x == gam ? (LEAF_BIT | (Sj.item_base + gam)) : Sj.node_base + gam;
            child[2 * g + 1] = rl.y == gam + 1 ? (LEAF_BIT | (Sj.item_base + gam + 1)) : Sj.node_base + gam + 1;
            range[2 * g] = Sj.item_base + rl.x;
            range[2 * g + 1] = Sj.item_base + rl.y;
#pragma unroll
            for (int k = 0; k < 6; k++) nbox[6 * (size_t)g + k] = sbox[6 * l + k];
            height[g] = sheight[l];
            kept[g] = (rl.y - rl.x + 1u) > Sj.leaf_cap ? 1u : 0u;
        }
    }
}

// Top pass: one climb per recorded arrival, device-wide, with the hand-off described above bottom_up_local_kernel (node records published
// with write-through stores, drained before the arrival's agent-scope atomic, read with sc1 loads).  Arrival bits per
// split in `flag` (indexed by split position); the second arrival clears them for the next build.
__device__ __forceinline__ uint32_t ld_sc1(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(uint32_t *p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// a node box (6 floats, 8-byte aligned) as three 64-bit sc1 accesses
__device__ __forceinline__ void ld_box_sc1(const float *box, float *out) {
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(box);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const unsigned long long v = __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out[2 * k] = __uint_as_float((uint32_t)v);
        out[2 * k + 1] = __uint_as_float((uint32_t)(v >> 32));
    }
}
__device__ __forceinline__ void st_box_sc1(float *box, const float *b) {
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(box);
#pragma unroll
    for (int k = 0; k < 3; k++)
        __hip_atomic_store(dst + k, (unsigned long long)__float_as_uint(b[2 * k]) |
                                        ((unsigned long long)__float_as_uint(b[2 * k + 1]) << 32),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void hierarchy_top_kernel(const LbvhSeg *segs, const uint32_t *seg_of, const uint32_t *keys, const uint32_t *vals,
                                     const float *item_box, uint32_t *child, uint32_t *range, float *nbox, uint32_t *height,
                                     uint32_t *kept, uint32_t *flag, const uint32_t *frontier, uint32_t n, RawPrimsGPU raw,
                                     PrimOutGPU out, const uint32_t *item_member, const TriHot *stage, uint32_t gather) {
    const uint32_t count = frontier[0];
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < count; i += gridDim.x * BLOCK) {
        uint32_t P = frontier[1 + 2 * i], bits = frontier[2 + 2 * i];
        const LbvhSeg S = segs[seg_of[P]];
        const SegKeys K = {keys, S.item_base, (int)S.count};
        for (;;) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this lane's sc1 stores have landed
            const uint32_t old = atomicOr(&flag[P], bits);
            if (old == 0u) break;
            flag[P] = 0u;                                              // no other arrival at P in this build
            const uint32_t a = old | bits;
            const int gam = (int)(P - S.item_base);
            const uint32_t g0 = S.node_base + (uint32_t)gam, g1 = g0 + 1u;
            float b[6], t[6];
            uint32_t h = 0;
            int lL, rR;
            if (a & 4u) {
                lL = gam;
                const float *src = item_box + 6 * (size_t)vals[P];
#pragma unroll
                for (int k = 0; k < 6; k++) b[k] = src[k];
            } else {
                lL = (int)(ld_sc1(range + 2 * (size_t)g0) - S.item_base);
                ld_box_sc1(nbox + 6 * (size_t)g0, b);
                h = ld_sc1(height + g0);
            }
            if (a & 8u) {
                rR = gam + 1;
                const float *src = item_box + 6 * (size_t)vals[P + 1];
#pragma unroll
                for (int k = 0; k < 6; k++) t[k] = src[k];
            } else {
                rR = (int)(ld_sc1(range + 2 * (size_t)g1 + 1) - S.item_base);
                ld_box_sc1(nbox + 6 * (size_t)g1, t);
                const uint32_t h1 = ld_sc1(height + g1);
                h = h1 > h ? h1 : h;
            }
            merge_into(b, t);
            const bool root = lL == 0 && rR == (int)S.count - 1;
            const bool nleft = !root && left_child(K, lL, rR);
            const uint32_t g = S.node_base + (uint32_t)(root ? 0 : (nleft ? rR : lL));
            const uint32_t size = (uint32_t)(rR - lL) + 1u;
            const bool keep = size > S.leaf_cap;
            st_box_sc1(nbox + 6 * (size_t)g, b);
            st_sc1(height + g, keep ? h + 1u : 0u);
            st_sc1(range + 2 * (size_t)g, S.item_base + (uint32_t)lL);
            st_sc1(range + 2 * (size_t)g + 1, S.item_base + (uint32_t)rR);
            child[2 * (size_t)g] = (a & 4u) ? (LEAF_BIT | P) : g0;
            child[2 * (size_t)g + 1] = (a & 8u) ? (LEAF_BIT | (P + 1u)) : g1;
            kept[g] = keep ? 1u : 0u;
            if (root) break;
            P = S.item_base + (uint32_t)(nleft ? rR : lL - 1);
            bits = nleft ? 1u : 2u;
        }
    }
    // the large trees' leaf-ordered primitive records (karras_kernel's fused gather for the small ones): bandwidth
    // work that fills the issue slots the climbs above leave idle while they wait on their hand-offs (on a side stream
    // beside the chunk and top kernels instead: rebuild 1.97 -> 2.06 ms, C5 frame 8.3 ms; profiles/r06/hierarchy/)
    if (gather)
        for (uint32_t p = blockIdx.x * BLOCK + threadIdx.x; p < n; p += gridDim.x * BLOCK) {
            const LbvhSeg S = segs[seg_of[p]];
            if (S.count > LOCAL_MAX) gather_item(S, p, vals, raw, out, item_member, stage);
        }
}

}  // namespace rtamd::lbvh
