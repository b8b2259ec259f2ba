// lbvh_tlas_small.hpp — a small per-frame TLAS by one workgroup: the builder's whole pipeline in LDS, one launch
// (lbvh.hip maps the headers).  Each step names the kernel it stands for; the helpers are the other headers'.
#pragma once
#include "lbvh_collapse.hpp"
#include "lbvh_hierarchy.hpp"

namespace rtamd::lbvh {

// ---- the whole per-frame GPU TLAS in one workgroup (GPU-built frames with few TLAS items) ---------------
// The multi-kernel chain (instance deltas -> records -> bounds -> Morton -> radix sort -> Karras -> boxes ->
// scan -> pairs -> roots -> quads -> slots -> slot-ordered records) is ~17 launches on one stream per frame:
// ~100 us of launch gaps for a C2-size TLAS, which bounded GPU-built C2 frames.  With option "group" a GPU-built
// scene's TLAS holds a handful of items (C2: 6, C5: 6 of 9,772 records), so one workgroup runs the same build
// in LDS: the same Morton codes, the stable (key, item) order, Karras' hierarchy, exact box unions, leaf
// collapse, node pairs, quads and slots — over the active records only (inactive ones are left out instead of
// being sorted behind them).
constexpr uint32_t SMALL_BLOCK = 1024;

__global__ __launch_bounds__(SMALL_BLOCK) void tlas_small_kernel(SmallTlasArgs a) {
    __shared__ unsigned long long skey[SMALL_TLAS_MAX];        // (Morton << 32 | live index), sorted
    __shared__ float snbox[(SMALL_TLAS_MAX - 1) * 6];
    __shared__ float sibox[SMALL_TLAS_MAX * 6];               // live item boxes
    __shared__ uint32_t schild[2 * (SMALL_TLAS_MAX - 1)], sparent[SMALL_TLAS_MAX - 1], srange[2 * (SMALL_TLAS_MAX - 1)];
    __shared__ uint32_t sparent_leaf[SMALL_TLAS_MAX], sflag[SMALL_TLAS_MAX - 1], sheight[SMALL_TLAS_MAX - 1];
    __shared__ uint32_t spidx[SMALL_TLAS_MAX], slive[SMALL_TLAS_MAX];
    __shared__ uint32_t scount[SMALL_BLOCK];
    __shared__ uint32_t sbound[6];
    const uint32_t t = threadIdx.x, n = a.n;
    if (t < 6) sbound[t] = bounds_seed(t);
    // 1. the live records (instance_update_kernel computed every record; centroid w != 0 marks an inactive one),
    // in record order: contiguous chunks per thread
    const uint32_t chunk = (n + SMALL_BLOCK - 1) / SMALL_BLOCK, i0 = t * chunk, i1 = min(n, i0 + chunk);
    uint32_t live = 0;
    for (uint32_t i = i0; i < i1; i++) live += a.tcent[i].w == 0.0f ? 1u : 0u;
    scount[t] = live;
    __syncthreads();
    if (t == 0) {                                            // exclusive scan of the per-thread live counts
        uint32_t acc = 0;
        for (uint32_t k = 0; k < SMALL_BLOCK; k++) { const uint32_t v = scount[k]; scount[k] = acc; acc += v; }
        sflag[0] = acc;                                      // (reused below) m
    }
    __syncthreads();
    const uint32_t m = sflag[0];
    uint32_t pos = scount[t];
    for (uint32_t i = i0; i < i1; i++)
        if (a.tcent[i].w == 0.0f && pos < SMALL_TLAS_MAX) slive[pos++] = i;
    __syncthreads();
    if (m == 0 || m > SMALL_TLAS_MAX) {                      // the host checked; nothing to build
        if (t == 0) { *a.pair_count = 0; }
        return;
    }
    // 2. item boxes / centroid bounds over the live items (bounds_kernel), Morton keys (morton_kernel)
    for (uint32_t k = t; k < m; k += SMALL_BLOCK) {
        const uint32_t i = slive[k];
#pragma unroll
        for (int q = 0; q < 6; q++) sibox[6 * k + q] = a.tbox[6 * (size_t)i + q];
        const float4 c = a.tcent[i];
        atomicMin(&sbound[0], f2o(c.x)); atomicMax(&sbound[1], f2o(c.x));
        atomicMin(&sbound[2], f2o(c.y)); atomicMax(&sbound[3], f2o(c.y));
        atomicMin(&sbound[4], f2o(c.z)); atomicMax(&sbound[5], f2o(c.z));
    }
    __syncthreads();
    uint32_t np = 1;
    while (np < m) np <<= 1;
    for (uint32_t k = t; k < np; k += SMALL_BLOCK) {
        unsigned long long key = ~0ull;
        if (k < m) {
            const float4 c = a.tcent[slive[k]];
            const uint32_t x = quant10(c.x, o2f(sbound[0]), o2f(sbound[1]));
            const uint32_t y = quant10(c.y, o2f(sbound[2]), o2f(sbound[3]));
            const uint32_t z = quant10(c.z, o2f(sbound[4]), o2f(sbound[5]));
            key = ((unsigned long long)((expand10(x) << 2) | (expand10(y) << 1) | expand10(z)) << 32) | k;   // morton_kernel's code
        }
        skey[k] = key;
    }
    __syncthreads();
    // bitonic sort of (code, item): the radix sort's stable order (local_sort_kernel's network, lbvh_sort.hpp)
    for (uint32_t size = 2; size <= np; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t k = t; k < np; k += SMALL_BLOCK) {
                const uint32_t o = k ^ stride;
                if (o > k) {
                    const unsigned long long x = skey[k], y = skey[o];
                    const bool up = (k & size) == 0;
                    if ((x > y) == up) { skey[k] = y; skey[o] = x; }
                }
            }
            __syncthreads();
        }
    // 3. Karras hierarchy over the sorted codes (karras_kernel's search, lbvh_hierarchy.hpp, over one segment)
    const int mi = (int)m;
    auto code = [&](int i) { return (uint32_t)(skey[i] >> 32); };
    auto delta = [&](int x, int y) -> int {
        if (y < 0 || y >= mi) return -1;
        return code_delta(code(x), code(y), (uint32_t)x, (uint32_t)y);
    };
    for (int i = (int)t; i < mi - 1; i += SMALL_BLOCK) {
        const int d = (delta(i, i + 1) - delta(i, i - 1)) >= 0 ? 1 : -1;
        const int dmin = delta(i, i - d);
        int lmax = 2;
        while (delta(i, i + lmax * d) > dmin) lmax <<= 1;
        int l = 0;
        for (int q = lmax >> 1; q >= 1; q >>= 1)
            if (delta(i, i + (l + q) * d) > dmin) l += q;
        const int j = i + l * d;
        const int dnode = delta(i, j);
        int sp = 0, q = l;
        do {
            q = (q + 1) >> 1;
            if (delta(i, i + (sp + q) * d) > dnode) sp += q;
        } while (q > 1);
        const int gamma = i + sp * d + (d < 0 ? -1 : 0);
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        uint32_t c0, c1;
        if (lo == gamma) { c0 = LEAF_BIT | (uint32_t)gamma; sparent_leaf[gamma] = (uint32_t)i; }
        else { c0 = (uint32_t)gamma; sparent[gamma] = (uint32_t)i; }
        if (hi == gamma + 1) { c1 = LEAF_BIT | (uint32_t)(gamma + 1); sparent_leaf[gamma + 1] = (uint32_t)i; }
        else { c1 = (uint32_t)gamma + 1; sparent[gamma + 1] = (uint32_t)i; }
        schild[2 * i] = c0; schild[2 * i + 1] = c1;
        srange[2 * i] = (uint32_t)lo; srange[2 * i + 1] = (uint32_t)hi;
        sflag[i] = 0;
        if (i == 0) sparent[0] = NONE;
    }
    if (m == 1 && t == 0) sparent_leaf[0] = NONE;
    __syncthreads();
    // 4. exact box unions bottom-up (bottom_up_local_kernel)
    const uint32_t cap = a.leaf_cap;
    const auto box_of = [&](uint32_t ch) -> const float * {     // child ch's box: a live item's or a node's
        return (ch & LEAF_BIT) ? sibox + 6 * (skey[ch & ~LEAF_BIT] & 0xFFFFFFFFu) : snbox + 6 * ch;
    };
    for (uint32_t li = t; li < m && m > 1; li += SMALL_BLOCK) {
        uint32_t g = sparent_leaf[li];
        while (g != NONE) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (atomicAdd(&sflag[g], 1u) == 0u) break;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            float b[6];
            uint32_t h = 0;
            for (int c = 0; c < 2; c++) {
                const uint32_t ch = schild[2 * g + c];
                const float *cb = box_of(ch);
                const uint32_t chh = (ch & LEAF_BIT) ? 0u : sheight[ch];
                if (c == 0) {
                    for (int k = 0; k < 6; k++) b[k] = cb[k];
                } else {
                    merge_into(b, cb);
                }
                h = chh > h ? chh : h;
            }
            const uint32_t size = srange[2 * g + 1] - srange[2 * g] + 1u;
#pragma unroll
            for (int k = 0; k < 6; k++) snbox[6 * g + k] = b[k];
            sheight[g] = size > cap ? h + 1u : 0u;
            g = sparent[g];
        }
    }
    __syncthreads();
    // 5. kept interior nodes -> pair index (exclusive scan), pairs (emit_kernel), root (roots_kernel), slots
    if (t == 0) {
        uint32_t acc = 0;
        for (uint32_t g = 0; g + 1 < m; g++) {
            spidx[g] = acc;
            acc += (srange[2 * g + 1] - srange[2 * g] + 1u) > cap ? 1u : 0u;
        }
        *a.pair_count = acc;
    }
    __syncthreads();
    auto ref_of = [&](uint32_t ch) -> uint32_t {
        if (ch & LEAF_BIT) return make_leaf_ref(ch & ~LEAF_BIT, 1u, 0u, false);
        const uint32_t first = srange[2 * ch], size = srange[2 * ch + 1] - first + 1u;
        if (size <= cap) return make_leaf_ref(first, size, 0u, false);
        return make_interior_ref(spidx[ch], false);
    };
    for (uint32_t g = t; g + 1 < m; g += SMALL_BLOCK) {
        if ((srange[2 * g + 1] - srange[2 * g] + 1u) <= cap) continue;
        const uint32_t c0 = schild[2 * g], c1 = schild[2 * g + 1];
        const float *b0 = box_of(c0), *b1 = box_of(c1);
        NodePair P;
#pragma unroll
        for (int k = 0; k < 6; k++) { P.c0[k] = b0[k]; P.c1[k] = b1[k]; }
        P.ref0 = ref_of(c0);
        P.ref1 = ref_of(c1);
        P.pad0 = 0; P.pad1 = 0;
        a.pairs[spidx[g]] = P;
    }
    for (uint32_t k = t; k < m; k += SMALL_BLOCK) a.slots[k] = slive[skey[k] & 0xFFFFFFFFu];
    if (t == 0) {
        TreeRoot R;
        const float *b = m == 1 ? sibox : snbox;
        for (int k = 0; k < 6; k++) R.box[k] = b[k];
        R.ref = m == 1 ? make_leaf_ref(0, 1u, 0u, false)
                       : (m <= cap ? make_leaf_ref(0, m, 0u, false) : make_interior_ref(spidx[0], false));
        R.height = m == 1 ? 0u : sheight[0];
        *a.root = R;
        *a.root_wide = R;                                    // quad root ref == pair root ref
    }
    __syncthreads();                                         // pairs and records (global, this workgroup) complete
    // 6. quads (collapse_all_kernel) and the records in leaf-slot order (slot_order_kernel)
    const uint32_t npairs = *a.pair_count;
    for (uint32_t q = t; q < npairs; q += SMALL_BLOCK) {
        const NodeQuad Q = collapse_pair(a.pairs, q);
        a.quads[q] = Q;
    }
    for (uint32_t k = t; k < m; k += SMALL_BLOCK) {
        const uint32_t i = slive[skey[k] & 0xFFFFFFFFu];
        a.hot_s[k] = a.hot[i];
        a.cold_s[k] = a.cold[i];
    }
}

}  // namespace rtamd::lbvh
