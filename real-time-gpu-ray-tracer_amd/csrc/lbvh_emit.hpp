// lbvh_emit.hpp — from the binary hierarchy to the traversal's layout (lbvh.hip maps the headers): every kept interior
// node becomes a NodePair at its scanned pair index (subtrees of <= leaf_cap items are leaf refs), every tree gets its
// root record, and a TLAS build its item per leaf slot.
#pragma once
#include "lbvh_items.hpp"

namespace rtamd::lbvh {

// a whole record of N 16-byte words, written as float4s (node pairs here, quads in lbvh_collapse.hpp)
template <int N, typename T>
__device__ __forceinline__ void store16(T *dst, const T &record) {
    static_assert(sizeof(T) == 16 * N, "the record's size");
    float4 *d = reinterpret_cast<float4 *>(dst);
    const float4 *src = reinterpret_cast<const float4 *>(&record);
#pragma unroll
    for (int k = 0; k < N; k++) d[k] = src[k];
}

__device__ __forceinline__ uint32_t child_ref(const LbvhSeg &S, uint32_t ch, const uint32_t *range, const uint32_t *pidx) {
    if (ch & LEAF_BIT)
        return make_leaf_ref(S.slot_base + ((ch & ~LEAF_BIT) - S.item_base), 1u, S.ptype, S.blas != 0);
    const uint32_t first = range[2 * ch], size = range[2 * ch + 1] - first + 1u;
    if (size <= S.leaf_cap) return make_leaf_ref(S.slot_base + (first - S.item_base), size, S.ptype, S.blas != 0);
    return make_interior_ref(pidx[ch], S.blas != 0);
}
__device__ __forceinline__ const float *child_box(uint32_t ch, const uint32_t *vals, const float *item_box, const float *nbox) {
    return (ch & LEAF_BIT) ? item_box + 6 * (size_t)vals[ch & ~LEAF_BIT] : nbox + 6 * (size_t)ch;
}

__global__ void emit_kernel(const LbvhSeg *segs, const uint32_t *seg_of, const uint32_t *vals, const float *item_box,
                            uint32_t n_int, const uint32_t *child, const uint32_t *range, const float *nbox,
                            const uint32_t *kept, const uint32_t *pidx, NodePair *pairs, uint32_t *pair_count) {
    const uint32_t g = blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_int) return;
    if (g == n_int - 1 && pair_count) *pair_count = pidx[g] + kept[g];
    if (!kept[g]) return;
    const LbvhSeg S = segs[seg_of[range[2 * g]]];
    const uint32_t c0 = child[2 * g], c1 = child[2 * g + 1];
    const float *b0 = child_box(c0, vals, item_box, nbox), *b1 = child_box(c1, vals, item_box, nbox);
    NodePair P;
#pragma unroll
    for (int k = 0; k < 6; k++) { P.c0[k] = b0[k]; P.c1[k] = b1[k]; }
    P.ref0 = child_ref(S, c0, range, pidx);
    P.ref1 = child_ref(S, c1, range, pidx);
    P.pad0 = 0; P.pad1 = 0;
    store16<4>(pairs + pidx[g], P);
}

__global__ void roots_kernel(const LbvhSeg *segs, uint32_t n_segs, const uint32_t *vals, const float *item_box,
                             const float *nbox, const uint32_t *height, const uint32_t *pidx, TreeRoot *roots) {
    const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n_segs) return;
    const LbvhSeg S = segs[s];
    TreeRoot R;
    const float *b;
    if (S.count == 0) {
        for (int k = 0; k < 6; k++) R.box[k] = 0.0f;
        R.ref = NONE; R.height = 0;
        roots[s] = R;
        return;
    }
    if (S.count == 1) {
        b = item_box + 6 * (size_t)vals[S.item_base];
        R.ref = make_leaf_ref(S.slot_base, 1u, S.ptype, S.blas != 0);
        R.height = 0;
    } else {
        b = nbox + 6 * (size_t)S.node_base;
        R.ref = S.count <= S.leaf_cap ? make_leaf_ref(S.slot_base, S.count, S.ptype, S.blas != 0)
                                      : make_interior_ref(pidx[S.node_base], S.blas != 0);
        R.height = height[S.node_base];
    }
    for (int k = 0; k < 6; k++) R.box[k] = b[k];
    roots[s] = R;
}

__global__ void gather_items_kernel(const LbvhSeg *segs, const uint32_t *seg_of, const uint32_t *vals, uint32_t n,
                                    uint32_t *slots) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const LbvhSeg S = segs[seg_of[p]];
    slots[S.slot_base + (p - S.item_base)] = vals[p];
}

}  // namespace rtamd::lbvh
