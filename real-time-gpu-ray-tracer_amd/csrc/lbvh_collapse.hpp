// lbvh_collapse.hpp — the 4-wide form of a built forest (lbvh.hip maps the headers): quad q from node pair q, by one
// workgroup per tree or, for forests with a very large tree, by one thread per pair.
#pragma once
#include "lbvh_emit.hpp"

namespace rtamd::lbvh {

// ---- 4-wide collapse of a built forest (the quad form the FAST persistent kernel traverses) -------
// Restates flatten_tree_wide (bvh_build.hpp) on the GPU: the quad of node pair q holds q's two binary
// levels as two halves (layout.hpp NodeQuad) — slots 0, 1 = the left child's children, slots 2, 3 = the
// right child's, a leaf child in its half's first slot and an empty slot with a copy of its box — so a ray
// descends half as many dependent levels and the kernel still visits the binary tree's order; leaves and
// boxes are the binary tree's.  Quad q is the quad rooted at node pair q (pair indices are unique across
// the forest, so the interior refs the pairs hold are also the quads' refs, and a tree's quad root ref
// equals its pair root ref).  One workgroup per tree walks it level by level: a frontier of quad roots in
// LDS (global scratch, this tree's pair range, for trees of more than LDS_FRONT pairs).
constexpr uint32_t LDS_FRONT = 1024;

__device__ __forceinline__ NodeQuad collapse_pair(const NodePair *pairs, uint32_t q) {
    const NodePair P = pairs[q];
    NodeQuad Q;
    for (uint32_t h = 0; h < 2; h++) {
        const float *b = h ? P.c1 : P.c0;
        const uint32_t r = h ? P.ref1 : P.ref0;
        if (r & REF_LEAF) {
            quad_set_slot(Q, 2 * h, b, r);
            quad_set_slot(Q, 2 * h + 1, b, REF_EMPTY);
        } else {
            const NodePair C = pairs[r & REF_INDEX_MASK];
            quad_set_slot(Q, 2 * h, C.c0, C.ref0);
            quad_set_slot(Q, 2 * h + 1, C.c1, C.ref1);
        }
    }
    return Q;
}

__global__ __launch_bounds__(BLOCK) void collapse_wide_kernel(const LbvhSeg *segs, const TreeRoot *roots, const NodePair *pairs,
                                                              NodeQuad *quads, uint32_t *scratch, uint32_t scratch_half,
                                                              TreeRoot *roots_wide) {
    __shared__ uint32_t lds_front[2][LDS_FRONT];
    __shared__ uint32_t n_cur, n_next;
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const TreeRoot R = roots[s];
    if (roots_wide && t == 0) roots_wide[s] = R;              // quad root ref == pair root ref
    if ((R.ref & REF_LEAF) || R.ref == NONE) return;          // a leaf (or empty) tree has no quads
    const uint32_t root = R.ref & REF_INDEX_MASK;
    const uint32_t max_pairs = segs[s].count > 1 ? segs[s].count - 1 : 1;
    uint32_t *front[2];
    if (max_pairs <= LDS_FRONT) { front[0] = lds_front[0]; front[1] = lds_front[1]; }
    else {          // this tree's own pair range [root, root + its pairs): a frontier never holds more
        front[0] = scratch + root;
        front[1] = scratch + scratch_half + root;
    }
    if (t == 0) { front[0][0] = root; n_cur = 1; n_next = 0; }
    __syncthreads();
    uint32_t cur = 0;
    while (n_cur > 0) {
        const uint32_t nc_level = n_cur;
        for (uint32_t i = t; i < nc_level; i += BLOCK) {
            const uint32_t q = front[cur][i];
            const NodeQuad Q = collapse_pair(pairs, q);
            for (uint32_t k = 0; k < 4; k++)
                if (Q.ref[k] != REF_EMPTY && !(Q.ref[k] & REF_LEAF))
                    front[cur ^ 1][atomicAdd(&n_next, 1u)] = Q.ref[k] & REF_INDEX_MASK;
            store16<8>(quads + q, Q);
        }
        __syncthreads();
        if (t == 0) { n_cur = n_next; n_next = 0; }
        cur ^= 1;
        __syncthreads();
    }
}

// The same quads for forests with a large tree (an instance group's merged BLAS: C5's 10 M triangles in one
// tree would keep the per-tree kernel's single workgroup walking level by level for ~60 ms): quad q is a pure
// function of node pair q (its children's children, collapse_pair), so every pair gets
// its quad, one thread each; the quads of pairs absorbed into a parent's quad are written but never reached.
__global__ void collapse_all_kernel(const NodePair *pairs, const uint32_t *n_pairs, NodeQuad *quads) {
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= *n_pairs) return;
    const NodeQuad Q = collapse_pair(pairs, q);
    store16<8>(quads + q, Q);
}

__global__ void copy_roots_kernel(const TreeRoot *roots, uint32_t n, TreeRoot *roots_wide) {
    const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
    if (s < n) roots_wide[s] = roots[s];                        // quad root ref == pair root ref
}

}  // namespace rtamd::lbvh
