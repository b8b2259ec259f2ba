// lbvh.hip — GPU BVH builder (RT_BUILD_LBVH): BLAS forests over primitives and the per-frame TLAS
// over instances, built on the device (interface and pipeline in lbvh.hpp).
//
// Karras, "Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees" (HPG 2012):
// with items sorted by Morton code, interior node i of an n-leaf radix tree covers a key range with
// one end at i; its direction, far end and split follow from the longest-common-prefix function
// δ(i, j) alone, so every interior node is built by one thread with no dependencies.  Here δ is
// evaluated per segment (indices outside the segment give -1), so one launch builds a whole forest
// (9,766 particle BLASes of config C5, or one TLAS).  Equal Morton codes are ordered by sorted
// position (the sort is stable, so by item index), making builds deterministic.
//
// Compiled with -ffp-contract=off: primitive boxes, centroids and the leaf-ordered hot / cold
// records are computed with the reference's float evaluation order (host_math.hpp restates the
// same functions on the host), so a GPU-built leaf holds the same bytes a host build would.
//
// This file is the one translation unit and holds the host side: LbvhBuilder, the two free launchers, and the two
// kernels outside namespace lbvh beside their launchers.  The device code, in namespace rtamd::lbvh, in build order:
//   lbvh_items.hpp       reference boxes / centroids of the primitives, leaf-ordered records (gather_item), constants
//   lbvh_sort.hpp        prep_blas, centroid bounds, Morton codes, the LDS bitonic sort, the rocPRIM configurations;
//                        LOCAL_SORT_MAX and LOCAL_MAX
//   lbvh_hierarchy.hpp   δ, Karras' searches, the single-workgroup climb, the chunk and top passes of large trees
//   lbvh_emit.hpp        node pairs, tree roots, TLAS slot items
//   lbvh_collapse.hpp    the 4-wide quads
//   lbvh_tlas_small.hpp  the whole pipeline for a small TLAS in one workgroup
#include "lbvh_items.hpp"
#include "lbvh_sort.hpp"
#include "lbvh_hierarchy.hpp"
#include "lbvh_emit.hpp"
#include "lbvh_collapse.hpp"
#include "lbvh_tlas_small.hpp"

namespace rtamd {

__global__ void extract_tri_verts_kernel(const rt_triangle *tris, float *verts, size_t first, size_t count) {
    const size_t k = (size_t)blockIdx.x * lbvh::BLOCK + threadIdx.x;
    if (k >= count) return;
    const rt_triangle &t = tris[first + k];
    float *v = verts + 9 * (first + k);
#pragma unroll
    for (int i = 0; i < 3; i++) { v[3 * i] = t.vertex[i].x; v[3 * i + 1] = t.vertex[i].y; v[3 * i + 2] = t.vertex[i].z; }
}

hipError_t extract_tri_verts(const rt_triangle *tris, float *verts, size_t first, size_t count, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(extract_tri_verts_kernel, dim3((uint32_t)((count + lbvh::BLOCK - 1) / lbvh::BLOCK)), dim3(lbvh::BLOCK), 0, stream, tris,
                       verts, first, count);
    return hipGetLastError();
}

hipError_t launch_tlas_small(const SmallTlasArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(lbvh::tlas_small_kernel, dim3(1), dim3(lbvh::SMALL_BLOCK), 0, stream, a);
    return hipGetLastError();
}

// ---- host --------------------------------------------------------------------------------------
using namespace lbvh;

#define LB_TRY(x)                               \
    do {                                        \
        hipError_t e_ = (x);                    \
        if (e_ != hipSuccess) return e_;        \
    } while (0)

void LbvhBuilder::release() {
    for (hipEvent_t &e : stage_ev_)
        if (e) { (void)hipEventDestroy(e); e = nullptr; }
    timing_ = false;
    last_timed_ = false;
    each_buf(*this, [](auto &b) { b.release(); });
    last_count_ = nullptr;
    box_ = nullptr; cent_ = nullptr;
    n_items_ = n_segs_ = 0;
    big_segs_.clear();
}

hipError_t LbvhBuilder::init(const std::vector<LbvhSeg> &segs, hipStream_t stream) {
    release();
    uint64_t n = 0;
    for (const LbvhSeg &s : segs) {
        if (s.item_base != n || s.leaf_cap < 1 || s.leaf_cap > 4) return hipErrorInvalidValue;
        n += s.count;
    }
    if (n >= (1ull << 31) || segs.empty()) return hipErrorInvalidValue;
    n_items_ = (uint32_t)n;
    n_segs_ = (uint32_t)segs.size();
    max_count_ = 0;
    for (const LbvhSeg &sg : segs) max_count_ = sg.count > max_count_ ? sg.count : max_count_;
    big_segs_.clear();
    uint32_t big_max = 0;
    for (const LbvhSeg &sg : segs)
        if (sg.count > LOCAL_SORT_MAX) { big_segs_.push_back({sg.item_base, sg.count}); big_max = std::max(big_max, sg.count); }
    const size_t N = n_items_, NI = max_pairs();
    LB_TRY(segs_.alloc(n_segs_));
    LB_TRY(hipMemcpyAsync(segs_.p, segs.data(), n_segs_ * sizeof(LbvhSeg), hipMemcpyHostToDevice, stream));
    std::vector<uint32_t> seg_of(N);
    for (uint32_t s = 0; s < n_segs_; s++)
        for (uint32_t k = 0; k < segs[s].count; k++) seg_of[segs[s].item_base + k] = s;
    LB_TRY(seg_of_.alloc(N));
    LB_TRY(hipMemcpyAsync(seg_of_.p, seg_of.data(), N * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    LB_TRY(bounds_.alloc(6 * (size_t)n_segs_));
    LB_TRY(k0_.alloc(N)); LB_TRY(k1_.alloc(N)); LB_TRY(v0_.alloc(N)); LB_TRY(v1_.alloc(N));
    LB_TRY(child_.alloc(2 * NI)); LB_TRY(parent_.alloc(NI)); LB_TRY(parent_leaf_.alloc(N));
    LB_TRY(range_.alloc(2 * NI)); LB_TRY(flag_.alloc(N)); LB_TRY(height_.alloc(NI));
    LB_TRY(nbox_.alloc(6 * NI)); LB_TRY(kept_.alloc(NI)); LB_TRY(pidx_.alloc(NI));
    size_t sort_bytes = 0, scan_bytes = 0;
    if (big_max) LB_TRY(rocprim::radix_sort_pairs<BigSortConfig>(nullptr, sort_bytes, k0_.p, k1_.p, v0_.p, v1_.p, big_max, 0, 32, stream));
    LB_TRY(rocprim::exclusive_scan<PairScanConfig>(nullptr, scan_bytes, kept_.p, pidx_.p, 0u, NI, rocprim::plus<uint32_t>(), stream));
    LB_TRY(tmp_.alloc(sort_bytes > scan_bytes ? sort_bytes : scan_bytes));
    // kept/pidx of nodes that no thread visits (none in a valid forest) start defined
    LB_TRY(hipMemsetAsync(kept_.p, 0, NI * sizeof(uint32_t), stream));
    // arrival bits of the top pass (hierarchy_top_kernel clears what it sets)
    LB_TRY(hipMemsetAsync(flag_.p, 0, N * sizeof(uint32_t), stream));
    // synchronous: seg_of (host vector) must outlive the copy
    return hipStreamSynchronize(stream);
}

const char *const LbvhBuilder::STAGE_NAMES[LbvhBuilder::STAGES] = {
    "prep", "bounds", "morton", "sort", "hierarchy_small", "hierarchy_large", "scan", "emit_roots", "collapse"};

hipError_t LbvhBuilder::set_timing(bool on) {
    if (on)
        for (hipEvent_t &e : stage_ev_)
            if (!e) LB_TRY(hipEventCreate(&e));
    timing_ = on;
    return hipSuccess;
}

hipError_t LbvhBuilder::stage_ms(float (&ms)[STAGES]) const {
    if (!last_timed_) return hipErrorNotReady;          // the last build ran without timing: no stale figures
    for (int k = 0; k < STAGES; k++) {
        ms[k] = 0.0f;
        if (!stage_ev_[k] || !stage_ev_[k + 1]) return hipErrorInvalidValue;
        LB_TRY(hipEventSynchronize(stage_ev_[k + 1]));
        LB_TRY(hipEventElapsedTime(&ms[k], stage_ev_[k], stage_ev_[k + 1]));
    }
    return hipSuccess;
}

hipError_t LbvhBuilder::prep_blas_items(const RawPrimsGPU &raw, hipStream_t stream, bool stage_hot) {
    last_timed_ = timing_;
    LB_TRY(mark(EV_START, stream));
    if (!own_box_.p) {
        LB_TRY(own_box_.alloc(6 * (size_t)n_items_));
        LB_TRY(own_cent_.alloc(n_items_));
    }
    if (stage_hot && !stage_.p) LB_TRY(stage_.alloc(n_items_));
    box_ = own_box_.p;
    cent_ = own_cent_.p;
    stage_ready_ = stage_hot;
    hipLaunchKernelGGL(prep_blas_kernel, dim3(blocks_for(n_items_)), dim3(BLOCK), 0, stream, segs_.p, seg_of_.p, n_items_, raw,
                       box_, cent_, stage_hot ? stage_.p : nullptr, item_member_.p);
    LB_TRY(hipGetLastError());
    return mark(EV_PREP, stream);
}

// item -> its member instance + 1 (group segments; 0 elsewhere), found once here instead of by every rebuild's gather
__global__ void member_map_kernel(const LbvhSeg *segs, const uint32_t *seg_of, uint32_t n, const uint32_t *members,
                                  uint32_t *item_member) {
    const uint32_t it = blockIdx.x * BLOCK + threadIdx.x;
    if (it >= n) return;
    const LbvhSeg S = segs[seg_of[it]];
    uint32_t v = 0;
    if (S.member_count) {
        const uint32_t prim = S.prim_base + (it - S.item_base);
        const uint32_t *M = members + 2 * (size_t)S.member_base;
        uint32_t lo = 0, hi = S.member_count;          // last member whose first primitive <= prim
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) / 2;
            if (M[2 * mid] <= prim) lo = mid; else hi = mid;
        }
        v = M[2 * lo + 1] + 1u;
    }
    item_member[it] = v;
}

hipError_t LbvhBuilder::set_members(const std::vector<uint32_t> &pairs, hipStream_t stream) {
    members_.release();
    item_member_.release();
    if (pairs.empty()) return hipSuccess;
    LB_TRY(members_.alloc(pairs.size()));
    LB_TRY(item_member_.alloc(n_items_));
    LB_TRY(hipMemcpyAsync(members_.p, pairs.data(), pairs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(member_map_kernel, dim3(blocks_for(n_items_)), dim3(BLOCK), 0, stream, segs_.p, seg_of_.p, n_items_,
                       members_.p, item_member_.p);
    LB_TRY(hipGetLastError());
    return hipStreamSynchronize(stream);            // `pairs` (host) must outlive the copy
}

size_t LbvhBuilder::workspace_bytes() const {
    size_t bytes = 0;
    each_buf(*this, [&](const auto &b) { bytes += b.bytes(); });
    return bytes;
}

hipError_t LbvhBuilder::set_items(const float *boxes, const float4 *centroids) {
    box_ = const_cast<float *>(boxes);
    cent_ = const_cast<float4 *>(centroids);
    return hipSuccess;
}

hipError_t LbvhBuilder::build(NodePair *pairs, TreeRoot *roots, uint32_t *pair_count, hipStream_t stream,
                              const RawPrimsGPU *raw, const PrimOutGPU *out) {
    if (!box_ || !cent_ || n_items_ == 0) return hipErrorInvalidValue;
    const uint32_t N = n_items_, NI = n_items_ - n_segs_;
    const bool tm = box_ == own_box_.p;             // a BLAS build (prep_blas_items' boxes): stage timing (TLAS builds record nothing)
    hipLaunchKernelGGL(init_bounds_kernel, dim3(blocks_for(6ull * n_segs_)), dim3(BLOCK), 0, stream, bounds_.p, n_segs_);
    {   // ~1024 blocks at most: one LDS-combined atomic set per block (bounds_kernel)
        const uint32_t ipt = std::max<uint32_t>(1u, (uint32_t)((N + (uint64_t)BLOCK * 1024 - 1) / ((uint64_t)BLOCK * 1024)));
        const uint32_t nb = (uint32_t)((N + (uint64_t)BLOCK * ipt - 1) / ((uint64_t)BLOCK * ipt));
        hipLaunchKernelGGL(bounds_kernel, dim3(nb), dim3(BLOCK), 0, stream, seg_of_.p, cent_, N, ipt, bounds_.p);
    }
    if (tm) LB_TRY(mark(EV_BOUNDS, stream));
    hipLaunchKernelGGL(morton_kernel, dim3(blocks_for(N)), dim3(BLOCK), 0, stream, seg_of_.p, cent_, N, bounds_.p, k0_.p, v0_.p);
    LB_TRY(hipGetLastError());
    if (tm) LB_TRY(mark(EV_MORTON, stream));
    size_t bytes = tmp_.n;
    if (big_segs_.size() < n_segs_)
        hipLaunchKernelGGL(local_sort_kernel, dim3(n_segs_), dim3(BLOCK), 0, stream, segs_.p, k0_.p, k1_.p, v1_.p);
    // BLAS codes are 30-bit Morton codes; TLAS items may be inactive (0xFFFFFFFF)
    const int end_bit = tm ? 30 : 32;
    for (const auto &b : big_segs_) {
        bytes = tmp_.n;
        LB_TRY(rocprim::radix_sort_pairs<BigSortConfig>(tmp_.p, bytes, k0_.p + b.first, k1_.p + b.first, v0_.p + b.first,
                                                        v1_.p + b.first, b.second, 0, end_bit, stream));
    }
    if (tm) LB_TRY(mark(EV_SORT, stream));
    // trees of > LOCAL_MAX items: hierarchy_chunk_kernel / hierarchy_top_kernel build them (and gather their records)
    const bool fused = max_count_ > LOCAL_MAX;
    const RawPrimsGPU graw = raw ? *raw : RawPrimsGPU{};
    const PrimOutGPU gout = out ? *out : PrimOutGPU{};
    const TriHot *gstage = stage_ready_ ? stage_.p : nullptr;
    hipLaunchKernelGGL(karras_kernel, dim3(blocks_for(N)), dim3(BLOCK), 0, stream, segs_.p, seg_of_.p, k1_.p, N, child_.p, parent_.p,
                       parent_leaf_.p, range_.p, flag_.p, v1_.p, graw, gout, item_member_.p, gstage, (uint32_t)(raw && out),
                       (uint32_t)fused);
    hipLaunchKernelGGL(bottom_up_local_kernel, dim3(n_segs_), dim3(BLOCK), 0, stream, segs_.p, v1_.p, box_, child_.p, parent_.p,
                       parent_leaf_.p, range_.p, nbox_.p, height_.p, kept_.p);
    if (tm) LB_TRY(mark(EV_HIERARCHY_SMALL, stream));
    if (fused) {
        if (!frontier_.p) LB_TRY(frontier_.alloc(1 + 2 * (size_t)N));    // <= 1 (split, bits) arrival per item
        LB_TRY(hipMemsetAsync(frontier_.p, 0, sizeof(uint32_t), stream));
        hipLaunchKernelGGL(hierarchy_chunk_kernel, dim3((N + CHUNK - 1) / CHUNK), dim3(CHUNK_THREADS), 0, stream, segs_.p, seg_of_.p,
                           k1_.p, v1_.p, box_, N, child_.p, range_.p, nbox_.p, height_.p, kept_.p, frontier_.p);
        hipLaunchKernelGGL(hierarchy_top_kernel, dim3(LBVH_TOP_BLOCKS), dim3(BLOCK), 0, stream, segs_.p, seg_of_.p, k1_.p, v1_.p, box_,
                           child_.p, range_.p, nbox_.p, height_.p, kept_.p, flag_.p, frontier_.p, N, graw, gout, item_member_.p, gstage,
                           (uint32_t)(raw && out));
    }
    stage_ready_ = false;
    LB_TRY(hipGetLastError());
    if (tm) LB_TRY(mark(EV_HIERARCHY_LARGE, stream));
    if (!pair_count) {                                // collapse_wide needs the count of this build's pairs
        if (!count_.p) LB_TRY(count_.alloc(1));
        pair_count = count_.p;
    }
    last_count_ = pair_count;
    if (NI > 0) {
        bytes = tmp_.n;
        LB_TRY(rocprim::exclusive_scan<PairScanConfig>(tmp_.p, bytes, kept_.p, pidx_.p, 0u, NI, rocprim::plus<uint32_t>(), stream));
        if (tm) LB_TRY(mark(EV_SCAN, stream));
        hipLaunchKernelGGL(emit_kernel, dim3(blocks_for(NI)), dim3(BLOCK), 0, stream, segs_.p, seg_of_.p, v1_.p, box_, NI, child_.p,
                           range_.p, nbox_.p, kept_.p, pidx_.p, pairs, pair_count);
    } else {
        if (pair_count) LB_TRY(hipMemsetAsync(pair_count, 0, sizeof(uint32_t), stream));
        if (tm) LB_TRY(mark(EV_SCAN, stream));
    }
    hipLaunchKernelGGL(roots_kernel, dim3(blocks_for(n_segs_)), dim3(BLOCK), 0, stream, segs_.p, n_segs_, v1_.p, box_, nbox_.p,
                       height_.p, pidx_.p, roots);
    LB_TRY(hipGetLastError());
    return tm ? mark(EV_EMIT_ROOTS, stream) : hipSuccess;
}

hipError_t LbvhBuilder::collapse_wide(const NodePair *pairs, const TreeRoot *roots, NodeQuad *quads, TreeRoot *roots_wide,
                                      hipStream_t stream) {
    const bool tm = box_ == own_box_.p;
    if (max_count_ > COLLAPSE_ALL_MIN && last_count_) {
        hipLaunchKernelGGL(collapse_all_kernel, dim3(blocks_for(max_pairs())), dim3(BLOCK), 0, stream, pairs, last_count_, quads);
        if (roots_wide)
            hipLaunchKernelGGL(copy_roots_kernel, dim3(blocks_for(n_segs_)), dim3(BLOCK), 0, stream, roots, n_segs_, roots_wide);
        LB_TRY(hipGetLastError());
        return tm ? mark(EV_COLLAPSE, stream) : hipSuccess;
    }
    if (max_count_ - 1 > LDS_FRONT && !front_.p) LB_TRY(front_.alloc(2 * (size_t)max_pairs()));
    hipLaunchKernelGGL(collapse_wide_kernel, dim3(n_segs_), dim3(BLOCK), 0, stream, segs_.p, roots, pairs, quads, front_.p,
                       max_pairs(), roots_wide);
    LB_TRY(hipGetLastError());
    return tm ? mark(EV_COLLAPSE, stream) : hipSuccess;
}

hipError_t LbvhBuilder::gather_items(uint32_t *slots, hipStream_t stream) {
    hipLaunchKernelGGL(gather_items_kernel, dim3(blocks_for(n_items_)), dim3(BLOCK), 0, stream, segs_.p, seg_of_.p, v1_.p, n_items_,
                       slots);
    return hipGetLastError();
}

}  // namespace rtamd
