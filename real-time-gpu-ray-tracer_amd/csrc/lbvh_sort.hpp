// lbvh_sort.hpp — the builder's passes over the items, up to the sorted Morton codes (lbvh.hip maps the headers):
// item boxes / centroids of a BLAS build (prep_blas_kernel), centroid bounds per segment, 30-bit Morton codes, and
// the two sorts — one workgroup's LDS bitonic sort for small trees, rocPRIM's radix sort (configured here) for
// large ones.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "lbvh_items.hpp"

namespace rtamd::lbvh {

// ---- Morton / ordered-float helpers --------------------------------------------------------
__device__ __forceinline__ uint32_t f2o(float f) {          // order-preserving float -> uint
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float o2f(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
__device__ __forceinline__ uint32_t expand10(uint32_t v) {  // 10 bits -> every third bit of 30
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__device__ __forceinline__ uint32_t quant10(float c, float lo, float hi) {
    const float ext = hi - lo;
    if (!(ext > 0.0f)) return 0u;
    const float q = (c - lo) / ext * 1024.0f;
    if (!(q > 0.0f)) return 0u;
    return q >= 1023.0f ? 1023u : (uint32_t)q;
}
// slot i of an empty set of ordered-uint bounds (even: min slots, odd: max slots)
__device__ __forceinline__ uint32_t bounds_seed(uint32_t i) { return (i & 1) ? 0u : 0xFFFFFFFFu; }

// ---- kernels -------------------------------------------------------------------------------
__global__ void init_bounds_kernel(uint32_t *bounds, uint32_t n_segs) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_segs * 6) return;
    bounds[i] = bounds_seed(i);
}

// stage (optional, BLAS builds without cold records): each triangle item's TriHot record in item order, so the
// gather after the sort reads one 48-B record per leaf slot instead of the vertices plus the member table
__global__ void prep_blas_kernel(const LbvhSeg *segs, const uint32_t *seg_of, uint32_t n, RawPrimsGPU raw,
                                 float *box, float4 *cent, TriHot *stage, const uint32_t *item_member) {
    const uint32_t it = blockIdx.x * BLOCK + threadIdx.x;
    if (it >= n) return;
    const LbvhSeg S = segs[seg_of[it]];
    const uint32_t prim = S.prim_base + (it - S.item_base);
    Box bx;
    V3 c;
    if (S.ptype == RT_PRIM_TRIANGLE) {
        const float *tv = raw.tri_verts + 9 * (size_t)prim;
        tri_box_centroid(tv, bx, c);
        if (stage) stage[it] = tri_hot_record(tv, prim, S.member_count ? item_member[it] : 0u);
    } else if (S.ptype == RT_PRIM_SPHERE) sphere_box_centroid(raw.spheres[prim], bx, c);
    else quad_box_centroid(raw.quads[prim], bx, c);
#pragma unroll
    for (int k = 0; k < 6; k++) box[6 * (size_t)it + k] = bx.b[k];
    cent[it] = make_float4(c.x, c.y, c.z, 0.0f);
}

// Centroid bounds per segment.  Each block walks `ipt` consecutive block-wide strides of items; a wave
// whose 64 items share one segment accumulates per lane across strides and reduces only when the segment
// changes (or at the end), into the block's LDS slot when the segment is the one the block starts in, else
// with global atomics; mixed waves (segment boundaries) fall back to per-lane atomics.  One global atomic
// set per block for the common case: one segment of 10M triangles (C5's group) took 10.6 ms with a set per
// wave, all on the same six words.  Inactive TLAS items (centroid w != 0, set_items) are left out.
__device__ __forceinline__ void bounds_flush(uint32_t seg, float (&lo)[3], float (&hi)[3], uint32_t bseg, uint32_t *sb,
                                             uint32_t *bounds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off));
        }
    }
    if ((threadIdx.x & 63) == 0 && lo[0] <= hi[0]) {      // at least one live item
        uint32_t *dst = seg == bseg ? sb : bounds + 6 * seg;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            atomicMin(&dst[2 * a], f2o(lo[a]));
            atomicMax(&dst[2 * a + 1], f2o(hi[a]));
        }
    }
}

__global__ __launch_bounds__(BLOCK) void bounds_kernel(const uint32_t *seg_of, const float4 *cent, uint32_t n, uint32_t ipt,
                                                       uint32_t *bounds) {
    __shared__ uint32_t sb[6];
    const uint64_t base = (uint64_t)blockIdx.x * BLOCK * ipt;
    const uint32_t bseg = base < n ? seg_of[base] : NONE;
    if (threadIdx.x < 6) sb[threadIdx.x] = bounds_seed(threadIdx.x);
    __syncthreads();
    const float inf = __builtin_huge_valf();
    uint32_t acc = NONE;                                   // wave-uniform: the segment lo/hi accumulate
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (uint32_t j = 0; j < ipt; j++) {
        const uint64_t it = base + (uint64_t)j * BLOCK + threadIdx.x;
        const bool valid = it < n;
        const uint32_t seg = valid ? seg_of[it] : NONE;
        const float4 c = valid ? cent[it] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const bool live = valid && c.w == 0.0f;
        const uint32_t seg0 = __builtin_amdgcn_readfirstlane(seg);
        if (__all(seg == seg0)) {
            if (seg0 == NONE) break;                       // past the end (uniform across the wave)
            if (seg0 != acc) {
                if (acc != NONE) bounds_flush(acc, lo, hi, bseg, sb, bounds);
                acc = seg0;
#pragma unroll
                for (int a = 0; a < 3; a++) { lo[a] = inf; hi[a] = -inf; }
            }
            if (live) {
                lo[0] = fminf(lo[0], c.x); hi[0] = fmaxf(hi[0], c.x);
                lo[1] = fminf(lo[1], c.y); hi[1] = fmaxf(hi[1], c.y);
                lo[2] = fminf(lo[2], c.z); hi[2] = fmaxf(hi[2], c.z);
            }
        } else if (live) {
            const float v[3] = {c.x, c.y, c.z};
#pragma unroll
            for (int a = 0; a < 3; a++) {
                atomicMin(&bounds[6 * seg + 2 * a], f2o(v[a]));
                atomicMax(&bounds[6 * seg + 2 * a + 1], f2o(v[a]));
            }
        }
    }
    if (acc != NONE) bounds_flush(acc, lo, hi, bseg, sb, bounds);
    __syncthreads();
    if (threadIdx.x < 6 && bseg != NONE && sb[0] != 0xFFFFFFFFu) {
        if (threadIdx.x & 1) atomicMax(&bounds[6 * bseg + threadIdx.x], sb[threadIdx.x]);
        else atomicMin(&bounds[6 * bseg + threadIdx.x], sb[threadIdx.x]);
    }
}

// 30-bit Morton codes over each segment's centroid bounds.  (Round 3's 2-bit size class above the code for the TLAS,
// option "tlas_classes", measured neutral and was removed in round 6.)
__global__ void morton_kernel(const uint32_t *seg_of, const float4 *cent, uint32_t n, const uint32_t *bounds,
                              uint32_t *keys, uint32_t *vals) {
    const uint32_t it = blockIdx.x * BLOCK + threadIdx.x;
    if (it >= n) return;
    const uint32_t seg = seg_of[it];
    const float4 c = cent[it];
    if (c.w != 0.0f) {                           // inactive item: behind every active one (no class bits reach ~0)
        keys[it] = 0xFFFFFFFFu;
        vals[it] = it;
        return;
    }
    const uint32_t *B = bounds + 6 * seg;
    const uint32_t x = quant10(c.x, o2f(B[0]), o2f(B[1]));
    const uint32_t y = quant10(c.y, o2f(B[2]), o2f(B[3]));
    const uint32_t z = quant10(c.z, o2f(B[4]), o2f(B[5]));
    keys[it] = (expand10(x) << 2) | (expand10(y) << 1) | expand10(z);   // (also tlas_small_kernel; shared, both kernels change)
    vals[it] = it;
}

// Sorting happens per segment (items never leave their segment's range): trees of <= LOCAL_SORT_MAX items are
// sorted by one workgroup in LDS (bitonic over (code, item) pairs, which is the stable radix order), larger ones by
// one rocPRIM radix sort each over their 30- or 32-bit codes (LbvhBuilder::build).  A 64-bit (segment, code) key
// over the whole forest cost C5 five 8-bit passes over 10 M 12-byte pairs per rebuild.
constexpr uint32_t LOCAL_SORT_MAX = 2048;
constexpr uint32_t LOCAL_MAX = 2048;    // trees of <= LOCAL_MAX items: bottom_up_local_kernel (one workgroup, LDS)
// one threshold: LbvhBuilder::large_items() counts the rocPRIM-sorted trees and bench.py's byte model charges them
// the chunk and top passes; tests/lbvh_sizes_ref.py places its sizes around the one figure
static_assert(LOCAL_SORT_MAX == LOCAL_MAX, "large_items(), bench.py and tests/lbvh_sizes_ref.py assume one threshold");
// The large trees' rocPRIM sort: onesweep over 10-bit digits (3 passes over a 30-bit code) instead of rocPRIM's gfx950
// default of 8 (4 passes).  Measured on 10 M clustered Morton pairs (scripts/sort_bench.hip, profiles/r06/sort/):
// 0.404 -> 0.279 ms per sort; 9 bits 0.401, 11 bits 0.376, 10 bits over 512 x 16 or 1024 x 24 items 0.33 / 0.35.
#ifndef LBVH_SORT_BITS
#define LBVH_SORT_BITS 10
#endif
using BigSortConfig = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<1024, 16>, rocprim::kernel_config<1024, 16>, LBVH_SORT_BITS,
                                        rocprim::block_radix_rank_algorithm::match>>;
// the pair-index scan over every interior node's kept flag: 256 x 32 items per block, 0.051 -> 0.036 ms over 10 M flags
// against rocPRIM's default (scripts/scan_bench.hip, profiles/r06/sort/)
using PairScanConfig = rocprim::scan_config<256, 32, rocprim::block_load_method::block_load_transpose,
                                            rocprim::block_store_method::block_store_transpose,
                                            rocprim::block_scan_algorithm::using_warp_scan>;
// (tlas_small_kernel runs the same bitonic network over its own keys; as one function the two kernels' code changes)
__global__ __launch_bounds__(BLOCK) void local_sort_kernel(const LbvhSeg *segs, const uint32_t *keys_in, uint32_t *keys_out,
                                                           uint32_t *vals_out) {
    __shared__ unsigned long long sk[LOCAL_SORT_MAX];
    const LbvhSeg S = segs[blockIdx.x];
    if (S.count == 0 || S.count > LOCAL_SORT_MAX) return;              // block-uniform
    const uint32_t m = S.count, t = threadIdx.x;
    uint32_t np = 1;
    while (np < m) np <<= 1;
    for (uint32_t k = t; k < np; k += BLOCK)
        sk[k] = k < m ? ((unsigned long long)keys_in[S.item_base + k] << 32) | k : ~0ull;
    __syncthreads();
    for (uint32_t size = 2; size <= np; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t k = t; k < np; k += BLOCK) {
                const uint32_t o = k ^ stride;
                if (o > k) {
                    const unsigned long long x = sk[k], y = sk[o];
                    if ((x > y) == ((k & size) == 0)) { sk[k] = y; sk[o] = x; }
                }
            }
            __syncthreads();
        }
    for (uint32_t k = t; k < m; k += BLOCK) {
        keys_out[S.item_base + k] = (uint32_t)(sk[k] >> 32);
        vals_out[S.item_base + k] = S.item_base + (uint32_t)sk[k];
    }
}

}  // namespace rtamd::lbvh
