// inst_bounds.hip — RT_TRI_UPDATE_BOUNDS: the local centroids of the triangle instances (and option-"group" groups) a
// device triangle update overlaps, from raw_verts, into the scene's device-bounded centroid array (one float4 per
// record: instances, then groups).  The local boxes need no kernel: instance_update_kernel (instances.hip) takes a
// device-bounded record's box from the BLAS root it already loads.
//
// inst_bounds_map.hpp holds the reduction's shape and the wave's load -> triangle transpose; the host replay
// tests/cpp/inst_bounds_map_check.cpp checks both.  No floating-point atomics, no data-dependent order: two runs give
// the same bits.  Built with -ffp-contract=off like instances.hip.
//   chunk kernel   work item = (instance, chunk of 1 024 triangles), one workgroup each, the grid capped and strided.
//                  An item whose instance the update's range does not overlap is skipped at once.  Per round a wave reads
//                  its 64 triangles as 9 loads of 64 consecutive dwords (256 B per instruction, whatever the parity of
//                  the instance's first triangle), transposes them with 9 cross-lane reads, forms the centroid in
//                  float and adds it in double.  LDS: the waves' 3 x 4 partial sums.  A one-chunk instance is finished
//                  here; otherwise the chunk's sums go to `partials`.
//   fold kernel    one workgroup per instance of more than one chunk: the strided sum over its chunks' partials.
//   group kernel   one workgroup per group with a member in the range: the strided sum over its members' centroids.
// Memory-bound: 36 B read per triangle.
#include <hip/hip_runtime.h>

#include "inst_bounds_map.hpp"
#include "launch.hpp"

namespace rtamd {

namespace {

constexpr uint32_t IB_MAX_GRID = 2048;   // 256 CUs x 8 workgroups; the rest by the grid stride

__device__ __forceinline__ bool overlaps(const InstBoundsEntry &e, uint64_t first, uint64_t count) {
    return (uint64_t)e.pindex + e.count > first && (uint64_t)e.pindex < first + count;
}

// inst_bounds_map.hpp's wave and block steps for the three axes; thread 0 returns with the block's sums in v
__device__ __forceinline__ void block_sum3(double v[3], double (*part)[3]) {
#pragma unroll
    for (uint32_t off = IB_WAVE / 2; off; off >>= 1)
#pragma unroll
        for (int a = 0; a < 3; a++) v[a] = v[a] + __shfl_down(v[a], off, IB_WAVE);
    const uint32_t w = threadIdx.x / IB_WAVE;
    __syncthreads();                                   // the previous use of `part` is over
    if (threadIdx.x % IB_WAVE == 0)
        for (int a = 0; a < 3; a++) part[w][a] = v[a];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int a = 0; a < 3; a++) v[a] = ((part[0][a] + part[1][a]) + part[2][a]) + part[3][a];
}

__device__ __forceinline__ float4 mean3(const double S[3], uint32_t n) {
    return make_float4((float)(S[0] / n), (float)(S[1] / n), (float)(S[2] / n), 0.0f);
}

__global__ __launch_bounds__(IB_BLOCK) void inst_centroid_kernel(const InstBoundsEntry *__restrict__ table,
                                                                 const uint32_t *__restrict__ chunk_inst, uint32_t chunks,
                                                                 const float *__restrict__ verts, uint64_t first,
                                                                 uint64_t count, double *__restrict__ partials,
                                                                 float4 *__restrict__ cent) {
    __shared__ double part[IB_WAVES][3];
    const uint32_t lane = threadIdx.x % IB_WAVE, wave = threadIdx.x / IB_WAVE;
    for (uint32_t item = blockIdx.x; item < chunks; item += gridDim.x) {
        const InstBoundsEntry e = table[chunk_inst[item]];
        if (!overlaps(e, first, count)) continue;
        const uint32_t c = item - e.first_chunk;
        double acc[3] = {0.0, 0.0, 0.0};
        float own[3] = {0.0f, 0.0f, 0.0f};             // thread 0: the instance's first triangle's centroid
#pragma unroll
        for (uint32_t r = 0; r < IB_ROUNDS; r++) {
            const uint64_t t0 = ib_tri(c, r, wave, 0);                  // the wave's first triangle of the round
            if (t0 >= e.count) break;                                   // wave-uniform
            const uint64_t left = e.count - t0;
            const uint32_t live = 9u * (uint32_t)(left < IB_WAVE ? left : IB_WAVE);   // floats of the wave's triangles
            const float *src = verts + ((uint64_t)e.pindex + t0) * 9u;
            float reg[IB_LOADS];
#pragma unroll
            for (uint32_t k = 0; k < IB_LOADS; k++) reg[k] = IB_WAVE * k + lane < live ? src[IB_WAVE * k + lane] : 0.0f;
            float v[9];
#pragma unroll
            for (uint32_t j = 0; j < 9; j++) {
                const uint32_t want = ib_src_reg(ib_asker(lane, j), j);  // the register this lane's asker needs
                float give = reg[0];
#pragma unroll
                for (uint32_t k = 1; k < IB_LOADS; k++) give = want == k ? reg[k] : give;
                v[j] = __shfl(give, (int)ib_src_lane(lane, j), IB_WAVE);
            }
            if (9u * lane < live) {
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const float ca = ib_tri_centroid(v, a);
                    if (r == 0) own[a] = ca;
                    acc[a] += (double)ca;
                }
            }
        }
        block_sum3(acc, part);
        if (threadIdx.x != 0) continue;
        if (ib_chunks(e.count) > 1) {
            for (int a = 0; a < 3; a++) partials[3 * (uint64_t)item + a] = acc[a];
        } else {
            cent[e.record] = e.count == 1 ? make_float4(own[0], own[1], own[2], 0.0f) : mean3(acc, e.count);
        }
    }
}

__global__ __launch_bounds__(IB_BLOCK) void inst_fold_kernel(const InstBoundsEntry *__restrict__ table,
                                                             const uint32_t *__restrict__ multi, uint32_t n_multi,
                                                             uint64_t first, uint64_t count,
                                                             const double *__restrict__ partials, float4 *__restrict__ cent) {
    __shared__ double part[IB_WAVES][3];
    for (uint32_t m = blockIdx.x; m < n_multi; m += gridDim.x) {
        const InstBoundsEntry e = table[multi[m]];
        if (!overlaps(e, first, count)) continue;
        const uint32_t nc = ib_chunks(e.count);
        double acc[3] = {0.0, 0.0, 0.0};
        for (uint32_t j = threadIdx.x; j < nc; j += IB_BLOCK)
            for (int a = 0; a < 3; a++) acc[a] += partials[3 * ((uint64_t)e.first_chunk + j) + a];
        block_sum3(acc, part);
        if (threadIdx.x == 0) cent[e.record] = mean3(acc, e.count);
    }
}

// groups: {first member, members} into `members` (table indices, in member order); group g's record is n_inst + g
__global__ __launch_bounds__(IB_BLOCK) void group_centroid_kernel(const InstBoundsEntry *__restrict__ table,
                                                                  const uint2 *__restrict__ groups, uint32_t n_groups,
                                                                  const uint32_t *__restrict__ members, uint32_t n_inst,
                                                                  uint64_t first, uint64_t count, float4 *cent) {
    __shared__ double part[IB_WAVES][3];
    for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const uint2 G = groups[g];
        double acc[3] = {0.0, 0.0, 0.0};
        int touched = 0;
        for (uint32_t j = threadIdx.x; j < G.y; j += IB_BLOCK) {
            const InstBoundsEntry e = table[members[G.x + j]];
            touched |= overlaps(e, first, count) ? 1 : 0;
            const float4 c = cent[e.record];
            acc[0] += (double)c.x; acc[1] += (double)c.y; acc[2] += (double)c.z;
        }
        touched = __syncthreads_or(touched);
        if (!touched) continue;                        // block-uniform
        block_sum3(acc, part);
        if (threadIdx.x == 0) cent[n_inst + g] = mean3(acc, G.y);
    }
}

uint32_t capped(uint32_t n) { return n < IB_MAX_GRID ? n : IB_MAX_GRID; }

}  // namespace

hipError_t launch_inst_bounds(const InstBoundsGPU &b, const float *raw_verts, uint64_t first, uint64_t count,
                              hipStream_t stream) {
    if (count == 0 || b.chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(inst_centroid_kernel, dim3(capped(b.chunks)), dim3(IB_BLOCK), 0, stream, b.table, b.chunk_inst,
                       b.chunks, raw_verts, first, count, b.partials, b.cent);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (b.n_multi) {
        hipLaunchKernelGGL(inst_fold_kernel, dim3(capped(b.n_multi)), dim3(IB_BLOCK), 0, stream, b.table, b.multi, b.n_multi,
                           first, count, b.partials, b.cent);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (b.n_groups) {
        hipLaunchKernelGGL(group_centroid_kernel, dim3(capped(b.n_groups)), dim3(IB_BLOCK), 0, stream, b.table, b.groups,
                           b.n_groups, b.members, b.n_inst, first, count, b.cent);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace rtamd
