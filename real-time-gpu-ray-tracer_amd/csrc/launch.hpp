// launch.hpp — every host-side kernel launcher, declared once: the TUs that define them (trace_kernel.hip with
// ray_query.hpp in its three flavours, schedule.hip, assemble.hip, instances.hip, tri_update.hip, inst_bounds.hip, and
// the image filters denoise.hip, accumulate.hip, guided.hip) and the host files that call them (the filters': filters.cpp)
// include this header, so a signature that drifts fails where it was changed.  (launch_tlas_small: lbvh.hpp.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt.h"
#include "inst_bounds_map.hpp"
#include "layout.hpp"

namespace rtamd {

// trace_kernel.hip, once per flavour: exact (the reference's arithmetic and traversal), fast (the default FAST kernels)
// and fastmath (option "fast_math": the FAST kernels with hardware reciprocals and FMA contraction, trace_fastmath.o)
#define RTAMD_TRACE_LAUNCHERS(sfx)                                                                                        \
    hipError_t launch_render_##sfx(const SceneGPU &, const CameraGPU &, const OutputGPU &, bool, unsigned long long *,   \
                                   hipStream_t);                                                                          \
    hipError_t launch_render_persistent_##sfx(const SceneGPU &, const CameraGPU &, const OutputGPU &, bool,              \
                                              unsigned long long *, uint32_t *, uint32_t, uint32_t, bool, hipStream_t);  \
    uint32_t persistent_blocks_per_cu_##sfx(uint32_t wide, bool raw);                                                     \
    hipError_t launch_trace_rays_##sfx(const SceneGPU &, const float *, uint32_t, rt_hit *, hipStream_t);                \
    hipError_t launch_ray_query_##sfx(const SceneGPU &, const RayQueryGPU &, bool, uint32_t, hipStream_t);               \
    hipError_t launch_camera_query_##sfx(const SceneGPU &, const CameraGPU &, RayQueryGPU, CameraQueryGPU, uint32_t,     \
                                         hipStream_t);
RTAMD_TRACE_LAUNCHERS(exact)
RTAMD_TRACE_LAUNCHERS(fast)
RTAMD_TRACE_LAUNCHERS(fastmath)
#undef RTAMD_TRACE_LAUNCHERS
// rt_box_test: the reference's slab test or the FAST one; it has no fast_math form of its own
hipError_t launch_box_test_exact(const float *, const float *, const float *, uint32_t, uint32_t, uint8_t *, float *, hipStream_t);
hipError_t launch_box_test_fast(const float *, const float *, const float *, uint32_t, uint32_t, uint8_t *, float *, hipStream_t);

// assemble.hip, schedule.hip, instances.hip
hipError_t launch_assemble(const void *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, void *, hipStream_t);
hipError_t launch_frame_copy(void *, const void *, size_t, unsigned long long *, uint32_t *, hipStream_t);
hipError_t launch_schedule(uint32_t *, uint32_t *, uint32_t *, uint32_t *, uint32_t, uint32_t, uint32_t, bool, uint32_t,
                           uint32_t, uint32_t, void *, const void *, size_t, unsigned long long *, hipStream_t);
hipError_t launch_instance_slot_order(const uint32_t *, const InstHot *, const InstCold *, uint32_t, InstHot *, InstCold *,
                                      hipStream_t);
// dev_cent: the device-bounded records' local centroids (inst_bounds.hip), read for records with InstParams::pad[1] set
hipError_t launch_instance_update(const InstDelta *, uint32_t, InstParams *, uint32_t, InstHot *, InstCold *, float *, float4 *,
                                  const uint32_t *, const TreeRoot *, const uint32_t *, const float4 *dev_cent, bool, hipStream_t);
// tri_update.hip: triangles [first, first + count) of raw_tris (vertices, normals if given, has_normals = 1 with them)
// and raw_verts from flat device streams of 9 floats per triangle
hipError_t launch_tri_update(rt_triangle *raw_tris, float *raw_verts, const float *vertices, const float *normals,
                             uint64_t first, uint64_t count, hipStream_t stream);
// inst_bounds.hip (RT_TRI_UPDATE_BOUNDS): the static tables of rt_scene_build and the arrays the kernels write.  The
// local centroid of every triangle instance that [first, first + count) overlaps, over the instance's whole range,
// and of every group with such a member, into cent[record]
struct InstBoundsGPU {
    const InstBoundsEntry *table;      // the triangle instances
    const uint32_t *chunk_inst;        // work item -> table index
    const uint32_t *multi;             // table indices of the instances of more than one chunk
    const uint2 *groups;               // per group {first member, members} into `members`
    const uint32_t *members;           // table indices, in member order
    uint32_t chunks, n_multi, n_groups, n_inst;
    double *partials;                  // 3 per work item
    float4 *cent;                      // one per record: instances, then groups
};
hipError_t launch_inst_bounds(const InstBoundsGPU &b, const float *raw_verts, uint64_t first, uint64_t count, hipStream_t stream);
// denoise.hip (rt_denoise): the caller's buffers and the four planes of its scratch, w * h float4 each
struct DenoiseGPU {
    const float *color;                // 3 floats per pixel
    const rt_hit *hits;
    const float *albedo;               // optional
    float *rgb;                        // optional output, may be `color`
    uint32_t *rgba;                    // optional output
    float4 *plane[2];                  // the passes' colour planes: pass i reads plane[i & 1]
    float4 *g0, *g1;                   // guides: {normal, flag}, {point, 0}
    uint32_t w, h;
};
constexpr uint64_t DENOISE_SCRATCH_PER_PIXEL = 4 * sizeof(float4);
// the pack pass and `iterations` (1..5) filter passes, the last one writing the outputs
hipError_t launch_denoise(const DenoiseGPU &g, uint32_t iterations, float sigma_color, float sigma_normal, float sigma_plane,
                          hipStream_t stream);
// accumulate.hip (rt_accumulate): the caller's buffers, the thresholds and the previous frame's rows
struct AccumulateGPU {
    const float *color;                // 3 floats per pixel
    const rt_hit *hits, *prev_hits;    // prev_hits and prev_history: both or neither
    const float4 *prev_history;
    float4 *history;
    float *rgb;                        // optional output, may be `color`
    uint32_t w, h;
    float max_history, normal_cos, plane_tolerance;
    uint32_t has_view;                 // 0: every pixel looks at itself and `view` is not read
    rt_reprojection view;
    // rt_accumulate_moments only (moments set): the albedo is optional, prev_moments goes with prev_history
    const float *albedo;
    const float2 *prev_moments;
    float2 *moments;
    // rt_accumulate_motion only (motion set): motion_count records indexed by rt_hit.instance; none past them is read
    const rt_instance_motion *motion;
    uint32_t motion_count;
};
// one launch, one thread per pixel
hipError_t launch_accumulate(const AccumulateGPU &g, hipStream_t stream);
// guided.hip (rt_denoise_guided): the caller's buffers and the four planes of its scratch, as DenoiseGPU's; the colour
// planes' .w lane carries the variance
struct GuidedGPU {
    const float4 *history;             // {r, g, b, length}
    const float2 *moments;
    const rt_hit *hits;
    const float *albedo;               // optional
    float *rgb;                        // optional output
    uint32_t *rgba;                    // optional output
    float *variance;                   // optional output: v_0
    float4 *plane[2];
    float4 *g0, *g1;
    uint32_t w, h;
};
// the pack and variance passes and `iterations` (1..5) filter passes, the last one writing the outputs.  feedback
// (rt_denoise_guided_feedback; nullptr: none): the first pass also writes {its result times the albedo, the history's
// length} there, and it may be g.history itself.  It is an argument of that pass's kernel alone and not a member of
// GuidedGPU: the filter kernels take their pass after the struct, so a member would move every later argument and
// with it the code of the kernels that were there (profiles/feedback/README.md)
hipError_t launch_denoise_guided(const GuidedGPU &g, uint32_t iterations, float sigma_luminance, float sigma_normal,
                                 float sigma_plane, float4 *feedback, hipStream_t stream);

// One flavour's launchers.  RT_RENDER_EXACT / RT_QUERY_EXACT win over option "fast_math".
struct TraceFlavour {
    decltype(&launch_render_exact) render;
    decltype(&launch_render_persistent_exact) render_persistent;
    decltype(&persistent_blocks_per_cu_exact) blocks_per_cu;
    decltype(&launch_trace_rays_exact) trace_rays;
    decltype(&launch_ray_query_exact) ray_query;
    decltype(&launch_camera_query_exact) camera_query;
};
inline const TraceFlavour &trace_flavour(bool exact, bool fast_math) {
#define RTAMD_FLAVOUR(sfx)                                                                                                \
    {launch_render_##sfx, launch_render_persistent_##sfx, persistent_blocks_per_cu_##sfx, launch_trace_rays_##sfx,       \
     launch_ray_query_##sfx, launch_camera_query_##sfx}
    static constexpr TraceFlavour table[3] = {RTAMD_FLAVOUR(exact), RTAMD_FLAVOUR(fast), RTAMD_FLAVOUR(fastmath)};
#undef RTAMD_FLAVOUR
    return table[exact ? 0 : (fast_math ? 2 : 1)];
}
// resident workgroups per CU of the flavour's persistent kernel: the EXACT kernel has one form, the FAST ones one per
// tree form and shading source of the scene
inline uint32_t persistent_blocks_per_cu(bool exact, bool fast_math, const SceneGPU &g) {
    const TraceFlavour &f = trace_flavour(exact, fast_math);
    return exact ? f.blocks_per_cu(0u, false) : f.blocks_per_cu(g.wide, g.raw_tris != nullptr);
}

}  // namespace rtamd
