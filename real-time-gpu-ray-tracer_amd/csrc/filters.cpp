// filters.cpp — the image filters: rt_denoise (denoise.hip), rt_accumulate / _moments / _motion (accumulate.hip) and
// rt_denoise_guided / _feedback (guided.hip).  They take no scene: `int device` and a descriptor of caller buffers.
// Every call has the same shape: the argument checks, which need no device and come in the order the ABI tests pin; the
// device and the buffers' accessibility from it; the launcher; the tail.  rt_instance_motion_records, the host-only
// helper that feeds rt_accumulate_motion, is here too (its arithmetic: instance_motion.hpp).
#include "instance_motion.hpp"
#include "launch.hpp"
#include "scene.hpp"

namespace rtamd {

// The device of a call that names one by index (the filters, rt_box_test): it exists, and it is current afterwards.
rt_status select_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count)
        return fail(RT_ERR_INVALID_ARGUMENT, "no such device");
    HIP_TRY(hipSetDevice(device));
    return RT_OK;
}

}  // namespace rtamd

namespace {

// a caller buffer as the overlap checks see it; a null one overlaps nothing
struct Range { const void *p; uint64_t bytes; };
bool overlap(const Range &x, const Range &y) {
    const uintptr_t a = (uintptr_t)x.p, b = (uintptr_t)y.p;
    return x.p && y.p && a < b + y.bytes && b < a + x.bytes;
}

uint64_t scratch_bytes(uint32_t width, uint32_t height) { return (uint64_t)width * height * DENOISE_SCRATCH_PER_PIXEL; }

// the scratch of n pixels into DenoiseGPU's / GuidedGPU's planes: colour plane 0 | colour plane 1 | guides
template <class G>
void split_scratch(G &g, void *scratch_device, size_t n) {
    float4 *scratch = static_cast<float4 *>(scratch_device);
    g.plane[0] = scratch; g.plane[1] = scratch + n; g.g0 = scratch + 2 * n; g.g1 = scratch + 3 * n;
}

// the tail of a call whose launches are on `st`
rt_status finish(hipStream_t st, bool no_sync) {
    if (no_sync) return RT_OK;
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
}

// rt_accumulate (m == nullptr, with_moments false), rt_accumulate_moments and rt_accumulate_motion (with_motion; m is
// then optional): one set of checks, one launcher
rt_status accumulate_call(int device, const rt_accumulate_desc *d, const rt_moments_desc *m, bool with_moments,
                          const rt_motion_desc *mo = nullptr, bool with_motion = false) {
    const std::string name = with_motion ? "rt_accumulate_motion" : with_moments ? "rt_accumulate_moments" : "rt_accumulate";
    // the argument checks need no device
    if (!d || (with_moments && !m) || (with_motion && !mo)) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (d->reserved != 0 || d->reserved1 != 0 || (d->flags & ~(uint32_t)RT_ACCUMULATE_NO_SYNC) || (m && m->reserved != 0))
        return fail(RT_ERR_INVALID_ARGUMENT, name + ": reserved bits set");
    if (d->width > 16384 || d->height > 16384) return fail(RT_ERR_INVALID_ARGUMENT, name + ": width and height are at most 16384");
    if (!(d->max_history >= 1.0f)) return fail(RT_ERR_INVALID_ARGUMENT, name + ": max_history must be >= 1");
    if (!(d->normal_cos <= 1.0f)) return fail(RT_ERR_INVALID_ARGUMENT, name + ": normal_cos must be <= 1 (-inf switches the test off)");
    if (!(d->plane_tolerance > 0.0f))
        return fail(RT_ERR_INVALID_ARGUMENT, name + ": plane_tolerance must be > 0 (+inf switches the test off)");
    if (!d->color_device || !d->hits_device || !d->history_device || (m && !m->moments_device))
        return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!d->prev_hits_device != !d->prev_history_device)
        return fail(RT_ERR_INVALID_ARGUMENT, name + ": prev_hits_device and prev_history_device go together");
    if (m && !m->prev_moments_device != !d->prev_history_device)
        return fail(RT_ERR_INVALID_ARGUMENT, name + ": prev_moments_device and prev_history_device go together");
    if (((uintptr_t)d->history_device | (uintptr_t)d->prev_history_device) & 15u)
        return fail(RT_ERR_INVALID_ARGUMENT, name + ": the history buffers must be 16-byte aligned");
    if (m && (((uintptr_t)m->moments_device | (uintptr_t)m->prev_moments_device) & 7u))
        return fail(RT_ERR_INVALID_ARGUMENT, name + ": the moments buffers must be 8-byte aligned");
    if (((uintptr_t)d->color_device | (uintptr_t)d->hits_device | (uintptr_t)d->prev_hits_device | (uintptr_t)d->rgb32_device |
         (uintptr_t)(m ? m->albedo_device : nullptr)) & 3u)
        return fail(RT_ERR_INVALID_ARGUMENT, name + ": the buffers must be 4-byte aligned");
    // no output may overlap an input or another output; rgb32_device may be color_device itself
    const uint64_t n = (uint64_t)d->width * d->height;
    const Range history{d->history_device, 16 * n}, rgb{d->rgb32_device, 12 * n};
    const Range moments{m ? m->moments_device : nullptr, 8 * n};
    const Range read[] = {{d->hits_device, sizeof(rt_hit) * n}, {d->prev_hits_device, sizeof(rt_hit) * n},
                          {d->prev_history_device, 16 * n}, {m ? m->albedo_device : nullptr, 12 * n},
                          {m ? m->prev_moments_device : nullptr, 8 * n}};
    const Range color{d->color_device, 12 * n};
    bool clash = overlap(history, rgb) || overlap(history, color) || (rgb.p != color.p && overlap(rgb, color)) ||
                 overlap(moments, history) || overlap(moments, rgb) || overlap(moments, color);
    for (const Range &r : read) clash = clash || overlap(history, r) || overlap(rgb, r) || overlap(moments, r);
    if (clash) return fail(RT_ERR_INVALID_ARGUMENT, name + ": an output overlaps another buffer");
    if (mo) {
        if (mo->reserved != 0) return fail(RT_ERR_INVALID_ARGUMENT, name + ": reserved bits set");
        if (mo->instance_count > 0xFFFFFFFEull) return fail(RT_ERR_INVALID_ARGUMENT, name + ": instance_count is at most 0xFFFFFFFE");
        if (!mo->motion_device != !mo->instance_count)
            return fail(RT_ERR_INVALID_ARGUMENT, name + ": motion_device and instance_count go together");
        if ((uintptr_t)mo->motion_device & 15u) return fail(RT_ERR_INVALID_ARGUMENT, name + ": motion_device must be 16-byte aligned");
        const Range records{mo->motion_device, sizeof(rt_instance_motion) * mo->instance_count};
        if (overlap(history, records) || overlap(rgb, records) || overlap(moments, records))
            return fail(RT_ERR_INVALID_ARGUMENT, name + ": an output overlaps the motion records");
        if (mo->instance_count && d->prev_history_device && !d->prev_view)
            return fail(RT_ERR_INVALID_ARGUMENT, name + ": motion records need prev_view (a still camera passes its own rows)");
    }
    if (n == 0) return RT_OK;
    DeviceRestore restore;
    RT_TRY(select_device(device));
    RT_TRY(all_accessible({d->color_device, d->hits_device, d->prev_hits_device, d->prev_history_device, d->history_device,
                           d->rgb32_device, m ? m->albedo_device : nullptr, m ? m->prev_moments_device : nullptr,
                           m ? m->moments_device : nullptr},
                          device, name + ": a buffer is not accessible from the device"));
    if (mo) RT_TRY(all_accessible({mo->motion_device}, device, name + ": motion_device is not accessible from the device"));

    AccumulateGPU g{};
    g.color = d->color_device; g.hits = d->hits_device; g.prev_hits = d->prev_hits_device;
    g.prev_history = reinterpret_cast<const float4 *>(d->prev_history_device);
    g.history = reinterpret_cast<float4 *>(d->history_device);
    g.rgb = d->rgb32_device;
    g.w = d->width; g.h = d->height;
    g.max_history = d->max_history; g.normal_cos = d->normal_cos; g.plane_tolerance = d->plane_tolerance;
    if (d->prev_view) { g.has_view = 1; g.view = *d->prev_view; }
    if (m) {
        g.albedo = m->albedo_device;
        g.prev_moments = reinterpret_cast<const float2 *>(m->prev_moments_device);
        g.moments = reinterpret_cast<float2 *>(m->moments_device);
    }
    if (mo) { g.motion = mo->motion_device; g.motion_count = (uint32_t)mo->instance_count; }   // none: MOTION = false kernels
    hipStream_t st = static_cast<hipStream_t>(d->stream);
    HIP_TRY(launch_accumulate(g, st));
    return finish(st, (d->flags & RT_ACCUMULATE_NO_SYNC) != 0);
}

// rt_denoise_guided (f == nullptr, with_feedback false) and rt_denoise_guided_feedback: one set of checks, one launcher
rt_status guided_call(int device, const rt_denoise_guided_desc *d, const rt_feedback_desc *f, bool with_feedback) {
    const std::string name = with_feedback ? "rt_denoise_guided_feedback" : "rt_denoise_guided";
    // the argument checks need no device
    if (!d || (with_feedback && !f)) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (d->reserved != 0 || (d->flags & ~(uint32_t)RT_DENOISE_NO_SYNC) || (f && f->reserved != 0))
        return fail(RT_ERR_INVALID_ARGUMENT, name + ": reserved bits set");
    if (d->iterations < 1 || d->iterations > 5) return fail(RT_ERR_INVALID_ARGUMENT, name + ": iterations must be in 1..5");
    if (!(d->sigma_luminance > 0.0f) || !(d->sigma_normal > 0.0f) || !(d->sigma_plane > 0.0f))
        return fail(RT_ERR_INVALID_ARGUMENT, name + ": every sigma must be > 0 (+inf switches its term off)");
    if (d->width > 16384 || d->height > 16384) return fail(RT_ERR_INVALID_ARGUMENT, name + ": width and height are at most 16384");
    if (!d->rgb32_device && !d->rgba8_device) return fail(RT_ERR_INVALID_ARGUMENT, name + ": no output buffer");
    if (!d->history_device || !d->moments_device || !d->hits_device || !d->scratch_device || (f && !f->feedback_device))
        return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (d->scratch_bytes < scratch_bytes(d->width, d->height))
        return fail(RT_ERR_INVALID_ARGUMENT, name + ": scratch_bytes is less than rt_denoise_guided_scratch_bytes(width, height)");
    if (((uintptr_t)d->scratch_device | (uintptr_t)d->history_device) & 15u)
        return fail(RT_ERR_INVALID_ARGUMENT, name + ": the scratch and the history must be 16-byte aligned");
    if (f && ((uintptr_t)f->feedback_device & 15u))
        return fail(RT_ERR_INVALID_ARGUMENT, name + ": feedback_device must be 16-byte aligned");
    if ((uintptr_t)d->moments_device & 7u) return fail(RT_ERR_INVALID_ARGUMENT, name + ": the moments must be 8-byte aligned");
    if (((uintptr_t)d->hits_device | (uintptr_t)d->albedo_device | (uintptr_t)d->rgb32_device | (uintptr_t)d->rgba8_device |
         (uintptr_t)d->variance_device) & 3u)
        return fail(RT_ERR_INVALID_ARGUMENT, name + ": the buffers must be 4-byte aligned");
    // no output (the scratch is one) may overlap an input or another output; the feedback may be the history itself
    const uint64_t n = (uint64_t)d->width * d->height;
    float *const feedback = f ? f->feedback_device : nullptr;
    const Range history{d->history_device, 16 * n};
    const Range in[] = {{d->moments_device, 8 * n}, {d->hits_device, sizeof(rt_hit) * n}, {d->albedo_device, 12 * n}};
    const Range out[] = {{d->rgb32_device, 12 * n}, {d->rgba8_device, 4 * n}, {d->variance_device, 4 * n},
                         {d->scratch_device, DENOISE_SCRATCH_PER_PIXEL * n}, {feedback, 16 * n}};
    bool clash = false;
    for (size_t i = 0; i < 5; i++) {
        const bool in_place = i == 4 && out[i].p == history.p;
        clash = clash || (!in_place && overlap(out[i], history));
        for (const Range &r : in) clash = clash || overlap(out[i], r);
        for (size_t j = i + 1; j < 5; j++) clash = clash || overlap(out[i], out[j]);
    }
    if (clash) return fail(RT_ERR_INVALID_ARGUMENT, name + ": an output overlaps another buffer");
    if (n == 0) return RT_OK;
    DeviceRestore restore;
    RT_TRY(select_device(device));
    RT_TRY(all_accessible({d->history_device, d->moments_device, d->hits_device, d->albedo_device, d->rgb32_device,
                           d->rgba8_device, d->variance_device, d->scratch_device, feedback},
                          device, name + ": a buffer is not accessible from the device"));

    GuidedGPU g{};
    g.history = reinterpret_cast<const float4 *>(d->history_device);
    g.moments = reinterpret_cast<const float2 *>(d->moments_device);
    g.hits = d->hits_device; g.albedo = d->albedo_device;
    g.rgb = d->rgb32_device; g.rgba = static_cast<uint32_t *>(d->rgba8_device); g.variance = d->variance_device;
    split_scratch(g, d->scratch_device, n);
    g.w = d->width; g.h = d->height;
    hipStream_t st = static_cast<hipStream_t>(d->stream);
    HIP_TRY(launch_denoise_guided(g, d->iterations, d->sigma_luminance, d->sigma_normal, d->sigma_plane,
                                  reinterpret_cast<float4 *>(feedback), st));
    return finish(st, (d->flags & RT_DENOISE_NO_SYNC) != 0);
}

}  // namespace

extern "C" {

uint64_t rt_denoise_scratch_bytes(uint32_t width, uint32_t height) { return scratch_bytes(width, height); }

rt_status rt_denoise(int device, const rt_denoise_desc *d) {
    // the argument checks need no device
    if (!d) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (d->reserved != 0 || (d->flags & ~(uint32_t)RT_DENOISE_NO_SYNC))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_denoise: reserved bits set");
    if (d->iterations < 1 || d->iterations > 5) return fail(RT_ERR_INVALID_ARGUMENT, "rt_denoise: iterations must be in 1..5");
    if (!(d->sigma_color > 0.0f) || !(d->sigma_normal > 0.0f) || !(d->sigma_plane > 0.0f))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_denoise: every sigma must be > 0 (+inf switches its term off)");
    if (d->width > 16384 || d->height > 16384) return fail(RT_ERR_INVALID_ARGUMENT, "rt_denoise: width and height are at most 16384");
    if (!d->rgb32_device && !d->rgba8_device) return fail(RT_ERR_INVALID_ARGUMENT, "rt_denoise: no output buffer");
    if (!d->color_device || !d->hits_device || !d->scratch_device) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (d->scratch_bytes < scratch_bytes(d->width, d->height))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_denoise: scratch_bytes is less than rt_denoise_scratch_bytes(width, height)");
    if ((uintptr_t)d->scratch_device & 15u) return fail(RT_ERR_INVALID_ARGUMENT, "rt_denoise: the scratch must be 16-byte aligned");
    if (((uintptr_t)d->color_device | (uintptr_t)d->hits_device | (uintptr_t)d->albedo_device | (uintptr_t)d->rgb32_device |
         (uintptr_t)d->rgba8_device) & 3u)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_denoise: the buffers must be 4-byte aligned");
    if (d->width == 0 || d->height == 0) return RT_OK;
    DeviceRestore restore;
    RT_TRY(select_device(device));
    RT_TRY(all_accessible({d->color_device, d->hits_device, d->albedo_device, d->rgb32_device, d->rgba8_device, d->scratch_device},
                          device, "rt_denoise: a buffer is not accessible from the device"));

    DenoiseGPU g{};
    g.color = d->color_device; g.hits = d->hits_device; g.albedo = d->albedo_device;
    g.rgb = d->rgb32_device; g.rgba = static_cast<uint32_t *>(d->rgba8_device);
    split_scratch(g, d->scratch_device, (size_t)d->width * d->height);
    g.w = d->width; g.h = d->height;
    hipStream_t st = static_cast<hipStream_t>(d->stream);
    HIP_TRY(launch_denoise(g, d->iterations, d->sigma_color, d->sigma_normal, d->sigma_plane, st));
    return finish(st, (d->flags & RT_DENOISE_NO_SYNC) != 0);
}

rt_status rt_accumulate(int device, const rt_accumulate_desc *d) { return accumulate_call(device, d, nullptr, false); }

rt_status rt_accumulate_moments(int device, const rt_accumulate_desc *d, const rt_moments_desc *m) {
    return accumulate_call(device, d, m, true);
}

rt_status rt_accumulate_motion(int device, const rt_accumulate_desc *d, const rt_moments_desc *m, const rt_motion_desc *mo) {
    return accumulate_call(device, d, m, m != nullptr, mo, true);
}

rt_status rt_instance_motion_records(const rt_xform *prev, const rt_xform *cur, size_t count, rt_instance_motion *out) {
    if (count == 0) return RT_OK;
    if (!prev || !cur || !out) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    for (size_t i = 0; i < count; i++) out[i] = motion_record(prev[i], cur[i]);
    return RT_OK;
}

uint64_t rt_denoise_guided_scratch_bytes(uint32_t width, uint32_t height) { return scratch_bytes(width, height); }

rt_status rt_denoise_guided(int device, const rt_denoise_guided_desc *d) { return guided_call(device, d, nullptr, false); }

rt_status rt_denoise_guided_feedback(int device, const rt_denoise_guided_desc *d, const rt_feedback_desc *f) {
    return guided_call(device, d, f, true);
}

}  // extern "C"
