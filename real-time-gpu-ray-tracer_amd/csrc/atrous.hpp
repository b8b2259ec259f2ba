// atrous.hpp — the device code the image filters share: denoise.hip and guided.hip (the a-trous passes) use all of
// it, accumulate.hip the albedo floor and the luminance.  Leaf functions only: the filters' 5 x 5 loops and their tap
// arithmetic differ and stay in their files.  A piece is here only if the kernels' code is byte for byte what it was
// with the piece written out; the pieces for which that failed stay as copies that name each other
// (profiles/refactor_filters/README.md).
//   The staged tile: a 16 x 16 tile with its halo in LDS, one thread per pixel.  A tap outside the image is staged with
//   flag AT_OUTSIDE, which equals no pixel's flag, so its weight is 0 and the inner loop has no coordinate test.  Rows
//   are AT_PITCH = 32 float4 apart: ds_read_b128 serves a wave in groups of 16 lanes that mix two tile rows (lanes
//   {0-3, 12-15, 20-27}, ...: 8 columns of one row and the other 8 columns of the next), and its bank is
//   (address / 4) mod 64, so the 16 lanes cover the 64 banks exactly when the row pitch is a multiple of 16 float4.
//   The staged row: a workgroup is AT_ROW = 256 consecutive pixels of one row.  Per tap row dy (in the image: the test
//   is block-uniform) it stages that row's AT_ROW + 4 * step pixels, then every thread takes its five dx taps from LDS:
//   5 staged rows of at most 320 pixels for 256 results, 5.6 (step 8) or 6.3 (step 16) pixel loads per result where a
//   direct form issues 25, every one of them a coalesced 16-byte load.  Two row buffers alternate, so one barrier per
//   row is enough: a buffer is overwritten two rows after its last read.  A wave reads 64 consecutive float4: no bank
//   conflict at any pitch.
//   The scratch planes (DenoiseGPU, GuidedGPU): the colour plane a pass reads, and the guides {normal, flag} and
//   {point, 0}, a float4 each, so the passes read aligned 16-byte vectors only.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>

#include "launch.hpp"

namespace rtamd {

namespace {

constexpr int AT_TILE = 16;              // the tile form's tile edge; one workgroup of 256 threads
constexpr int AT_PITCH = 32;             // float4 per staged row (see above); the widest staged row is 16 + 4 * 4 = 32
constexpr float AT_OUTSIDE = 2.0f;       // flag of a staged tap outside the image: hits carry 0, misses 1
constexpr int AT_ROW = 256;              // the row form's pixels per workgroup
constexpr int AT_ROW_SPAN = AT_ROW + 4 * 16;     // ... and its widest staged row: the halo of step 16 on both sides
constexpr float AT_ALBEDO_FLOOR = 1e-3f;  // the albedo a colour is divided by, and multiplied by again, is at least this

__device__ __forceinline__ float b3(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// the 3 x 3 Gaussian of guided.hip's variance
__device__ __forceinline__ float g3(int dx, int dy) { return (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f); }

// Color3::castToUchar4 as write_pixel (shade.hpp) has it
__device__ __forceinline__ uint32_t quantise(float r, float g, float b) {
    const float cr = fminf(fmaxf(sqrtf(r), 0.0f), 0.999f);
    const float cg = fminf(fmaxf(sqrtf(g), 0.0f), 0.999f);
    const float cb = fminf(fmaxf(sqrtf(b), 0.0f), 0.999f);
    return (uint32_t)(uint8_t)(256.0f * cr) | ((uint32_t)(uint8_t)(256.0f * cg) << 8) |
           ((uint32_t)(uint8_t)(256.0f * cb) << 16) | (255u << 24);
}

// 1 / sigma^2 as the kernels multiply by it: 0 for +inf, and never +inf itself (0 * inf would be NaN for equal pixels)
float inv_sq(float sigma) {
    const float inv = 1.0f / (sigma * sigma);
    return inv < FLT_MAX ? inv : FLT_MAX;
}

// The last pass's result for pixel i multiplied by the albedo it was divided by, into the outputs there are.  (The
// division stays written out in the two pack kernels and in accumulate.hip: cross-referenced there.)
__device__ __forceinline__ void write_outputs(const float *albedo, float *rgb, uint32_t *rgba, size_t i, float r, float g,
                                              float b) {
    float ar = 1.0f, ag = 1.0f, ab = 1.0f;
    if (albedo) {
        ar = fmaxf(albedo[3 * i + 0], AT_ALBEDO_FLOOR);
        ag = fmaxf(albedo[3 * i + 1], AT_ALBEDO_FLOOR);
        ab = fmaxf(albedo[3 * i + 2], AT_ALBEDO_FLOOR);
    }
    const float o0 = r * ar, o1 = g * ag, o2 = b * ab;
    if (rgb) {
        rgb[3 * i + 0] = o0;
        rgb[3 * i + 1] = o1;
        rgb[3 * i + 2] = o2;
    }
    if (rgba) rgba[i] = quantise(o0, o1, o2);
}

// the guides of a pixel from its rt_hit record: {normal, flag} with flag 1 for a miss, and {point, 0}
__device__ __forceinline__ float4 guide_normal(const rt_hit *hit) {
    return make_float4(hit->normal.x, hit->normal.y, hit->normal.z, hit->instance == 0xFFFFFFFFu ? 1.0f : 0.0f);
}
__device__ __forceinline__ float4 guide_point(const rt_hit *hit) {
    return make_float4(hit->point.x, hit->point.y, hit->point.z, 0.0f);
}

// Row qy's `span` pixels from x0 on, of `src` and the guides (G: DenoiseGPU or GuidedGPU), into one LDS row buffer
// each; the caller's barrier follows.  (The tile's staging loop stays written out in both filter_lds: cross-referenced there.)
template <class G>
__device__ __forceinline__ void stage_row(const G &g, const float4 *__restrict__ src, int x0, int qy, int span, float4 *sc,
                                          float4 *sn, float4 *sx) {
    for (int k = (int)threadIdx.x; k < span; k += AT_ROW) {
        const int qx = x0 + k;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n = make_float4(0.0f, 0.0f, 0.0f, AT_OUTSIDE), q = c;
        if (qx >= 0 && qx < (int)g.w) {
            const size_t i = (size_t)qy * g.w + (size_t)qx;
            c = src[i];
            n = g.g0[i];
            q = g.g1[i];
        }
        sc[k] = c;
        sn[k] = n;
        sx[k] = q;
    }
}

}  // namespace

}  // namespace rtamd
