// guided.hip — rt_denoise_guided and rt_denoise_guided_feedback: the a-trous filter of denoise.hip steered by a
// per-pixel variance of the accumulated colour, in the manner of SVGF (Schied et al. 2017).  include/rt.h
// ("Variance-guided denoising") states the filter;
// tests/guided_ref.py restates it in numpy with this file's operation order.  Built with -ffp-contract=off: every
// product and sum rounds where the reference's does, so a result differs from the float32 restatement only through
// expf.  The staged tile, the staged row, the scratch planes and the leaf functions it shares with denoise.hip:
// atrous.hpp.
//   pack kernel      one thread per pixel: reads the history texel, the moments, the albedo and the rt_hit record once;
//                    writes the demodulated colour and the guides.  The colour
//                    plane's .w lane, which rt_denoise leaves 0, carries the variance: v_0 = v_t / N where the history
//                    is at least GD_MIN_LENGTH frames long, else -N, a request for the spatial estimate.
//   variance kernel  where the pack kernel left a request, the 7 x 7 window of moments weighted by the guides; a thread
//                    reads other pixels' guides and moments but only its own .w lane, so the kernel works in place.
//                    On a first frame every pixel asks; in steady state only sky and disocclusions.  Two forms, the
//                    same sums in the same order and so the same bits (GD_PREP):
//     tile form      the staged tile with its halo of 3 (guides and moments, 40 B per pixel), after a block-wide
//                    vote: a tile without a request reads 4 bytes per pixel and leaves before staging.  A staged
//                    tap outside the image carries AT_OUTSIDE and zero moments: weight 0, no coordinate test.
//     direct form    a wave is 64 consecutive pixels of a row; direct loads under the per-pixel branch, every tap's
//                    coordinates tested before its loads.
//   filter passes    pass i has step 2^i and ping-pongs between the two colour planes, variance included, so a pass's
//                    traffic stays 48 + 16 B per pixel.  The last one multiplies by the albedo and writes the outputs.
//     tile form      steps 1 and 2: the staged tile with its halo of 2 * step.  The 3 x 3 Gaussian of the variance
//                    reads the centre's neighbours at distance 1 from it.
//     row form       steps 4, 8 and 16: the staged row.  Rows y - 1 and y + 1 are not among the tap rows, so the nine
//                    variances come from the source plane by direct loads (4 bytes each, from lines the previous
//                    pass has just written).
//   feedback         rt_denoise_guided_feedback (include/rt.h, "History feedback"): a second instantiation of the
//                    step-1 pass also writes its result times the albedo, with the history's length, as next frame's
//                    history: 16 B per pixel more written and, unless it is the last pass, the albedo's 12 B read.
//                    The other kernels are the same code for both calls.
// Pixel indices are size_t.  No scratch memory and no spills (profiles/guided/kernel_resources.txt, and
// profiles/feedback/kernel_resources.txt for the feedback pass).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "atrous.hpp"
#include "launch.hpp"

namespace rtamd {

namespace {

constexpr float GD_MIN_LENGTH = 4.0f;    // shorter histories take the spatial variance estimate
constexpr int GD_WINDOW = 3;             // its window's radius

struct GuidedPass {
    float sigma_l;                       // sigma_luminance; lum_on = 0 when it is +inf
    float inv_n, inv_p;                  // 1 / sigma^2, at most FLT_MAX; 0 for sigma = +inf
    int step;
    uint32_t lum_on;
    uint32_t last;                       // write the outputs, not the other colour plane
};

struct GuidedSums { float r, g, b, v, w; };

// 1 / (sigma_luminance sqrt(vbar) + 1e-6), 0 with the term off
__device__ __forceinline__ float lum_scale(const GuidedPass &ps, float vsum, float ksum) {
    const float vbar = vsum / ksum;
    return ps.lum_on ? 1.0f / (ps.sigma_l * sqrtf(vbar) + 1e-6f) : 0.0f;
}

// One tap: h w(p, q) into the colour sums, (h w)^2 into the variance's.  cq.w is v_i(q).  (dn2 and dot are also
// written out in window_weight below and in denoise.hip's add_tap.)
__device__ __forceinline__ void add_tap(float lp, float kp, const float4 &np, const float4 &xp, const float4 &cq,
                                        const float4 &nq, const float4 &xq, float h, const GuidedPass &ps, GuidedSums &s) {
    const float dl = fabsf(lp - lum(cq.x, cq.y, cq.z));
    const float nx = np.x - nq.x, ny = np.y - nq.y, nz = np.z - nq.z;
    const float dn2 = (nx * nx + ny * ny) + nz * nz;
    const float ex = xq.x - xp.x, ey = xq.y - xp.y, ez = xq.z - xp.z;
    const float dot = (np.x * ex + np.y * ey) + np.z * ez;
    const float d = (dl * kp + dn2 * ps.inv_n) + (dot * dot) * ps.inv_p;
    const float w = nq.w == np.w ? expf(-d) : 0.0f;
    const float hw = h * w;
    s.r = s.r + hw * cq.x;
    s.g = s.g + hw * cq.y;
    s.b = s.b + hw * cq.z;
    s.v = s.v + (hw * hw) * cq.w;
    s.w = s.w + hw;
}

__device__ __forceinline__ void add_centre(const float4 &cp, float h, GuidedSums &s) {       // w = 1
    s.r = s.r + h * cp.x;
    s.g = s.g + h * cp.y;
    s.b = s.b + h * cp.z;
    s.v = s.v + (h * h) * cp.w;
    s.w = s.w + h;
}

// a pass's result for pixel i: the next plane, or (last pass) the outputs
__device__ __forceinline__ void write_result(const GuidedGPU &g, const GuidedPass &ps, float4 *__restrict__ dst, size_t i,
                                             const GuidedSums &s) {
    const float r = s.r / s.w, gr = s.g / s.w, b = s.b / s.w;
    if (!ps.last) {
        dst[i] = make_float4(r, gr, b, s.v / (s.w * s.w));
        return;
    }
    write_outputs(g.albedo, g.rgb, g.rgba, i, r, gr, b);
}

// The first pass of rt_denoise_guided_feedback: write_result, and {the result times the albedo, the history's length}
// into `feedback`, next frame's prev_history.  With iterations = 1 the outputs and the feedback are the same three
// products.  `feedback` may be g.history itself: the pack kernel has read the colour, and the length is read here by
// the one thread that then writes the texel.  (The albedo's floor and the stores: as atrous.hpp's write_outputs.)
__device__ __forceinline__ void write_result_feedback(const GuidedGPU &g, const GuidedPass &ps, float4 *__restrict__ dst,
                                                      float4 *feedback, size_t i, const GuidedSums &s) {
    const float r = s.r / s.w, gr = s.g / s.w, b = s.b / s.w;
    float ar = 1.0f, ag = 1.0f, ab = 1.0f;
    if (g.albedo) {
        ar = fmaxf(g.albedo[3 * i + 0], AT_ALBEDO_FLOOR);
        ag = fmaxf(g.albedo[3 * i + 1], AT_ALBEDO_FLOOR);
        ab = fmaxf(g.albedo[3 * i + 2], AT_ALBEDO_FLOOR);
    }
    const float o0 = r * ar, o1 = gr * ag, o2 = b * ab;
    const float length = reinterpret_cast<const float *>(g.history + i)[3];
    feedback[i] = make_float4(o0, o1, o2, length);
    if (!ps.last) {
        dst[i] = make_float4(r, gr, b, s.v / (s.w * s.w));
        return;
    }
    if (g.rgb) {
        g.rgb[3 * i + 0] = o0;
        g.rgb[3 * i + 1] = o1;
        g.rgb[3 * i + 2] = o2;
    }
    if (g.rgba) g.rgba[i] = quantise(o0, o1, o2);
}

__global__ __launch_bounds__(256) void guided_pack_kernel(GuidedGPU g) {
    const size_t n = (size_t)g.w * g.h;
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 hist = g.history[i];
    float r = hist.x, gr = hist.y, b = hist.z;
    if (g.albedo) {                                          // as denoise_pack_kernel and accumulate_pixel divide
        r = r / fmaxf(g.albedo[3 * i + 0], AT_ALBEDO_FLOOR);
        gr = gr / fmaxf(g.albedo[3 * i + 1], AT_ALBEDO_FLOOR);
        b = b / fmaxf(g.albedo[3 * i + 2], AT_ALBEDO_FLOOR);
    }
    const float2 m = g.moments[i];
    float v = -hist.w;                                       // the variance kernel's business
    if (hist.w >= GD_MIN_LENGTH) {
        v = fmaxf(0.0f, m.y - m.x * m.x) / hist.w;
        if (g.variance) g.variance[i] = v;
    }
    const rt_hit *hit = g.hits + i;
    g.plane[0][i] = make_float4(r, gr, b, v);
    g.g0[i] = guide_normal(hit);
    g.g1[i] = guide_point(hit);
}

// One window tap into the sums; the centre has w = 1.  (dn2 and dot: as add_tap has them.)
__device__ __forceinline__ float window_weight(const float4 &np, const float4 &xp, const float4 &nq, const float4 &xq,
                                               float inv_n, float inv_p) {
    const float nx = np.x - nq.x, ny = np.y - nq.y, nz = np.z - nq.z;
    const float dn2 = (nx * nx + ny * ny) + nz * nz;
    const float ex = xq.x - xp.x, ey = xq.y - xp.y, ez = xq.z - xp.z;
    const float dot = (np.x * ex + np.y * ey) + np.z * ez;
    const float d = dn2 * inv_n + (dot * dot) * inv_p;
    return nq.w == np.w ? expf(-d) : 0.0f;
}

// blockDim 256, a 16 x 16 tile, one thread per pixel
__global__ __launch_bounds__(256) void guided_variance_tile_kernel(GuidedGPU g, float inv_n, float inv_p) {
    constexpr int EDGE = AT_TILE + 2 * GD_WINDOW;
    static_assert(EDGE <= AT_PITCH, "the staged row does not fit its pitch");
    __shared__ float4 sn[EDGE * AT_PITCH], sx[EDGE * AT_PITCH];
    __shared__ float2 sm[EDGE * AT_PITCH];
    const int tx = (int)threadIdx.x % AT_TILE, ty = (int)threadIdx.x / AT_TILE;
    const int x = (int)blockIdx.x * AT_TILE + tx, y = (int)blockIdx.y * AT_TILE + ty;
    float *slot = nullptr;
    float length = 0.0f;
    if (x < (int)g.w && y < (int)g.h) {
        slot = reinterpret_cast<float *>(g.plane[0] + ((size_t)y * g.w + (size_t)x)) + 3;
        length = -*slot;
    }
    const bool asks = length > 0.0f;                         // else the pack kernel wrote v_0 itself
    if (!__syncthreads_or(asks ? 1 : 0)) return;
    const int x0 = (int)blockIdx.x * AT_TILE - GD_WINDOW, y0 = (int)blockIdx.y * AT_TILE - GD_WINDOW;
    // as filter_lds stages its tile, with the moments in the colour's place
    for (int k = (int)threadIdx.x; k < EDGE * EDGE; k += 256) {
        const int ly = k / EDGE, lx = k - ly * EDGE;
        const int qx = x0 + lx, qy = y0 + ly;
        float4 n = make_float4(0.0f, 0.0f, 0.0f, AT_OUTSIDE), p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float2 m = make_float2(0.0f, 0.0f);
        if (qx >= 0 && qy >= 0 && qx < (int)g.w && qy < (int)g.h) {
            const size_t q = (size_t)qy * g.w + (size_t)qx;
            n = g.g0[q];
            p = g.g1[q];
            m = g.moments[q];
        }
        sn[ly * AT_PITCH + lx] = n;
        sx[ly * AT_PITCH + lx] = p;
        sm[ly * AT_PITCH + lx] = m;
    }
    __syncthreads();
    if (!asks) return;
    const int centre = (ty + GD_WINDOW) * AT_PITCH + tx + GD_WINDOW;
    const float4 np = sn[centre], xp = sx[centre];
    float sg = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int dy = -GD_WINDOW; dy <= GD_WINDOW; dy++) {
#pragma unroll
        for (int dx = -GD_WINDOW; dx <= GD_WINDOW; dx++) {
            const int q = centre + dy * AT_PITCH + dx;
            const float2 m = sm[q];
            const float w = (dx == 0 && dy == 0) ? 1.0f : window_weight(np, xp, sn[q], sx[q], inv_n, inv_p);
            sg = sg + w;
            s1 = s1 + w * m.x;
            s2 = s2 + w * m.y;
        }
    }
    const float m1 = s1 / sg, m2 = s2 / sg;                  // as guided_variance_direct_kernel ends
    const float v = fmaxf(0.0f, m2 - m1 * m1) / length;
    *slot = v;
    if (g.variance) g.variance[(size_t)y * g.w + (size_t)x] = v;
}

// blockDim (64, 4): a wave is 64 consecutive pixels of one row
__global__ __launch_bounds__(256) void guided_variance_direct_kernel(GuidedGPU g, float inv_n, float inv_p) {
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    if (x >= (int)g.w || y >= (int)g.h) return;
    const size_t p = (size_t)y * g.w + (size_t)x;
    float *slot = reinterpret_cast<float *>(g.plane[0] + p) + 3;
    const float length = -*slot;
    if (!(length > 0.0f)) return;                            // the pack kernel wrote v_0 itself
    const float4 np = g.g0[p], xp = g.g1[p];
    float sg = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int dy = -GD_WINDOW; dy <= GD_WINDOW; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= (int)g.h) continue;
        for (int dx = -GD_WINDOW; dx <= GD_WINDOW; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= (int)g.w) continue;
            const size_t q = (size_t)qy * g.w + (size_t)qx;
            const float2 m = g.moments[q];
            const float w = (dx == 0 && dy == 0) ? 1.0f : window_weight(np, xp, g.g0[q], g.g1[q], inv_n, inv_p);
            sg = sg + w;
            s1 = s1 + w * m.x;
            s2 = s2 + w * m.y;
        }
    }
    const float m1 = s1 / sg, m2 = s2 / sg;                  // as guided_variance_tile_kernel ends
    const float v = fmaxf(0.0f, m2 - m1 * m1) / length;
    *slot = v;
    if (g.variance) g.variance[p] = v;
}

template <int STEP, bool FEEDBACK>
__device__ __forceinline__ void filter_lds(const GuidedGPU &g, const GuidedPass &ps, const float4 *__restrict__ src,
                                           float4 *__restrict__ dst, float4 *feedback = nullptr) {
    constexpr int HALO = 2 * STEP, EDGE = AT_TILE + 2 * HALO;
    static_assert(EDGE <= AT_PITCH, "the staged row does not fit its pitch");
    __shared__ float4 sc[EDGE * AT_PITCH], sn[EDGE * AT_PITCH], sx[EDGE * AT_PITCH];
    const int x0 = (int)blockIdx.x * AT_TILE - HALO, y0 = (int)blockIdx.y * AT_TILE - HALO;
    // the same loop stages denoise.hip's filter_lds tile
    for (int k = (int)threadIdx.x; k < EDGE * EDGE; k += 256) {
        const int ly = k / EDGE, lx = k - ly * EDGE;
        const int x = x0 + lx, y = y0 + ly;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n = make_float4(0.0f, 0.0f, 0.0f, AT_OUTSIDE), p = c;
        if (x >= 0 && y >= 0 && x < (int)g.w && y < (int)g.h) {
            const size_t q = (size_t)y * g.w + (size_t)x;
            c = src[q];
            n = g.g0[q];
            p = g.g1[q];
        }
        sc[ly * AT_PITCH + lx] = c;
        sn[ly * AT_PITCH + lx] = n;
        sx[ly * AT_PITCH + lx] = p;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x % AT_TILE, ty = (int)threadIdx.x / AT_TILE;
    const int x = (int)blockIdx.x * AT_TILE + tx, y = (int)blockIdx.y * AT_TILE + ty;
    if (x >= (int)g.w || y >= (int)g.h) return;
    const int centre = (ty + HALO) * AT_PITCH + tx + HALO;
    const float4 cp = sc[centre], np = sn[centre], xp = sx[centre];
    // the 3 x 3 Gaussian of the variance, distance 1 at every step; a staged tap outside the image carries AT_OUTSIDE
    float vsum = 0.0f, ksum = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int q = centre + dy * AT_PITCH + dx;
            if (sn[q].w == AT_OUTSIDE) continue;
            const float k = g3(dx, dy);
            vsum = vsum + k * sc[q].w;
            ksum = ksum + k;
        }
    }
    const float kp = lum_scale(ps, vsum, ksum), lp = lum(cp.x, cp.y, cp.z);
    GuidedSums s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float h = b3(dx) * b3(dy);
            if (dx == 0 && dy == 0) {
                add_centre(cp, h, s);
            } else {
                const int q = centre + dy * STEP * AT_PITCH + dx * STEP;
                add_tap(lp, kp, np, xp, sc[q], sn[q], sx[q], h, ps, s);
            }
        }
    }
    if (FEEDBACK)
        write_result_feedback(g, ps, dst, feedback, (size_t)y * g.w + (size_t)x, s);
    else
        write_result(g, ps, dst, (size_t)y * g.w + (size_t)x, s);
}

__global__ __launch_bounds__(256) void guided_filter_lds1_kernel(GuidedGPU g, GuidedPass ps, const float4 *__restrict__ src,
                                                                 float4 *__restrict__ dst) {
    filter_lds<1, false>(g, ps, src, dst);
}
// rt_denoise_guided_feedback's first pass
__global__ __launch_bounds__(256) void guided_filter_lds1_feedback_kernel(GuidedGPU g, GuidedPass ps,
                                                                          const float4 *__restrict__ src,
                                                                          float4 *__restrict__ dst, float4 *feedback) {
    filter_lds<1, true>(g, ps, src, dst, feedback);
}
__global__ __launch_bounds__(256) void guided_filter_lds2_kernel(GuidedGPU g, GuidedPass ps, const float4 *__restrict__ src,
                                                                 float4 *__restrict__ dst) {
    filter_lds<2, false>(g, ps, src, dst);
}

// The row form (atrous.hpp, "the staged row")
__global__ __launch_bounds__(256) void guided_filter_rows_kernel(GuidedGPU g, GuidedPass ps, const float4 *__restrict__ src,
                                                                 float4 *__restrict__ dst) {
    __shared__ float4 sc[2][AT_ROW_SPAN], sn[2][AT_ROW_SPAN], sx[2][AT_ROW_SPAN];
    const int halo = 2 * ps.step, span = AT_ROW + 2 * halo;
    const int x0 = (int)blockIdx.x * AT_ROW - halo, y = (int)blockIdx.y;
    const int x = (int)blockIdx.x * AT_ROW + (int)threadIdx.x;
    const bool live = x < (int)g.w;
    const int xc = live ? x : 0;
    const size_t p = (size_t)y * g.w + (size_t)xc;
    const float4 cp = src[p], np = g.g0[p], xp = g.g1[p];
    float vsum = 0.0f, ksum = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = xc + dx;
            if (qx < 0 || qy < 0 || qx >= (int)g.w || qy >= (int)g.h) continue;
            const float k = g3(dx, dy);
            const float vq = (dx == 0 && dy == 0) ? cp.w : reinterpret_cast<const float *>(src + ((size_t)qy * g.w + (size_t)qx))[3];
            vsum = vsum + k * vq;
            ksum = ksum + k;
        }
    }
    const float kp = lum_scale(ps, vsum, ksum), lp = lum(cp.x, cp.y, cp.z);
    GuidedSums s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int buf = 0;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * ps.step;
        if (qy < 0 || qy >= (int)g.h) continue;            // block-uniform
        stage_row(g, src, x0, qy, span, sc[buf], sn[buf], sx[buf]);
        __syncthreads();
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float h = b3(dx) * b3(dy);
            if (dx == 0 && dy == 0) {
                add_centre(cp, h, s);
            } else {
                const int k = (int)threadIdx.x + halo + dx * ps.step;
                add_tap(lp, kp, np, xp, sc[buf][k], sn[buf][k], sx[buf][k], h, ps, s);
            }
        }
        buf ^= 1;
    }
    if (live) write_result(g, ps, dst, p, s);
}

// The variance kernel's form: 't' the LDS tile, 'd' direct.  Both give the same bits.  scripts/guided_bench.py measures
// them side by side, alternating in one process, through RTAMD_GUIDED_PREP (read per call; anything but one valid
// letter is ignored); the default is the faster of profiles/guided/README.md.
constexpr char GD_PREP = 't';
char prep_form() {
    const char *e = std::getenv("RTAMD_GUIDED_PREP");
    return e && (e[0] == 't' || e[0] == 'd') && e[1] == 0 ? e[0] : GD_PREP;
}

}  // namespace

hipError_t launch_denoise_guided(const GuidedGPU &g, uint32_t iterations, float sigma_luminance, float sigma_normal,
                                 float sigma_plane, float4 *feedback, hipStream_t stream) {
    const size_t n = (size_t)g.w * g.h;
    GuidedPass ps{};
    ps.sigma_l = sigma_luminance;
    ps.lum_on = std::isinf(sigma_luminance) ? 0u : 1u;
    ps.inv_n = inv_sq(sigma_normal);
    ps.inv_p = inv_sq(sigma_plane);
    hipLaunchKernelGGL(guided_pack_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 tiles((g.w + AT_TILE - 1) / AT_TILE, (g.h + AT_TILE - 1) / AT_TILE);
    if (prep_form() == 't')
        hipLaunchKernelGGL(guided_variance_tile_kernel, tiles, dim3(256), 0, stream, g, ps.inv_n, ps.inv_p);
    else
        hipLaunchKernelGGL(guided_variance_direct_kernel, dim3((g.w + 63u) / 64u, (g.h + 3u) / 4u), dim3(64, 4), 0, stream, g,
                           ps.inv_n, ps.inv_p);
    e = hipGetLastError();
    for (uint32_t i = 0; i < iterations && e == hipSuccess; i++) {
        ps.step = 1 << i;
        ps.last = i + 1 == iterations ? 1u : 0u;
        const float4 *src = g.plane[i & 1u];
        float4 *dst = g.plane[(i + 1u) & 1u];
        if (ps.step == 1 && feedback)
            hipLaunchKernelGGL(guided_filter_lds1_feedback_kernel, tiles, dim3(256), 0, stream, g, ps, src, dst, feedback);
        else if (ps.step == 1)
            hipLaunchKernelGGL(guided_filter_lds1_kernel, tiles, dim3(256), 0, stream, g, ps, src, dst);
        else if (ps.step == 2)
            hipLaunchKernelGGL(guided_filter_lds2_kernel, tiles, dim3(256), 0, stream, g, ps, src, dst);
        else
            hipLaunchKernelGGL(guided_filter_rows_kernel, dim3((g.w + AT_ROW - 1) / AT_ROW, g.h), dim3(AT_ROW), 0, stream, g, ps,
                               src, dst);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace rtamd
