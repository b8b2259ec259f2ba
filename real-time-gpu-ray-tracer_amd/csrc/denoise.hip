// denoise.hip — rt_denoise: the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on a frame's guides.
// include/rt.h states the filter; tests/denoise_ref.py restates it in numpy with this file's operation order.
// Built with -ffp-contract=off: every product and sum below rounds where the reference's does, so a result differs
// from the float32 restatement only through expf.
// The staged tile, the staged row, the scratch planes and the leaf functions it shares with guided.hip: atrous.hpp.
//   pack kernel     one thread per pixel: reads the colour, the albedo and the 48-byte rt_hit record once; writes the
//                   demodulated colour (float4) and the guides, 32 bytes per pixel, into scratch.  Since no pass
//                   reads color_device again, rgb32_device may be color_device itself.
//   filter passes   pass i has step 2^i and ping-pongs between the two colour planes of scratch.  The last one
//                   multiplies by the albedo again and writes rgb32 / rgba8 itself.
//     tile form     steps 1 and 2: the staged tile with its halo of 2 * step.
//     row form      steps 4, 8 and 16, where the halo reaches or exceeds the tile: the staged row.
//     direct form   a wave is 64 consecutive pixels of a row and reads 64 consecutive pixels at every tap: three
//                   coalesced 1 KiB loads, from L2 / Infinity Cache after the first touch; each tap's coordinates are
//                   tested before its loads.  Measured slower than the row form at every step (DN_FORMS), as is the
//                   tile form at step 4; both stay selectable for scripts/denoise_bench.py's side-by-side runs.
// Pixel indices are size_t.  Compulsory traffic: 72 B read + 48 B written per pixel by the pack pass, 48 + 16 B by a
// filter pass (the last one: 12 + 4 B written, and the albedo's 12 B read again).  The LDS forms are bound by their
// arithmetic, not by that traffic: about 60 VALU instructions per tap, 24 taps ("Denoiser").
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "atrous.hpp"
#include "launch.hpp"

namespace rtamd {

namespace {

struct DenoisePass {
    float inv_c, inv_n, inv_p;           // 1 / sigma^2 of this pass, at most FLT_MAX; 0 for sigma = +inf
    int step;
    uint32_t last;                       // write the outputs, not the other colour plane
};

struct Sums { float r, g, b, w; };

// One tap: h * w(p, q) into the sums.  The flags differ for hit / miss pairs and for staged taps outside the image.
// (dn2 and dot are also written out in guided.hip's add_tap and window_weight.)
__device__ __forceinline__ void add_tap(const float4 &cp, const float4 &np, const float4 &xp, const float4 &cq,
                                        const float4 &nq, const float4 &xq, float h, const DenoisePass &ps, Sums &s) {
    const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
    const float dc2 = (dr * dr + dg * dg) + db * db;
    const float nx = np.x - nq.x, ny = np.y - nq.y, nz = np.z - nq.z;
    const float dn2 = (nx * nx + ny * ny) + nz * nz;
    const float ex = xq.x - xp.x, ey = xq.y - xp.y, ez = xq.z - xp.z;
    const float dot = (np.x * ex + np.y * ey) + np.z * ez;
    const float d = (dc2 * ps.inv_c + dn2 * ps.inv_n) + (dot * dot) * ps.inv_p;
    const float w = nq.w == np.w ? expf(-d) : 0.0f;
    const float hw = h * w;
    s.r = s.r + hw * cq.x;
    s.g = s.g + hw * cq.y;
    s.b = s.b + hw * cq.z;
    s.w = s.w + hw;
}

__device__ __forceinline__ void add_centre(const float4 &cp, float h, Sums &s) {       // w = 1
    s.r = s.r + h * cp.x;
    s.g = s.g + h * cp.y;
    s.b = s.b + h * cp.z;
    s.w = s.w + h;
}

// a pass's result for pixel i: the next plane, or (last pass) the outputs
__device__ __forceinline__ void write_result(const DenoiseGPU &g, const DenoisePass &ps, float4 *__restrict__ dst, size_t i,
                                             const Sums &s) {
    const float r = s.r / s.w, gr = s.g / s.w, b = s.b / s.w;
    if (!ps.last) {
        dst[i] = make_float4(r, gr, b, 0.0f);
        return;
    }
    write_outputs(g.albedo, g.rgb, g.rgba, i, r, gr, b);
}

__global__ __launch_bounds__(256) void denoise_pack_kernel(DenoiseGPU g, float4 *__restrict__ plane) {
    const size_t n = (size_t)g.w * g.h;
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float r = g.color[3 * i + 0], gr = g.color[3 * i + 1], b = g.color[3 * i + 2];
    if (g.albedo) {                                          // as guided_pack_kernel and accumulate_pixel divide
        r = r / fmaxf(g.albedo[3 * i + 0], AT_ALBEDO_FLOOR);
        gr = gr / fmaxf(g.albedo[3 * i + 1], AT_ALBEDO_FLOOR);
        b = b / fmaxf(g.albedo[3 * i + 2], AT_ALBEDO_FLOOR);
    }
    const rt_hit *hit = g.hits + i;
    plane[i] = make_float4(r, gr, b, 0.0f);
    g.g0[i] = guide_normal(hit);
    g.g1[i] = guide_point(hit);
}

template <int STEP>
__device__ __forceinline__ void filter_lds(const DenoiseGPU &g, const DenoisePass &ps, const float4 *__restrict__ src,
                                           float4 *__restrict__ dst) {
    constexpr int HALO = 2 * STEP, EDGE = AT_TILE + 2 * HALO;
    static_assert(EDGE <= AT_PITCH, "the staged row does not fit its pitch");
    __shared__ float4 sc[EDGE * AT_PITCH], sn[EDGE * AT_PITCH], sx[EDGE * AT_PITCH];
    const int x0 = (int)blockIdx.x * AT_TILE - HALO, y0 = (int)blockIdx.y * AT_TILE - HALO;
    // the same loop stages guided.hip's filter_lds tile, and a similar one its variance tile
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
    Sums s{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float h = b3(dx) * b3(dy);
            if (dx == 0 && dy == 0) {
                add_centre(cp, h, s);
            } else {
                const int q = centre + dy * STEP * AT_PITCH + dx * STEP;
                add_tap(cp, np, xp, sc[q], sn[q], sx[q], h, ps, s);
            }
        }
    }
    write_result(g, ps, dst, (size_t)y * g.w + (size_t)x, s);
}

__global__ __launch_bounds__(256) void denoise_filter_lds1_kernel(DenoiseGPU g, DenoisePass ps, const float4 *__restrict__ src,
                                                                  float4 *__restrict__ dst) {
    filter_lds<1>(g, ps, src, dst);
}
__global__ __launch_bounds__(256) void denoise_filter_lds2_kernel(DenoiseGPU g, DenoisePass ps, const float4 *__restrict__ src,
                                                                  float4 *__restrict__ dst) {
    filter_lds<2>(g, ps, src, dst);
}
__global__ __launch_bounds__(256) void denoise_filter_lds4_kernel(DenoiseGPU g, DenoisePass ps, const float4 *__restrict__ src,
                                                                  float4 *__restrict__ dst) {
    filter_lds<4>(g, ps, src, dst);
}

// blockDim (64, 4): a wave is 64 consecutive pixels of one row
__global__ __launch_bounds__(256) void denoise_filter_direct_kernel(DenoiseGPU g, DenoisePass ps, const float4 *__restrict__ src,
                                                                    float4 *__restrict__ dst) {
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    if (x >= (int)g.w || y >= (int)g.h) return;
    const size_t p = (size_t)y * g.w + (size_t)x;
    const float4 cp = src[p], np = g.g0[p], xp = g.g1[p];
    Sums s{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * ps.step;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float h = b3(dx) * b3(dy);
            if (dx == 0 && dy == 0) {
                add_centre(cp, h, s);
                continue;
            }
            const int qx = x + dx * ps.step;
            if (qx < 0 || qy < 0 || qx >= (int)g.w || qy >= (int)g.h) continue;
            const size_t q = (size_t)qy * g.w + (size_t)qx;
            add_tap(cp, np, xp, src[q], g.g0[q], g.g1[q], h, ps, s);
        }
    }
    write_result(g, ps, dst, p, s);
}

// The row form (atrous.hpp, "the staged row"); the taps are summed in the order of the other forms.
__global__ __launch_bounds__(256) void denoise_filter_rows_kernel(DenoiseGPU g, DenoisePass ps, const float4 *__restrict__ src,
                                                                  float4 *__restrict__ dst) {
    __shared__ float4 sc[2][AT_ROW_SPAN], sn[2][AT_ROW_SPAN], sx[2][AT_ROW_SPAN];
    const int halo = 2 * ps.step, span = AT_ROW + 2 * halo;
    const int x0 = (int)blockIdx.x * AT_ROW - halo, y = (int)blockIdx.y;
    const int x = (int)blockIdx.x * AT_ROW + (int)threadIdx.x;
    const bool live = x < (int)g.w;
    const size_t p = (size_t)y * g.w + (size_t)(live ? x : 0);
    const float4 cp = src[p], np = g.g0[p], xp = g.g1[p];
    Sums s{0.0f, 0.0f, 0.0f, 0.0f};
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
                add_tap(cp, np, xp, sc[buf][k], sn[buf][k], sx[buf][k], h, ps, s);
            }
        }
        buf ^= 1;
    }
    if (live) write_result(g, ps, dst, p, s);
}

// The form of the passes of step 4, 8 and 16, one letter each: 't' the LDS tile (step 4 only: a 32 x 32 staged tile,
// 48 KiB), 'd' direct, 'r' rows.  All forms give the same bits.  scripts/denoise_bench.py measures them side by side,
// alternating in one process, through RTAMD_DENOISE_FORMS (read per call; anything but three valid letters is
// ignored); the defaults are the fastest of profiles/denoise/README.md.
constexpr char DN_FORMS[4] = "rrr";
void pass_forms(char f[3]) {
    const char *e = std::getenv("RTAMD_DENOISE_FORMS");
    const bool ok = e && (e[0] == 't' || e[0] == 'd' || e[0] == 'r') && (e[1] == 'd' || e[1] == 'r') &&
                    (e[2] == 'd' || e[2] == 'r') && e[3] == 0;
    for (int k = 0; k < 3; k++) f[k] = ok ? e[k] : DN_FORMS[k];
}

}  // namespace

hipError_t launch_denoise(const DenoiseGPU &g, uint32_t iterations, float sigma_color, float sigma_normal, float sigma_plane,
                          hipStream_t stream) {
    const size_t n = (size_t)g.w * g.h;
    hipLaunchKernelGGL(denoise_pack_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, g, g.plane[0]);
    hipError_t e = hipGetLastError();
    const dim3 tiles((g.w + AT_TILE - 1) / AT_TILE, (g.h + AT_TILE - 1) / AT_TILE);
    char forms[3];
    pass_forms(forms);
    for (uint32_t i = 0; i < iterations && e == hipSuccess; i++) {
        DenoisePass ps{};
        ps.step = 1 << i;
        ps.inv_c = inv_sq(sigma_color * (1.0f / (float)ps.step));
        ps.inv_n = inv_sq(sigma_normal);
        ps.inv_p = inv_sq(sigma_plane);
        ps.last = i + 1 == iterations ? 1u : 0u;
        const float4 *src = g.plane[i & 1u];
        float4 *dst = g.plane[(i + 1u) & 1u];
        const char form = i < 2 ? 't' : forms[i - 2];
        if (ps.step == 1)
            hipLaunchKernelGGL(denoise_filter_lds1_kernel, tiles, dim3(256), 0, stream, g, ps, src, dst);
        else if (ps.step == 2)
            hipLaunchKernelGGL(denoise_filter_lds2_kernel, tiles, dim3(256), 0, stream, g, ps, src, dst);
        else if (form == 't')
            hipLaunchKernelGGL(denoise_filter_lds4_kernel, tiles, dim3(256), 0, stream, g, ps, src, dst);
        else if (form == 'r')
            hipLaunchKernelGGL(denoise_filter_rows_kernel, dim3((g.w + AT_ROW - 1) / AT_ROW, g.h), dim3(AT_ROW), 0, stream, g, ps,
                               src, dst);
        else
            hipLaunchKernelGGL(denoise_filter_direct_kernel, dim3((g.w + 63u) / 64u, (g.h + 3u) / 4u), dim3(64, 4), 0, stream,
                               g, ps, src, dst);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace rtamd
