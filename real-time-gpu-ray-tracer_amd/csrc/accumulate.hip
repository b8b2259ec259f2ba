// accumulate.hip — rt_accumulate: temporal accumulation by reprojecting each pixel's hit point into the last frame.
// include/rt.h ("Temporal accumulation") states the filter; tests/accumulate_ref.py restates it in numpy with this
// file's operation order.  Built with -ffp-contract=off; the kernel uses +, -, *, IEEE division, floorf, fabsf and
// fminf only, so the float32 restatement gives its bits.
//   One launch, one thread per pixel, no LDS.  A thread reads its colour (12 B), its rt_hit record (48 B: t, instance,
//   point, normal are used), up to four of last frame's records and history texels, and writes a history texel (16 B)
//   and optionally the colour (12 B): 152 B of compulsory traffic per pixel when neighbouring lanes' taps share the
//   previous records.  Records are 4-byte aligned by contract, so they are read with dword loads; the history planes
//   are float4.
//   Two pixel-to-lane mappings, same arithmetic and so the same bits (ACC_FORM):
//     rows    blockDim (64, 4): a wave is 64 consecutive pixels of a row; its own records are one contiguous 3 KiB.
//     blocks  a 16 x 16 tile per workgroup, a wave an 8 x 8 block of it: the four taps of neighbouring lanes share
//             cache lines in both axes once the camera turns.
//   Measured on C2's frames (profiles/accumulate/README.md): rows is 7 to 8 % faster with a still camera, and the two
//   tie within 0.6 % when it moves, so rows is the default.
// Every tap's coordinates are tested before its loads; pixel indices are size_t.
//   rt_accumulate_moments is the same function with MOMENTS = true: the same taps, validity and weights also carry
//   the first two moments of the demodulated luminance (include/rt.h, "Variance-guided denoising"): 12 B of albedo and
//   up to four float2 read, one float2 written.  MOMENTS = false compiles to what it was before the template
//   (profiles/guided/kernel_resources.txt: 33 VGPRs, as profiles/accumulate/kernel_resources.txt).
//   rt_accumulate_motion is the same function with MOTION = true (include/rt.h, "Moving instances"): before the
//   reprojection the pixel's point and normal are carried to where their instance stood in the previous frame by the
//   instance's rt_instance_motion record, 96 B that the lanes of a wave mostly share (a near-uniform gather, read with
//   plain vector loads: the flags first, the five float4 and one float of the matrices only when the instance moved).
//   The four MOTION = false instantiations are the kernels they were, byte for byte (profiles/motion/README.md).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "atrous.hpp"
#include "launch.hpp"

namespace rtamd {

namespace {

constexpr uint32_t ACC_MISS = 0xFFFFFFFFu;

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

template <bool MOMENTS, bool MOTION>
__device__ __forceinline__ void accumulate_pixel(const AccumulateGPU &g, int i, int j) {
    const size_t k = (size_t)j * g.w + (size_t)i;
    const float cr = g.color[3 * k + 0], cg = g.color[3 * k + 1], cb = g.color[3 * k + 2];
    float4 out = make_float4(cr, cg, cb, 1.0f);                       // reset(p)
    float lum = 0.0f, lum2 = 0.0f;
    float2 mom = make_float2(0.0f, 0.0f);
    if (MOMENTS) {                                                    // L = lum(c / a), reset: (L, L L)
        float lr = cr, lg = cg, lb = cb;
        if (g.albedo) {                                               // as denoise.hip's and guided.hip's pack kernels divide
            lr = cr / fmaxf(g.albedo[3 * k + 0], AT_ALBEDO_FLOOR);
            lg = cg / fmaxf(g.albedo[3 * k + 1], AT_ALBEDO_FLOOR);
            lb = cb / fmaxf(g.albedo[3 * k + 2], AT_ALBEDO_FLOOR);
        }
        lum = rtamd::lum(lr, lg, lb);
        lum2 = lum * lum;
        mom = make_float2(lum, lum2);
    }
    const rt_hit *rec = g.hits + k;
    const uint32_t inst = rec->instance;
    if (g.prev_history && inst != ACC_MISS) {
        float px = rec->point.x, py = rec->point.y, pz = rec->point.z;
        float nx = rec->normal.x, ny = rec->normal.y, nz = rec->normal.z;
        const float tol = g.plane_tolerance * rec->t;
        int ix = i, iy = j;
        float wx = 0.0f, wy = 0.0f;
        bool ok = true;
        if (MOTION && inst < g.motion_count) {                        // past the records: static, and nothing is read
            const rt_instance_motion *mr = g.motion + inst;
            const uint32_t f = mr->flags;
            if (f == RT_MOTION_MOVED) {                               // the point and the normal where the instance was
                const float4 *rows = reinterpret_cast<const float4 *>(mr);          // 16-byte aligned by contract
                const float4 p0 = rows[0], p1 = rows[1], p2 = rows[2], n0 = rows[3], n1 = rows[4];
                const float n22 = mr->normal[8];
                const float qx = ((p0.x * px + p0.y * py) + p0.z * pz) + p0.w;
                const float qy = ((p1.x * px + p1.y * py) + p1.z * pz) + p1.w;
                const float qz = ((p2.x * px + p2.y * py) + p2.z * pz) + p2.w;
                const float ux = dot3(n0.x, n0.y, n0.z, nx, ny, nz);
                const float uy = dot3(n0.w, n1.x, n1.y, nx, ny, nz);
                const float uz = dot3(n1.z, n1.w, n22, nx, ny, nz);
                const float l2 = dot3(ux, uy, uz, ux, uy, uz);
                ok = l2 > 0.0f;                                       // a NaN fails
                const float s = sqrtf(l2);
                px = qx; py = qy; pz = qz;
                nx = ux / s; ny = uy / s; nz = uz / s;
            } else if (f != RT_MOTION_STATIC) {
                ok = false;                                           // RT_MOTION_NO_HISTORY and every unknown value
            }
        }
        if ((!MOTION || ok) && g.has_view) {
            const rt_reprojection &m = g.view;
            const float vx = px - m.centre[0], vy = py - m.centre[1], vz = pz - m.centre[2];
            const float r0 = dot3(m.rx[0], m.rx[1], m.rx[2], vx, vy, vz);
            const float r1 = dot3(m.ry[0], m.ry[1], m.ry[2], vx, vy, vz);
            const float r2 = dot3(m.rw[0], m.rw[1], m.rw[2], vx, vy, vz);
            const float fx = r0 / r2, fy = r1 / r2;
            ok = r2 > 0.0f && fx >= -1.0f && fx < (float)g.w && fy >= -1.0f && fy < (float)g.h;
            if (ok) {
                const float flx = floorf(fx), fly = floorf(fy);
                ix = (int)flx; iy = (int)fly;
                wx = fx - flx; wy = fy - fly;
            }
        }
        if (ok) {
            float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, den = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int tap = 0; tap < 4; tap++) {
                const int tx = tap & 1, ty = tap >> 1;
                if (!g.has_view && tap) break;
                const int qx = ix + tx, qy = iy + ty;
                if (qx < 0 || qy < 0 || qx >= (int)g.w || qy >= (int)g.h) continue;
                const size_t q = (size_t)qy * g.w + (size_t)qx;
                const rt_hit *m = g.prev_hits + q;
                if (m->instance != inst) continue;
                if (!(dot3(nx, ny, nz, m->normal.x, m->normal.y, m->normal.z) >= g.normal_cos)) continue;
                const float ex = m->point.x - px, ey = m->point.y - py, ez = m->point.z - pz;
                if (!(fabsf(dot3(nx, ny, nz, ex, ey, ez)) <= tol)) continue;
                const float b = g.has_view ? (tx ? wx : 1.0f - wx) * (ty ? wy : 1.0f - wy) : 1.0f;
                const float4 hq = g.prev_history[q];
                sr = sr + b * hq.x;
                sg = sg + b * hq.y;
                sb = sb + b * hq.z;
                sw = sw + b * hq.w;
                den = den + b;
                if (MOMENTS) {
                    const float2 mq = g.prev_moments[q];
                    s1 = s1 + b * mq.x;
                    s2 = s2 + b * mq.y;
                }
            }
            if (den > 0.0f) {
                const float hr = sr / den, hg = sg / den, hb = sb / den, hw = sw / den;
                const float n = fminf(hw + 1.0f, g.max_history);
                const float a = 1.0f / n;
                out = make_float4(hr + a * (cr - hr), hg + a * (cg - hg), hb + a * (cb - hb), n);
                if (MOMENTS) {
                    const float m1 = s1 / den, m2 = s2 / den;
                    mom = make_float2(m1 + a * (lum - m1), m2 + a * (lum2 - m2));
                }
            }
        }
    }
    g.history[k] = out;
    if (MOMENTS) g.moments[k] = mom;
    if (g.rgb) {
        g.rgb[3 * k + 0] = out.x;
        g.rgb[3 * k + 1] = out.y;
        g.rgb[3 * k + 2] = out.z;
    }
}

// blockDim (64, 4): a wave is 64 consecutive pixels of one row
template <bool MOMENTS, bool MOTION>
__global__ __launch_bounds__(256) void accumulate_rows_kernel(AccumulateGPU g) {
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    if (x >= (int)g.w || y >= (int)g.h) return;
    accumulate_pixel<MOMENTS, MOTION>(g, x, y);
}

// blockDim 256, a 16 x 16 tile: wave w is the 8 x 8 block (w & 1, w >> 1) of it, lane l its pixel (l & 7, l >> 3)
template <bool MOMENTS, bool MOTION>
__global__ __launch_bounds__(256) void accumulate_blocks_kernel(AccumulateGPU g) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int x = (int)(blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u));
    const int y = (int)(blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3));
    if (x >= (int)g.w || y >= (int)g.h) return;
    accumulate_pixel<MOMENTS, MOTION>(g, x, y);
}

// The mapping: 'r' rows, 'b' blocks.  scripts/accumulate_bench.py measures them side by side, alternating in one
// process, through RTAMD_ACCUMULATE_FORM (read per call; anything but one valid letter is ignored); the default is
// the faster of profiles/accumulate/README.md.
constexpr char ACC_FORM = 'r';
char pixel_mapping() {
    const char *e = std::getenv("RTAMD_ACCUMULATE_FORM");
    return e && (e[0] == 'r' || e[0] == 'b') && e[1] == 0 ? e[0] : ACC_FORM;
}

template <bool MOMENTS, bool MOTION>
void launch_mapping(const AccumulateGPU &g, bool rows, hipStream_t stream) {
    const dim3 grid = rows ? dim3((g.w + 63u) / 64u, (g.h + 3u) / 4u) : dim3((g.w + 15u) / 16u, (g.h + 15u) / 16u);
    const dim3 block = rows ? dim3(64, 4) : dim3(256);
    hipLaunchKernelGGL((rows ? accumulate_rows_kernel<MOMENTS, MOTION> : accumulate_blocks_kernel<MOMENTS, MOTION>), grid, block,
                       0, stream, g);
}

}  // namespace

// g.moments set: rt_accumulate_moments' instantiation; g.motion set: rt_accumulate_motion's
hipError_t launch_accumulate(const AccumulateGPU &g, hipStream_t stream) {
    const bool rows = pixel_mapping() == 'r';
    if (g.motion) {
        if (g.moments) launch_mapping<true, true>(g, rows, stream);
        else launch_mapping<false, true>(g, rows, stream);
    } else {
        if (g.moments) launch_mapping<true, false>(g, rows, stream);
        else launch_mapping<false, false>(g, rows, stream);
    }
    return hipGetLastError();
}

}  // namespace rtamd
