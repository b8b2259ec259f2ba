"""rt_denoise's filter (include/rt.h, "Denoising") restated in numpy, and a seeded synthetic guide generator.

denoise() is parameterised by dtype — float64 is the reference; float32 uses the operation order of csrc/denoise.hip,
so the kernel differs from it only in its expf — and by an optional (pass, dx, dy) tap to leave out, which
tests/test_denoise_ref.py uses to show that the GPU test's bar would notice any single missing tap.
"""
import numpy as np

K = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)      # B3 spline
ALBEDO_FLOOR = np.float32(1e-3)
MISS = 0xFFFFFFFF

# the GPU cases of tests/test_gpu_denoise.py: (width, height, iterations)
GPU_CASES = ((1, 1, 1), (7, 1, 3), (1, 7, 3), (16, 16, 2), (17, 17, 2), (64, 9, 3), (65, 9, 3), (37, 23, 5),
             (96, 64, 5), (65, 33, 4))
SIGMAS = (2.0, 1.0, 1.0)        # colour, normal, plane: the test calls' sigmas (float32-exact)


def inv_sq(sigma, dtype):
    """1 / sigma^2 as the kernels multiply by it: 0 for +inf, capped at the format's largest finite value."""
    with np.errstate(over="ignore", divide="ignore"):
        s = dtype(sigma)
        return min(dtype(1) / (s * s), np.finfo(dtype).max)


def lands(width, height, step, dx, dy):
    """Does tap (dx, dy) of a pass with this step lie inside the image for at least one pixel?"""
    return abs(step * dx) < width and abs(step * dy) < height


def denoise(color, normal, point, miss, albedo=None, *, iterations, sigma_color, sigma_normal, sigma_plane,
            dtype=np.float64, skip=None):
    """color, normal, point [H, W, 3], miss [H, W] bool, albedo [H, W, 3] or None -> the filtered image [H, W, 3] in
    `dtype`.  skip = (pass, dx, dy): that tap is left out of that pass."""
    H, W = miss.shape
    a = None if albedo is None else np.maximum(albedo.astype(dtype), dtype(ALBEDO_FLOOR))
    c = color.astype(dtype) if a is None else color.astype(dtype) / a
    n, x, flag = normal.astype(dtype), point.astype(dtype), np.asarray(miss, bool)
    inv_n, inv_p = inv_sq(sigma_normal, dtype), inv_sq(sigma_plane, dtype)
    for i in range(iterations):
        s = 1 << i
        inv_c = inv_sq(dtype(sigma_color) * dtype(2.0 ** -i), dtype)
        num = np.zeros((H, W, 3), dtype)
        den = np.zeros((H, W), dtype)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if skip == (i, dx, dy) or not lands(W, H, s, dx, dy):
                    continue
                h = dtype(K[dx + 2] * K[dy + 2])
                if dx == 0 and dy == 0:
                    num = num + h * c
                    den = den + h
                    continue
                ox, oy = s * dx, s * dy
                py, px = slice(max(0, -oy), H - max(0, oy)), slice(max(0, -ox), W - max(0, ox))
                qy, qx = slice(max(0, oy), H - max(0, -oy)), slice(max(0, ox), W - max(0, -ox))
                cp, cq = c[py, px], c[qy, qx]
                d = cp - cq
                dc2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                d = n[py, px] - n[qy, qx]
                dn2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                e = x[qy, qx] - x[py, px]
                m = n[py, px]
                dot = (m[..., 0] * e[..., 0] + m[..., 1] * e[..., 1]) + m[..., 2] * e[..., 2]
                with np.errstate(over="ignore"):
                    arg = (dc2 * inv_c + dn2 * inv_n) + (dot * dot) * inv_p
                    w = np.where(flag[py, px] == flag[qy, qx], np.exp(-arg), dtype(0))
                hw = h * w
                assert hw.dtype == dtype and cq.dtype == dtype
                num[py, px] = num[py, px] + hw[..., None] * cq
                den[py, px] = den[py, px] + hw
        with np.errstate(invalid="ignore", divide="ignore"):
            c = num / den[..., None]
    return c if a is None else c * a


def quantise(rgb):
    """Color3::castToUchar4 as write_pixel (csrc/shade.hpp) has it, on a float32 image -> uint8 [H, W, 4]."""
    rgb = np.asarray(rgb, np.float32)
    with np.errstate(invalid="ignore"):
        g = np.minimum(np.maximum(np.sqrt(rgb), np.float32(0.0)), np.float32(0.999))
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = (np.float32(256.0) * g).astype(np.uint8)
    return out


def synth(width, height, seed=0):
    """Seeded guides of a small scene seen head-on: a floor plane (z = 0, 0.05 world units per pixel) with a stripe of
    near-black albedo below the denoiser's floor of 1e-3, a sphere resting on it, and a band of sky (misses, all-zero
    records) across the middle — columns 0.35 W .. 0.55 W, or those rows of an image narrower than 4 — so that even
    the widest taps of a small image join two pixels of one kind.  colour = albedo x noise in [0.5, 1.5).  float32."""
    rng = np.random.default_rng(1000 * seed + 31 * width + height)
    W, H = width, height
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    normal = np.zeros((H, W, 3))
    normal[..., 2] = 1.0
    point = np.stack([0.05 * xx, 0.05 * yy, np.zeros((H, W))], axis=-1)
    albedo = np.empty((H, W, 3))
    albedo[:] = (0.7, 0.6, 0.5)
    albedo[(xx % 5) == 3] = (0.0005, 0.6, 0.5)
    cx, cy, R = 0.75 * W, 0.4 * H, 0.3 * min(W, H)
    u, v = (xx - cx) / max(R, 1e-9), (yy - cy) / max(R, 1e-9)
    inside = (u * u + v * v < 1.0) & (R >= 2.0)
    nz = np.sqrt(np.maximum(1.0 - u * u - v * v, 0.0))
    sn = np.stack([u, v, nz], axis=-1)
    normal[inside] = sn[inside]
    point[inside] = (np.array([0.05 * cx, 0.05 * cy, 0.0]) + 0.05 * R * sn)[inside]
    albedo[inside] = (0.2, 0.5, 0.8)
    t, n = (xx, W) if W >= 4 else (yy, H)
    miss = (t >= 0.35 * n) & (t < 0.55 * n) & (n >= 4)
    normal[miss] = 0.0
    point[miss] = 0.0
    albedo[miss] = (0.5, 0.7, 1.0)          # rt_query_camera's convention: the background
    albedo = albedo.astype(np.float32)
    color = albedo * rng.uniform(0.5, 1.5, (H, W, 3)).astype(np.float32)
    return {"color": color, "albedo": albedo, "normal": normal.astype(np.float32), "point": point.astype(np.float32),
            "miss": miss}


def hit_records(g, dtype):
    """The guides as rt_hit records in `dtype` (rtamd.renderer.HIT_DTYPE, hits_to_numpy's layout), [H * W]."""
    miss = g["miss"].reshape(-1)
    rec = np.zeros(miss.size, dtype)
    rec["t"] = np.where(miss, np.float32(np.inf), np.float32(1.0))
    rec["instance"] = np.where(miss, MISS, 0).astype(np.uint32)
    rec["point"] = g["point"].reshape(-1, 3)
    rec["normal"] = g["normal"].reshape(-1, 3)
    return rec


_cache = {}


def reference(width, height, iterations, with_albedo=True, sigmas=SIGMAS, seed=0):
    """(guides, ref64, ref32, F, bar) of one case, computed once and shared: F = max |ref32 - ref64|, and the GPU
    test's bar 4 F + 4 eps32 max |color|."""
    key = (width, height, iterations, with_albedo, tuple(float(s) for s in sigmas), seed)
    if key not in _cache:
        g = synth(width, height, seed)
        kw = dict(iterations=iterations, sigma_color=sigmas[0], sigma_normal=sigmas[1], sigma_plane=sigmas[2])
        alb = g["albedo"] if with_albedo else None
        r64 = denoise(g["color"], g["normal"], g["point"], g["miss"], alb, dtype=np.float64, **kw)
        r32 = denoise(g["color"], g["normal"], g["point"], g["miss"], alb, dtype=np.float32, **kw)
        assert r32.dtype == np.float32
        F = float(np.abs(r32.astype(np.float64) - r64).max())
        bar = 4.0 * F + 4.0 * float(np.finfo(np.float32).eps) * float(np.abs(g["color"]).max())
        for arr in (r64, r32, *g.values()):
            arr.setflags(write=False)
        _cache[key] = (g, r64, r32, F, bar)
    return _cache[key]
