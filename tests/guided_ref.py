"""rt_accumulate_moments and rt_denoise_guided (include/rt.h, "Variance-guided denoising") restated in numpy, and a
seeded generator of accumulated frames.

Both restatements are parameterised by dtype.  float64 on the float32 inputs is the reference; float32 uses the
operation order of csrc/accumulate.hip and csrc/guided.hip, so accumulate_moments gives the kernel's bits and guided
differs from its kernels only through expf.  guided() also takes the faults tests/test_guided_ref.py uses to show that
the GPU test's bar would notice them: v_0 scaled, the 3 x 3 pre-filter of the variance left out, another length
threshold, and a single (pass, dx, dy) tap left out.

The guides are denoise_ref.synth's and the accumulation cases are accumulate_ref.case's; neither file is changed.
"""
import numpy as np

import accumulate_ref as A
import denoise_ref as D

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
MISS = 0xFFFFFFFF
LUM = (F32(0.2126), F32(0.7152), F32(0.0722))           # the kernels' float constants
K_EPS = F32(1e-6)
MIN_LENGTH = 4                                            # shorter histories take the spatial variance estimate
WINDOW = 3                                                # its window's radius
G3 = (0.25, 0.5, 0.25)                                    # the variance's pre-filter, per axis

# the filter cases of the CPU and GPU tests: (width, height, iterations)
CASES = ((1, 1, 1), (7, 1, 3), (1, 7, 3), (4, 4, 2), (16, 16, 2), (17, 17, 2), (65, 9, 3), (37, 23, 5), (257, 5, 4),
         (96, 64, 5))
SIGMAS = (4.0, 1.0, 1.0)                                  # luminance, normal, plane: the test calls' sigmas
LENGTHS = (1, 2, 3, 4, 5, 19)
AMP_HIT, AMP_SKY = 0.5, 0.02


def lum(c, f):
    return (f(LUM[0]) * c[..., 0] + f(LUM[1]) * c[..., 1]) + f(LUM[2]) * c[..., 2]


def demodulate(color, albedo, f):
    c = np.asarray(color, F32).astype(f)
    if albedo is None:
        return c, None
    a = np.maximum(np.asarray(albedo, F32).astype(f), f(D.ALBEDO_FLOOR))
    return c / a, a


# ---- rt_accumulate_moments -------------------------------------------------------------------------------------------

def accumulate_moments(color, albedo, hits, prev_hits, prev_history, prev_moments, view, *, max_history, normal_cos,
                       plane_tolerance, dtype=np.float64):
    """accumulate_ref.accumulate with the moments: the same taps, validity and weights.  color [H, W, 3], albedo
    [H, W, 3] or None, prev_moments [H, W, 2] (None with prev_history None) -> (history [H, W, 4], moments [H, W, 2])
    in `dtype`."""
    f = dtype
    H, W = color.shape[:2]
    c = np.asarray(color, F32).astype(f)
    L = lum(demodulate(color, albedo, f)[0], f)
    L2 = L * L
    out = np.concatenate([c, np.ones((H, W, 1), f)], axis=-1)
    mom = np.stack([L, L2], axis=-1)
    if prev_history is None:
        assert prev_hits is None and prev_moments is None
        return out, mom
    hits, prev_hits = hits.reshape(H, W), prev_hits.reshape(H, W)
    prev_history = np.asarray(prev_history, F32).reshape(H, W, 4)
    prev_moments = np.asarray(prev_moments, F32).reshape(H, W, 2)
    inst = hits["instance"]
    x, n, t = hits["point"].astype(f), hits["normal"].astype(f), hits["t"].astype(f)
    ok = inst != MISS
    jj, ii = np.mgrid[0:H, 0:W]
    one = f(1.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if view is None:
            ix, iy, taps = ii, jj, 1
            wx = wy = np.zeros((H, W), f)
        else:
            taps = 4
            ctr, rx, ry, rw = (np.asarray(view[k], F32).astype(f) for k in ("centre", "rx", "ry", "rw"))
            v = x - ctr
            r0, r1, r2 = A._dot(rx, v), A._dot(ry, v), A._dot(rw, v)
            fx, fy = r0 / r2, r1 / r2
            ok = ok & (r2 > 0) & (fx >= -one) & (fx < f(W)) & (fy >= -one) & (fy < f(H))
            flx, fly = np.floor(np.where(ok, fx, 0)), np.floor(np.where(ok, fy, 0))
            ix, iy = flx.astype(np.int64), fly.astype(np.int64)
            wx, wy = fx - flx, fy - fly
        tol = f(plane_tolerance) * t
        S = np.zeros((H, W, 4), f)
        SM = np.zeros((H, W, 2), f)
        Dn = np.zeros((H, W), f)
        for tap in range(taps):
            tx, ty = tap & 1, tap >> 1
            qx, qy = ix + tx, iy + ty
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            qy, qx = np.divmod((qy * W + qx) % (W * H), W)
            m = prev_hits[qy, qx]
            e = m["point"].astype(f) - x
            val = (ok & inside & (m["instance"] == inst) & (A._dot(n, m["normal"].astype(f)) >= f(normal_cos))
                   & (np.abs(A._dot(n, e)) <= tol))
            b = ((wx if tx else one - wx) * (wy if ty else one - wy)) if view is not None else np.ones((H, W), f)
            S = np.where(val[..., None], S + b[..., None] * prev_history[qy, qx].astype(f), S)
            SM = np.where(val[..., None], SM + b[..., None] * prev_moments[qy, qx].astype(f), SM)
            Dn = np.where(val, Dn + b, Dn)
        good = Dn > 0
        Hm = S / Dn[..., None]
        N = np.fmin(Hm[..., 3] + one, f(max_history))
        a = one / N
        rgb = Hm[..., :3] + a[..., None] * (c - Hm[..., :3])
        M = SM / Dn[..., None]
        M1 = M[..., 0] + a * (L - M[..., 0])
        M2 = M[..., 1] + a * (L2 - M[..., 1])
    res = np.where(good[..., None], np.concatenate([rgb, N[..., None]], axis=-1), out)
    mres = np.where(good[..., None], np.stack([M1, M2], axis=-1), mom)
    assert res.dtype == f and mres.dtype == f
    return res, mres


_mcache = {}
KW = dict(max_history=A.MAX_HISTORY, normal_cos=A.NORMAL_COS, plane_tolerance=A.PLANE_TOLERANCE)


def moments_case(width, height, view, seed=0):
    """accumulate_ref.case(width, height, view) with what the moments need: a random albedo (a fifth of it below the
    floor of 1e-3), random previous moments, and the float32 restatements with and without albedo and of a first
    frame.  Computed once, shared, read-only."""
    key = (width, height, view, seed)
    if key not in _mcache:
        g = dict(A.case(width, height, view, seed))
        rng = np.random.default_rng(50021 * seed + 977 * width + 13 * height + A.VIEWS.index(view))
        alb = rng.uniform(0.05, 1.0, (height, width, 3))
        alb[rng.uniform(0.0, 1.0, (height, width)) < 0.2] = (0.0004, 0.3, 0.0)
        g["albedo"] = alb.astype(F32)
        m1 = rng.uniform(0.0, 1.5, (height, width))
        g["prev_moments"] = np.stack([m1, m1 * m1 + rng.uniform(0.0, 0.3, (height, width))], axis=-1).astype(F32)
        args = (g["hits"], g["prev_hits"], g["prev_history"], g["prev_moments"], g["view"])
        g["with_albedo32"] = accumulate_moments(g["color"], g["albedo"], *args, dtype=np.float32, **KW)
        g["without_albedo32"] = accumulate_moments(g["color"], None, *args, dtype=np.float32, **KW)
        g["first32"] = accumulate_moments(g["color"], g["albedo"], g["hits"], None, None, None, g["view"],
                                          dtype=np.float32, **KW)
        for arr in g.values():
            for a in (arr if isinstance(arr, tuple) else (arr,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _mcache[key] = g
    return _mcache[key]


# ---- rt_denoise_guided -----------------------------------------------------------------------------------------------

def _shifted(H, W, ox, oy):
    """(p, q) index pairs of the pixels p whose tap q = p + (ox, oy) lies inside the image."""
    py, px = slice(max(0, -oy), H - max(0, oy)), slice(max(0, -ox), W - max(0, ox))
    qy, qx = slice(max(0, oy), H - max(0, -oy)), slice(max(0, ox), W - max(0, -ox))
    return (py, px), (qy, qx)


def _guide_terms(n, x, p, q, inv_n, inv_p):
    d = n[p] - n[q]
    dn2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    e = x[q] - x[p]
    m = n[p]
    dot = (m[..., 0] * e[..., 0] + m[..., 1] * e[..., 1]) + m[..., 2] * e[..., 2]
    return dn2 * inv_n, (dot * dot) * inv_p


def variance(history, moments, normal, point, miss, *, sigma_normal, sigma_plane, dtype=np.float64, threshold=MIN_LENGTH):
    """v_0 [H, W] in `dtype`: the temporal estimate where the length is at least `threshold`, else the spatial one."""
    f = dtype
    H, W = miss.shape
    N = np.asarray(history, F32)[..., 3].astype(f)
    m = np.asarray(moments, F32).astype(f)
    n, x, flag = np.asarray(normal, F32).astype(f), np.asarray(point, F32).astype(f), np.asarray(miss, bool)
    inv_n, inv_p = D.inv_sq(sigma_normal, f), D.inv_sq(sigma_plane, f)
    vt = np.maximum(f(0), m[..., 1] - m[..., 0] * m[..., 0])
    sg, s1, s2 = np.zeros((H, W), f), np.zeros((H, W), f), np.zeros((H, W), f)
    for dy in range(-WINDOW, WINDOW + 1):
        for dx in range(-WINDOW, WINDOW + 1):
            if abs(dx) >= W or abs(dy) >= H:
                continue
            p, q = _shifted(H, W, dx, dy)
            if dx == 0 and dy == 0:
                w = np.ones((H, W), f)
            else:
                tn, tp = _guide_terms(n, x, p, q, inv_n, inv_p)
                with np.errstate(over="ignore"):
                    w = np.where(flag[p] == flag[q], np.exp(-(tn + tp)), f(0))
            sg[p] = sg[p] + w
            s1[p] = s1[p] + w * m[q][..., 0]
            s2[p] = s2[p] + w * m[q][..., 1]
    m1, m2 = s1 / sg, s2 / sg
    vs = np.maximum(f(0), m2 - m1 * m1)
    v0 = np.where(N >= f(threshold), vt, vs) / N
    assert v0.dtype == f
    return v0


def guided(history, moments, normal, point, miss, albedo=None, *, iterations, sigma_luminance, sigma_normal, sigma_plane,
           dtype=np.float64, v0_scale=None, prefilter=True, threshold=MIN_LENGTH, skip=None):
    """history [H, W, 4], moments [H, W, 2], normal, point [H, W, 3], miss [H, W] bool, albedo [H, W, 3] or None ->
    (the filtered image [H, W, 3], v_0 [H, W]) in `dtype`.  The faults: v0_scale multiplies v_0 before the passes,
    prefilter=False uses v_i(p) for vbar_i(p), threshold replaces the 4 of the length test, skip = (pass, dx, dy)
    leaves that tap out of that pass."""
    f = dtype
    H, W = miss.shape
    c, a = demodulate(np.asarray(history, F32)[..., :3], albedo, f)
    n, x, flag = np.asarray(normal, F32).astype(f), np.asarray(point, F32).astype(f), np.asarray(miss, bool)
    inv_n, inv_p = D.inv_sq(sigma_normal, f), D.inv_sq(sigma_plane, f)
    v0 = variance(history, moments, normal, point, miss, sigma_normal=sigma_normal, sigma_plane=sigma_plane, dtype=f,
                  threshold=threshold)
    v = v0 if v0_scale is None else v0 * f(v0_scale)
    for i in range(iterations):
        s = 1 << i
        if prefilter:
            vsum, ksum = np.zeros((H, W), f), np.zeros((H, W), f)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if abs(dx) >= W or abs(dy) >= H:
                        continue
                    p, q = _shifted(H, W, dx, dy)
                    k = f(G3[dx + 1] * G3[dy + 1])
                    vsum[p] = vsum[p] + k * v[q]
                    ksum[p] = ksum[p] + k
            vbar = vsum / ksum
        else:
            vbar = v
        if np.isinf(sigma_luminance):
            kp = np.zeros((H, W), f)
        else:
            kp = f(1) / (f(sigma_luminance) * np.sqrt(vbar) + f(K_EPS))
        l = lum(c, f)
        num, vs, den = np.zeros((H, W, 3), f), np.zeros((H, W), f), np.zeros((H, W), f)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if skip == (i, dx, dy) or not D.lands(W, H, s, dx, dy):
                    continue
                h = f(D.K[dx + 2] * D.K[dy + 2])
                if dx == 0 and dy == 0:
                    num = num + h * c
                    vs = vs + (h * h) * v
                    den = den + h
                    continue
                p, q = _shifted(H, W, s * dx, s * dy)
                tn, tp = _guide_terms(n, x, p, q, inv_n, inv_p)
                with np.errstate(over="ignore"):
                    arg = (np.abs(l[p] - l[q]) * kp[p] + tn) + tp
                    w = np.where(flag[p] == flag[q], np.exp(-arg), f(0))
                hw = h * w
                assert hw.dtype == f
                num[p] = num[p] + hw[..., None] * c[q]
                vs[p] = vs[p] + (hw * hw) * v[q]
                den[p] = den[p] + hw
        c = num / den[..., None]
        v = vs / (den * den)
    out = c if a is None else c * a
    assert out.dtype == f
    return out, v0


def synth(width, height, seed=0, lengths="mixed"):
    """An accumulated frame on denoise_ref.synth's guides.  Lengths N from LENGTHS indexed by (x // 3 + 2 (y // 2)) % 6
    ("mixed"), or 1 everywhere ("first": a first frame); 1 on misses either way.  `lengths` may also be a tuple of
    ((x, y), (samples, length)) pairs (tests/filter_edges_ref.py): 8 samples and length 8.0 everywhere, misses
    included, except at those pixels, whose stored length need not be their sample count.  Per pixel N samples, each a
    smooth truth x (1 + amp U(-1, 1)) per channel with amp 0.5 on hits and 0.02 on sky, times the albedo; the history
    is their mean and their length, the moments the means of lum(sample / a) and its square — with and without albedo,
    since the moments are of the demodulated luminance.  float32."""
    g = dict(D.synth(width, height, seed))
    W, H = width, height
    rng = np.random.default_rng(77003 + 1000 * seed + 31 * width + height)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    miss = g["miss"]
    N = np.asarray(LENGTHS)[((xx.astype(int) // 3) + 2 * (yy.astype(int) // 2)) % 6] if lengths == "mixed" else np.ones((H, W), int)
    N = np.where(miss, 1, N)
    length = N.astype(np.float64)
    if isinstance(lengths, tuple):
        N, length = np.full((H, W), 8), np.full((H, W), 8.0)
        for (x, y), (count, stored) in lengths:
            N[y, x], length[y, x] = count, stored
    truth = np.stack([0.55 + 0.35 * np.sin(0.11 * xx + 0.7 * ch) * np.cos(0.13 * yy - 0.4 * ch) for ch in range(3)], axis=-1)
    amp = np.where(miss, AMP_SKY, AMP_HIT)[None, ..., None]
    u = rng.uniform(-1.0, 1.0, (max(LENGTHS), H, W, 3))
    samples = (g["albedo"].astype(np.float64) * truth * (1.0 + amp * u)).astype(F32)
    use = (np.arange(max(LENGTHS))[:, None, None] < N[None])[..., None]
    mean = (samples.astype(np.float64) * use).sum(axis=0) / N[..., None]
    g["history"] = np.concatenate([mean, length[..., None]], axis=-1).astype(F32)
    for name, alb in (("moments", g["albedo"]), ("moments_plain", None)):
        L = lum(demodulate(samples, alb, np.float64)[0], np.float64)
        m1 = (L * use[..., 0]).sum(axis=0) / N
        m2 = (L * L * use[..., 0]).sum(axis=0) / N
        g[name] = np.stack([m1, m2], axis=-1).astype(F32)
    del g["color"]
    return g


def constant(width, height, seed=0):
    """One constant colour and exactly zero variance on synth's guides, without albedo: every length 8."""
    g = dict(D.synth(width, height, seed))
    H, W = height, width
    g["history"] = np.tile(np.array([0.25, 0.5, 0.75, 8.0], F32), (H, W, 1))
    g["moments_plain"] = np.tile(np.array([0.5, 0.25], F32), (H, W, 1))      # m2 = m1 m1 exactly, in any format
    del g["color"]
    return g


_cache = {}


def reference(width, height, iterations, with_albedo=True, sigmas=SIGMAS, seed=0, lengths="mixed"):
    """One filter case, computed once and shared (read-only): {"g": inputs, "moments": the moments that go with
    with_albedo, "out64", "v64", "out32", "v32", "F", "bar", "Fv", "barv"}.  F = max |out32 - out64| and the GPU
    test's bar 4 F + 4 eps32 max |colour| (rt_denoise's bar); the same form for v_0."""
    key = (width, height, iterations, with_albedo, tuple(float(s) for s in sigmas), seed, lengths)
    if key not in _cache:
        g = (constant(width, height, seed) if lengths == "constant" else synth(width, height, seed, lengths))
        alb = g["albedo"] if with_albedo else None
        mom = g["moments"] if with_albedo else g["moments_plain"]
        kw = dict(iterations=iterations, sigma_luminance=sigmas[0], sigma_normal=sigmas[1], sigma_plane=sigmas[2])
        args = (g["history"], mom, g["normal"], g["point"], g["miss"], alb)
        o64, v64 = guided(*args, dtype=np.float64, **kw)
        o32, v32 = guided(*args, dtype=np.float32, **kw)
        F = float(np.abs(o32.astype(np.float64) - o64).max())
        Fv = float(np.abs(v32.astype(np.float64) - v64).max())
        r = {"g": g, "moments": mom, "albedo": alb, "kw": kw, "out64": o64, "v64": v64, "out32": o32, "v32": v32, "F": F, "Fv": Fv,
             "bar": 4.0 * F + 4.0 * EPS32 * float(np.abs(g["history"][..., :3]).max()),
             "barv": 4.0 * Fv + 4.0 * EPS32 * float(v64.max())}
        for arr in (o64, v64, o32, v32, *g.values()):
            arr.setflags(write=False)
        _cache[key] = r
    return _cache[key]
