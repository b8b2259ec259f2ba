"""rt_accumulate's filter (include/rt.h, "Temporal accumulation") restated in numpy, the reprojection rows in float64,
and a seeded synthetic guide generator.

accumulate() is parameterised by dtype.  float32 uses the operation order of csrc/accumulate.hip — every product and
sum on its own, IEEE division, floor, fabs, fmin and nothing else — so it gives the kernel's bits; float64 on the same
float32 inputs is the reference it is pinned against (tests/test_accumulate_ref.py).  skip_tap leaves one of the four
taps out and drop ignores one validity test: the CPU test uses them to show that such a change cannot hide.

The generator ray-casts a floor plane y = 0 (instance 0), a unit sphere at (0, 1, 0) (instance 1) and sky through a
camera derived as rt_camera_set derives it, with per-pixel jitter, and stores float32 rt_hit records.
"""
import numpy as np

MISS = 0xFFFFFFFF
F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)

# The thresholds and the history range of the test calls: lengths 1 .. 19 run past max_history, so the clamp is taken.
# Between two points of a unit sphere n . e = cos(angle) - 1, so with t about 5 a plane tolerance of 0.02 and a normal
# bound of 0.9 reject the same taps; 0.98 lets the normal test decide alone near the sphere's limb.  The plane test
# decides alone where the instance has moved: last frame's sphere stands PREV_SPHERE_SHIFT to the side.
MAX_HISTORY, NORMAL_COS, PLANE_TOLERANCE = 16.0, 0.98, 0.02
SPHERE = (0.0, 1.0, 0.0)
PREV_SPHERE_SHIFT = 0.12
MAX_LENGTH = 19
FOV = 60.0
CAMERA = ((0.0, 2.0, -5.0), (0.0, 1.0, 0.0))                 # centre, target: this frame
MOVED = ((0.3, 2.1, -4.8), (0.05, 1.0, 0.0))                 # last frame, a small move
PAN = ((0.0, 2.0, -5.0), (2.3, 1.0, 0.0))                    # last frame looked right: about a third lands outside
BEHIND = ((0.0, 2.0, -5.0), (0.0, 3.0, -10.0))               # last frame looked the other way: rw . v <= 0 everywhere
UP = (0.0, 1.0, 0.0)

# the GPU cases of tests/test_gpu_accumulate.py: sizes x views
SIZES = ((1, 1), (7, 1), (1, 7), (8, 8), (9, 9), (64, 2), (65, 2), (37, 23), (96, 64))
VIEWS = ("null", "same", "moved", "pan", "behind")
PREV_CAMERA = {"null": CAMERA, "same": CAMERA, "moved": MOVED, "pan": PAN, "behind": BEHIND}


def _unit(v):
    v = np.asarray(v, F32)
    l2 = F32(0.0)
    for a in range(3):
        l2 = l2 + v[a] * v[a]
    return (v / np.sqrt(l2)).astype(F32)


def derive_camera(centre, target, width, height, fov=FOV, up=UP):
    """pixel_origin, dx, dy, centre as rt_camera_set derives them (RenderPin.cu:73-95), in float32."""
    c, t, u = np.asarray(centre, F32), np.asarray(target, F32), np.asarray(up, F32)
    d = t - c
    fd = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).astype(F32)
    theta = F32(fov) * F32(np.pi) / F32(180.0)
    vw = F32(2.0) * np.tan(theta / F32(2.0), dtype=F32) * fd
    vh = vw / (F32(width) * F32(1.0) / F32(height))
    Wv = _unit(d)
    U = _unit(np.cross(Wv, u).astype(F32))
    V = _unit(np.cross(U, Wv).astype(F32))
    vx, vy = U * vw, V * vh
    dx, dy = vx / F32(width), vy / F32(height)
    vorg = c + Wv * fd - vx * F32(0.5) - vy * F32(0.5)
    po = vorg + dx * F32(0.5) + dy * F32(0.5)
    cam = {"po": po, "dx": dx, "dy": dy, "centre": c}
    assert all(v.dtype == F32 for v in cam.values())
    return cam


def reprojection_rows(cam):
    """The rows of rt_camera_reprojection from a camera's float32 pixel_origin, dx, dy and centre, in float64:
    fx = (rx . v) / (rw . v), fy = (ry . v) / (rw . v), v = x - centre."""
    dx, dy, c = (np.asarray(cam[k], np.float64) for k in ("dx", "dy", "centre"))
    p0 = np.asarray(cam["po"], np.float64) - c
    rx, ry, rw = np.cross(dy, p0), np.cross(p0, dx), np.cross(dx, dy)
    with np.errstate(divide="ignore", invalid="ignore"):
        det = float(np.dot(dx, rx))
        return {"centre": c, "rx": rx / det, "ry": ry / det, "rw": rw / det}


def rows32(rows):
    """The rows as the call receives them: rounded to float32."""
    return {k: np.asarray(v, np.float64).astype(F32) for k, v in rows.items()}


def project(rows, x):
    """(fx, fy, rw . v) of world points x [..., 3], in float64."""
    v = np.asarray(x, np.float64) - np.asarray(rows["centre"], np.float64)
    r = [v @ np.asarray(rows[k], np.float64) for k in ("rx", "ry", "rw")]
    with np.errstate(divide="ignore", invalid="ignore"):
        return r[0] / r[2], r[1] / r[2], r[2]


def hit_dtype():
    from rtamd.renderer import HIT_DTYPE
    return HIT_DTYPE


def raycast(cam, width, height, rng, sphere=SPHERE):
    """float32 rt_hit records [H, W] (denoise_ref.hit_records' layout) of the floor, the unit sphere at `sphere` and
    the sky seen through `cam`, one jittered ray per pixel, intersected analytically in float64."""
    sphere = np.asarray(sphere, np.float64)
    H, W = height, width
    jj, ii = np.mgrid[0:H, 0:W].astype(np.float64)
    ii = ii + rng.uniform(-0.5, 0.5, (H, W))
    jj = jj + rng.uniform(-0.5, 0.5, (H, W))
    po, dx, dy, c = (np.asarray(cam[k], np.float64) for k in ("po", "dx", "dy", "centre"))
    d = po + ii[..., None] * dx + jj[..., None] * dy - c
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_floor = np.where(d[..., 1] < 0.0, -c[1] / d[..., 1], np.inf)
        oc = c - sphere
        b = d @ oc
        disc = b * b - (oc @ oc - 1.0)
        t_sph = np.where(disc > 0.0, -b - np.sqrt(np.maximum(disc, 0.0)), np.inf)
    t_sph = np.where(t_sph > 0.0, t_sph, np.inf)
    t = np.minimum(t_floor, t_sph)
    hit = np.isfinite(t)
    on_sphere = hit & (t_sph <= t_floor)
    point = c + np.where(hit, t, 0.0)[..., None] * d
    normal = np.zeros((H, W, 3))
    normal[hit & ~on_sphere] = (0.0, 1.0, 0.0)
    normal[on_sphere] = (point - sphere)[on_sphere]
    rec = np.zeros((H, W), hit_dtype())
    rec["t"] = np.where(hit, t, np.inf).astype(F32)
    rec["instance"] = np.where(hit, np.where(on_sphere, 1, 0), MISS).astype(np.uint32)
    rec["point"] = np.where(hit[..., None], point, 0.0).astype(F32)
    rec["normal"] = np.where(hit[..., None], normal, 0.0).astype(F32)
    return rec


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def accumulate(color, hits, prev_hits, prev_history, view, *, max_history, normal_cos, plane_tolerance,
               dtype=np.float64, skip_tap=None, drop=None):
    """color [H, W, 3] float32, hits / prev_hits [H, W] rt_hit records, prev_history [H, W, 4] float32 (both prev None:
    the first frame), view = float32 rows {"centre", "rx", "ry", "rw"} or None -> (history [H, W, 4] in `dtype`,
    valid [H, W, 4] bool: which taps entered the blend).  skip_tap in 0..3: that tap is left out; drop in ("inside",
    "instance", "normal", "plane"): that validity test always passes.  A tap outside the image then reads what the
    index j W + i of a kernel without the test would reach, the neighbouring row's other end (modulo the image);
    clamping it to the edge instead would show nothing, since the blend is normalised."""
    f = dtype
    H, W = color.shape[:2]
    c = np.asarray(color, F32).astype(f)
    out = np.concatenate([c, np.ones((H, W, 1), f)], axis=-1)
    valid = np.zeros((H, W, 4), bool)
    if prev_history is None:
        assert prev_hits is None
        return out, valid
    hits, prev_hits = hits.reshape(H, W), prev_hits.reshape(H, W)
    prev_history = np.asarray(prev_history, F32).reshape(H, W, 4)
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
            r0, r1, r2 = _dot(rx, v), _dot(ry, v), _dot(rw, v)
            fx, fy = r0 / r2, r1 / r2
            ok = ok & (r2 > 0) & (fx >= -one) & (fx < f(W)) & (fy >= -one) & (fy < f(H))
            flx, fly = np.floor(np.where(ok, fx, 0)), np.floor(np.where(ok, fy, 0))
            ix, iy = flx.astype(np.int64), fly.astype(np.int64)
            wx, wy = fx - flx, fy - fly
        tol = f(plane_tolerance) * t
        S = np.zeros((H, W, 4), f)
        D = np.zeros((H, W), f)
        for tap in range(taps):
            tx, ty = tap & 1, tap >> 1
            qx, qy = ix + tx, iy + ty
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            qy, qx = np.divmod((qy * W + qx) % (W * H), W)
            m = prev_hits[qy, qx]
            e = m["point"].astype(f) - x
            tests = {"inside": inside, "instance": m["instance"] == inst,
                     "normal": _dot(n, m["normal"].astype(f)) >= f(normal_cos), "plane": np.abs(_dot(n, e)) <= tol}
            val = ok.copy()
            for name, passed in tests.items():
                if name != drop:
                    val &= passed
            if tap == skip_tap:
                val[:] = False
            b = ((wx if tx else one - wx) * (wy if ty else one - wy)) if view is not None else np.ones((H, W), f)
            Hq = prev_history[qy, qx].astype(f)
            S = np.where(val[..., None], S + b[..., None] * Hq, S)
            D = np.where(val, D + b, D)
            valid[..., tap] = val
        good = D > 0
        Hm = S / D[..., None]
        N = np.fmin(Hm[..., 3] + one, f(max_history))
        a = one / N
        rgb = Hm[..., :3] + a[..., None] * (c - Hm[..., :3])
    res = np.where(good[..., None], np.concatenate([rgb, N[..., None]], axis=-1), out)
    assert res.dtype == f
    return res, valid


_cache = {}


def case(width, height, view, seed=0):
    """One GPU case, computed once and shared (read-only): this frame's colour and records through CAMERA, last
    frame's records through the view's camera (another jitter), a random previous history with lengths 1 .. MAX_LENGTH,
    the rows the call gets ("null": None) and the two references."""
    key = (width, height, view, seed)
    if key not in _cache:
        rng = np.random.default_rng(7919 * seed + 131 * width + 17 * height + VIEWS.index(view))
        cur = derive_camera(*CAMERA, width, height)
        prev = derive_camera(*PREV_CAMERA[view], width, height)
        moved_sphere = (SPHERE[0] + PREV_SPHERE_SHIFT, SPHERE[1], SPHERE[2])
        g = {"hits": raycast(cur, width, height, rng), "prev_hits": raycast(prev, width, height, rng, moved_sphere),
             "color": rng.uniform(0.0, 1.5, (height, width, 3)).astype(F32)}
        hist = np.empty((height, width, 4), F32)
        hist[..., :3] = rng.uniform(0.0, 1.5, (height, width, 3))
        hist[..., 3] = rng.integers(1, MAX_LENGTH + 1, (height, width))
        g["prev_history"] = hist
        g["view"] = None if view == "null" else rows32(reprojection_rows(prev))
        kw = dict(max_history=MAX_HISTORY, normal_cos=NORMAL_COS, plane_tolerance=PLANE_TOLERANCE)
        args = (g["color"], g["hits"], g["prev_hits"], g["prev_history"], g["view"])
        g["ref64"], g["valid64"] = accumulate(*args, dtype=np.float64, **kw)
        g["ref32"], g["valid32"] = accumulate(*args, dtype=np.float32, **kw)
        for arr in g.values():
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
        _cache[key] = g
    return _cache[key]


def bound(width, height, longest=MAX_LENGTH):
    """What float32 may cost a pixel whose taps agree with float64's.  fx and fy are each a quotient of two
    three-term dot products whose terms are no larger than the frame is wide or high in pixels (times rw . v): about
    four roundings of size eps32 (W + H) each, which is what the bilinear weights inherit.  A weight's error moves the
    blend by at most that times the spread of the tapped values — at most `longest` on the length channel, the largest
    — for wx and for wy; the blend's own dozen roundings add eps32 `longest` each."""
    return (8.0 * (width + height) + 12.0) * EPS32 * float(longest)
