"""Ray sets and range bounds shared by the ranged-oracle tests (tests/test_oracle_kat.py) and the GPU ray-query edge
tests (tests/test_gpu_ray_query_edges.py).  Pure numpy: no GPU, no oracle.

The reference's range test (Range.cuh:33-43) is closed at both ends with an absolute 1e-6 window: t is accepted when
|t - tmax| < 1e-6 or tmin < t < tmax.  boundary_tmax places tmax on, one ulp off, inside and outside that window around
the closest hit t_c of every ray, which is where a wrong comparison in a kernel shows.
"""
import numpy as np

F32 = np.float32
INF32 = F32(np.inf)

# tmax for rays the oracle misses with an unbounded range: any finite range is a miss as well
MISS_TMAX = F32(10.0)


def boundary_tmax(tc, hit):
    """{name: float32 tmax[N]} around the closest t_c (float32 [N]) of the rays with hit[i]; MISS_TMAX elsewhere.

    The +-5e-7 and +-2e-6 offsets are added in float32, as a caller would: for large t_c they round to a whole number
    of ulps (possibly 0), which is part of what the cases pin."""
    tc = np.asarray(tc, F32)
    safe = np.where(hit, tc, F32(1.0)).astype(F32)
    cases = {
        "t_c": safe,
        "next_down": np.nextafter(safe, -INF32),
        "next_up": np.nextafter(safe, INF32),
        "minus_5e-7": safe - F32(5e-7),
        "plus_5e-7": safe + F32(5e-7),
        "minus_2e-6": safe - F32(2e-6),
        "plus_2e-6": safe + F32(2e-6),
    }
    return {k: np.where(hit, v, MISS_TMAX).astype(F32) for k, v in cases.items()}


# the lower end of the range, for rays that start on a surface (hits at t < 0.001 are self-hits and ignored)
TMIN_TMAX = (F32(0.001), np.nextafter(F32(0.001), INF32), F32(0.0010005), F32(0.002))


# ---- degenerate ray classes ------------------------------------------------------------------------------------------
# BoundingBox::hit (BoundingBox.cu:34-72) treats |d| < 1e-6 on an axis as parallel to the slab; the values straddle it
SUB_THRESHOLD = (F32(5e-7), F32(-5e-7), F32(9.99e-7), F32(1.0001e-6), F32(1e-20))


def zero_component_rays(rays):
    """d.x = 0 on every ray and d.z = 0 on every second one (directions are not renormalised)."""
    r = np.array(rays, F32)
    r[:, 3] = 0.0
    r[1::2, 5] = 0.0
    return r


def sub_threshold_rays(rays):
    """The components zero_component_rays clears, set to the SUB_THRESHOLD values in turn (d.x and d.z of one ray get
    different ones)."""
    r = np.array(rays, F32)
    i = np.arange(len(r))
    v = np.asarray(SUB_THRESHOLD, F32)
    r[:, 3] = v[i % len(v)]
    r[1::2, 5] = v[(i // 2 + 2) % len(v)][1::2]
    return r


def down_rays(n, seed, y=8.0):
    """d = (0, -1, 0) from height y, x and z uniform over the scene's footprint ([-4, 4]^2, where gen_rays aims)."""
    g = np.random.default_rng(seed)
    r = np.zeros((n, 6), F32)
    r[:, 0] = g.uniform(-4, 4, n)
    r[:, 2] = g.uniform(-4, 4, n)
    r[:, 1] = y
    r[:, 4] = -1.0
    return r


def on_box_faces(rays, boxes):
    """The rays with each origin's y moved exactly onto a top or bottom face of one of `boxes` ([K, 6]: xmin, xmax,
    ymin, ymax, zmin, zmax).  Ray i takes a box whose x-z footprint holds its origin where there is one (so it starts on
    the face itself, not only in its plane), in turn among those, and alternates top / bottom."""
    r = np.array(rays, F32)
    b = np.asarray(boxes, F32)
    inside = (r[:, None, 0] >= b[None, :, 0]) & (r[:, None, 0] <= b[None, :, 1]) & \
             (r[:, None, 2] >= b[None, :, 4]) & (r[:, None, 2] <= b[None, :, 5])
    for i in range(len(r)):
        cand = np.flatnonzero(inside[i])
        k = cand[(i // 2) % len(cand)] if len(cand) else (i // 2) % len(b)
        r[i, 1] = b[k, 3] if i % 2 == 0 else b[k, 2]
    return r


def scaled_rays(rays, scales=(2.0 ** -10, 2.0 ** 10, 1e-3, 1e3)):
    """Unnormalised directions: quarter k of the rays has its direction multiplied by scales[k] in float32."""
    r = np.array(rays, F32)
    q = len(r) // len(scales)
    for k, s in enumerate(scales):
        r[k * q:(k + 1) * q if k + 1 < len(scales) else len(r), 3:] *= F32(s)
    return r


def aimed_rays(rays, boxes):
    """The rays re-aimed (normalised) at points well inside `boxes` in turn: a point within 0.55 of the half extent
    from the centre lies inside the sphere inscribed in a cubic box, so every ray crosses a particle's mesh."""
    r = np.array(rays, np.float64)
    b = np.asarray(boxes, np.float64)[np.arange(len(r)) % len(boxes)]
    g = np.random.default_rng(len(r) + 1)
    u = g.uniform(-0.55, 0.55, (len(r), 3))
    tgt = np.stack([0.5 * (b[:, 2 * a] + b[:, 2 * a + 1]) + 0.5 * u[:, a] * (b[:, 2 * a + 1] - b[:, 2 * a])
                    for a in range(3)], 1)
    d = tgt - r[:, :3]
    r[:, 3:] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return r.astype(F32)


def inside_rays(rays, centres, cloud_box, hits, hit):
    """Origins inside geometry, directions as given: a third at sphere centres (in turn), a third uniform inside
    `cloud_box` (the particle cloud's box), and a third at the hit points of `hits` (records for `rays`, hit[i] set
    where valid) pushed 1e-4 along -normal, i.e. just under the surface the ray reached."""
    r = np.array(rays, F32)
    n = len(r)
    a, b = n // 3, 2 * n // 3
    c = np.asarray(centres, F32)
    r[:a, :3] = c[np.arange(a) % len(c)]
    g = np.random.default_rng(n)
    box = np.asarray(cloud_box, F32)
    for ax in range(3):
        r[a:b, ax] = g.uniform(box[2 * ax], box[2 * ax + 1], b - a)
    src = np.flatnonzero(hit)
    src = src[np.arange(n - b) % len(src)]
    r[b:, :3] = hits["point"][src] - F32(1e-4) * hits["normal"][src]
    return r
