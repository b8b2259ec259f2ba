"""The camera's rays in numpy float32, for tests/test_camera_rays_ref.py (which pins this file against the oracle's
frames) and tests/test_gpu_camera_query.py (which judges rt_query_camera with it).

Built from oracle.OracleScene.camera_export() — pixel_origin, dx, dy, centre, cu, cv (3 floats each), recip_sqrt,
sqrt_s — in the operation order of render_pixel (oracle/rt_oracle.c:961-979): every float32 operation on its own (numpy
does not contract), vunit as x * (1 / sqrtf(len2)) with len2 summed x, y, z from 0, random_plane_vector's rejection
loop on -1 + 2 u.  The RNG is the oracle's exported one (oracle_rng_init / oracle_rng_uniform): the pixel's stream is
keyed by pixel = pitch * y + x with pitch = ceil(frame_width / 16) * 16.

Rays are returned row-major over the rectangle rect = (x0, y0, w, h): pixel (x0 + i, y0 + j) is row j * w + i of a
float32 [w * h, 6] array (origin xyz, direction xyz).
"""
import ctypes as C

import numpy as np

F32 = np.float32
DEFAULT_SEED = 0x5EED          # rt_render_opts.frame_seed == 0


def _cam(cam_export):
    c = np.asarray(cam_export, F32)
    return {"po": c[0:3], "dx": c[3:6], "dy": c[6:9], "centre": c[9:12], "cu": c[12:15], "cv": c[15:18],
            "recip_sqrt": F32(c[18]), "sqrt_s": int(c[19])}


def _pixels(rect):
    x0, y0, w, h = rect
    j, i = np.divmod(np.arange(w * h, dtype=np.int64), w)
    return (x0 + i).astype(np.uint32), (y0 + j).astype(np.uint32)


def rays_from_offsets(cam_export, rect, ox, oy, disk):
    """Rays of the rectangle's pixels with sample offsets ox, oy (float32 [w h], added to (float)x / (float)y) and
    focus-disk vectors disk (float32 [w h, 2], or None: the origin is the camera's centre, not centre + 0)."""
    c = _cam(cam_export)
    px, py = _pixels(rect)
    n = len(px)
    fx = px.astype(F32) + np.asarray(ox, F32)
    fy = py.astype(F32) + np.asarray(oy, F32)
    sp = (c["po"][None, :] + c["dx"][None, :] * fx[:, None]) + c["dy"][None, :] * fy[:, None]
    o = np.broadcast_to(c["centre"], (n, 3)).astype(F32)
    if disk is not None:
        d = np.asarray(disk, F32)
        o = (o + c["cu"][None, :] * d[:, 0:1]) + c["cv"][None, :] * d[:, 1:2]
    v = sp - o
    l2 = np.zeros(n, F32)
    for a in range(3):
        l2 = l2 + v[:, a] * v[:, a]
    f = F32(1.0) / np.sqrt(l2)
    out = np.concatenate([o, v * f[:, None]], 1)
    assert out.dtype == F32
    return out


def centre_rays(cam_export, rect):
    """The ray through each pixel's centre: no jitter, no focus disk, no RNG."""
    n = rect[2] * rect[3]
    return rays_from_offsets(cam_export, rect, np.zeros(n, F32), np.zeros(n, F32), None)


def first_sample_draws(cam_export, frame_width, rect, frame_seed, focus_radius):
    """(ox, oy, disk) of sample 0 of every pixel of the rectangle: the offsets inside sample cell (0, 0) and, with a
    focus disk, the accepted disk vector — the draws of render_pixel's first iteration, in its order."""
    from oracle.oracle import lib
    L = lib()
    c = _cam(cam_export)
    seed = int(frame_seed) or DEFAULT_SEED
    pitch = (int(frame_width) + 15) // 16 * 16
    px, py = _pixels(rect)
    n = len(px)
    u = np.zeros((n, 2), F32)
    disk = np.zeros((n, 2), F32) if focus_radius > 0.0 else None
    r2 = F32(focus_radius) * F32(focus_radius)
    for k in range(n):
        pixel = pitch * int(py[k]) + int(px[k])
        st = C.c_uint64(L.oracle_rng_init((pixel ^ seed) & 0xFFFFFFFFFFFFFFFF, pixel, 0))
        u[k, 0] = L.oracle_rng_uniform(C.byref(st))
        u[k, 1] = L.oracle_rng_uniform(C.byref(st))
        if disk is not None:
            while True:                           # random_plane_vector (rt_oracle.c:121-128)
                x = F32(-1.0) + F32(2.0) * F32(L.oracle_rng_uniform(C.byref(st)))
                y = F32(-1.0) + F32(2.0) * F32(L.oracle_rng_uniform(C.byref(st)))
                if not (x * x + y * y > r2):
                    break
            disk[k] = (x, y)
    ox = ((F32(0.0) + u[:, 0]) * c["recip_sqrt"]) - F32(0.5)
    oy = ((F32(0.0) + u[:, 1]) * c["recip_sqrt"]) - F32(0.5)
    return ox.astype(F32), oy.astype(F32), disk


def first_sample_rays(cam_export, frame_width, rect, frame_seed, focus_radius):
    """The ray render_pixel starts each pixel's first path with for frame_seed (0 means 0x5EED)."""
    ox, oy, disk = first_sample_draws(cam_export, frame_width, rect, frame_seed, focus_radius)
    return rays_from_offsets(cam_export, rect, ox, oy, disk)


# ---- the scene and cameras both test files use ------------------------------------------------------------------------
W, H = 100, 60                 # pitch 112, not the width; 13 x 8 units of 8 x 8 with partial right and top edges
CAMERAS = {                    # camera overrides: (focus_disk_radius, sample_count)
    "pinhole": dict(focus_disk_radius=0.0, sample_count=1),
    "disk": dict(focus_disk_radius=0.8, sample_count=1),
    "disk_4spp": dict(focus_disk_radius=0.8, sample_count=4),
}


def rough_only_scene(particles=6):
    """The demo scene with particles, its metal references pointed at the four roughs in turn."""
    from rtamd import abi, scenes
    s = scenes.demo_with_particles(particles)
    metal = s.triangles["material_type"] == abi.METAL
    s.triangles["material_index"][metal] = (np.arange(int(metal.sum())) // 7 % len(s.roughs)).astype(np.uint32)
    s.triangles["material_type"][metal] = abi.ROUGH
    return s


def albedo_of(scene, hits, background):
    """float32 [N, 3]: the material table's albedo for each record's (mtype, midx); the background on a miss."""
    from rtamd import abi
    rough = np.asarray([a for a in scene.roughs], F32).reshape(-1, 3)
    metal = np.asarray([a for a, _ in scene.metals], F32).reshape(-1, 3)
    out = np.broadcast_to(np.asarray(background, F32), (len(hits), 3)).copy()
    hit = hits["instance"] != abi.MISS
    is_m = hit & (hits["mtype"] == abi.METAL)
    is_r = hit & (hits["mtype"] == abi.ROUGH)
    out[is_r] = rough[hits["midx"][is_r]]
    if is_m.any():
        out[is_m] = metal[hits["midx"][is_m]]
    return out
