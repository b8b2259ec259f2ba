"""tests/camera_rays_ref.py against the oracle's frames, before it judges rt_query_camera (no GPU).

At depth 1 a path is one segment: ray_color returns 1 * albedo of the hit's material for a rough surface (Rough never
absorbs) and 1 * background on a miss, and with 1 spp the pixel is that value (0 + v, times recip_sqrt^2 = 1).  So on a
scene with rough materials only, oracle.render's rgb equals — bit for bit, on every pixel — the albedo of
oracle.trace(first_sample_rays(...))'s hit material: that holds exactly when first_sample_rays restates the ray
render_pixel traces, RNG draws included.
"""
import ctypes as C

import numpy as np
import pytest

import camera_rays_ref as ref
from rtamd import abi

F32 = np.float32
BUILD_SEED = 9
WHOLE = (0, 0, ref.W, ref.H)


@pytest.fixture(scope="module")
def scene_oracle(oracle_lib):
    from oracle.oracle import OracleScene
    s = ref.rough_only_scene()
    assert not (s.triangles["material_type"] == abi.METAL).any()
    return s, OracleScene(s, build_seed=BUILD_SEED)


def camera(o, name, **over):
    o.camera(ref.W, ref.H, ray_trace_depth=1, **dict(ref.CAMERAS[name], **over))
    return o.camera_export()


@pytest.mark.parametrize("seed", [0x5EED, 0xC0FFEE12345])
@pytest.mark.parametrize("name", ["pinhole", "disk"])
def test_frame_is_the_albedo_of_the_first_sample_rays(scene_oracle, name, seed):
    s, o = scene_oracle
    cam = camera(o, name)
    assert int(cam[19]) == 1
    rgb, _, _ = o.render(frame_seed=seed, threads=8, want_rgba=False)
    rays = ref.first_sample_rays(cam, ref.W, WHOLE, seed, ref.CAMERAS[name]["focus_disk_radius"])
    hits, _ = o.trace(rays)
    want = ref.albedo_of(s, hits, s.camera["background"]).reshape(ref.H, ref.W, 3)
    hit = (hits["instance"] != abi.MISS)
    assert 0.2 < hit.mean() < 0.98 and len(np.unique(hits["midx"][hit])) >= 4      # every rough and the sky in view
    assert np.array_equal(rgb.view(np.uint32), want.view(np.uint32)), int((rgb != want).any(axis=2).sum())


def test_seed_zero_is_the_default_seed(scene_oracle):
    _, o = scene_oracle
    cam = camera(o, "disk")
    a = ref.first_sample_rays(cam, ref.W, (90, 50, 10, 10), 0, 0.8)
    b = ref.first_sample_rays(cam, ref.W, (90, 50, 10, 10), ref.DEFAULT_SEED, 0.8)
    c = ref.first_sample_rays(cam, ref.W, (90, 50, 10, 10), 77, 0.8)
    assert np.array_equal(a, b) and (a != c).any()


def test_first_sample_of_four_against_a_per_pixel_restatement(scene_oracle):
    """sample_count 4 (a 2 x 2 grid, recip_sqrt 0.5): the frame is no longer one ray per pixel, so the vectorised rays
    are held against render_pixel's first iteration written out pixel by pixel with numpy scalars."""
    from oracle.oracle import lib
    L = lib()
    _, o = scene_oracle
    cam = camera(o, "disk_4spp")
    assert int(cam[19]) == 2 and F32(cam[18]) == F32(0.5)
    seed = 0xC0FFEE12345
    rect = (3, 5, 70, 9)
    got = ref.first_sample_rays(cam, ref.W, rect, seed, 0.8)
    po, dx, dy, centre, cu, cv = (cam[3 * k:3 * k + 3].astype(F32) for k in range(6))
    recip, radius = F32(cam[18]), F32(0.8)
    pitch = (ref.W + 15) // 16 * 16
    assert pitch == 112
    k = 0
    for y in range(rect[1], rect[1] + rect[3]):
        for x in range(rect[0], rect[0] + rect[2]):
            pixel = pitch * y + x
            st = C.c_uint64(L.oracle_rng_init(pixel ^ seed, pixel, 0))
            rnd = lambda: F32(L.oracle_rng_uniform(C.byref(st)))
            ox = ((F32(0) + rnd()) * recip) - F32(0.5)
            oy = ((F32(0) + rnd()) * recip) - F32(0.5)
            sp = [(po[a] + dx[a] * (F32(x) + ox)) + dy[a] * (F32(y) + oy) for a in range(3)]
            while True:
                vx = F32(-1) + (F32(1) - F32(-1)) * rnd()
                vy = F32(-1) + (F32(1) - F32(-1)) * rnd()
                if not (vx * vx + vy * vy > radius * radius):
                    break
            org = [(centre[a] + cu[a] * vx) + cv[a] * vy for a in range(3)]
            v = [sp[a] - org[a] for a in range(3)]
            l2 = F32(0)
            for a in range(3):
                l2 = l2 + v[a] * v[a]
            f = F32(1) / np.sqrt(l2)
            want = np.asarray(org + [v[a] * f for a in range(3)], F32)
            assert want.dtype == F32 and np.array_equal(got[k].view(np.uint32), want.view(np.uint32)), (x, y)
            k += 1
    assert k == len(got)


@pytest.mark.parametrize("name", list(ref.CAMERAS))
def test_centre_rays(scene_oracle, name):
    """Independent of seed, sample count and focus disk by construction (no such argument); equal to the first-sample
    formula with jitter and disk forced to zero; origin the camera's centre; unit directions through the frame."""
    _, o = scene_oracle
    cam = camera(o, name)
    rect = (3, 5, 70, 9)
    n = rect[2] * rect[3]
    c = ref.centre_rays(cam, rect)
    assert c.shape == (n, 6) and c.dtype == F32
    assert np.array_equal(c, ref.centre_rays(camera(o, "pinhole"), rect))
    zero = ref.rays_from_offsets(cam, rect, np.zeros(n, F32), np.zeros(n, F32), np.zeros((n, 2), F32))
    assert np.array_equal(c[:, 3:], zero[:, 3:]) and np.array_equal(c[:, :3], zero[:, :3])
    assert np.all(c[:, :3] == cam[9:12])
    assert np.allclose(np.linalg.norm(c[:, 3:].astype(np.float64), axis=1), 1.0, atol=1e-6)
    # a rectangle is a cut of the whole frame
    whole = ref.centre_rays(cam, WHOLE).reshape(ref.H, ref.W, 6)
    assert np.array_equal(c.reshape(rect[3], rect[2], 6), whole[5:14, 3:73])
    # the jittered rays differ from them, by less than a pixel's extent
    j = ref.first_sample_rays(cam, ref.W, rect, 1, ref.CAMERAS[name]["focus_disk_radius"])
    assert (j[:, 3:] != c[:, 3:]).any()
