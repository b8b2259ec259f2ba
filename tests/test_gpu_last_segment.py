"""A path's last segment on a rough surface shades from the hit's material word alone (csrc/shade.hpp hit_material,
render_persistent_body's T.found arm): no surface is reconstructed there, and the scatter draws are consumed exactly
while the pixel has samples left.

Every comparison is exact.  EXACT is bit-identical to the oracle on the reference's trees, and so is the default FAST
kernel (tests/test_gpu_parity.py); the grid kernel ("kernel" 0) does not take the shortcut, so persistent against grid is
the cross-check on the other trees.

* camera settings that put the last segment at every place of a pixel's RNG stream: depth 1 (every hit is a last
  segment), 2, 3 at one sample; depth 1, 2 at four samples (a last segment that is not the last sample must consume
  its draws, or every later sample shifts); four samples through a defocus disk;
* metal last hits (fuzz 0.3): they keep the full path, fuzz draws and absorption included;
* a hit triangle's material from its cold record (mode "sah") and from the caller's triangle (mode "lbvh" with
  "rebuild" set before the build: no cold records), on a placement of the same scene in which no two surfaces touch.
"""
import functools

import numpy as np
import pytest

from rtamd import Renderer, abi, scenes

pytestmark = pytest.mark.gpu

THREADS = 16
W, H = 96, 64
SEED = 7
CAMERAS = {
    "d1": dict(ray_trace_depth=1),
    "d2": dict(ray_trace_depth=2),
    "d3": dict(ray_trace_depth=3),
    "d1s4": dict(ray_trace_depth=1, sample_count=4),
    "d2s4": dict(ray_trace_depth=2, sample_count=4),
    "defocus_s4": dict(focus_disk_radius=0.3, ray_trace_depth=3, sample_count=4),
}
METAL_CAMERAS = {"d1": dict(ray_trace_depth=1), "d2": dict(ray_trace_depth=2)}


def scene(metal_fuzz=False):
    s = scenes.demo_with_particles(6)
    if metal_fuzz:
        s.metals = [((0.8, 0.85, 0.88), 0.3)]             # test_metal_fuzz's material
    return s


def apart_scene():
    """The scene with its five demo instances placed by hand, none touching another (the animation rests the
    parallelogram's edge on the ground sphere: two hits inside the reference's 1e-6 window, which the quad kernel on
    greedily collapsed host SAH trees and the grid kernel's binary pairs may take in different orders), and every
    other particle rough, so that last segments end on triangles of both material types."""
    s = scene()
    s.animated = False
    for d, shift in zip(s.instances, ((0.0, -1000.0, 0.0), (3.0, 2.5, 0.0), (-5.0, 0.5, 0.0), (-3.0, 2.0, 1.5), (-3.0, 7.0, 0.0))):
        d["shift"] = shift
    s.instances[3]["scale"] = (3.0, 3.0, 3.0)
    for p in range(0, 6, 2):
        s.triangles["material_type"][p * 1024:(p + 1) * 1024] = abi.ROUGH
        s.triangles["material_index"][p * 1024:(p + 1) * 1024] = p % 4
    return s


@functools.lru_cache(maxsize=None)
def oracle_frame(metal_fuzz, cam):
    """The oracle's (float RGB, RGBA8, counters) for one camera setting, computed once."""
    from oracle.oracle import OracleScene
    o = OracleScene(scene(metal_fuzz), build_seed=SEED)
    o.camera(W, H, **(METAL_CAMERAS if metal_fuzz else CAMERAS)[cam])
    rgb, rgba, cnt = o.render(threads=THREADS)
    rgb.setflags(write=False)
    rgba.setflags(write=False)
    return rgb, rgba, cnt


def check_against_oracle(metal_fuzz, cam, settings):
    orgb, orgba, ocnt = oracle_frame(metal_fuzz, cam)
    r = Renderer(scene(metal_fuzz)).build_acceleration_structure(SEED).configure_camera(W, H, **settings)
    frames = {}
    for kernel in (1, 0):
        r.set_option("kernel", kernel)
        for exact in (True, False):
            rgba, rgb, st = r.render(0, exact=exact, want_rgb=True, count_work=True)
            frames[kernel, exact] = (rgba, rgb, st)
    r.cleanup()
    for (kernel, exact), (rgba, rgb, st) in frames.items():
        what = (cam, "persistent" if kernel else "grid", "exact" if exact else "fast")
        print(what, "pixels differing from the oracle:", int((rgb != orgb).any(axis=2).sum()), "rays", st["rays"], ocnt["rays"])
        assert np.array_equal(rgb, orgb), (what, int((rgb != orgb).any(axis=2).sum()), float(np.abs(rgb - orgb).max()))
        assert np.array_equal(rgba, orgba), what
        assert st["rays"] == ocnt["rays"], (what, st["rays"], ocnt["rays"])
    for exact in (True, False):                               # persistent against grid, byte for byte
        assert np.array_equal(frames[1, exact][0], frames[0, exact][0]), (cam, exact)
        assert np.array_equal(frames[1, exact][1], frames[0, exact][1]), (cam, exact)
    hits = frames[1, True][2]["hits"]
    assert hits > 0.3 * W * H, hits                           # the frame does hit the scene
    return frames


@pytest.mark.parametrize("cam", list(CAMERAS))
def test_last_segment_equals_oracle(gpu_lib, oracle_lib, cam):
    """96 x 64, the demo scene plus 6 particles on the reference's trees: persistent and grid kernels, EXACT and FAST,
    float RGB, RGBA8 and the ray count equal the oracle's; persistent and grid frames equal each other."""
    check_against_oracle(False, cam, CAMERAS[cam])


@pytest.mark.parametrize("cam", list(METAL_CAMERAS))
def test_metal_last_hits_take_the_full_path(gpu_lib, oracle_lib, cam):
    """The same with a fuzzy metal (0.3): a last hit on metal draws its fuzz vector and may be absorbed, which only the
    normal decides — bit-identical to the oracle and to the grid kernel.  The frame does hit metal: with the metal's
    albedo changed the frame changes."""
    frames = check_against_oracle(True, cam, METAL_CAMERAS[cam])
    s = scene(True)
    s.metals = [((0.2, 0.3, 0.9), 0.3)]
    r = Renderer(s).build_acceleration_structure(SEED).configure_camera(W, H, **METAL_CAMERAS[cam])
    rgba, _, _ = r.render(0)
    r.cleanup()
    assert not np.array_equal(rgba, frames[1, False][0])


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("mode", ["sah", "lbvh"])
def test_triangle_material_sources(gpu_lib, mode, depth):
    """A hit triangle's material from its TriCold record (host SAH trees) and from the caller's triangle through
    TriHot::pad0 (GPU-built trees with "rebuild" set before the build: no cold records), rough and metal.  Two frames:
    persistent and grid frames byte-identical, in EXACT (the same binary trees) and in FAST (quads against binary
    pairs: the same hits wherever no two lie inside the reference's 1e-6 window, and apart_scene() has no such pair)."""
    r = Renderer(apart_scene())
    if mode == "lbvh":
        r.set_option("rebuild", 1)
    r.build_acceleration_structure(0, mode=mode).configure_camera(W, H, ray_trace_depth=depth)
    for frame in (0, 37):
        out = {}
        for kernel in (1, 0):
            r.set_option("kernel", kernel)
            for exact in (True, False):
                rgba, rgb, st = r.render(frame, exact=exact, want_rgb=True, count_work=True)
                out[kernel, exact] = (rgba, rgb, st)
        for exact in (True, False):
            p, g = out[1, exact], out[0, exact]
            what = (mode, depth, frame, "exact" if exact else "fast")
            print(what, "pixels differing:", int((p[1] != g[1]).any(axis=2).sum()), "triangle hits frame:", p[2]["hits"])
            assert np.array_equal(p[1], g[1]) and np.array_equal(p[0], g[0]), what
            assert p[2]["rays"] == g[2]["rays"], what
            assert p[2]["hits"] > 0.3 * W * H, what
    r.cleanup()
