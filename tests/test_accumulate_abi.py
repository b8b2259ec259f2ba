"""rt_accumulate and rt_camera_reprojection at the C-ABI boundary, without a GPU (the manner of
tests/test_denoise_abi.py): the struct layouts against the C compiler's, the exported symbols, the ABI version, every
argument check of rt_accumulate — all of which answer before any device work — and rt_camera_reprojection against
the oracle's camera: every pixel centre of a frame lands on its own coordinates."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import accumulate_ref as R
import camera_rays_ref as cref
from rtamd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "real-time-gpu-ray-tracer_amd")
HEADER = os.path.join(REPO, "include", "rt.h")
INVALID = 1                                    # RT_ERR_INVALID_ARGUMENT


def test_struct_layouts_match_c(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){']
    for cname, mirror in (("rt_accumulate_desc", abi.AccumulateDesc), ("rt_reprojection", abi.Reprojection)):
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in mirror._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    for name in ("RT_ACCUMULATE_NO_SYNC", "RT_DENOISE_NO_SYNC", "RT_QUERY_NO_SYNC", "RT_CAMERA_QUERY_NO_SYNC", "RT_ABI_VERSION"):
        lines.append(f'printf("{name} %u\\n", (unsigned){name});')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lay = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    assert lay["rt_accumulate_desc"] == C.sizeof(abi.AccumulateDesc) == 96
    assert lay["rt_reprojection"] == C.sizeof(abi.Reprojection) == 48
    for cname, mirror in (("rt_accumulate_desc", abi.AccumulateDesc), ("rt_reprojection", abi.Reprojection)):
        for fname, _ in mirror._fields_:
            assert lay[f"{cname}.{fname}"] == getattr(mirror, fname).offset, fname
    # the queries' NO_SYNC bit
    assert (lay["RT_ACCUMULATE_NO_SYNC"] == abi.RT_ACCUMULATE_NO_SYNC == lay["RT_DENOISE_NO_SYNC"] == lay["RT_QUERY_NO_SYNC"]
            == lay["RT_CAMERA_QUERY_NO_SYNC"] == 4)
    assert lay["RT_ABI_VERSION"] == abi.RT_ABI_VERSION == 5


def test_symbols_and_abi_version(rtlib_path):
    lib = abi.load_library(rtlib_path)
    macro = int(re.search(r"#define RT_ABI_VERSION (\d+)u", open(HEADER).read()).group(1))
    assert lib.rt_abi_version() == macro == abi.RT_ABI_VERSION == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", rtlib_path], check=True, capture_output=True, text=True).stdout
    for name in ("rt_accumulate", "rt_camera_reprojection"):
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert re.search(rf"\bT {name}$", nm, re.M), name


N = 8 * 4                                      # pixels of valid_desc's image


def valid_desc(width=8, height=4):
    """A description that passes every argument check: the pointers are never dereferenced on the host (fake, aligned,
    disjoint addresses), prev_view is real host memory, and nothing is enqueued without a device."""
    d = abi.AccumulateDesc()
    d.width, d.height, d.flags = width, height, 0
    d.max_history, d.normal_cos, d.plane_tolerance = 32.0, 0.9, 0.02
    d.color_device, d.hits_device, d.prev_hits_device = 0x10000, 0x20000, 0x30000
    d.prev_history_device, d.history_device, d.rgb32_device = 0x40000, 0x50000, 0x60000
    d.prev_view = C.pointer(abi.Reprojection())
    return d


def edit(**fields):
    def apply(d):
        for k, v in fields.items():
            setattr(d, k, v)
    return apply


BAD = {
    "reserved": edit(reserved=1),
    "reserved1": edit(reserved1=1),
    "unknown_flag": edit(flags=1),
    "unknown_flag_high": edit(flags=abi.RT_ACCUMULATE_NO_SYNC | (1 << 31)),
    "width_16385": edit(width=16385),
    "height_16385": edit(height=16385),
    "max_history_below_1": edit(max_history=0.999),
    "max_history_0": edit(max_history=0.0),
    "max_history_nan": edit(max_history=math.nan),
    "max_history_minus_inf": edit(max_history=-math.inf),
    "normal_cos_above_1": edit(normal_cos=1.0001),
    "normal_cos_nan": edit(normal_cos=math.nan),
    "normal_cos_inf": edit(normal_cos=math.inf),
    "plane_tolerance_0": edit(plane_tolerance=0.0),
    "plane_tolerance_negative": edit(plane_tolerance=-0.02),
    "plane_tolerance_nan": edit(plane_tolerance=math.nan),
    "null_color": edit(color_device=None),
    "null_hits": edit(hits_device=None),
    "null_history": edit(history_device=None),
    "prev_hits_without_history": edit(prev_history_device=None),
    "prev_history_without_hits": edit(prev_hits_device=None),
    "history_misaligned": edit(history_device=0x50008),
    "prev_history_misaligned": edit(prev_history_device=0x40004),
    "color_misaligned": edit(color_device=0x10002),
    "hits_misaligned": edit(hits_device=0x20001),
    "prev_hits_misaligned": edit(prev_hits_device=0x30002),
    "rgb_misaligned": edit(rgb32_device=0x60003),
    "history_is_prev_history": edit(history_device=0x40000),
    "history_overlaps_prev_history_tail": edit(history_device=0x40000 + 16 * N - 16),
    "history_ends_inside_prev_history": edit(history_device=0x40000 - 16 * N + 16),
    "history_overlaps_prev_hits": edit(history_device=0x30000 + 48 * N - 16),
    "history_overlaps_hits": edit(history_device=0x20000),
    "history_overlaps_color": edit(history_device=0x10000),
    "history_overlaps_rgb": edit(rgb32_device=0x50000 + 16),
    "rgb_overlaps_prev_hits": edit(rgb32_device=0x30000 + 48 * N - 4),
    "rgb_overlaps_hits": edit(rgb32_device=0x20000 - 12 * N + 4),
    "rgb_overlaps_prev_history": edit(rgb32_device=0x40000),
    "rgb_overlaps_color_shifted": edit(rgb32_device=0x10000 + 12),
    "no_such_device": None,                     # a valid, non-empty call on a machine without a GPU (as rt_box_test)
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_argument_errors(rtlib_path, name):
    lib = abi.load_library(rtlib_path)
    d = valid_desc()
    device = 0
    if BAD[name] is None:
        device = max(lib.rt_device_count(), 0) + 7          # past the last device, GPU or not
    else:
        BAD[name](d)
    assert lib.rt_tile_pixels(0, 0, 0, 0, 0, 0, 0, 0, None) == INVALID      # leaves another call's message behind
    before = lib.rt_last_error()
    assert lib.rt_accumulate(device, C.byref(d)) == INVALID, name
    msg = lib.rt_last_error()
    assert msg and msg != before, name


def expected_without_launch(lib):
    """What a call that passes the argument checks answers here: without a GPU it fails as rt_box_test does; with one,
    the fake addresses are rejected by the pointer check.  Either way nothing is enqueued."""
    if lib.rt_device_count() > 0:
        return INVALID
    one = np.zeros(6, np.float32)
    hit, te = np.zeros(1, np.uint8), np.zeros(1, np.float32)
    want = lib.rt_box_test(0, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 0, hit.ctypes.data, te.ctypes.data)
    assert want != abi.RT_OK
    return want


ALLOWED = {
    "as_is": edit(),
    "first_frame": edit(prev_hits_device=None, prev_history_device=None),
    "no_view": edit(prev_view=None),
    "no_rgb": edit(rgb32_device=None),
    "in_place": edit(rgb32_device=0x10000),
    "tests_off": edit(normal_cos=-math.inf, plane_tolerance=math.inf, max_history=math.inf),
    "limits": edit(normal_cos=1.0, max_history=1.0, flags=abi.RT_ACCUMULATE_NO_SYNC),
    "buffers_back_to_back": edit(prev_history_device=0x50000 - 16 * N, rgb32_device=0x50000 + 16 * N),
}


@pytest.mark.parametrize("name", sorted(ALLOWED))
def test_valid_calls_pass_the_argument_checks(rtlib_path, name):
    """These reach the device check (and no further: no device, or fake addresses); the message is not an argument's."""
    lib = abi.load_library(rtlib_path)
    d = valid_desc()
    ALLOWED[name](d)
    assert lib.rt_accumulate(0, C.byref(d)) == expected_without_launch(lib), name
    msg = lib.rt_last_error()
    assert msg and (b"device" in msg or b"accessible" in msg), msg


def test_null_desc(rtlib_path):
    lib = abi.load_library(rtlib_path)
    assert lib.rt_accumulate(0, None) == INVALID
    assert lib.rt_last_error()


@pytest.mark.parametrize("size", ((0, 0), (0, 7), (7, 0)))
def test_empty_image_is_ok_and_touches_no_device(rtlib_path, size):
    lib = abi.load_library(rtlib_path)
    d = valid_desc(*size)
    assert lib.rt_accumulate(0, C.byref(d)) == abi.RT_OK
    assert lib.rt_accumulate(12345, C.byref(d)) == abi.RT_OK   # not even the device index is looked at
    d.flags = abi.RT_ACCUMULATE_NO_SYNC
    assert lib.rt_accumulate(0, C.byref(d)) == abi.RT_OK
    d.history_device = d.prev_history_device                   # empty ranges do not overlap
    assert lib.rt_accumulate(0, C.byref(d)) == abi.RT_OK
    d.reserved1 = 1                                            # ... but the argument checks still come first
    assert lib.rt_accumulate(0, C.byref(d)) == INVALID


# ---- rt_camera_reprojection ------------------------------------------------------------------------------------------

def moved_pair():
    return {"this_frame": dict(center=R.CAMERA[0], target=R.CAMERA[1], fov=R.FOV),
            "last_frame": dict(center=R.MOVED[0], target=R.MOVED[1], fov=R.FOV)}


REPROJECTION_CAMERAS = dict(cref.CAMERAS, **moved_pair())


@pytest.mark.parametrize("size", ((cref.W, cref.H), (96, 64)), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(REPROJECTION_CAMERAS))
def test_reprojection_sends_the_oracles_pixel_centres_to_themselves(rtlib_path, oracle_lib, name, size):
    """The oracle's camera (camera_export: pixel_origin, dx, dy, centre) against the rows: the point pixel_origin +
    i dx + j dy, formed in float64, must land on (i, j) within 16 eps32 (W + H) pixels, evaluated in float64."""
    import rtamd
    W, H = size
    scene = cref.rough_only_scene()
    o = oracle_lib.OracleScene(scene, build_seed=0)
    o.camera(W, H, ray_trace_depth=1, **REPROJECTION_CAMERAS[name])
    cam = np.asarray(o.camera_export(), np.float64)
    o.close()
    po, dx, dy, centre = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    abi.load_library(rtlib_path)
    r = rtamd.reprojection(scene.camera_input(ray_trace_depth=1, **REPROJECTION_CAMERAS[name]), W, H)
    rows = {k: np.array(list(getattr(r, k)), np.float64) for k in ("centre", "rx", "ry", "rw")}
    assert np.array_equal(rows["centre"], centre)
    jj, ii = np.mgrid[0:H, 0:W].astype(np.float64)
    x = po + ii[..., None] * dx + jj[..., None] * dy
    fx, fy, r2 = R.project(rows, x)
    err = max(float(np.abs(fx - ii).max()), float(np.abs(fy - jj).max()))
    bar = 16.0 * R.EPS32 * (W + H)
    print(f"{name} {W}x{H}: max(|fx - i|, |fy - j|) = {err:.3g} pixels, bar {bar:.3g}")
    assert (r2 > 0.0).all()
    assert err <= bar
    # the numpy statement of the same rows, from the same floats
    ref = R.rows32(R.reprojection_rows({"po": cam[0:3], "dx": dx, "dy": dy, "centre": centre}))
    for k in ("rx", "ry", "rw"):
        assert np.array_equal(ref[k], rows[k].astype(np.float32)), k


def test_reprojection_rejects_bad_arguments(rtlib_path):
    from rtamd import scenes
    lib = abi.load_library(rtlib_path)
    scene = scenes.demo_scene()
    ci, out = scene.camera_input(), abi.Reprojection()
    assert lib.rt_camera_reprojection(C.byref(ci), 96, 64, C.byref(out)) == abi.RT_OK
    assert lib.rt_camera_reprojection(None, 96, 64, C.byref(out)) == INVALID
    assert lib.rt_camera_reprojection(C.byref(ci), 96, 64, None) == INVALID
    for w, h in ((0, 64), (96, 0), (32769, 64), (96, 32769)):
        assert lib.rt_camera_reprojection(C.byref(ci), w, h, C.byref(out)) == INVALID, (w, h)
    assert lib.rt_camera_reprojection(C.byref(ci), 32768, 32768, C.byref(out)) == abi.RT_OK
    sample0 = scene.camera_input(sample_count=0)             # rt_camera_set's business, not the rows'
    assert lib.rt_camera_reprojection(C.byref(sample0), 96, 64, C.byref(out)) == abi.RT_OK


def test_degenerate_cameras_are_rejected(rtlib_path):
    from rtamd import scenes
    lib = abi.load_library(rtlib_path)
    scene = scenes.demo_scene()
    c = scene.camera["center"]
    keep = abi.Reprojection()
    keep.rx[0] = 123.0
    for over in (dict(target=c), dict(up=(0.0, 0.0, -1.0)), dict(fov=0.0), dict(center=(math.nan, 0.0, 0.0)),
                 dict(center=(math.inf, 0.0, 0.0))):
        ci = scene.camera_input(**over)                      # centre == target; up along the view; no field of view
        assert lib.rt_tile_pixels(0, 0, 0, 0, 0, 0, 0, 0, None) == INVALID
        before = lib.rt_last_error()
        assert lib.rt_camera_reprojection(C.byref(ci), 96, 64, C.byref(keep)) == INVALID, over
        assert lib.rt_last_error() != before
        assert keep.rx[0] == 123.0                           # the output is left alone


def test_import_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "import rtamd, rtamd.renderer\n"
            "assert hasattr(rtamd.Renderer, 'accumulate') and callable(rtamd.reprojection)\n"
            "assert len(rtamd.renderer.ACCUMULATE_DEFAULTS) == 3\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    subprocess.run([sys.executable, "-c", code], check=True, env=env)
