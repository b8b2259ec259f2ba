"""rt_accumulate_moments and rt_denoise_guided at the C-ABI boundary, without a GPU (the manner of
tests/test_accumulate_abi.py): the struct layouts against the C compiler's, the exported symbols, the ABI version, and
every argument check of the two calls — all of which answer before any device work."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from rtamd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "real-time-gpu-ray-tracer_amd")
HEADER = os.path.join(REPO, "include", "rt.h")
INVALID = 1                                    # RT_ERR_INVALID_ARGUMENT
STRUCTS = (("rt_moments_desc", abi.MomentsDesc), ("rt_denoise_guided_desc", abi.DenoiseGuidedDesc),
           ("rt_accumulate_desc", abi.AccumulateDesc))


def test_struct_layouts_match_c(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){']
    for cname, mirror in STRUCTS:
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in mirror._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("RT_ABI_VERSION %u\\n", (unsigned)RT_ABI_VERSION);')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lay = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    assert lay["rt_moments_desc"] == C.sizeof(abi.MomentsDesc) == 32
    assert lay["rt_denoise_guided_desc"] == C.sizeof(abi.DenoiseGuidedDesc) == 112
    assert lay["rt_accumulate_desc"] == C.sizeof(abi.AccumulateDesc) == 96          # unchanged
    for cname, mirror in STRUCTS:
        for fname, _ in mirror._fields_:
            assert lay[f"{cname}.{fname}"] == getattr(mirror, fname).offset, (cname, fname)
    assert lay["RT_ABI_VERSION"] == abi.RT_ABI_VERSION == 5


def test_symbols_and_abi_version(rtlib_path):
    lib = abi.load_library(rtlib_path)
    header = open(HEADER).read()
    macro = int(re.search(r"#define RT_ABI_VERSION (\d+)u", header).group(1))
    assert lib.rt_abi_version() == macro == abi.RT_ABI_VERSION == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", rtlib_path], check=True, capture_output=True, text=True).stdout
    for name in ("rt_accumulate_moments", "rt_denoise_guided", "rt_denoise_guided_scratch_bytes"):
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert re.search(rf"\bT {name}$", nm, re.M), name
        assert re.search(rf"\b{name}\(", header), name
    assert lib.rt_denoise_guided_scratch_bytes(1920, 1080) == 64 * 1920 * 1080 == lib.rt_denoise_scratch_bytes(1920, 1080)
    assert lib.rt_denoise_guided_scratch_bytes(16384, 16384) == 64 * 16384 * 16384


def edit(**fields):
    def apply(d, m):
        for k, v in fields.items():
            setattr(m if k in ("albedo_device", "prev_moments_device", "moments_device", "m_reserved") else d,
                    "reserved" if k == "m_reserved" else k, v)
    return apply


def box_test_status(lib):
    """What a call that passes the argument checks answers here: without a GPU it fails as rt_box_test does; with one,
    the fake addresses are rejected by the pointer check.  Either way nothing is enqueued."""
    if lib.rt_device_count() > 0:
        return INVALID
    one = np.zeros(6, np.float32)
    hit, te = np.zeros(1, np.uint8), np.zeros(1, np.float32)
    want = lib.rt_box_test(0, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 0, hit.ctypes.data, te.ctypes.data)
    assert want != abi.RT_OK
    return want


# ---- rt_accumulate_moments -------------------------------------------------------------------------------------------

N = 8 * 4                                      # pixels of the valid descriptions' image


def valid_moments(width=8, height=4):
    """Descriptions that pass every argument check: fake, aligned, disjoint addresses, never dereferenced on the host."""
    d = abi.AccumulateDesc()
    d.width, d.height, d.flags = width, height, 0
    d.max_history, d.normal_cos, d.plane_tolerance = 32.0, 0.9, 0.02
    d.color_device, d.hits_device, d.prev_hits_device = 0x10000, 0x20000, 0x30000
    d.prev_history_device, d.history_device, d.rgb32_device = 0x40000, 0x50000, 0x60000
    d.prev_view = C.pointer(abi.Reprojection())
    m = abi.MomentsDesc()
    m.albedo_device, m.prev_moments_device, m.moments_device = 0x70000, 0x80000, 0x90000
    return d, m


BAD_MOMENTS = {
    # rt_accumulate's own checks still hold
    "reserved": edit(reserved=1),
    "unknown_flag": edit(flags=1),
    "width_16385": edit(width=16385),
    "max_history_nan": edit(max_history=math.nan),
    "normal_cos_above_1": edit(normal_cos=1.0001),
    "plane_tolerance_0": edit(plane_tolerance=0.0),
    "null_color": edit(color_device=None),
    "null_history": edit(history_device=None),
    "prev_hits_without_history": edit(prev_history_device=None, prev_moments_device=None),
    "history_misaligned": edit(history_device=0x50008),
    "history_is_prev_history": edit(history_device=0x40000),
    "rgb_overlaps_hits": edit(rgb32_device=0x20000 - 12 * N + 4),
    # the moments'
    "moments_reserved": edit(m_reserved=1),
    "moments_reserved_high": edit(m_reserved=1 << 63),
    "null_moments_device": edit(moments_device=None),
    "prev_moments_without_prev_history": edit(prev_hits_device=None, prev_history_device=None),
    "prev_history_without_prev_moments": edit(prev_moments_device=None),
    "moments_misaligned": edit(moments_device=0x90004),
    "prev_moments_misaligned": edit(prev_moments_device=0x80004),
    "albedo_misaligned": edit(albedo_device=0x70002),
    "moments_is_prev_moments": edit(moments_device=0x80000),
    "moments_overlaps_prev_moments_tail": edit(moments_device=0x80000 + 8 * N - 8),
    "moments_ends_inside_prev_moments": edit(moments_device=0x80000 - 8 * N + 8),
    "moments_overlaps_albedo": edit(moments_device=0x70000 + 12 * N - 8),
    "moments_overlaps_color": edit(moments_device=0x10000),
    "moments_overlaps_hits": edit(moments_device=0x20000 + 48 * N - 8),
    "moments_overlaps_prev_hits": edit(moments_device=0x30000),
    "moments_overlaps_prev_history": edit(moments_device=0x40000 + 16),
    "moments_overlaps_history": edit(moments_device=0x50000 + 16 * N - 8),
    "moments_overlaps_rgb": edit(moments_device=0x60000 - 8 * N + 8),
    "history_overlaps_albedo": edit(history_device=0x70000),
    "history_overlaps_prev_moments": edit(history_device=0x80000),
    "rgb_overlaps_albedo": edit(rgb32_device=0x70000 + 4),
    "rgb_overlaps_prev_moments": edit(rgb32_device=0x80000 - 12 * N + 4),
    "no_such_device": None,
}


@pytest.mark.parametrize("name", sorted(BAD_MOMENTS))
def test_accumulate_moments_argument_errors(rtlib_path, name):
    lib = abi.load_library(rtlib_path)
    d, m = valid_moments()
    device = 0
    if BAD_MOMENTS[name] is None:
        device = max(lib.rt_device_count(), 0) + 7
    else:
        BAD_MOMENTS[name](d, m)
    assert lib.rt_tile_pixels(0, 0, 0, 0, 0, 0, 0, 0, None) == INVALID      # leaves another call's message behind
    before = lib.rt_last_error()
    assert lib.rt_accumulate_moments(device, C.byref(d), C.byref(m)) == INVALID, name
    msg = lib.rt_last_error()
    assert msg and msg != before, name


ALLOWED_MOMENTS = {
    "as_is": edit(),
    "first_frame": edit(prev_hits_device=None, prev_history_device=None, prev_moments_device=None),
    "no_albedo": edit(albedo_device=None),
    "no_view": edit(prev_view=None),
    "no_rgb": edit(rgb32_device=None),
    "in_place": edit(rgb32_device=0x10000),
    "no_sync": edit(flags=abi.RT_ACCUMULATE_NO_SYNC),
    "buffers_back_to_back": edit(prev_moments_device=0x90000 - 8 * N, albedo_device=0x90000 + 8 * N),
}


@pytest.mark.parametrize("name", sorted(ALLOWED_MOMENTS))
def test_accumulate_moments_valid_calls_pass_the_argument_checks(rtlib_path, name):
    lib = abi.load_library(rtlib_path)
    d, m = valid_moments()
    ALLOWED_MOMENTS[name](d, m)
    assert lib.rt_accumulate_moments(0, C.byref(d), C.byref(m)) == box_test_status(lib), name
    msg = lib.rt_last_error()
    assert msg and (b"device" in msg or b"accessible" in msg), msg


def test_accumulate_moments_null_arguments(rtlib_path):
    lib = abi.load_library(rtlib_path)
    d, m = valid_moments()
    assert lib.rt_accumulate_moments(0, None, C.byref(m)) == INVALID
    assert lib.rt_accumulate_moments(0, C.byref(d), None) == INVALID
    assert lib.rt_last_error()
    d, m = valid_moments(0, 7)
    assert lib.rt_accumulate_moments(0, C.byref(d), None) == INVALID         # even for an empty image


@pytest.mark.parametrize("size", ((0, 0), (0, 7), (7, 0)))
def test_accumulate_moments_empty_image_is_ok_and_touches_no_device(rtlib_path, size):
    lib = abi.load_library(rtlib_path)
    d, m = valid_moments(*size)
    assert lib.rt_accumulate_moments(0, C.byref(d), C.byref(m)) == abi.RT_OK
    assert lib.rt_accumulate_moments(12345, C.byref(d), C.byref(m)) == abi.RT_OK   # not even the device index is looked at
    m.moments_device = m.prev_moments_device                    # empty ranges do not overlap
    assert lib.rt_accumulate_moments(0, C.byref(d), C.byref(m)) == abi.RT_OK
    m.reserved = 1                                              # ... but the argument checks still come first
    assert lib.rt_accumulate_moments(0, C.byref(d), C.byref(m)) == INVALID


# ---- rt_denoise_guided -----------------------------------------------------------------------------------------------

def valid_guided(width=8, height=4):
    d = abi.DenoiseGuidedDesc()
    d.width, d.height, d.iterations, d.flags = width, height, 5, 0
    d.sigma_luminance, d.sigma_normal, d.sigma_plane = 4.0, 0.1, 0.1
    d.history_device, d.moments_device, d.hits_device, d.albedo_device = 0x10000, 0x20000, 0x30000, 0x40000
    d.rgb32_device, d.rgba8_device, d.variance_device, d.scratch_device = 0x50000, 0x60000, 0x70000, 0x80000
    d.scratch_bytes = 64 * width * height
    return d


def gedit(**fields):
    def apply(d):
        for k, v in fields.items():
            setattr(d, k, v)
    return apply


BAD_GUIDED = {
    "reserved": gedit(reserved=1),
    "unknown_flag": gedit(flags=1),
    "unknown_flag_high": gedit(flags=abi.RT_DENOISE_NO_SYNC | (1 << 31)),
    "iterations_0": gedit(iterations=0),
    "iterations_6": gedit(iterations=6),
    "sigma_luminance_0": gedit(sigma_luminance=0.0),
    "sigma_luminance_negative": gedit(sigma_luminance=-1.0),
    "sigma_luminance_nan": gedit(sigma_luminance=math.nan),
    "sigma_normal_0": gedit(sigma_normal=0.0),
    "sigma_normal_nan": gedit(sigma_normal=math.nan),
    "sigma_plane_0": gedit(sigma_plane=0.0),
    "sigma_plane_nan": gedit(sigma_plane=math.nan),
    "width_16385": gedit(width=16385, scratch_bytes=1 << 40),
    "height_16385": gedit(height=16385, scratch_bytes=1 << 40),
    "no_output": gedit(rgb32_device=None, rgba8_device=None),
    "null_history": gedit(history_device=None),
    "null_moments": gedit(moments_device=None),
    "null_hits": gedit(hits_device=None),
    "null_scratch": gedit(scratch_device=None),
    "scratch_too_small": gedit(scratch_bytes=64 * N - 1),
    "scratch_misaligned": gedit(scratch_device=0x80008),
    "history_misaligned": gedit(history_device=0x10008),
    "moments_misaligned": gedit(moments_device=0x20004),
    "hits_misaligned": gedit(hits_device=0x30002),
    "albedo_misaligned": gedit(albedo_device=0x40001),
    "rgb_misaligned": gedit(rgb32_device=0x50002),
    "rgba_misaligned": gedit(rgba8_device=0x60002),
    "variance_misaligned": gedit(variance_device=0x70002),
    "rgb_is_history": gedit(rgb32_device=0x10000),
    "rgb_overlaps_history_tail": gedit(rgb32_device=0x10000 + 16 * N - 4),
    "rgb_overlaps_moments": gedit(rgb32_device=0x20000 - 12 * N + 4),
    "rgb_overlaps_hits": gedit(rgb32_device=0x30000 + 48 * N - 4),
    "rgb_overlaps_albedo": gedit(rgb32_device=0x40000),
    "rgba_overlaps_history": gedit(rgba8_device=0x10000),
    "rgba_overlaps_rgb": gedit(rgba8_device=0x50000 + 12 * N - 4),
    "variance_overlaps_moments": gedit(variance_device=0x20000 + 8 * N - 4),
    "variance_overlaps_rgba": gedit(variance_device=0x60000),
    "scratch_overlaps_history": gedit(scratch_device=0x10000 - 64 * N + 16),
    "scratch_overlaps_rgb": gedit(scratch_device=0x50000),
    "scratch_overlaps_variance": gedit(variance_device=0x80000 + 64 * N - 4),
    "no_such_device": None,
}


@pytest.mark.parametrize("name", sorted(BAD_GUIDED))
def test_denoise_guided_argument_errors(rtlib_path, name):
    lib = abi.load_library(rtlib_path)
    d = valid_guided()
    device = 0
    if BAD_GUIDED[name] is None:
        device = max(lib.rt_device_count(), 0) + 7
    else:
        BAD_GUIDED[name](d)
    assert lib.rt_tile_pixels(0, 0, 0, 0, 0, 0, 0, 0, None) == INVALID
    before = lib.rt_last_error()
    assert lib.rt_denoise_guided(device, C.byref(d)) == INVALID, name
    msg = lib.rt_last_error()
    assert msg and msg != before, name


ALLOWED_GUIDED = {
    "as_is": gedit(),
    "no_albedo": gedit(albedo_device=None),
    "rgb_only": gedit(rgba8_device=None, variance_device=None),
    "rgba_only": gedit(rgb32_device=None),
    "one_pass": gedit(iterations=1),
    "terms_off": gedit(sigma_luminance=math.inf, sigma_normal=math.inf, sigma_plane=math.inf),
    "no_sync": gedit(flags=abi.RT_DENOISE_NO_SYNC),
    "bigger_scratch": gedit(scratch_bytes=1 << 20),
    "buffers_back_to_back": gedit(rgb32_device=0x10000 + 16 * N, variance_device=0x80000 - 4 * N),
}


@pytest.mark.parametrize("name", sorted(ALLOWED_GUIDED))
def test_denoise_guided_valid_calls_pass_the_argument_checks(rtlib_path, name):
    lib = abi.load_library(rtlib_path)
    d = valid_guided()
    ALLOWED_GUIDED[name](d)
    assert lib.rt_denoise_guided(0, C.byref(d)) == box_test_status(lib), name
    msg = lib.rt_last_error()
    assert msg and (b"device" in msg or b"accessible" in msg), msg


def test_denoise_guided_null_desc(rtlib_path):
    lib = abi.load_library(rtlib_path)
    assert lib.rt_denoise_guided(0, None) == INVALID
    assert lib.rt_last_error()


@pytest.mark.parametrize("size", ((0, 0), (0, 7), (7, 0)))
def test_denoise_guided_empty_image_is_ok_and_touches_no_device(rtlib_path, size):
    lib = abi.load_library(rtlib_path)
    d = valid_guided(*size)
    assert lib.rt_denoise_guided(0, C.byref(d)) == abi.RT_OK
    assert lib.rt_denoise_guided(12345, C.byref(d)) == abi.RT_OK
    d.reserved = 1
    assert lib.rt_denoise_guided(0, C.byref(d)) == INVALID


def test_import_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "import inspect, rtamd, rtamd.renderer\n"
            "assert hasattr(rtamd.Renderer, 'denoise_guided') and len(rtamd.renderer.GUIDED_SIGMAS) == 3\n"
            "p = inspect.signature(rtamd.Renderer.accumulate).parameters\n"
            "assert p['albedo'].default is None and p['moments'].default is False\n"
            "q = inspect.signature(rtamd.Renderer.denoise_guided).parameters\n"
            "assert q['sigma_luminance'].default == rtamd.renderer.GUIDED_SIGMAS[0] and q['iterations'].default == 5\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    subprocess.run([sys.executable, "-c", code], check=True, env=env)
