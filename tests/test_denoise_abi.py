"""rt_denoise at the C-ABI boundary, without a GPU (the manner of tests/test_camera_query_abi.py): the struct layout
against the C compiler's, the exported symbols, the ABI version, the scratch size, and every argument check — all of
which answer before any device work."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import pytest

from rtamd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "real-time-gpu-ray-tracer_amd")
HEADER = os.path.join(REPO, "include", "rt.h")
INVALID = 1                                    # RT_ERR_INVALID_ARGUMENT


def test_denoise_desc_layout_matches_c(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("rt_denoise_desc %zu\\n", sizeof(rt_denoise_desc));']
    for fname, _ in abi.DenoiseDesc._fields_:
        lines.append(f'printf("rt_denoise_desc.{fname} %zu\\n", offsetof(rt_denoise_desc, {fname}));')
    for name in ("RT_DENOISE_NO_SYNC", "RT_QUERY_NO_SYNC", "RT_CAMERA_QUERY_NO_SYNC", "RT_ABI_VERSION"):
        lines.append(f'printf("{name} %u\\n", (unsigned){name});')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lay = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    assert lay["rt_denoise_desc"] == C.sizeof(abi.DenoiseDesc) == 96
    for fname, _ in abi.DenoiseDesc._fields_:
        assert lay[f"rt_denoise_desc.{fname}"] == getattr(abi.DenoiseDesc, fname).offset, fname
    # the queries' NO_SYNC bit
    assert lay["RT_DENOISE_NO_SYNC"] == abi.RT_DENOISE_NO_SYNC == lay["RT_QUERY_NO_SYNC"] == lay["RT_CAMERA_QUERY_NO_SYNC"] == 4
    assert lay["RT_ABI_VERSION"] == abi.RT_ABI_VERSION == 5


def test_symbols_and_abi_version(rtlib_path):
    lib = abi.load_library(rtlib_path)
    macro = int(re.search(r"#define RT_ABI_VERSION (\d+)u", open(HEADER).read()).group(1))
    assert lib.rt_abi_version() == macro == abi.RT_ABI_VERSION == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", rtlib_path], check=True, capture_output=True, text=True).stdout
    for name in ("rt_denoise", "rt_denoise_scratch_bytes"):
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert re.search(rf"\bT {name}$", nm, re.M), name


def test_scratch_bytes_is_monotone_and_zero_when_empty(rtlib_path):
    lib = abi.load_library(rtlib_path)
    f = lib.rt_denoise_scratch_bytes
    assert f(0, 0) == f(0, 1080) == f(1920, 0) == 0
    sizes = (1, 2, 15, 16, 17, 64, 1080, 1920, 3840, 16384)
    for a in sizes:
        assert f(a, a) > 0 and f(a, a) % 16 == 0
        for b in sizes:
            assert f(a, b) <= f(a + 1, b) and f(a, b) <= f(a, b + 1)
            assert f(a, b) == f(b, a)
    assert f(16384, 16384) == 64 * 16384 * 16384              # no 32-bit wrap


def valid_desc(width=8, height=4):
    """A description that passes every argument check: the pointers are never dereferenced on the host (fake, aligned
    addresses), and nothing is enqueued without a device."""
    d = abi.DenoiseDesc()
    d.width, d.height, d.iterations, d.flags = width, height, 3, 0
    d.sigma_color, d.sigma_normal, d.sigma_plane = 1.0, 0.5, float("inf")
    d.color_device, d.hits_device, d.albedo_device = 0x10000, 0x20000, 0x30000
    d.rgb32_device, d.rgba8_device, d.scratch_device = 0x40000, 0x50000, 0x60000
    d.scratch_bytes = 64 * width * height
    return d


def edit(**fields):
    def apply(d):
        for k, v in fields.items():
            setattr(d, k, v)
    return apply


BAD = {
    "reserved": edit(reserved=1),
    "unknown_flag": edit(flags=1),
    "unknown_flag_high": edit(flags=abi.RT_DENOISE_NO_SYNC | (1 << 31)),
    "iterations_0": edit(iterations=0),
    "iterations_6": edit(iterations=6),
    "sigma_color_0": edit(sigma_color=0.0),
    "sigma_color_negative": edit(sigma_color=-1.0),
    "sigma_color_nan": edit(sigma_color=math.nan),
    "sigma_normal_0": edit(sigma_normal=0.0),
    "sigma_normal_nan": edit(sigma_normal=math.nan),
    "sigma_plane_minus_inf": edit(sigma_plane=-math.inf),
    "sigma_plane_nan": edit(sigma_plane=math.nan),
    "width_16385": edit(width=16385, scratch_bytes=1 << 40),
    "height_16385": edit(height=16385, scratch_bytes=1 << 40),
    "no_output": edit(rgb32_device=None, rgba8_device=None),
    "null_color": edit(color_device=None),
    "null_hits": edit(hits_device=None),
    "null_scratch": edit(scratch_device=None),
    "scratch_one_byte_short": edit(scratch_bytes=64 * 8 * 4 - 1),
    "scratch_misaligned": edit(scratch_device=0x60008),
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
    assert lib.rt_denoise(device, C.byref(d)) == INVALID, name
    msg = lib.rt_last_error()
    assert msg and msg != before, name


def test_null_desc(rtlib_path):
    lib = abi.load_library(rtlib_path)
    assert lib.rt_denoise(0, None) == INVALID
    assert lib.rt_last_error()


def test_valid_call_is_refused_before_any_launch(rtlib_path):
    """Without a GPU a valid non-empty call fails as rt_box_test does; with one, the fake addresses are rejected by the
    pointer check.  Either way nothing is enqueued."""
    import numpy as np
    lib = abi.load_library(rtlib_path)
    want = INVALID
    if lib.rt_device_count() == 0:
        one = np.zeros(6, np.float32)
        hit, te = np.zeros(1, np.uint8), np.zeros(1, np.float32)
        want = lib.rt_box_test(0, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 0, hit.ctypes.data, te.ctypes.data)
        assert want != abi.RT_OK
    d = valid_desc()
    assert lib.rt_denoise(0, C.byref(d)) == want
    assert lib.rt_last_error()


@pytest.mark.parametrize("size", ((0, 0), (0, 7), (7, 0)))
def test_empty_image_is_ok_and_touches_no_device(rtlib_path, size):
    lib = abi.load_library(rtlib_path)
    d = valid_desc(*size)
    assert d.scratch_bytes == 0
    assert lib.rt_denoise(0, C.byref(d)) == abi.RT_OK
    assert lib.rt_denoise(12345, C.byref(d)) == abi.RT_OK   # not even the device index is looked at
    d.flags = abi.RT_DENOISE_NO_SYNC
    assert lib.rt_denoise(0, C.byref(d)) == abi.RT_OK
    d.reserved = 1                                          # ... but the argument checks still come first
    assert lib.rt_denoise(0, C.byref(d)) == INVALID


def test_import_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "import rtamd, rtamd.renderer\n"
            "assert hasattr(rtamd.Renderer, 'denoise')\n"
            "assert len(rtamd.renderer.DENOISE_SIGMAS) == 3\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    subprocess.run([sys.executable, "-c", code], check=True, env=env)
