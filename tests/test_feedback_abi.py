"""rt_denoise_guided_feedback at the C-ABI boundary, without a GPU (the manner of tests/test_guided_abi.py): the layout
of rt_feedback_desc against the C compiler's, the exported symbol, the ABI version, every new argument check — the
permitted exact alias of the history, its partial overlap, an overlap with each output and with the scratch — and every
check of rt_denoise_guided through the new entry point.  All of them answer before any device work."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from rtamd import Renderer, abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rt.h")
INVALID = 1                                    # RT_ERR_INVALID_ARGUMENT
N = 8 * 4                                      # pixels of the valid descriptions' image
HISTORY, MOMENTS, HITS, ALBEDO, RGB, RGBA, VARIANCE, SCRATCH, FEEDBACK = (0x10000 * k for k in range(1, 10))


def test_struct_layout_matches_c(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(rt_feedback_desc));',
             'printf("guided %zu\\n", sizeof(rt_denoise_guided_desc));']
    for fname, _ in abi.FeedbackDesc._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(rt_feedback_desc, {fname}));')
    lines += ['printf("RT_ABI_VERSION %u\\n", (unsigned)RT_ABI_VERSION);', 'return 0;}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lay = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    assert lay["size"] == C.sizeof(abi.FeedbackDesc) == 16
    assert lay["guided"] == C.sizeof(abi.DenoiseGuidedDesc) == 112          # unchanged
    assert [f for f, _ in abi.FeedbackDesc._fields_] == ["feedback_device", "reserved"]
    for fname, _ in abi.FeedbackDesc._fields_:
        assert lay[fname] == getattr(abi.FeedbackDesc, fname).offset, fname
    assert lay["RT_ABI_VERSION"] == abi.RT_ABI_VERSION == 5


def test_symbol_and_abi_version(rtlib_path):
    lib = abi.load_library(rtlib_path)
    header = open(HEADER).read()
    macro = int(re.search(r"#define RT_ABI_VERSION (\d+)u", header).group(1))
    assert lib.rt_abi_version() == macro == abi.RT_ABI_VERSION == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", rtlib_path], check=True, capture_output=True, text=True).stdout
    name = "rt_denoise_guided_feedback"
    assert name in abi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(rf"\bT {name}$", nm, re.M)
    assert re.search(rf"\b{name}\(", header)
    assert "rt_denoise_guided_feedback / rt_feedback_desc arrived within 5 the same way" in header


def valid(width=8, height=4):
    """Descriptions that pass every argument check: fake, aligned, disjoint addresses, never dereferenced on the host."""
    d = abi.DenoiseGuidedDesc()
    d.width, d.height, d.iterations, d.flags = width, height, 5, 0
    d.sigma_luminance, d.sigma_normal, d.sigma_plane = 4.0, 0.1, 0.1
    d.history_device, d.moments_device, d.hits_device, d.albedo_device = HISTORY, MOMENTS, HITS, ALBEDO
    d.rgb32_device, d.rgba8_device, d.variance_device, d.scratch_device = RGB, RGBA, VARIANCE, SCRATCH
    d.scratch_bytes = 64 * width * height
    f = abi.FeedbackDesc()
    f.feedback_device = FEEDBACK
    return d, f


def edit(**fields):
    def apply(d, f):
        for k, v in fields.items():
            setattr(f if k in ("feedback_device", "f_reserved") else d, "reserved" if k == "f_reserved" else k, v)
    return apply


def box_test_status(lib):
    """What a call that passes the argument checks answers here (tests/test_guided_abi.py): without a GPU it fails as
    rt_box_test does; with one, the fake addresses are rejected by the pointer check.  Nothing is enqueued."""
    if lib.rt_device_count() > 0:
        return INVALID
    one = np.zeros(6, np.float32)
    hit, te = np.zeros(1, np.uint8), np.zeros(1, np.float32)
    want = lib.rt_box_test(0, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 0, hit.ctypes.data, te.ctypes.data)
    assert want != abi.RT_OK
    return want


BAD = {
    # the feedback's own
    "feedback_reserved": edit(f_reserved=1),
    "feedback_reserved_high": edit(f_reserved=1 << 63),
    "null_feedback_device": edit(feedback_device=None),
    "feedback_misaligned_8": edit(feedback_device=FEEDBACK + 8),
    "feedback_misaligned_4": edit(feedback_device=FEEDBACK + 4),
    "feedback_inside_history": edit(feedback_device=HISTORY + 16),
    "feedback_ends_inside_history": edit(feedback_device=HISTORY - 16 * N + 16),
    "feedback_overlaps_history_tail": edit(feedback_device=HISTORY + 16 * N - 16),
    "feedback_overlaps_moments": edit(feedback_device=MOMENTS),
    "feedback_overlaps_moments_tail": edit(feedback_device=MOMENTS + 8 * N - 16),
    "feedback_overlaps_hits": edit(feedback_device=HITS + 48 * N - 16),
    "feedback_overlaps_albedo": edit(feedback_device=ALBEDO),
    "feedback_overlaps_rgb": edit(feedback_device=RGB),
    "feedback_ends_inside_rgb": edit(feedback_device=RGB - 16 * N + 16),
    "feedback_overlaps_rgba": edit(feedback_device=RGBA + 4 * N - 16),
    "feedback_overlaps_variance": edit(feedback_device=VARIANCE),
    "feedback_overlaps_scratch": edit(feedback_device=SCRATCH),
    "feedback_overlaps_scratch_tail": edit(feedback_device=SCRATCH + 64 * N - 16),
    "feedback_ends_inside_scratch": edit(feedback_device=SCRATCH - 16 * N + 16),
    "rgb_on_aliased_history": edit(feedback_device=HISTORY, rgb32_device=HISTORY),
    # rt_denoise_guided's (tests/test_guided_abi.py, BAD_GUIDED), through the new entry point
    "reserved": edit(reserved=1),
    "unknown_flag": edit(flags=1),
    "unknown_flag_high": edit(flags=abi.RT_DENOISE_NO_SYNC | (1 << 31)),
    "iterations_0": edit(iterations=0),
    "iterations_6": edit(iterations=6),
    "sigma_luminance_0": edit(sigma_luminance=0.0),
    "sigma_luminance_negative": edit(sigma_luminance=-1.0),
    "sigma_luminance_nan": edit(sigma_luminance=math.nan),
    "sigma_normal_0": edit(sigma_normal=0.0),
    "sigma_normal_nan": edit(sigma_normal=math.nan),
    "sigma_plane_0": edit(sigma_plane=0.0),
    "sigma_plane_nan": edit(sigma_plane=math.nan),
    "width_16385": edit(width=16385, scratch_bytes=1 << 40),
    "height_16385": edit(height=16385, scratch_bytes=1 << 40),
    "no_output": edit(rgb32_device=None, rgba8_device=None),
    "null_history": edit(history_device=None),
    "null_moments": edit(moments_device=None),
    "null_hits": edit(hits_device=None),
    "null_scratch": edit(scratch_device=None),
    "scratch_too_small": edit(scratch_bytes=64 * N - 1),
    "scratch_misaligned": edit(scratch_device=SCRATCH + 8),
    "history_misaligned": edit(history_device=HISTORY + 8),
    "moments_misaligned": edit(moments_device=MOMENTS + 4),
    "hits_misaligned": edit(hits_device=HITS + 2),
    "albedo_misaligned": edit(albedo_device=ALBEDO + 1),
    "rgb_misaligned": edit(rgb32_device=RGB + 2),
    "rgba_misaligned": edit(rgba8_device=RGBA + 2),
    "variance_misaligned": edit(variance_device=VARIANCE + 2),
    "rgb_is_history": edit(rgb32_device=HISTORY),
    "rgb_overlaps_history_tail": edit(rgb32_device=HISTORY + 16 * N - 4),
    "rgb_overlaps_moments": edit(rgb32_device=MOMENTS - 12 * N + 4),
    "rgb_overlaps_hits": edit(rgb32_device=HITS + 48 * N - 4),
    "rgb_overlaps_albedo": edit(rgb32_device=ALBEDO),
    "rgba_overlaps_history": edit(rgba8_device=HISTORY),
    "rgba_overlaps_rgb": edit(rgba8_device=RGB + 12 * N - 4),
    "variance_overlaps_moments": edit(variance_device=MOMENTS + 8 * N - 4),
    "variance_overlaps_rgba": edit(variance_device=RGBA),
    "scratch_overlaps_history": edit(scratch_device=HISTORY - 64 * N + 16),
    "scratch_overlaps_rgb": edit(scratch_device=RGB),
    "scratch_overlaps_variance": edit(variance_device=SCRATCH + 64 * N - 4),
    "no_such_device": None,
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_argument_errors(rtlib_path, name):
    lib = abi.load_library(rtlib_path)
    d, f = valid()
    device = 0
    if BAD[name] is None:
        device = max(lib.rt_device_count(), 0) + 7
    else:
        BAD[name](d, f)
    assert lib.rt_tile_pixels(0, 0, 0, 0, 0, 0, 0, 0, None) == INVALID      # leaves another call's message behind
    before = lib.rt_last_error()
    assert lib.rt_denoise_guided_feedback(device, C.byref(d), C.byref(f)) == INVALID, name
    msg = lib.rt_last_error()
    assert msg and msg != before, name
    if name != "no_such_device":
        assert b"device" not in msg.replace(b"_device", b"") and b"accessible" not in msg, msg   # an argument check answered


ALLOWED = {
    "as_is": edit(),
    "feedback_is_the_history": edit(feedback_device=HISTORY),
    "feedback_right_after_the_history": edit(feedback_device=HISTORY + 16 * N),
    "feedback_right_before_the_scratch": edit(feedback_device=SCRATCH - 16 * N),
    "no_albedo": edit(albedo_device=None),
    "rgb_only": edit(rgba8_device=None, variance_device=None),
    "rgba_only": edit(rgb32_device=None),
    "one_pass": edit(iterations=1),
    "terms_off": edit(sigma_luminance=math.inf, sigma_normal=math.inf, sigma_plane=math.inf),
    "no_sync": edit(flags=abi.RT_DENOISE_NO_SYNC),
}


@pytest.mark.parametrize("name", sorted(ALLOWED))
def test_valid_calls_pass_the_argument_checks(rtlib_path, name):
    lib = abi.load_library(rtlib_path)
    d, f = valid()
    ALLOWED[name](d, f)
    assert lib.rt_denoise_guided_feedback(0, C.byref(d), C.byref(f)) == box_test_status(lib), name
    msg = lib.rt_last_error()
    assert msg and (b"device" in msg or b"accessible" in msg), msg


def test_null_arguments(rtlib_path):
    lib = abi.load_library(rtlib_path)
    d, f = valid()
    assert lib.rt_denoise_guided_feedback(0, None, C.byref(f)) == INVALID
    assert lib.rt_denoise_guided_feedback(0, C.byref(d), None) == INVALID
    assert lib.rt_denoise_guided_feedback(0, None, None) == INVALID
    assert lib.rt_last_error()
    d, f = valid(0, 7)
    assert lib.rt_denoise_guided_feedback(0, C.byref(d), None) == INVALID    # even for an empty image


@pytest.mark.parametrize("size", ((0, 0), (0, 7), (7, 0)))
def test_empty_image_is_ok_and_touches_no_device(rtlib_path, size):
    lib = abi.load_library(rtlib_path)
    d, f = valid(*size)
    assert lib.rt_denoise_guided_feedback(0, C.byref(d), C.byref(f)) == abi.RT_OK
    assert lib.rt_denoise_guided_feedback(12345, C.byref(d), C.byref(f)) == abi.RT_OK   # not even the device index is looked at
    f.feedback_device = RGB                                     # empty ranges do not overlap
    assert lib.rt_denoise_guided_feedback(0, C.byref(d), C.byref(f)) == abi.RT_OK
    f.feedback_device = FEEDBACK + 8                            # ... but the argument checks still come first
    assert lib.rt_denoise_guided_feedback(0, C.byref(d), C.byref(f)) == INVALID
    f.feedback_device, f.reserved = FEEDBACK, 1
    assert lib.rt_denoise_guided_feedback(0, C.byref(d), C.byref(f)) == INVALID
    f.reserved, d.reserved = 0, 1
    assert lib.rt_denoise_guided_feedback(0, C.byref(d), C.byref(f)) == INVALID


def test_renderer_option_defaults_to_off():
    p = inspect.signature(Renderer.denoise_guided).parameters
    assert p["feedback"].default is False and p["feedback"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "rt_denoise_guided_feedback" in Renderer.denoise_guided.__doc__
