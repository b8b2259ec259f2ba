"""rt_accumulate_motion and rt_instance_motion_records at the C-ABI boundary, without a GPU (the manner of
tests/test_accumulate_abi.py, whose descriptions this file borrows): the struct layouts against the C compiler's, the
exported symbols, and every argument check of rt_accumulate_motion — rt_accumulate's, rt_accumulate_moments' and its
own, all of which answer before any device work."""
import ctypes as C
import re
import subprocess

import pytest

import test_accumulate_abi as TA
from rtamd import abi

INVALID = 1
N = TA.N
MOTION = 0x80000                               # a fake, aligned address disjoint from valid_desc's buffers
COUNT = 5


def test_struct_layouts_match_c(tmp_path):
    pairs = (("rt_instance_motion", abi.InstanceMotion), ("rt_motion_desc", abi.MotionDesc))
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{TA.HEADER}"', 'int main(void){']
    for cname, mirror in pairs:
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in mirror._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    for name in ("RT_MOTION_STATIC", "RT_MOTION_MOVED", "RT_MOTION_NO_HISTORY", "RT_ABI_VERSION"):
        lines.append(f'printf("{name} %u\\n", (unsigned){name});')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lay = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    assert lay["rt_instance_motion"] == C.sizeof(abi.InstanceMotion) == 96
    assert lay["rt_motion_desc"] == C.sizeof(abi.MotionDesc) == 24
    for cname, mirror in pairs:
        for fname, _ in mirror._fields_:
            assert lay[f"{cname}.{fname}"] == getattr(mirror, fname).offset, fname
    assert [lay["rt_instance_motion." + f] for f in ("point", "normal", "flags", "reserved")] == [0, 48, 84, 88]
    assert [lay["rt_motion_desc." + f] for f in ("motion_device", "instance_count", "reserved")] == [0, 8, 16]
    assert (lay["RT_MOTION_STATIC"], lay["RT_MOTION_MOVED"], lay["RT_MOTION_NO_HISTORY"]) == \
           (abi.RT_MOTION_STATIC, abi.RT_MOTION_MOVED, abi.RT_MOTION_NO_HISTORY) == (0, 1, 2)
    assert lay["RT_ABI_VERSION"] == abi.RT_ABI_VERSION == 5
    from rtamd.renderer import MOTION_DTYPE, XFORM_DTYPE
    assert MOTION_DTYPE.itemsize == 96 and XFORM_DTYPE.itemsize == C.sizeof(abi.Xform) == 36
    assert [MOTION_DTYPE.fields[f][1] for f in ("point", "normal", "flags", "reserved")] == [0, 48, 84, 88]


def test_symbols(rtlib_path):
    lib = abi.load_library(rtlib_path)
    assert lib.rt_abi_version() == abi.RT_ABI_VERSION == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", rtlib_path], check=True, capture_output=True, text=True).stdout
    for name in ("rt_accumulate_motion", "rt_instance_motion_records"):
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert re.search(rf"\bT {name}$", nm, re.M), name


def motion_desc(device=MOTION, count=COUNT):
    m = abi.MotionDesc()
    m.motion_device, m.instance_count = device, count
    return m


def call(lib, d, moments, motion, device=0):
    return lib.rt_accumulate_motion(device, C.byref(d) if d is not None else None,
                                    C.byref(moments) if moments is not None else None,
                                    C.byref(motion) if motion is not None else None)


def medit(**fields):
    return lambda d, m, mo: [setattr(mo, k, v) for k, v in fields.items()]


def dedit(**fields):
    return lambda d, m, mo: [setattr(d, k, v) for k, v in fields.items()]


# the call's own checks
OWN = {
    "reserved": medit(reserved=1),
    "reserved_high": medit(reserved=1 << 63),
    "count_above_bound": medit(instance_count=0xFFFFFFFF),
    "count_2_64": medit(instance_count=(1 << 64) - 1),
    "device_without_count": medit(instance_count=0),
    "count_without_device": medit(motion_device=None),
    "misaligned_8": medit(motion_device=MOTION + 8),
    "misaligned_4": medit(motion_device=MOTION + 4),
    "overlaps_history": medit(motion_device=0x50000),
    "overlaps_history_tail": medit(motion_device=0x50000 + 16 * N - 16),
    "ends_inside_history": medit(motion_device=0x50000 - 96 * COUNT + 16),
    "overlaps_rgb": medit(motion_device=0x60000 + 16),
    "motion_without_prev_view": dedit(prev_view=None),
}


def moments_desc():
    m = abi.MomentsDesc()
    m.albedo_device, m.prev_moments_device, m.moments_device = 0x70000, 0x74000, 0x78000
    return m


OWN_WITH_MOMENTS = {
    "overlaps_moments": medit(motion_device=0x78000),
    "overlaps_moments_tail": medit(motion_device=0x78000 + 8 * N - 16),
}


@pytest.mark.parametrize("with_moments", (False, True), ids=("plain", "moments"))
@pytest.mark.parametrize("name", sorted(OWN))
def test_own_argument_errors(rtlib_path, name, with_moments):
    lib = abi.load_library(rtlib_path)
    d, m, mo = TA.valid_desc(), (moments_desc() if with_moments else None), motion_desc()
    OWN[name](d, m, mo)
    assert lib.rt_tile_pixels(0, 0, 0, 0, 0, 0, 0, 0, None) == INVALID      # leaves another call's message behind
    before = lib.rt_last_error()
    assert call(lib, d, m, mo) == INVALID, name
    msg = lib.rt_last_error()
    assert msg and msg != before and b"no such device" not in msg and b"accessible" not in msg, name


@pytest.mark.parametrize("name", sorted(OWN_WITH_MOMENTS))
def test_motion_records_may_not_overlap_the_moments(rtlib_path, name):
    lib = abi.load_library(rtlib_path)
    d, m, mo = TA.valid_desc(), moments_desc(), motion_desc()
    OWN_WITH_MOMENTS[name](d, m, mo)
    assert call(lib, d, m, mo) == INVALID
    assert b"overlap" in lib.rt_last_error()


def test_null_motion(rtlib_path):
    lib = abi.load_library(rtlib_path)
    assert call(lib, TA.valid_desc(), None, None) == INVALID
    assert call(lib, TA.valid_desc(), moments_desc(), None) == INVALID
    assert call(lib, None, None, motion_desc()) == INVALID
    assert lib.rt_last_error()


@pytest.mark.parametrize("name", sorted(k for k, v in TA.BAD.items() if v is not None))
def test_rt_accumulates_argument_errors_apply(rtlib_path, name):
    lib = abi.load_library(rtlib_path)
    d = TA.valid_desc()
    TA.BAD[name](d)
    assert call(lib, d, None, motion_desc()) == INVALID, name
    assert call(lib, d, None, motion_desc(None, 0)) == INVALID, name


def test_rt_accumulate_moments_argument_errors_apply(rtlib_path):
    lib = abi.load_library(rtlib_path)
    for edit in (dict(reserved=1), dict(moments_device=None), dict(prev_moments_device=None), dict(moments_device=0x78004),
                 dict(albedo_device=0x70002), dict(moments_device=0x50000), dict(moments_device=0x60000)):
        d, m = TA.valid_desc(), moments_desc()
        assert lib.rt_accumulate_moments(0, C.byref(d), C.byref(m)) == TA.expected_without_launch(lib)
        for k, v in edit.items():
            setattr(m, k, v)
        assert lib.rt_accumulate_moments(0, C.byref(d), C.byref(m)) == INVALID, edit
        assert call(lib, d, m, motion_desc()) == INVALID, edit


ALLOWED = {
    "as_is": lambda d, m, mo: None,
    "no_records": medit(motion_device=None, instance_count=0),
    "no_records_no_view": lambda d, m, mo: (setattr(mo, "motion_device", None), setattr(mo, "instance_count", 0),
                                            setattr(d, "prev_view", None)),
    "first_frame_no_view": dedit(prev_hits_device=None, prev_history_device=None, prev_view=None),
    "largest_count": medit(instance_count=0xFFFFFFFE, motion_device=0x7000_0000_0000),
    "records_back_to_back": medit(motion_device=0x50000 - 96 * COUNT),
    "records_are_an_input": medit(motion_device=0x40000),           # inputs may overlap inputs
}


@pytest.mark.parametrize("with_moments", (False, True), ids=("plain", "moments"))
@pytest.mark.parametrize("name", sorted(ALLOWED))
def test_valid_calls_pass_the_argument_checks(rtlib_path, name, with_moments):
    """These reach the device check (and no further: no device, or fake addresses); the message is not an argument's."""
    lib = abi.load_library(rtlib_path)
    d, m, mo = TA.valid_desc(), (moments_desc() if with_moments else None), motion_desc()
    if name == "first_frame_no_view" and with_moments:
        m.prev_moments_device = None
    ALLOWED[name](d, m, mo)
    assert call(lib, d, m, mo) == TA.expected_without_launch(lib), (name, lib.rt_last_error())
    msg = lib.rt_last_error()
    assert msg and (b"device" in msg or b"accessible" in msg), msg


@pytest.mark.parametrize("size", ((0, 0), (0, 7), (7, 0)))
def test_empty_image_is_ok_and_touches_no_device(rtlib_path, size):
    lib = abi.load_library(rtlib_path)
    d, mo = TA.valid_desc(*size), motion_desc()
    assert call(lib, d, None, mo) == abi.RT_OK
    assert call(lib, d, moments_desc(), mo) == abi.RT_OK
    assert call(lib, d, None, mo, device=12345) == abi.RT_OK   # not even the device index is looked at
    mo.motion_device = d.history_device                        # empty outputs overlap nothing
    assert call(lib, d, None, mo) == abi.RT_OK
    mo.reserved = 1                                            # ... but the argument checks still come first
    assert call(lib, d, None, mo) == INVALID
