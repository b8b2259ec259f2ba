"""RT_TRI_UPDATE_BOUNDS at the C-ABI boundary, without a GPU: the flag's value in the header, the library and the ctypes
mirror, the struct it travels in, and the ABI version, which the flag does not raise."""
import ctypes as C
import inspect
import os
import re
import subprocess

from rtamd import Renderer, abi
from rtamd.vtk import VtkSeriesPlayer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rt.h")


def test_flag_value_and_struct_size_as_c_compiles_them(tmp_path):
    src = tmp_path / "flag.c"
    src.write_text(f'#include <stdio.h>\n#include "{HEADER}"\nint main(void){{'
                   'printf("%u %u %zu %u\\n", (unsigned)RT_TRI_UPDATE_BOUNDS, (unsigned)RT_TRI_UPDATE_NO_SYNC, '
                   'sizeof(rt_triangle_update), (unsigned)RT_ABI_VERSION); return 0;}\n')
    exe = tmp_path / "flag"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    bounds, no_sync, size, version = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert bounds == abi.RT_TRI_UPDATE_BOUNDS == 1 << 1
    assert no_sync == abi.RT_TRI_UPDATE_NO_SYNC == 1 << 0
    assert size == C.sizeof(abi.TriangleUpdate) == 48
    assert version == abi.RT_ABI_VERSION


def test_abi_version_equals_the_headers(rtlib_path):
    lib = abi.load_library(rtlib_path)
    macro = int(re.search(r"#define RT_ABI_VERSION (\d+)u", open(HEADER).read()).group(1))
    assert lib.rt_abi_version() == macro == abi.RT_ABI_VERSION
    assert "RT_TRI_UPDATE_BOUNDS arrived within 5" in open(HEADER).read()


def test_library_accepts_the_flag_where_it_rejects_unknown_ones(rtlib_path):
    """Without a scene the call fails on its NULL scene either way; what the library does with the flag on a scene is
    tests/test_gpu_update_device_bounds.py's.  Here: the launcher the flag enqueues is linked in."""
    lib = abi.load_library(rtlib_path)
    u = abi.TriangleUpdate()
    u.flags = abi.RT_TRI_UPDATE_BOUNDS
    assert lib.rt_scene_update_triangles_device(None, C.byref(u)) == 1      # RT_ERR_INVALID_ARGUMENT: null scene
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", rtlib_path], check=True, capture_output=True, text=True).stdout
    assert "rtamd::launch_inst_bounds(" in out


def test_python_entry_points():
    assert inspect.signature(Renderer.update_triangles_device).parameters["bounds"].default is False
    assert inspect.signature(VtkSeriesPlayer.preload).parameters["derive_bounds"].default is False
