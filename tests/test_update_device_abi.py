"""rt_scene_update_triangles_device at the C-ABI boundary, without a GPU: the struct layout against the C compiler's,
the flag's value, the ABI version, argument checks that precede any device work, and the Python entry point without
torch."""
import ctypes as C
import os
import re
import subprocess
import sys

from rtamd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "real-time-gpu-ray-tracer_amd")
HEADER = os.path.join(REPO, "include", "rt.h")


def test_triangle_update_layout_matches_c(tmp_path):
    """sizeof / offsetof as gcc -std=c11 compiles rt.h (the method of tests/test_abi.py)."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("rt_triangle_update %zu\\n", sizeof(rt_triangle_update));']
    for fname, _ in abi.TriangleUpdate._fields_:
        lines.append(f'printf("rt_triangle_update.{fname} %zu\\n", offsetof(rt_triangle_update, {fname}));')
    for name in ("RT_TRI_UPDATE_NO_SYNC", "RT_ABI_VERSION"):
        lines.append(f'printf("{name} %u\\n", (unsigned){name});')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lay = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    assert lay["rt_triangle_update"] == C.sizeof(abi.TriangleUpdate) == 48
    for fname, _ in abi.TriangleUpdate._fields_:
        assert lay[f"rt_triangle_update.{fname}"] == getattr(abi.TriangleUpdate, fname).offset, fname
    assert [f for f, _ in abi.TriangleUpdate._fields_] == ["first", "count", "vertices_device", "normals_device",
                                                           "flags", "reserved", "stream"]
    assert lay["RT_TRI_UPDATE_NO_SYNC"] == abi.RT_TRI_UPDATE_NO_SYNC == 1
    assert lay["RT_ABI_VERSION"] == abi.RT_ABI_VERSION == 5


def test_abi_version_is_5_everywhere(rtlib_path):
    lib = abi.load_library(rtlib_path)
    macro = int(re.search(r"#define RT_ABI_VERSION (\d+)u", open(HEADER).read()).group(1))
    assert lib.rt_abi_version() == macro == abi.RT_ABI_VERSION == 5
    assert "rt_scene_update_triangles_device" in abi.EXPORTED_SYMBOLS
    assert hasattr(lib, "rt_scene_update_triangles_device")


def test_null_arguments_are_rejected(rtlib_path):
    lib = abi.load_library(rtlib_path)
    assert lib.rt_scene_update_triangles_device(None, None) == 1      # RT_ERR_INVALID_ARGUMENT
    u = abi.TriangleUpdate()
    assert lib.rt_scene_update_triangles_device(None, C.byref(u)) == 1
    assert lib.rt_last_error()


def test_entry_point_without_torch():
    """`import rtamd` and Renderer.update_triangles_device must not need torch."""
    code = ("import sys; sys.modules['torch'] = None\n"
            "import rtamd, rtamd.renderer, rtamd.vtk\n"
            "assert callable(rtamd.Renderer.update_triangles_device)\n"
            "assert hasattr(rtamd.vtk.VtkSeriesPlayer, 'preload')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    subprocess.run([sys.executable, "-c", code], check=True, env=env)
