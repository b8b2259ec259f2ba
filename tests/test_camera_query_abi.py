"""rt_query_camera at the C-ABI boundary, without a GPU (the manner of tests/test_ray_query_abi.py): the struct layout
against the C compiler's, the flag values, argument checks that precede any device work, the exported symbol, the ABI
version, and `import rtamd` without torch."""
import ctypes as C
import os
import re
import subprocess
import sys

from rtamd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "real-time-gpu-ray-tracer_amd")
HEADER = os.path.join(REPO, "include", "rt.h")
FLAGS = ("RT_CAMERA_QUERY_EXACT", "RT_CAMERA_QUERY_NO_SYNC", "RT_CAMERA_QUERY_FIRST_SAMPLE")


def test_camera_query_layout_matches_c(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("rt_camera_query %zu\\n", sizeof(rt_camera_query));']
    for fname, _ in abi.CameraQuery._fields_:
        lines.append(f'printf("rt_camera_query.{fname} %zu\\n", offsetof(rt_camera_query, {fname}));')
    for name in FLAGS + ("RT_QUERY_EXACT", "RT_QUERY_NO_SYNC", "RT_ABI_VERSION"):
        lines.append(f'printf("{name} %u\\n", (unsigned){name});')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lay = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    assert lay["rt_camera_query"] == C.sizeof(abi.CameraQuery) == 72
    for fname, _ in abi.CameraQuery._fields_:
        assert lay[f"rt_camera_query.{fname}"] == getattr(abi.CameraQuery, fname).offset, fname
    for name in FLAGS:
        assert lay[name] == getattr(abi, name), name
    assert (lay["RT_CAMERA_QUERY_EXACT"], lay["RT_CAMERA_QUERY_NO_SYNC"], lay["RT_CAMERA_QUERY_FIRST_SAMPLE"]) == (1, 4, 8)
    # the shared flags sit on rt_query_rays' bits
    assert lay["RT_CAMERA_QUERY_EXACT"] == lay["RT_QUERY_EXACT"] and lay["RT_CAMERA_QUERY_NO_SYNC"] == lay["RT_QUERY_NO_SYNC"]
    assert lay["RT_ABI_VERSION"] == abi.RT_ABI_VERSION


def test_null_arguments_are_rejected(rtlib_path):
    lib = abi.load_library(rtlib_path)
    assert lib.rt_query_camera(None, None) == 1                     # RT_ERR_INVALID_ARGUMENT
    q = abi.CameraQuery()
    assert lib.rt_query_camera(None, C.byref(q)) == 1
    assert lib.rt_last_error()


def test_symbol_and_abi_version(rtlib_path):
    lib = abi.load_library(rtlib_path)
    macro = int(re.search(r"#define RT_ABI_VERSION (\d+)u", open(HEADER).read()).group(1))
    assert lib.rt_abi_version() == macro == abi.RT_ABI_VERSION
    assert "rt_query_camera" in abi.EXPORTED_SYMBOLS
    assert hasattr(lib, "rt_query_camera")
    nm = subprocess.run(["nm", "-D", "--defined-only", rtlib_path], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT rt_query_camera$", nm, re.M)


def test_import_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "import rtamd, rtamd.renderer\n"
            "assert hasattr(rtamd.Renderer, 'query_camera')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    subprocess.run([sys.executable, "-c", code], check=True, env=env)
