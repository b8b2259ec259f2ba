"""rt_query_rays at the C-ABI boundary, without a GPU: the struct layout against the C compiler's, argument checks
that precede any device work, the ABI version, and `import rtamd` without torch."""
import ctypes as C
import os
import subprocess
import sys

from rtamd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "real-time-gpu-ray-tracer_amd")
HEADER = os.path.join(REPO, "include", "rt.h")


def test_ray_query_layout_matches_c(tmp_path):
    """sizeof / offsetof as gcc -std=c11 compiles rt.h (the method of tests/test_abi.py)."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("rt_ray_query %zu\\n", sizeof(rt_ray_query));']
    for fname, _ in abi.RayQuery._fields_:
        lines.append(f'printf("rt_ray_query.{fname} %zu\\n", offsetof(rt_ray_query, {fname}));')
    for name in ("RT_QUERY_EXACT", "RT_QUERY_ANY_HIT", "RT_QUERY_NO_SYNC", "RT_ABI_VERSION"):
        lines.append(f'printf("{name} %u\\n", (unsigned){name});')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lay = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    assert lay["rt_ray_query"] == C.sizeof(abi.RayQuery) == 64
    for fname, _ in abi.RayQuery._fields_:
        assert lay[f"rt_ray_query.{fname}"] == getattr(abi.RayQuery, fname).offset, fname
    assert lay["RT_QUERY_EXACT"] == abi.RT_QUERY_EXACT
    assert lay["RT_QUERY_ANY_HIT"] == abi.RT_QUERY_ANY_HIT
    assert lay["RT_QUERY_NO_SYNC"] == abi.RT_QUERY_NO_SYNC
    assert lay["RT_ABI_VERSION"] == abi.RT_ABI_VERSION


def test_null_arguments_are_rejected(rtlib_path):
    lib = abi.load_library(rtlib_path)
    assert lib.rt_query_rays(None, None) == 1                       # RT_ERR_INVALID_ARGUMENT
    q = abi.RayQuery()
    assert lib.rt_query_rays(None, C.byref(q)) == 1
    assert lib.rt_last_error()


def test_abi_version_is_the_headers(rtlib_path):
    import re
    lib = abi.load_library(rtlib_path)
    macro = int(re.search(r"#define RT_ABI_VERSION (\d+)u", open(HEADER).read()).group(1))
    assert lib.rt_abi_version() == macro == abi.RT_ABI_VERSION
    assert "rt_query_rays" in abi.EXPORTED_SYMBOLS


def test_import_without_torch():
    """`import rtamd` (and the renderer module that holds query_rays) must not need torch."""
    code = ("import sys; sys.modules['torch'] = None\n"
            "import rtamd, rtamd.renderer\n"
            "assert hasattr(rtamd.Renderer, 'query_rays') and hasattr(rtamd.renderer, 'hits_to_numpy')\n"
            "import numpy as np\n"
            "assert rtamd.renderer.hits_to_numpy(np.zeros((3, 48), np.uint8)).shape == (3,)\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, REPO]))
    subprocess.run([sys.executable, "-c", code], check=True, env=env)
