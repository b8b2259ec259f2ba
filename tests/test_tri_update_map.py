"""CPU check of the index mapping of rt_scene_update_triangles_device's kernel (csrc/tri_update_map.hpp, shared with
csrc/tri_update.hip): tests/cpp/tri_update_map_check.cpp replays the kernel's work items on host arrays, built with
the address and undefined-behaviour sanitizers and run as a process of its own.  Every target float is written exactly
once from its source element, nothing outside the vertex / normal fields of the range changes (materials, reserved,
neighbouring records), has_normals is written only with normals, 8-byte record stores are 8-byte aligned for either
parity of `first`, and raw_verts receives the vertex stream."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
N = 300


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tri_update") / "tri_update_map_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "cpp", "tri_update_map_check.cpp")], check=True)
    return exe


@pytest.mark.parametrize("normals", [1, 0])
@pytest.mark.parametrize("first,count", [(0, 1), (1, 1), (0, 255), (3, 256), (5, 257), (N - 1, 1), (N - 4, 4)])
def test_work_items_cover_the_range_exactly(checker, first, count, normals):
    p = subprocess.run([checker, str(N), str(first), str(count), str(normals)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout)
    assert r["written_once"] == 1 and r["wrong_source"] == 0 and r["verts_equal"] == 1, r
    assert r["outside_bytes"] == 0 and r["out_of_array"] == 0 and r["misaligned"] == 0, r
    assert r["flag_writes"] == (count if normals else 0) and r["flag_bad"] == 0, r
