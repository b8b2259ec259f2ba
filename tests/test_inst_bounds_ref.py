"""RT_TRI_UPDATE_BOUNDS without a GPU: the centroid reduction's bookkeeping (tests/cpp/inst_bounds_map_check.cpp replays
csrc/inst_bounds.hip's kernels with csrc/inst_bounds_map.hpp, built with the address and undefined-behaviour sanitizers and
run as a process of its own), its shape against the numpy restatement (tests/inst_bounds_ref.py), and the conditions
tests/test_gpu_update_device_bounds.py rests on, so that a failure there is never the inputs' fault."""
import json
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import inst_bounds_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK = ref.CHUNK
COUNTS = [1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 70001]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inst_bounds") / "inst_bounds_map_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "cpp", "inst_bounds_map_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def replay(checker, tmp_path_factory):
    """One run over instances of every count, back to back from an odd first triangle."""
    rng = np.random.default_rng(11)
    first = 3
    verts = rng.uniform(1.0, 16.0, (first + sum(COUNTS), 3, 3)).astype(np.float32)
    path = str(tmp_path_factory.mktemp("inst_bounds_in") / "verts.f32")
    verts.tofile(path)
    p = subprocess.run([checker, path, str(first)] + [str(c) for c in COUNTS], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return verts, first, json.loads(p.stdout)


def test_header_constants_match_the_restatement():
    text = open(os.path.join(HERE, "..", "real-time-gpu-ray-tracer_amd", "csrc", "inst_bounds_map.hpp")).read()
    assert "IB_WAVE = 64;" in text and "IB_WAVES = 4;" in text and "IB_ROUNDS = 4;" in text
    assert "IB_CHUNK = IB_BLOCK * IB_ROUNDS;" in text and "IB_BLOCK = IB_WAVE * IB_WAVES;" in text
    assert CHUNK == 1024


def test_every_triangle_is_summed_exactly_once(replay):
    _, _, r = replay
    assert r["covered_once"] == 1 and r["transpose_bad"] == 0 and r["asker_bad"] == 0, r
    assert r["items_bad"] == 0 and r["shape_bad"] == 0, r


def test_replay_equals_the_numpy_restatement(replay):
    verts, first, r = replay
    at = first
    for i, n in enumerate(COUNTS):
        c = ref.tri_centroids(verts[at:at + n])
        want = ref.device_sum(c)
        got = [struct.unpack("<d", bytes.fromhex(h)[::-1])[0] for h in r["sums"][3 * i:3 * i + 3]]
        assert [float(x).hex() for x in want] == [x.hex() for x in got], n
        cen = ref.centroid(verts[at:at + n])
        got_c = [struct.unpack("<f", bytes.fromhex(h)[::-1])[0] for h in r["centroids"][3 * i:3 * i + 3]]
        assert np.array_equal(np.asarray(got_c, np.float32), cen), n
        # coordinates in [1, 16): the sums are exact, so the shape equals the host's sequential sum
        assert np.array_equal(want, ref.sequential_sum(c)), n
        at += n


def test_shape_is_not_the_sequential_sum_in_general():
    """With coordinates of mixed magnitude the two orders round differently somewhere: the 1 ulp the contract allows
    is needed, and the restatement is not the sequential sum under another name."""
    rng = np.random.default_rng(3)
    c = (rng.standard_normal((5000, 3)) * 10.0 ** rng.uniform(-6, 6, (5000, 3))).astype(np.float32)
    assert not np.array_equal(ref.device_sum(c), ref.sequential_sum(c))


def _scenes():
    for t in ref.T_CASES:
        for lb in (False, True):
            yield f"T{t}-bounds{int(lb)}", ref.particles(ref.P, t, lb), ref.P * t
    yield "groups", ref.particles(8, 64, True), 8 * 64


@pytest.mark.parametrize("shift", [(0, 0, 0), ref.SHIFTS["near"], ref.SHIFTS["away"]] + ref.SHIFTS["frames"])
def test_conditions_of_the_gpu_tests(shift):
    """Every test scene, before and after every shift the GPU tests apply: each centroid coordinate of each triangle
    (the demo's own included) lies in [1, 16); the host's sequential double sums — per instance over its triangles,
    per group over its members' centroids — are exact (math.fsum); no box extreme is +-0."""
    for name, s, n_p in _scenes():
        tris = ref.moved(s.triangles, 0, len(s.triangles), shift)
        c = ref.tri_centroids(tris["vertex"])
        assert (c >= 1.0).all() and (c < 16.0).all(), name
        assert (ref.tri_boxes(tris["vertex"]) != 0).all(), name
        members = []
        for d in s.instances:
            if d["type"] != 2 or d.get("count", 0) == 0:
                continue
            ci = c[d["index"]:d["index"] + d["count"]]
            seq = ref.sequential_sum(ci)
            assert [math.fsum(ci[:, a].astype(np.float64)) for a in range(3)] == list(seq), name
            assert np.array_equal(ref.device_sum(ci), seq), name
            members.append(ref.centroid(tris["vertex"][d["index"]:d["index"] + d["count"]]))
        m = np.asarray(members, np.float32)
        assert (m >= 1.0).all() and (m < 16.0).all(), name
        seq = ref.sequential_sum(m)
        assert [math.fsum(m[:, a].astype(np.float64)) for a in range(3)] == list(seq), name
        assert np.array_equal(ref.group_centroid(m), (seq / np.float64(len(m))).astype(np.float32)), name


def test_unquantised_particles_round_differently_by_at_most_one_ulp():
    """The inexact case of the GPU tests (scenes.synth_particles as it comes, coordinates around 0): both sums carry a
    relative error below 2^-40 before the one rounding to float, so the centroids differ by at most 1 float ulp."""
    tris, inst = ref.scenes.synth_particles(ref.P, CHUNK + 64)
    for d in inst:
        v = tris["vertex"][d["index"]:d["index"] + d["count"]]
        a, b = ref.centroid(v), ref.centroid(v, total=ref.sequential_sum)
        assert (np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)) <= 1).all()
