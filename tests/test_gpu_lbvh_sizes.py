"""The GPU builder (csrc/lbvh.hip, lbvh_*.hpp) at its size thresholds and on degenerate centroid sets, on the scenes of
tests/lbvh_sizes_ref.py (tests/test_lbvh_sizes_ref.py checks on the CPU that they hit what they aim at).

The builder picks its code path by item count, and nothing but tests/lbvh_ref.py says what a GPU-built tree should be:

* BLAS forest, 26 sizes x 4 centroid kinds x 2 orders: every exported BLAS equals the restatement bit for bit (node
  boxes, count / index, leaf order), after the build and after two per-frame rebuilds; every quad equals the collapse
  rule applied to the GPU's own pairs.  That pins m == 1 and the one-leaf trees (2..4 items), the bitonic sort's padding,
  2048 / 2049 (LDS sort + bottom_up_local_kernel against rocPRIM sort + chunk and top pass), trees that end 0, 1 or 2
  items past a chunk edge, 1025 / 1026 items (collapse_wide_kernel's frontier in LDS or in scratch, adjacent trees in
  scratch slices), ties and a flat axis on the chunk and top path (sdel[], seg_delta), with and without TriCold records;
* leaf records: per-ray hits through those trees against the oracle's tree-free trace, every field bit-equal;
* TLAS sizes around SMALL_TLAS_MAX = 512 and 2048, distinct and tied centroids: export, height, one-workgroup against
  multi-kernel builder, a frame against the oracle's; the multi-kernel TLAS with inactive records against the
  restatement with an `active` mask;
* rt_scene_update_triangles over a range that starts and ends inside BLASes (extract_tri_verts_kernel, first > 0).
"""
import dataclasses

import numpy as np
import pytest

import lbvh_sizes_ref as S
from lbvh_ref import assert_tree_equal, check_tree, lbvh_tree
from rtamd import Renderer, abi, scenes
from test_gpu_lbvh import PAIR_DT, QUAD_DT, REF_LEAF, ROOT_DT, _expected_quads, frac_within, prim_items, unique_blas

pytestmark = pytest.mark.gpu

THREADS = 16
SAME_SURFACE = 0.999         # the project's bar for surfaces that tie within the reference's 1e-6 window
W = H = 64


def build_forest(f, cold=None):
    r = Renderer(f.scene, update=False).set_option("group", 0)
    if cold is not None:
        r.set_option("cold_records", cold)
    return r.build_acceleration_structure(0, mode="lbvh").configure_camera(W, H)


def check_forest(r, f, want, what):
    """Every BLAS of the forest against `want[b]` (a lbvh_sizes_ref.Restated per BLAS), and its quads against the
    collapse rule applied to the GPU's own pairs."""
    assert unique_blas(f.scene) == [(abi.TRIANGLE, first, size) for size, first in f.trees]
    assert r.info()["blas_count"] == len(f.trees)
    pairs = r.debug_read("blas_pairs").view(PAIR_DT)
    quads = r.debug_read("blas_quads").view(QUAD_DT)
    roots = r.debug_read("blas_roots").view(ROOT_DT)
    assert len(roots) == len(f.trees) and len(pairs) == len(quads)
    seen = 0
    for b, (size, first) in enumerate(f.trees):
        w = want[b]
        nb, ci, refs = r.export_blas(b)
        wb, wci, wrefs = w.tree
        at = what + (size, first)
        assert np.array_equal(ci, wci), at
        assert np.array_equal(refs, wrefs + first), at
        assert np.array_equal(nb, wb), at
        assert int(roots[b]["height"]) == w.height, at
        assert np.array_equal(roots[b]["box"], wb[0]), at
        expected = _expected_quads(pairs, int(roots[b]["ref"]))
        if size <= S.BLAS_LEAF:                          # the root ref is a leaf: no pairs, no quads, the items' union
            assert int(roots[b]["ref"]) & REF_LEAF and not expected and w.height == 0, at
            u = np.empty(6, np.float32)
            u[0::2], u[1::2] = w.boxes[:, 0::2].min(axis=0), w.boxes[:, 1::2].max(axis=0)
            assert np.array_equal(roots[b]["box"], u), at
        else:
            assert not int(roots[b]["ref"]) & REF_LEAF and len(expected) >= 1, at
        for q, (box, ref) in expected.items():
            g = quads[q]
            assert list(g["ref"]) == ref, at + (q,)
            have = np.stack([g["lo_x"], g["hi_x"], g["lo_y"], g["hi_y"], g["lo_z"], g["hi_z"]], axis=1)
            assert np.array_equal(have, np.asarray(box, np.float32)), at + (q,)
        seen += len(expected)
    assert 0 < seen <= len(pairs)


FOREST_CASES = [(k, o, None) for k in S.KINDS for o in S.ORDERS if (k, o) != ("random", "shuffled")] + \
               [("random", "shuffled", 0), ("random", "shuffled", 1)]


@pytest.mark.parametrize("kind,order,cold", FOREST_CASES)
def test_blas_forest_equals_restatement(gpu_lib, oracle_lib, kind, order, cold):
    """One scene with a BLAS of every size in S.SIZES: after rt_scene_build, and again after two frames of per-frame
    rebuilds (the spare BLAS sets; the top pass's arrival flags must have been cleared for the next build), every tree
    equals the restatement and blas_height_max is the largest restated height.  "random" / "shuffled" runs without and
    with TriCold records ("cold_records" 0: the staged TriHot gather; 1: the cold-record gather)."""
    f = S.forest(kind, order)
    want = [S.restated(kind, size) for size, _ in f.trees]
    for size, first in f.trees[:3]:                      # the items are tests/test_gpu_lbvh.py's prim_items
        boxes, cents = prim_items(f.scene, abi.TRIANGLE, first, size)
        assert np.array_equal(boxes, S.restated(kind, size).boxes) and np.array_equal(cents, S.restated(kind, size).cents)
    r = build_forest(f, cold)
    check_forest(r, f, want, (kind, order, "built"))
    assert r.info()["blas_height_max"] == max(w.height for w in want)
    r.set_option("rebuild", 1)
    r.render(0)
    r.render(1)
    check_forest(r, f, want, (kind, order, "rebuilt"))
    assert r.info()["blas_height_max"] == max(w.height for w in want)
    r.cleanup()


# ---- leaf records through the trace ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree_free(oracle_lib):
    """kind -> (forest, the oracle's tree-free records of the aimed rays), computed once per kind."""
    from oracle.oracle import OracleScene
    done = {}

    def get(kind):
        if kind not in done:
            f = S.forest(kind, "shuffled")
            want = S.tree_free_trace(OracleScene(f.scene, build_seed=0), S.aimed_rays(), THREADS)
            want.setflags(write=False)
            done[kind] = (f, want)
        return done[kind]
    return get


@pytest.mark.parametrize("cold", [0, 1])
def test_leaf_records_random(gpu_lib, tree_free, cold):
    """rt_trace_rays (EXACT) through the "random" forest's GPU-built trees against the oracle's tree-free trace: the same
    (instance, pindex) on >= 99.9 % of the rays, and on those every field of the record bit-equal — what gather_item
    wrote into the leaf slots (hot records, TriCold or the index in the pads) is what the caller's triangles say."""
    f, want = tree_free("random")
    r = build_forest(f, cold)
    got = r.trace_rays(S.aimed_rays(), exact=True)
    same = (got["instance"] == want["instance"]) & (got["pindex"] == want["pindex"])
    hit = want["instance"] != abi.MISS
    print(f"random cold {cold}: same surface {same.mean():.5f}, hit {hit.mean():.3f}")
    assert same.mean() >= SAME_SURFACE, same.mean()
    assert np.array_equal(np.isfinite(got["t"]), got["instance"] != abi.MISS)
    for k in ("t", "point", "normal", "ptype", "mtype", "midx"):
        bad = same & hit & (got[k] != want[k]).reshape(len(got), -1).any(axis=1)
        assert not bad.any(), (k, int(bad.sum()), np.flatnonzero(bad)[:8])
    r.cleanup()


@pytest.mark.parametrize("cold", [0, 1])
def test_leaf_records_dup8(gpu_lib, tree_free, cold):
    """The same rays through the "dup8" forest: wherever the oracle hits, instance, t, point, normal and material are
    bit-equal; pindex may name another copy of the same triangle (9 vertex floats bytewise equal) and nothing else."""
    f, want = tree_free("dup8")
    r = build_forest(f, cold)
    got = r.trace_rays(S.aimed_rays(), exact=True)
    hit = want["instance"] != abi.MISS
    assert np.array_equal(got["instance"] != abi.MISS, hit)
    for k in ("instance", "t", "point", "normal", "ptype", "mtype", "midx"):
        bad = hit & (got[k] != want[k]).reshape(len(got), -1).any(axis=1)
        assert not bad.any(), (k, int(bad.sum()), np.flatnonzero(bad)[:8])
    v = f.scene.triangles["vertex"]
    other = np.flatnonzero(hit & (got["pindex"] != want["pindex"]))
    print(f"dup8 cold {cold}: hit {hit.mean():.3f}, another copy named on {len(other)} rays")
    for i in other:
        assert v[got["pindex"][i]].tobytes() == v[want["pindex"][i]].tobytes(), i
    r.cleanup()


# ---- TLAS sizes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.TLAS_KINDS)
@pytest.mark.parametrize("K", S.TLAS_SIZES)
def test_tlas_sizes_equal_restatement(gpu_lib, oracle_lib, K, kind):
    """K instances of one sphere: the exported TLAS equals lbvh_tree(world boxes, centroids, 1) of the GPU's own instance
    records (which are the oracle's), with its height.  K <= 512: built by one workgroup ("tlas_small" 1) and by the
    multi-kernel builder (0), identical exports.  K > 512: "tlas_small" 1 changes nothing (the host falls back to the
    multi-kernel builder; K > 2048 takes the rocPRIM sort over 32 bits and the chunk and top pass with one-item
    leaves).  At 512, 513, 2048 and 2049 one 64 x 64 EXACT frame stays within the FAST bar of the oracle's."""
    from oracle.oracle import OracleScene
    s = S.tlas_scene(K, kind)
    o = OracleScene(s, build_seed=0)
    state = o.instance_state()
    r = Renderer(s, update=False).set_option("group", 0).build_acceleration_structure(0, mode="lbvh").configure_camera(W, H)
    out = {}
    for frame, small in enumerate((1, 0) if K <= S.SMALL_TLAS_MAX else (0, 1)):
        r.set_option("tlas_small", small)
        r.update(1 + frame)                                  # the scene is static: another frame number, the same TLAS
        rec = r.debug_read("instances").view(np.float32).reshape(-1, 45)
        assert np.array_equal(rec, state)
        want, height = S.restate_tlas(rec)
        out[small] = r.export_tlas()
        assert_tree_equal(out[small], want, (K, kind, small))
        assert r.info()["tlas_height"] == height, (K, kind, small)
        assert r.info()["tlas_node_pairs"] == K - 1
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    if K in S.TLAS_FRAME_SIZES:
        o.camera(W, H)
        _, orgba, _ = o.render(threads=THREADS)
        rgba, _, _ = r.render(3, exact=True)
        f, mx = frac_within(rgba, orgba)
        print(f"K {K} {kind}: within 1 LSB {f:.5f} (max {mx})")
        assert f >= 0.999, (f, mx)
    r.cleanup()


def test_multi_kernel_tlas_with_inactive_records(gpu_lib, oracle_lib):
    """demo_with_particles(12) with "group" 1 and "tlas_small" 0: the multi-kernel TLAS holds all 17 + 1 records — the 12
    members of the intact group inactive (key 0xFFFFFFFF, box all +inf, out of the centroid bounds), the group's record
    behind them.  Its export equals lbvh_tree(..., active) over the GPU's instance records and the group's record.

    rt_scene_debug_read("instances") returns the instance records only, so the group's record (box = union of its
    members' local boxes, centroid = their mean, the members' transform) is restated through the oracle, as one more
    instance with those bounds."""
    from oracle.oracle import OracleScene
    P, frame = 12, 5
    s = scenes.demo_with_particles(P)
    n = len(s.instances)
    members = s.instances[n - P:]
    lb = np.asarray([m["bounds"] for m in members], np.float32)
    box = np.empty(6, np.float32)
    box[0::2], box[1::2] = lb[:, 0::2].min(axis=0), lb[:, 1::2].max(axis=0)
    c = np.zeros(3)
    for m in members:                                        # build_groups: a double sum in member order
        c += np.asarray(m["centroid"], np.float32).astype(np.float64)
    s2 = scenes.demo_with_particles(P)
    s2.instances.append(dict(members[0], index=0, count=P * 1024, bounds=tuple(float(x) for x in box),
                             centroid=tuple(float(x) for x in (c / P).astype(np.float32))))
    o = OracleScene(s2, build_seed=0)
    o.update(frame)
    state = o.instance_state()
    r = Renderer(s).set_option("group", 1).build_acceleration_structure(0, mode="lbvh").configure_camera(W, H)
    r.set_option("tlas_small", 0)
    r.update(frame)
    rec = r.debug_read("instances").view(np.float32).reshape(-1, 45)
    assert rec.shape[0] == n
    assert np.array_equal(rec[:n - P], state[:n - P])
    assert np.isposinf(rec[n - P:, 36:42]).all()                # launch_instance_update(inf_inactive = true)
    records = np.concatenate([rec, state[n:]])
    active = np.ones(n + 1, bool)
    active[n - P:n] = False
    want = lbvh_tree(records[:, 36:42], records[:, 42:45], S.TLAS_LEAF, active)
    height = check_tree(*want, records[:, 36:42], S.TLAS_LEAF)
    got = r.export_tlas()
    assert_tree_equal(got, want, "inactive")
    assert sorted(got[2].tolist()) == list(range(n + 1))
    assert r.info()["tlas_height"] == height
    r.cleanup()


# ---- partial triangle update -------------------------------------------------------------------------------------------
def test_partial_triangle_update(gpu_lib, oracle_lib):
    """rt_scene_update_triangles over [1000, 4000) of the ascending "random" forest — the range starts inside the
    1023-triangle BLAS, covers the 1024-triangle one and ends inside the 1025-triangle one: the next frame and every
    exported tree equal those of a scene created with the moved triangles (and the restatement over them)."""
    first, count = 1000, 3000
    f = S.forest("random", "ascending")
    moved = f.scene.triangles.copy()
    moved["vertex"][first:first + count] += np.asarray([0.05, -0.02, 0.03], np.float32)
    r = build_forest(f)
    before = r.render(0, exact=True)[0]
    r.update_triangles(first, moved[first:first + count])
    after = r.render(0, exact=True)[0]
    assert not np.array_equal(before, after)
    f2 = S.forest("random", "ascending")
    f2.scene = dataclasses.replace(f2.scene, triangles=moved)
    fresh = build_forest(f2)
    assert np.array_equal(after, fresh.render(0, exact=True)[0])
    touched = [b for b, (size, at) in enumerate(f.trees) if at < first + count and at + size > first]
    assert len(touched) == 3
    want = [S.restate(moved[at:at + size]) if b in touched else S.restated("random", size)
            for b, (size, at) in enumerate(f.trees)]
    assert any(not np.array_equal(want[b].tree[1], S.restated("random", f.trees[b][0]).tree[1]) for b in touched)
    for b in range(len(f.trees)):
        assert_tree_equal(r.export_blas(b), fresh.export_blas(b), b)
    check_forest(r, f2, want, ("updated",))
    r.cleanup()
    fresh.cleanup()
