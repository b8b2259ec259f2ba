"""CPU conditions on the inputs of tests/test_gpu_lbvh_sizes.py (tests/lbvh_sizes_ref.py): every scene hits the
threshold or the degenerate case it was made for, so the GPU comparisons cannot pass on input that missed its target."""
import numpy as np
import pytest

import lbvh_sizes_ref as S
from lbvh_ref import check_tree, lbvh_tree, morton_codes
from rtamd import abi


def test_sizes_straddle_every_threshold():
    assert sum(S.SIZES) == 26604 and sorted(S.SIZES) == S.SIZES
    for edge in (S.BLAS_LEAF, 8, 64, 256, 1024, 1025, S.LOCAL_MAX, 3 * S.CHUNK):   # 1025 items = LDS_FRONT + 1 pairs
        assert {edge, edge + 1} <= set(S.SIZES), edge
    assert {1, 2, S.LOCAL_MAX - 1, S.LOCAL_MAX + 2, 4 * S.CHUNK + 1} <= set(S.SIZES)
    for edge in (S.SMALL_TLAS_MAX, S.LOCAL_MAX):
        assert {edge - 1, edge, edge + 1} <= set(S.TLAS_SIZES)
    assert set(S.TLAS_FRAME_SIZES) <= set(S.TLAS_SIZES)


@pytest.mark.parametrize("kind", S.KINDS)
def test_restated_trees(oracle_lib, kind):
    """Every size's restated tree is valid and at most HEIGHT_MAX high (a condition, not a measurement: the heights seen
    are at most 14); 2..4 items give one leaf node; "same" has one code per tree, "planar" no centroid extent in z and
    no z bits in any code; "dup8" has a run of equal codes across sorted position 1024 of a tree of more than 2048."""
    highest, crossing = 0, []
    for size in S.SIZES:
        r = S.restated(kind, size)
        nb, ci, refs = r.tree
        assert r.height == check_tree(nb, ci, refs, r.boxes, S.BLAS_LEAF) <= S.HEIGHT_MAX, size
        highest = max(highest, r.height)
        if size <= S.BLAS_LEAF:
            assert nb.shape[0] == 1 and ci[0, 0] == size and r.height == 0
        else:
            assert ci[0, 0] == 0
        v = S.tree_triangles(kind, size)["vertex"]
        if kind != "same" and size >= 63:                                # both signs: f2o / o2f order negative floats
            assert v[:, :, :2].min() < -0.5 and v[:, :, :2].max() > 0.5
        if kind == "same":
            assert len(set(r.sorted_codes.tolist())) == 1 and r.sorted_codes[0] == 0
            assert refs.tolist() == list(range(size))                    # the position rule alone, stable order
        if kind == "planar":
            assert np.ptp(r.cents[:, 2]) == 0 and (v[:, :, 2] == np.float32(S.PLANE_Z)).all()
            assert np.ptp(r.boxes[:, 4]) == 0 and (r.boxes[:, 5] > r.boxes[:, 4]).all()
            assert not (r.sorted_codes & 0x09249249).any()
        if kind == "dup8" and size > S.LOCAL_MAX and S.runs_across(r.sorted_codes, S.CHUNK):
            crossing.append(size)
        if kind in ("random", "planar") and size >= 63:
            assert len(set(r.sorted_codes.tolist())) > size // 2       # not degenerate by accident
    print(f"{kind}: largest restated height {highest}, dup8 runs across position 1024 in {crossing}")
    if kind == "dup8":
        assert crossing


@pytest.mark.parametrize("order", S.ORDERS)
def test_dup8_runs_cross_chunk_edges_of_the_forest(oracle_lib, order):
    """The chunk pass cuts the forest's sorted items every 1024 positions, wherever a tree starts: in both orders a run
    of equal codes lies across such a cut inside a tree of more than 2048 items (sdel[] holds a tie's delta there), and
    in the shuffled order a small tree lies inside a chunk that also holds items of a large one (the big[j] mix)."""
    f = S.forest("dup8", order)
    cuts, mixed = [], []
    for size, first in f.trees:
        lo, hi = first // S.CHUNK, (first + size - 1) // S.CHUNK
        if size > S.LOCAL_MAX:
            codes = S.restated("dup8", size).sorted_codes
            cuts += [(size, c) for c in range(lo + 1, hi + 1) if S.runs_across(codes, c * S.CHUNK - first)]
        else:
            big = [s for s, b in f.trees if s > S.LOCAL_MAX and b // S.CHUNK <= hi and (b + s - 1) // S.CHUNK >= lo]
            if big:
                mixed.append(size)
    print(f"{order}: tie runs across chunk cuts {cuts}, small trees in chunks of large ones {mixed}")
    assert cuts
    if order == "shuffled":
        assert len(mixed) >= 3
        assert [s for s, _ in f.trees] != S.SIZES and sorted(s for s, _ in f.trees) == S.SIZES


def test_forest_layout():
    for order in S.ORDERS:
        f = S.forest("random", order)
        assert f.scene.triangle_count == sum(S.SIZES) and len(f.scene.instances) == len(S.SIZES)
        at = 0
        for (size, first), d in zip(f.trees, f.scene.instances):
            assert first == at and (d["type"], d["index"], d["count"]) == (abi.TRIANGLE, first, size)
            assert np.array_equal(f.scene.triangles[first:first + size], S.tree_triangles("random", size))
            at += size
        xf = {(d["shift"], d["rotate"], d["scale"]) for d in f.scene.instances}
        assert len(xf) == len(S.SIZES)                                  # no two alike: option "group" or not, 26 BLASes
    t = S.tree_triangles("dup8", 2049)["vertex"]
    assert all(np.array_equal(t[k], t[k - k % S.DUP]) for k in range(2049)) and not np.array_equal(t[7], t[8])
    # the partial update of test_partial_triangle_update starts and ends inside a BLAS and crosses several
    a = S.forest("random", "ascending")
    inside = [s for s, b in a.trees if b < 1000 < b + s - 1 or b < 4000 < b + s - 1]
    whole = [s for s, b in a.trees if 1000 <= b and b + s <= 4000]
    assert len(inside) == 2 and whole


@pytest.fixture(scope="module")
def traced(oracle_lib):
    """The oracle's own traces of the aimed rays on the "random" and "dup8" forests (shuffled order)."""
    from oracle.oracle import OracleScene
    out = {}
    for kind in ("random", "dup8"):
        f = S.forest(kind, "shuffled")
        o = OracleScene(f.scene, build_seed=0)
        out[kind] = (f, S.tree_free_trace(o, S.aimed_rays()), o.trace(S.aimed_rays())[0])
    return out


def test_rays_stay_inside_the_surface_cap(traced):
    """The GPU test allows 0.1 % of the rays another surface than the tree-free trace names (ties within the
    reference's 1e-6 window resolve by visit order).  The oracle's own compat-tree trace must stay well inside that:
    >= 99.95 % the same surface.  Every tree is hit, the small ones included: their leaf records are read."""
    f, brute, tree = traced["random"]
    same = (brute["instance"] == tree["instance"]) & (brute["pindex"] == tree["pindex"])
    hit = brute["instance"] != abi.MISS
    per_tree = np.bincount(brute["instance"][hit], minlength=len(f.trees))
    print(f"random: oracle tree / tree-free same surface {same.mean():.5f}, hit {hit.mean():.3f}, "
          f"fewest hits in a tree {per_tree.min()} (size {f.trees[int(per_tree.argmin())][0]})")
    assert same.mean() >= 0.9995
    assert hit.mean() >= 0.9
    assert (per_tree >= 10).all(), per_tree
    first = np.asarray([b for _, b in f.trees])[brute["instance"][hit]]
    size = np.asarray([s for s, _ in f.trees])[brute["instance"][hit]]
    assert ((brute["pindex"][hit] >= first) & (brute["pindex"][hit] < first + size)).all()


def test_dup8_rays_hit_and_tie(traced):
    """On "dup8" an eighth of the triangles is left, eight times each, so at least the eighth of the rays that were
    aimed at one of those still hits (bar 1 / 8); the oracle's two traces agree on t — they may name different copies of
    one triangle, and nothing else."""
    f, brute, tree = traced["dup8"]
    hit = brute["instance"] != abi.MISS
    assert hit.mean() >= 1.0 / S.DUP, hit.mean()
    assert (brute["t"] == tree["t"]).mean() >= 0.9995
    v = f.scene.triangles["vertex"]
    other = hit & (brute["pindex"] != tree["pindex"]) & (brute["instance"] == tree["instance"])
    copies = np.asarray([v[a].tobytes() == v[b].tobytes() for a, b in zip(brute["pindex"][other], tree["pindex"][other])])
    print(f"dup8: hit {hit.mean():.3f}, another copy named on {int(other.sum())} rays")
    assert copies.all()


@pytest.mark.parametrize("kind", S.TLAS_KINDS)
def test_tlas_scenes(oracle_lib, kind):
    """The restated TLAS over the oracle's instance records is valid and at most HEIGHT_MAX high for every K; "lattice"
    has at most 64 distinct centroids (ties decided by position), "random" none equal and boxes of several shapes."""
    from oracle.oracle import OracleScene
    for K in S.TLAS_SIZES:
        rec = OracleScene(S.tlas_scene(K, kind)).instance_state()
        assert rec.shape == (K, 45)
        tree, height = S.restate_tlas(rec)
        assert height <= S.HEIGHT_MAX, (K, height)
        assert sorted(tree[2].tolist()) == list(range(K))
        distinct = len({c.tobytes() for c in rec[:, 42:45]})
        shapes = len({(b[1::2] - b[0::2]).tobytes() for b in rec[:, 36:42]})
        if kind == "lattice":
            assert distinct <= 64 and (K < 100 or (distinct == 64 and shapes >= 3))
            assert len(set(morton_codes(rec[:, 42:45]).tolist())) <= 64
        else:
            assert distinct == K and (K < 100 or shapes > K // 10)


def test_inactive_items_sort_behind_and_leave_the_bounds():
    """lbvh_ref's `active` mask: inactive items get the code 0xFFFFFFFF and stay out of the centroid bounds, so the
    active items' codes and subtree are those of the active items alone, and the inactive ones form one dead subtree."""
    g = np.random.default_rng(3)
    c = g.uniform(-1, 1, (40, 3)).astype(np.float32)
    c[::4] = 1e6                                                        # would stretch the bounds if counted
    active = np.ones(40, bool)
    active[::4] = False
    codes = morton_codes(c, active)
    assert (codes[~active] == 0xFFFFFFFF).all()
    assert np.array_equal(codes[active], morton_codes(c[active]))
    boxes = np.repeat(c, 2, axis=1).astype(np.float32)
    boxes[~active] = np.inf
    nb, ci, refs = lbvh_tree(boxes, c, 1, active)
    check_tree(nb, ci, refs, boxes, 1)
    live = np.flatnonzero(active)
    assert refs[:30].tolist() == live[lbvh_tree(boxes[active], c[active], 1)[2]].tolist()
    assert refs[30:].tolist() == np.flatnonzero(~active).tolist()
    assert np.isinf(nb[int(ci[0, 1]) + 1]).all() and np.isfinite(nb[int(ci[0, 1])]).all()
    assert np.array_equal(morton_codes(c), morton_codes(c, np.ones(40, bool)))
