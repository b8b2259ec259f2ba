"""The conditions that make tests/test_gpu_deep_stack.py mean something, on the CPU: the two scenes of
tests/deep_tree_ref.py give chain trees with tied Morton codes, their rays fill the trace kernels' 16-entry stack window
once and twice, closest hits are found below entries that went through scratch, and few rays are ambiguous.

Everything here is evaluated with the restatement of the builder (tests/lbvh_ref.py) and the stack model
(deep_tree_ref.StackModel); the bounds are the issue's conditions on the inputs, not measurements of a kernel.
Measured with the committed generator (model, binary traversal):

                    height (TLAS + BLAS)  max entries  >= 17   >= 25   hit below a paged-in entry  ambiguous rays
    deep_blas       0 + 29                29           99.1 %  72.3 %  47.6 %                      14 of 3072
    deep_two_level  10 + 29               38           100 %   98.7 %  46.2 %                      12 of 2048

and in deep_two_level every ray pops at least one TLAS entry that was paged out under BLAS work (at most 9 entries
are on the stack when a BLAS is entered).  The TLAS is restated with one instance per leaf, the GPU builder's fixed
"tlas_leaf" setting (deep_tree_ref.TLAS_LEAF), not the reference's two.
"""
import numpy as np
import pytest

import deep_tree_ref as D
from lbvh_ref import check_tree, morton_codes
from rtamd import abi

CASES = ["deep_blas", "deep_two_level"]


@pytest.fixture(scope="module", params=CASES)
def case(request, oracle_lib):
    return D.case(request.param)


def share(flags):
    return float(np.mean(flags))


def test_depth(case):
    """deep_blas: height >= 28.  deep_two_level: TLAS height >= 10 and TLAS + BLAS height <= 40 — 40 binary levels keep
    every kernel form under the 64-entry capacity (a quad pushes at most 3 entries per two binary levels, a leaf adds
    at most 2), so the GPU tests never overflow."""
    hb = check_tree(*case.blas, case.boxes, D.BLAS_LEAF)
    assert hb == D.tree_height(case.blas[1])
    n_inst = len(case.scene.instances)
    state = case.oracle.instance_state()
    ht = check_tree(*case.tlas, state[:, 36:42], D.TLAS_LEAF)
    print(f"{case.name}: BLAS height {hb}, TLAS height {ht}, {len(case.blas[1])} + {len(case.tlas[1])} nodes")
    assert hb >= 28
    assert hb + ht <= 40
    if case.name == "deep_two_level":
        assert ht >= 10 and 10 <= n_inst <= 14
        assert all(d["index"] == 0 and d["count"] == case.scene.triangle_count for d in case.scene.instances)
    else:
        assert n_inst == 1 and case.scene.instances[0]["count"] == case.scene.triangle_count


def test_ties(case):
    """The trees hold equal Morton codes: fewer distinct codes than items (3 triangles per code; two instances in
    one cell)."""
    codes = morton_codes(case.cents)
    assert len(np.unique(codes)) == len(codes) // D.PER_CLUSTER == D.CODE_BITS + 1
    assert sorted(np.unique(codes).tolist()) == [1 << b for b in range(D.CODE_BITS)] + [(1 << D.CODE_BITS) - 1]
    if case.name == "deep_two_level":
        state = case.oracle.instance_state()
        icodes = morton_codes(state[:, 42:45])
        assert len(np.unique(icodes)) == len(icodes) - 1
        assert sorted(np.unique(icodes).tolist()) == [1 << b for b in range(D.TLAS_CHAIN)] + [(1 << D.CODE_BITS) - 1]
    mats = {(int(t["material_type"]), int(t["material_index"])) for t in case.scene.triangles}
    assert len(mats) >= 10                                   # the records differ by more than pindex
    assert all(i < (len(D.ROUGHS) if m == abi.ROUGH else len(D.METALS)) for m, i in mats)


def test_rays_fill_the_window(case):
    """At least 80 % of the rays reach 17 entries (one page-out), 25 % reach 25 (a second page-out before any page-in),
    no ray comes near the 64-entry capacity, and what was paged out comes back: as many page-ins as page-outs."""
    m = D.modelled(case.name)
    occ = np.array([r.max_occupancy for r in m])
    print(f"{case.name}: max occupancy {occ.max()}, >= 17: {share(occ >= 17):.4f}, >= 25: {share(occ >= 25):.4f}, "
          f"page-outs per ray up to {max(r.page_outs for r in m)}")
    assert share(occ >= 17) >= 0.80
    assert share(occ >= 25) >= 0.25
    assert occ.max() <= 41                                   # one sibling per binary level and a TLAS leaf's remainder
    assert all(r.page_ins == r.page_outs and r.end_spilled == 0 for r in m)
    assert all((r.page_outs > 0) == (r.max_occupancy > D.LDS_DEPTH) for r in m)


def test_page_ins_matter(case):
    """At least 10 % of the rays take their final hit from an entry that came back through a page-in: a page-in that
    loses or reorders an entry changes those rays' records.  The model's hit is the oracle's tree-free hit on every
    unambiguous ray, so the share is about the hits the GPU tests compare."""
    m = D.modelled(case.name)
    paged = np.array([r.hit_paged for r in m])
    got_i = np.array([r.hit_instance for r in m])
    got_p = np.array([r.hit_prim for r in m])
    hit = case.want["instance"] != abi.MISS
    want_i = np.where(hit, case.want["instance"], -1).astype(np.int64)
    want_p = np.where(hit, case.want["pindex"], -1).astype(np.int64)
    same = (got_i == want_i) & (got_p == want_p)
    print(f"{case.name}: hit below a paged-in entry {share(paged):.4f}; model == oracle on {int(same.sum())} of "
          f"{len(m)} rays, hits {share(hit):.4f}")
    assert same[~case.ambiguous].all()
    assert share(hit) >= 0.99
    assert share(paged & same & ~case.ambiguous) >= 0.10


def test_paging_across_the_instance_boundary():
    """deep_two_level: TLAS entries are paged out under BLAS work and paged back on the return to the TLAS, on at least
    10 % of the rays.

    The issue words this condition as "above 16 entries at the moment they enter a BLAS".  With the depths it also
    sets that cannot happen: near-first traversal holds one sibling per level of the current path, so at most TLAS
    height entries (+ 1 where a leaf holds a second instance) are on the stack when a BLAS is entered, and TLAS
    height <= 40 - 29 = 11 (the cap that rules out an overflow).  What the sentence explains — "TLAS entries paged
    out under BLAS work and paged back on return" — is measured directly instead: a ray counts when it pops at least
    one TLAS entry (a node or a leaf's remainder) that had been moved to scratch and came back through a page-in."""
    m = D.modelled("deep_two_level")
    back = np.array([r.tlas_paged_back for r in m])
    enter = max(r.enter_blas_max for r in m)
    print(f"deep_two_level: rays with a TLAS entry paged out and back {share(back > 0):.4f}, up to {back.max()} such "
          f"entries per ray; at most {enter} entries on the stack when a BLAS is entered")
    c = D.case("deep_two_level")
    assert 0 < enter <= D.tree_height(c.tlas[1]) + 1
    assert share(back > 0) >= 0.10


def test_unambiguous_rays(case):
    """At most 2 % of the rays are excluded from per-ray equality (two nearest hits within 1e-4 t, or the hit within
    1e-5 of a triangle edge), and the oracle's tree-free trace agrees with the float64 intersections on the others."""
    amb = case.ambiguous
    print(f"{case.name}: {int(amb.sum())} of {len(amb)} rays ambiguous")
    assert len(case.rays) >= 2000
    assert share(amb) <= 0.02
    flat = case.t.reshape(len(amb), -1)
    k = flat.argmin(axis=1)
    n_tri = case.scene.triangle_count
    hit = np.isfinite(flat.min(axis=1))
    ok = ~amb & hit
    assert np.array_equal(case.want["instance"][ok], (k // n_tri)[ok])
    assert np.array_equal(case.want["pindex"][ok], (k % n_tri)[ok])
    rel = np.abs(case.want["t"][ok] - flat.min(axis=1)[ok]) / flat.min(axis=1)[ok]
    assert rel.max() <= 1e-4, rel.max()        # the project's t tolerance between two roundings of one hit (DT_REL)
    assert np.all(case.want["instance"][~amb & ~hit] == abi.MISS)


def test_ranged_rays_still_page():
    """The GPU tests' ranged queries.  tmax = 2 t starts the traversal with a finite range and pages like the unbounded
    one.  tmax = 0.5 t does not page at all on these rays: they start outside the soup, whose root box they enter at
    more than half the distance to the first hit, so the root's own test culls the whole tree (the comparison with the
    ranged oracle stays, as a range-start check).  tmax = 0.999 t is the range that ends a deep traversal without a
    hit: every box in front of the closest hit is visited and the stack drains through its page-ins with nothing
    found.  At least 10 % of the rays must fill the window there."""
    c = D.case("deep_blas")
    model = D.StackModel(c.tlas, c.blas, c.inv, c.t)
    idx = np.flatnonzero(~c.ambiguous)[:256]
    for f, need in ((2.0, 0.10), (0.5, 0.0), (D.NEAR_MISS, 0.10)):
        runs = [model.run(i, c.rays[i], tmax=np.float32(f) * c.want["t"][i]) for i in idx]
        occ = np.array([r.max_occupancy for r in runs])
        print(f"deep_blas, tmax = {f} t: max occupancy {occ.max()}, >= 17: {share(occ >= 17):.4f}")
        assert share(occ >= 17) >= need
        if f < 1:
            assert all(r.hit_prim < 0 for r in runs)


def test_broken_page_in_changes_hits_on_the_deep_trees_only(case):
    """The sensitivity the GPU tests rely on, shown on the model: a page-in that brings back 7 of its 8 entries
    changes the closest hit of unambiguous rays on the chain trees (measured: 90 and 209 of the first 512), where the
    GPU tests demand equality on every such ray, so one changed ray is a failure; on the oracle's balanced compat
    trees over the same scene — the GPU tests' control — no ray fills the window (at most 5 / 9 entries) and nothing
    changes."""
    good = D.modelled(case.name)
    idx = np.flatnonzero(~case.ambiguous)[:512]

    def changed(model):
        runs = [model.run(i, case.rays[i], page_in_entries=D.HALF - 1) for i in idx]
        diff = sum((r.hit_instance, r.hit_prim) != (good[i].hit_instance, good[i].hit_prim) for i, r in zip(idx, runs))
        return diff, max(r.max_occupancy for r in runs)

    deep, _ = changed(D.StackModel(case.tlas, case.blas, case.inv, case.t))
    o = case.oracle
    control, occ = changed(D.StackModel(o.export_tlas(), o.export_blas(0), case.inv, case.t))
    print(f"{case.name}: broken page-in changes {deep} of {len(idx)} rays on the chain trees, {control} on the compat "
          f"trees (at most {occ} entries there)")
    assert deep > 0
    assert control == 0 and occ <= D.LDS_DEPTH
