"""The oracle against a float64 reference where the three primitive tests decide: shared edges and vertices of a mesh,
coincident and coplanar triangles, slivers at the determinant threshold, tangent, grazing, inner and coincident
spheres, a sphere resting on a parallelogram, parallelogram edges, corners, thresholds and box faces, and hits at
t = 0.001 (tests/prim_edges_ref.py).  tests/test_gpu_prim_edges.py holds the GPU to the oracle on the same scene and
rays bit for bit; this file is what says the oracle is right there, and that the rays are where they claim to be.  No GPU.

The margins (prim_edges_ref.MARGINS, per class and copy, and one row for the pairs of a ray with an object it was not
aimed at) are 4 x the largest deviation of the oracle's arithmetic from float64: of the deciding quantities and t from
the float32 restatement of prim_edges_ref.evaluate — whose t is the oracle's bit for bit on every hit,
test_restatement_is_the_oracle — and of point and normal from the oracle's records.  test_margins_are_the_measured_ones
measures them again: a measurement is the written margin's quarter on x86-64, gcc, glibc; on another compiler or libm
it may reach the margin itself, and no margin may exceed 16 x its measurement (or the floor of 1e-8): the table is not
stale.  profiles/prim_edges/README.md has the table and the counts below.
"""
import ctypes as C

import numpy as np
import pytest

import deep_tree_ref as D
import prim_edges_ref as P
from lbvh_ref import lbvh_tree
from rtamd import abi

BUILD_SEED = 5
FLOOR = 1e-8                       # no margin is written below this
RANGE = np.asarray([P.TMIN, np.inf], np.float32)


class Case:
    def __init__(self, move=0.0):
        from oracle.oracle import OracleScene
        self.move = move
        self.scene = P.scene(move)
        self.oracle = OracleScene(self.scene, build_seed=BUILD_SEED)
        self.rays = P.rays(move)
        self.state = self.oracle.instance_state()
        self.got = self.oracle.trace(self.rays.world)[0]
        self.ev = P.evaluate(self.scene, self.rays, P.margins(move), state=self.state)
        self.verdict = P.judge(self.ev, self.got)
        self.point, self.normal = P.record64(self.scene, self.rays.world, self.ev, np.maximum(self.verdict.chosen, 0))
        self.own = P.own_instances(self.rays)


@pytest.fixture(scope="module")
def case(oracle_lib):
    c = Case()
    yield c
    c.oracle.close()


@pytest.fixture(scope="module")
def moved(oracle_lib):
    c = Case(P.MOVE)
    yield c
    c.oracle.close()


def hit_one(kind, prim, rays):
    """(accepted [n] bool, out [n, 9]: t, point, normal, u, v) of the oracle's single-primitive function on local rays."""
    from oracle.oracle import lib
    fn = {"tri": lib().oracle_hit_triangle, "sphere": lib().oracle_hit_sphere, "quad": lib().oracle_hit_parallelogram}[kind]
    rays = np.ascontiguousarray(rays, np.float32)
    out, ok = np.zeros((len(rays), 9), np.float32), np.zeros(len(rays), bool)
    for i in range(len(rays)):
        ok[i] = fn(C.byref(prim), rays[i].ctypes.data, RANGE.ctypes.data, out[i].ctypes.data)
    return ok, out


def tri_prim(sc, k):
    return abi.Triangle.from_buffer_copy(sc.triangles[k].tobytes())


def sphere_prim(sc, name):
    mt, mi, c, r = sc.spheres[P.SPHERE_INDEX[name]]
    return abi.Sphere(abi.Vec3.of(c), float(r), mt, mi)


def quad_prim(sc, name):
    mt, mi, q, u, v = sc.parallelograms[P.QUAD_INDEX[name]]
    return abi.Parallelogram(abi.Vec3.of(q), abi.Vec3.of(u), abi.Vec3.of(v), mt, mi)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def test_scene_is_the_stated_one(case):
    s, r = case.scene, case.rays
    assert len(s.instances) == 32 and s.triangle_count == 142 and len(s.spheres) == 5 and len(s.parallelograms) == 6
    assert not s.animated and not s.triangles["has_normals"].any()
    assert len(r.world) == 2 * sum(n for _, n in P.CLASSES.values()) == 24640 and r.world.dtype == np.float32
    shifts = np.array([d["shift"] for d in s.instances])
    assert len({tuple(x) for x in np.round(shifts, 4)}) == 28                      # two pairs share a cell, twice
    assert not np.any(np.abs(shifts - np.round(shifts)) < 0.05)                    # no round offsets
    # wherever a tie is intended the primitives differ in material: neighbours on the sheet and the fan, the twins and
    # the triangle across them, the coincident spheres, the ball and the parallelogram it rests on
    mat = s.triangles["material_type"].astype(int) * 100 + s.triangles["material_index"]
    _, faces, _, _ = P.sheet_edges()
    assert np.all(mat[faces[:, 0]] != mat[faces[:, 1]])
    fan = mat[P.TRI_FIRST["fan"]:P.TRI_FIRST["fan"] + 6]
    assert np.all(fan != np.roll(fan, 1))
    tw = mat[P.TRI_FIRST["twins"]:P.TRI_FIRST["twins"] + 3]
    assert len(set(tw)) == 3
    assert s.spheres[P.SPHERE_INDEX["co_a"]][:2] != s.spheres[P.SPHERE_INDEX["co_b"]][:2]
    assert s.spheres[P.SPHERE_INDEX["touch_ball"]][:2] != s.parallelograms[P.QUAD_INDEX["touch_quad"]][:2]
    # lengths: [0.5, 2] in the world; the two threshold classes set theirs in the object's frame (times GENERAL's scale)
    length = np.linalg.norm(r.world[:, 3:].astype(np.float64), axis=1)
    local = np.isin(r.cls, [P.NAMES.index("sliver_det"), P.NAMES.index("quad_ndd")])
    assert np.all((length[~local] > 0.4999) & (length[~local] < 2.0001))
    assert np.all((length[local] > 0.5 * 0.8) & (length[local] < 2.0 * 1.3)) and np.ptp(length) > 1.4
    # every ray but the radius-1000 spheres' own travels upwards, away from them
    big = r.cls == P.NAMES.index("sph_big")
    inside = r.cls == P.NAMES.index("sph_inside")
    assert np.all(r.world[~big & ~inside, 5] >= 0)
    # the second copy's local rays are not axis-aligned and not unit
    ll = np.linalg.norm(r.local[:, 3:].astype(np.float64), axis=1)
    assert np.abs(ll[r.copy == 1] / length[r.copy == 1] - 1.0).max() > 0.2


def test_restatement_is_the_oracle(case, moved):
    """The float32 restatement the margins are measured with gives, for the surface the oracle names, the oracle's t:
    every hit of both ray sets, bit for bit."""
    for c in (case, moved):
        s, got = c.ev.surf, c.got
        hit = got["instance"] != abi.MISS
        named = (got["instance"][:, None] == s.inst[None]) & (got["ptype"][:, None] == s.ptype[None]) & \
            (got["pindex"][:, None] == s.pindex[None])
        same = (named & (c.ev.t32 == got["t"][:, None])).any(axis=1)
        assert hit.sum() > 15000 and same[hit].all(), np.flatnonzero(hit & ~same)[:8]


def record_deviations(c):
    """{class: [copy 0, copy 1]: {point, normal}, stray: {...}}: the oracle's records against float64 on the surface
    they name."""
    out = {n: [dict(point=0.0, normal=0.0) for _ in (0, 1)] for n in P.NAMES}
    out[P.STRAY] = dict(point=0.0, normal=0.0)
    sel = c.verdict.chosen >= 0
    mine = np.zeros(len(sel), bool)
    mine[sel] = c.own[np.flatnonzero(sel), c.got["instance"][sel]]
    dp = np.abs(c.got["point"] - c.point).max(axis=1)
    dn = np.abs(c.got["normal"] - c.normal).max(axis=1)
    for k, d in (("point", dp), ("normal", dn)):
        if (sel & ~mine).any():
            out[P.STRAY][k] = float(d[sel & ~mine].max())
        for ci, n in enumerate(P.NAMES):
            for cp in (0, 1):
                m = sel & mine & (c.rays.cls == ci) & (c.rays.copy == cp)
                if m.any():
                    out[n][cp][k] = float(d[m].max())
    return out


def measured(c):
    dev = c.ev.deviation
    rec = record_deviations(c)
    for n in P.NAMES:
        for cp in (0, 1):
            dev[n][cp].update(rec[n][cp])
    dev[P.STRAY].update(rec[P.STRAY])
    return dev


def test_margins_are_the_measured_ones(case, moved):
    """4 x the measurement, never under FLOOR: the written margin covers the measurement, and is not stale by more
    than its factor 4."""
    for c, names in ((case, P.NAMES + [P.STRAY]), (moved, P.SHEET_CLASSES)):
        dev, written = measured(c), P.margins(c.move)
        for n in names:
            for cp, (d, w) in enumerate(zip(*((dev[n], written[n]) if n != P.STRAY else ([dev[n]], [written[n]])))):
                print(f"{n}/{cp} move {c.move:g}: " + " ".join(f"{k} {v:.2g}" for k, v in d.items() if v))
                for k, v in d.items():
                    assert v <= w[k], (n, cp, k, v, w[k])
                    assert w[k] <= max(16.0 * v, FLOOR), (n, cp, k, v, w[k])


# ---- the oracle against float64 --------------------------------------------------------------------------------------
def check_against_float64(c, name):
    idx = c.rays.of(name)
    v, got = c.verdict, c.got
    hit = got["instance"][idx] != abi.MISS
    decided = c.ev.certain[idx].any(axis=1)
    print(f"{name} move {c.move:g}: {len(idx)} rays, {int(hit.sum())} hits, {int(decided.sum())} with a certain surface, "
          f"tie sets of {v.tie[idx].sum(axis=1).mean():.2f} surfaces")
    assert v.ok[idx].all(), (name, idx[~v.ok[idx]][:8])
    sel = idx[hit]
    ch = v.chosen[sel]
    written = P.margins(c.move)
    mine = c.own[sel, got["instance"][sel]]
    for k, dev in (("t", np.abs(got["t"][sel] - c.ev.t[sel, ch])),
                   ("point", np.abs(got["point"][sel] - c.point[sel]).max(axis=1)),
                   ("normal", np.abs(got["normal"][sel] - c.normal[sel]).max(axis=1))):
        m = np.where(mine, np.asarray([written[name][cp][k] for cp in (0, 1)])[c.rays.copy[sel]], written[P.STRAY][k])
        assert np.all(dev <= m), (name, k, float((dev - m).max()))
    return hit, decided


#          class: the least share of its rays that has a certain surface — there the class is decided, not only allowed
#          (measured: 1.0 for the first five, 0.505, 0.74, 0.503)
DECIDED = {"twins": 0.99, "sph_inside": 0.99, "sph_coincident": 0.99, "contact": 0.99, "quad_thin_in": 0.99,
           "sliver_det": 0.4, "sph_big": 0.6, "sph_surface": 0.4}


@pytest.mark.parametrize("name", P.NAMES)
def test_oracle_names_a_member_of_the_tie_set(case, name):
    """Every ray of the class: a hit names a possible surface whose t64 is at most the smallest certain t64 + 1e-6 + m;
    a miss has no certain surface; t, point and normal within the margins of the named surface's float64 values."""
    hit, decided = check_against_float64(case, name)
    assert decided.mean() >= DECIDED.get(name, 0.0), decided.mean()
    if name == "quad_degenerate":
        aimed = [P.instance_of("degenerate", cp) for cp in (0, 1)]
        assert not np.isin(case.got["instance"], aimed).any()                      # nor does any other ray hit it


@pytest.mark.parametrize("name", P.SHEET_CLASSES)
def test_oracle_on_the_moved_sheet(moved, name):
    check_against_float64(moved, name)


def test_no_record_holds_a_nan(case, moved):
    for c in (case, moved):
        got = c.got
        hit = got["instance"] != abi.MISS
        for k in ("t", "point", "normal"):
            assert np.isfinite(got[k][hit]).all(), k
        assert np.all(got["t"][~hit] == np.inf) and not got["point"][~hit].any() and not got["normal"][~hit].any()
        assert np.all(np.abs(np.linalg.norm(got["normal"][hit].astype(np.float64), axis=1) - 1.0) < 1e-6)


# ---- conditions that keep the scene honest ---------------------------------------------------------------------------
def both_faces(c, idx, faces):
    """The oracle's triangle test of the local rays idx against faces [n, k] of the sheet: (accepted [n, k], t [n, k])."""
    first = P.TRI_FIRST["sheet"]
    ok, t = np.zeros(faces.shape, bool), np.zeros(faces.shape, np.float32)
    for f in np.unique(faces):
        prim = tri_prim(c.scene, first + f)
        for col in range(faces.shape[1]):
            m = np.flatnonzero(faces[:, col] == f)
            if len(m):
                a, out = hit_one("tri", prim, c.rays.local[idx[m]])
                ok[m, col], t[m, col] = a, out[:, 0]
    return ok, t


def sheet_edge_faces(c):
    """(the rays of sheet_edge, [n, 2]: the faces on either side of the edge each is aimed at)."""
    idx = c.rays.of("sheet_edge")
    return idx, P.sheet_edges()[1][c.rays.hint[idx]]


def test_edge_rays_tie(case):
    """Interior-edge rays: both adjacent triangles accept the ray, with t's within 1e-6 of each other, on >= 95 %."""
    idx, faces = sheet_edge_faces(case)
    ok, t = both_faces(case, idx, faces)
    tie = ok.all(axis=1) & (np.abs(t[:, 0].astype(np.float64) - t[:, 1]) < 1e-6)
    gap = np.abs(t[:, 0].astype(np.float64) - t[:, 1])[ok.all(axis=1)].max()
    print(f"interior-edge rays: both accepted {ok.all(axis=1).sum()} of {len(idx)}, tied {tie.sum()}, largest gap {gap:.3g}")
    assert tie.mean() >= 0.95


def test_moved_edge_rays_mostly_hit_one_triangle(moved):
    """With the sheet at x + 1000 a float32 ray cannot be aimed at an edge to 1e-6: most rays hit one triangle only."""
    idx, faces = sheet_edge_faces(moved)
    ok, _ = both_faces(moved, idx, faces)
    n = ok.sum(axis=1)
    print(f"moved interior-edge rays: both {int((n == 2).sum())}, one {int((n == 1).sum())}, none {int((n == 0).sum())}")
    assert (n == 1).mean() >= 0.5 and (n == 2).mean() <= 0.3


def test_vertex_and_hub_rays_hit_all_six(case):
    v, f = P._sheet()
    idx = case.rays.of("sheet_vertex")
    around = {h: np.flatnonzero((f == h).any(axis=1)) for h in P.SHEET_HUBS}
    assert all(len(a) == 6 and np.all(f[a, 0] == h) for h, a in around.items())
    faces = np.asarray([around[int(h)] for h in case.rays.hint[idx]])
    ok, _ = both_faces(case, idx, faces)
    print(f"interior-vertex rays: all six accepted {ok.all(axis=1).sum()} of {len(idx)}")
    assert ok.all(axis=1).mean() >= 0.95
    idx = case.rays.of("fan_hub")
    six = np.zeros((len(idx), 6), bool)
    for k in range(6):
        six[:, k], _ = hit_one("tri", tri_prim(case.scene, P.TRI_FIRST["fan"] + k), case.rays.local[idx])
    print(f"hub rays: all six accepted {six.all(axis=1).sum()} of {len(idx)}")
    assert six.all(axis=1).mean() >= 0.95


def test_threshold_classes_fall_on_both_sides(case):
    r = case.rays
    ok, _ = hit_one("sphere", sphere_prim(case.scene, "ball"), r.local[r.of("sph_tangent")])
    print(f"tangent rays: {ok.sum()} hit, {(~ok).sum()} miss")
    assert ok.mean() >= 0.2 and (~ok).mean() >= 0.2
    ok, _ = hit_one("tri", tri_prim(case.scene, P.TRI_FIRST["sliver"]), r.local[r.of("sliver_det")])
    print(f"det rays: {ok.sum()} accepted, {(~ok).sum()} rejected")
    assert ok.mean() >= 0.2 and (~ok).mean() >= 0.2
    ok, _ = hit_one("quad", quad_prim(case.scene, "quad"), r.local[r.of("quad_ndd")])
    print(f"n.d rays: {ok.sum()} accepted, {(~ok).sum()} rejected")
    assert ok.mean() >= 0.2 and (~ok).mean() >= 0.2
    out, _ = hit_one("quad", quad_prim(case.scene, "thin_out"), r.local[r.of("quad_thin_out")])
    inn, _ = hit_one("quad", quad_prim(case.scene, "thin_in"), r.local[r.of("quad_thin_in")])
    print(f"den pair: {out.sum()} and {inn.sum()} hits")
    assert not out.any() and inn.sum() >= 100
    deg, _ = hit_one("quad", quad_prim(case.scene, "degenerate"), r.local[r.of("quad_degenerate")])
    assert not deg.any()


def test_tmin_offsets(case):
    """Hits placed at t = 0 and at 0.001 + (0, 5e-7, -5e-7, 2e-6, -2e-6): Range::inRange over [0.001, inf) with its 1e-6
    windows (Range.cuh:33-43) accepts the middle four and rejects the first and the last — every ray, both copies'."""
    want = np.asarray([False, True, True, True, True, False])
    for name, kind, prim in (("tri_tmin", "tri", tri_prim(case.scene, P.TRI_FIRST["tmin_tri"])),
                             ("quad_tmin", "quad", quad_prim(case.scene, "tmin_quad"))):
        idx = case.rays.of(name)
        ok, out = hit_one(kind, prim, case.rays.local[idx])
        k = case.rays.hint[idx]
        print(name, [int(ok[k == j].sum()) for j in range(6)], "of", int((k == 0).sum()), "each")
        assert np.array_equal(ok, want[k]), [(j, int(ok[k == j].sum())) for j in range(6)]


def leaf_of(ci, refs, n, first=0):
    """Leaf number per primitive of a tree in node form whose refs are primitive indices (minus `first`)."""
    leaf = np.full(n, -1)
    for j in np.flatnonzero(ci[:, 0] > 0):
        leaf[refs[ci[j, 1]:ci[j, 1] + ci[j, 0]].astype(int) - first] = j
    assert (leaf >= 0).all()
    return leaf


def test_edge_ties_cross_leaves_and_follow_the_tree(case):
    """Interior-edge rays whose two triangles lie in different leaves: >= 100 in the oracle's BLAS of the sheet and
    >= 100 in the restated GPU tree; and on the reference's tree the winner of a tie is the tree's, not the index's:
    the lower-index and the higher-index triangle each win >= 10 % of the ties."""
    idx, faces = sheet_edge_faces(case)
    first, n = P.TRI_FIRST["sheet"], 128
    mine = None
    for b in range(case.oracle.blas_count()):
        _, ci, refs = case.oracle.export_blas(b)
        if len(refs) == n and refs.min() == first:
            mine = leaf_of(ci, refs, n, first)
    assert mine is not None
    across = mine[faces[:, 0]] != mine[faces[:, 1]]
    boxes, cents = D.triangle_items(case.scene)
    _, ci, refs = lbvh_tree(boxes[first:first + n], cents[first:first + n], D.BLAS_LEAF)
    gpu = leaf_of(ci, refs, n)
    across_gpu = gpu[faces[:, 0]] != gpu[faces[:, 1]]
    print(f"edge rays across leaves: {across.sum()} (reference's tree), {across_gpu.sum()} (GPU tree) of {len(idx)}")
    assert across.sum() >= 100 and across_gpu.sum() >= 100
    ok, t = both_faces(case, idx, faces)
    got = case.got[idx]
    tied = ok.all(axis=1) & np.isin(got["instance"], [P.instance_of("sheet", 0), P.instance_of("sheet", 1)])
    win = got["pindex"][tied].astype(int) - first
    low, high = faces[tied].min(axis=1), faces[tied].max(axis=1)
    assert np.all((win == low) | (win == high))
    print(f"edge ties: lower index wins {np.mean(win == low):.3f}, higher {np.mean(win == high):.3f} of {tied.sum()}")
    assert np.mean(win == low) >= 0.1 and np.mean(win == high) >= 0.1
