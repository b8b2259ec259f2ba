"""The three primitive tests where they decide, on the GPU: the scene and the 24 640 rays of tests/prim_edges_ref.py —
shared edges and vertices of a mesh, a fan's hub, coincident and coplanar triangles, slivers at the determinant
threshold, tangent, grazing, inner and coincident spheres, a sphere resting on a parallelogram, parallelogram edges,
corners, thresholds and box faces, hits at t = 0.001 +- (0, 5e-7, 2e-6) — each object under the identity and under a
general transform.  tests/test_prim_edges_ref.py holds the oracle to a float64 reference there and asserts that the rays
are where they claim to be (ties on >= 95 % of the edge rays, both sides of every threshold); here:

a. on the reference's trees (compat, "wide" 1 and 0), EXACT and FAST, every ray equals the oracle in all 8 fields, as
   closest records, t alone, any-hit and rt_trace_rays: the tie rule (the later-tested primitive wins within 1e-6), the
   order inside a leaf, the visit order across leaves and the TLAS order, for the binary pairs and the quad order;
b. on SAH and GPU-built trees (rows 3-8 of tests/test_gpu_ray_query_edges.py::ROWS) every hit names a member of the
   float64 tie set, a miss occurs only where no surface is certain, a record that names the oracle's primitive has the
   oracle's t, point and normal bit for bit (the IEEE primitive arithmetic does not depend on the tree), the forms
   agree, and with "exact_decisions" FAST equals EXACT bit for bit;
c. "fast_math" 1 on one compat and one LBVH row: the tie set with margins FM_SCALE times the oracle's, finite records,
   no miss where a surface is certain by those margins;
d. one 128 x 96 frame, depth 3, 4 samples, of the sheet and the spheres: EXACT equals the oracle's float RGB bit for
   bit with equal work counters through both kernels, FAST on the reference's trees too, FAST on LBVH trees within
   the frame bar of tests/test_gpu_parity.py;
e. after rt_scene_update_triangles moved the sheet to x + 1000 (where a float32 ray cannot be aimed at an edge to 1e-6:
   most edge rays hit one triangle only) and a rebuild: (a) and (b) again, against a fresh oracle and fresh rays.

Every comparison in (a), (d, EXACT and compat) and the record fields of (b) is an equality of bits.  The margins of (b)
are the CPU's (prim_edges_ref.MARGINS); FM_SCALE is the one number measured on the GPU (profiles/prim_edges/README.md).

What (a) found ("tmax can grow"; profiles/prim_edges/README.md): rt_trace_rays equalled the oracle on
all 24 640 rays, but rt_query_rays named another triangle of the tie on 9 rays of "sheet_vertex" (indices 2025, 2089,
2127, 2224, 2267, 2275, 2305, 2439, 2960), EXACT and FAST, "wide" 1 and 0 alike, t differing by at most 2.4e-7: the
speculative traversal assumes that tmax only shrinks, and Range::inRange's 1e-6 window lets a later primitive up to
1e-6 BEYOND the closest hit replace it.  The query kernel now traces a ray whose tmax grew a second time, in the
reference's order (csrc/ray_query.hpp), and both reference-tree tests pass on every ray.
"""
import numpy as np
import pytest

import prim_edges_ref as P
from rtamd import Renderer
from test_gpu_lbvh import frac_within
from test_gpu_ray_query import assert_records_equal, closest, occluded
from test_gpu_ray_query_edges import ROWS, check_all_forms, is_hit

pytestmark = pytest.mark.gpu

BUILD_SEED = 5
THREADS = 16
W, H = P.FRAME
# tests/test_gpu_parity.py's bars for FAST frames on other trees: 0.999 at depth 1 and 2, 0.995 at depth 4 and 10; a
# depth-3 frame takes the bar of the deeper ones
FRAME_NEED = 0.995
# "fast_math" (reciprocals for divisions, contracted multiply-adds): its records against float64, on the surfaces they
# name, deviate at most 1.79 x as far as the oracle's do on any class and copy (t 1.47, point 1.36, normal 1.79: the
# largest ratios over the classes, compat and LBVH trees alike, measured on an MI355X: profiles/prim_edges/README.md).
# Its margins are FM_SCALE x the oracle's, which are 4 x the oracle's deviation: 4 x 2.0 >= 4 x 1.79.  One class has
# no deviation of the oracle's to scale — the sliver's flat normal on the identity copy is the same three floats for
# every ray, 1e-8 is its written floor — and fast_math rounds one component the other way (6.0e-8): for a unit
# normal's component no margin is under 4 last bits of a float32 in [0.5, 1), 4 x 2^-24.
FM_SCALE = 2.0
RECORD_FLOOR = {"t": 0.0, "point": 0.0, "normal": 4 * 2.0 ** -24}


class Case:
    def __init__(self, move=0.0):
        from oracle.oracle import OracleScene
        self.move = move
        self.scene = P.scene(move)
        self.oracle = OracleScene(self.scene, build_seed=BUILD_SEED)
        self.rays = P.rays(move)
        self.want = self.oracle.trace(self.rays.world)[0]
        self.want.setflags(write=False)
        self.ev = P.evaluate(self.scene, self.rays, P.margins(move))
        self.own = P.own_instances(self.rays)
        assert P.judge(self.ev, self.want).ok.all()          # the oracle itself (tests/test_prim_edges_ref.py)


@pytest.fixture(scope="module")
def case(gpu_lib, oracle_lib):
    c = Case()
    assert len(c.rays.world) == 24640 and 0.6 < is_hit(c.want).mean() < 0.9
    yield c
    c.oracle.close()


@pytest.fixture(scope="module")
def moved(gpu_lib, oracle_lib):
    c = Case(P.MOVE)
    yield c
    c.oracle.close()


def built(scene, mode, **options):
    r = Renderer(scene, update=False)
    for k, v in options.items():
        r.set_option(k, v)                                   # raises unless the option is accepted
    return r.build_acceleration_structure(BUILD_SEED, mode=mode).configure_camera(W, H)


# ---- a. the reference's trees ----------------------------------------------------------------------------------------
def check_reference_trees(r, c, what, trace=True, query=True):
    for exact in (True, False):
        if trace:
            assert_records_equal(r.trace_rays(c.rays.world, exact=exact), c.want)
        if query:
            check_all_forms(r, c.rays.world, None, c.want, exact, (what, exact))


@pytest.mark.parametrize("wide", [1, 0])
def test_reference_trees_trace_rays(case, wide):
    """rt_trace_rays (trav_step: every decision where the reference takes it): every ray, all 8 fields."""
    r = built(case.scene, "compat", wide=wide)
    check_reference_trees(r, case, wide, query=False)
    r.cleanup()


@pytest.mark.parametrize("wide", [1, 0])
def test_reference_trees_bit_identical(case, wide):
    """rt_query_rays (spec_round, and trav_step once more for a ray whose tmax grew): closest records, t alone and
    any-hit, every ray, all 8 fields."""
    r = built(case.scene, "compat", wide=wide)
    check_reference_trees(r, case, wide, trace=False)
    r.cleanup()


# ---- b. the other kernel instances -----------------------------------------------------------------------------------
def check_tie_sets(r, c, opts, what, ev=None, scale=1.0, forms_agree=True):
    """The forms of one renderer against each other and its records against the float64 tie sets; -> the records.
    forms_agree False ("fast_math": the any-hit, t-only and record instances of the kernel are compiled apart and
    contract their multiply-adds differently): t alone and any-hit are held to the tie sets each on its own."""
    ev = c.ev if ev is None else ev
    rays, want = c.rays.world, c.want
    t, h = closest(r, rays)
    t_only, _ = closest(r, rays, want_hits=False)
    occ = occluded(r, rays)
    assert np.array_equal(is_hit(h), np.isfinite(h["t"])) and np.array_equal(t, h["t"])
    v = P.judge(ev, h)
    if forms_agree:
        assert np.array_equal(occ, np.isfinite(t)), int((occ != np.isfinite(t)).sum())
        assert np.array_equal(t_only, h["t"])
    else:
        apart = (occ != np.isfinite(t)) | (np.isfinite(t_only) != np.isfinite(t))
        print(f"{what}: any-hit or t alone decide otherwise than the records on {int(apart.sum())} rays: "
              f"{np.bincount(c.rays.cls[apart], minlength=len(P.NAMES)).tolist()}")
        for found in (occ, np.isfinite(t_only)):
            assert v.may_miss[~found].all() and ev.possible[found].any(axis=1).all()
    bad = np.flatnonzero(~v.ok)
    same = (h["instance"] == want["instance"]) & (h["pindex"] == want["pindex"]) & (h["ptype"] == want["ptype"])
    print(f"{what}: {len(bad)} rays outside their tie set; the oracle's primitive on {same.mean():.5f} "
          f"({int((~same).sum())} other: {np.bincount(c.rays.cls[~same], minlength=len(P.NAMES)).tolist()})")
    assert bad.size == 0, (what, [(int(i), P.NAMES[c.rays.cls[i]], int(c.rays.copy[i])) for i in bad[:8]])
    # t, point and normal of the named surface's float64 values, within the margins
    sel = np.flatnonzero(is_hit(h))
    point, normal = P.record64(c.scene, rays, ev, np.maximum(v.chosen, 0))
    written = P.margins(c.move)
    mine = c.own[sel, h["instance"][sel]]
    for k, dev in (("t", np.abs(h["t"][sel] - ev.t[sel, v.chosen[sel]])),
                   ("point", np.abs(h["point"][sel] - point[sel]).max(axis=1)),
                   ("normal", np.abs(h["normal"][sel] - normal[sel]).max(axis=1))):
        m = np.asarray([[written[n][cp][k] for cp in (0, 1)] for n in P.NAMES])[c.rays.cls[sel], c.rays.copy[sel]]
        m = np.maximum(scale * np.where(mine, m, written[P.STRAY][k]), RECORD_FLOOR[k] if scale != 1.0 else 0.0)
        assert np.all(dev <= m), (what, k, float((dev / m).max()))
    return h, same


@pytest.fixture(scope="module")
def row_scene(case):
    made = {}

    def get(row):
        if row not in made:
            mode, opts = ROWS[row]
            made[row] = built(case.scene, mode, **opts)
        return made[row]

    yield get
    for r in made.values():
        r.cleanup()


def check_other_trees(r, c, opts, what):
    h, same = check_tie_sets(r, c, opts, what)
    both = same & is_hit(c.want)
    for k in ("t", "point", "normal", "mtype", "midx"):
        assert np.array_equal(h[k][both], c.want[k][both]), (what, k)
    assert both.sum() > 0.5 * is_hit(c.want).sum()           # (another tree may name the other side of any tie)
    if opts.get("exact_decisions"):
        te, he = closest(r, c.rays.world, exact=True)
        assert_records_equal(h, he)
        assert np.array_equal(h["t"], te)
        assert np.array_equal(occluded(r, c.rays.world), occluded(r, c.rays.world, exact=True))


@pytest.mark.parametrize("row", [3, 4, 5, 6, 7, 8])
def test_other_kernel_instances(case, row_scene, row):
    check_other_trees(row_scene(row), case, ROWS[row][1], f"row {row}")


# ---- c. fast_math ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fm_eval(case):
    written = P.margins()
    scaled = {n: ([{k: FM_SCALE * v for k, v in d.items()} for d in rows] if n != P.STRAY else
                  {k: FM_SCALE * v for k, v in rows.items()}) for n, rows in written.items()}
    return P.evaluate(case.scene, case.rays, scaled)


@pytest.mark.parametrize("row", [1, 5])
def test_fast_math(case, fm_eval, row):
    mode, opts = ROWS[row]
    r = built(case.scene, mode, **opts)
    r.set_option("fast_math", 0)
    _, base = closest(r, case.rays.world)
    r.set_option("fast_math", 1)
    h, _ = check_tie_sets(r, case, opts, f"fast_math row {row}", ev=fm_eval, scale=FM_SCALE, forms_agree=False)
    hit = is_hit(h)
    assert np.isfinite(h["t"][hit]).all() and np.isfinite(h["point"][hit]).all() and np.isfinite(h["normal"][hit]).all()
    assert (h["t"] != base["t"]).any()                       # the fast-math kernel ran: other roundings somewhere
    r.cleanup()


# ---- d. one frame ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame(case):
    s = case.scene
    assert s.camera["ray_trace_depth"] == 3 and s.camera["sample_count"] == 4
    case.oracle.camera(W, H)
    orgb, orgba, ocnt = case.oracle.render(threads=THREADS)
    assert ocnt["rays"] > 4 * W * H + 10000 and ocnt["triangle_tests"] > 10000     # bounces; the sheet is in view
    return orgb, orgba, ocnt


@pytest.mark.parametrize("kernel", [1, 0])
def test_frame_on_reference_trees_bit_identical(case, frame, kernel):
    orgb, orgba, ocnt = frame
    r = built(case.scene, "compat")
    r.set_option("kernel", kernel)
    _, rgb, st = r.render(0, exact=True, want_rgb=True, count_work=True)
    assert np.array_equal(rgb, orgb), (int((rgb != orgb).any(axis=2).sum()), float(np.abs(rgb - orgb).max()))
    for k in ("rays", "triangle_tests", "sphere_quad_tests"):
        assert st[k] == ocnt[k], (k, st[k], ocnt[k])
    _, frgb, _ = r.render(0, want_rgb=True)
    assert np.array_equal(frgb, orgb), (int((frgb != orgb).any(axis=2).sum()), float(np.abs(frgb - orgb).max()))
    r.cleanup()


def test_fast_frame_on_lbvh_trees(case, frame):
    _, orgba, _ = frame
    r = built(case.scene, "lbvh")
    rgba, _, _ = r.render(0)
    f, mx = frac_within(rgba, orgba)
    print(f"FAST on LBVH trees: within 1 LSB {f:.5f} (max {mx})")
    assert f >= FRAME_NEED, (f, mx)
    r.cleanup()


# ---- e. a rebuild ----------------------------------------------------------------------------------------------------
def test_rebuild_with_the_sheet_moved(case, moved):
    """rt_scene_update_triangles with the sheet's 128 triangles at x + 1000 (and rt_scene_update_instances with the
    bounds that go with them), a frame update that rebuilds, then (b) against the moved scene's oracle — on the trees
    the GPU rebuilt, with and without cold records — and (a) on the reference's trees of the moved scene."""
    first = P.TRI_FIRST["sheet"]
    tris = moved.scene.triangles[first:first + 128]
    assert np.all(tris["vertex"][..., 0] > 990) and np.array_equal(tris["vertex"][..., 1:],
                                                                   case.scene.triangles["vertex"][first:first + 128, :, 1:])
    for row in (7, 6):
        mode, opts = ROWS[row]
        r = built(case.scene, mode, **opts)
        r.update(0)
        r.update_triangles(first, tris)
        r.update_instances(0, P.instance_dicts(P.MOVE))
        r.update(1)
        check_other_trees(r, moved, opts, f"moved, row {row}")
        r.cleanup()
    for wide in (1, 0):
        r = built(moved.scene, "compat", wide=wide)
        check_reference_trees(r, moved, ("moved", wide))
        r.cleanup()
