"""Instance transforms at their edges on the GPU: the 22 classes of tests/xform_edges_ref.py (quarter turns, wrapped
angles, mirrors, anisotropic scales, scales of 1e-3 and 1e3, near-singular and singular matrices), 66 instances in one
scene, 26 400 rays.  tests/test_oracle_xform_edges.py holds the oracle to a float64 reference on the same scene and
rays; here the GPU is held to the oracle:

a. the instance records (csrc/instances.hip: hm::inverse with its pivot search, both singular exits, the transformed
   box) equal the oracle's bit for bit, on the LBVH build and under "gpu_tlas" over SAH BLASes;
b. the GPU's TLAS over those boxes — some without extent, one 1e3 times the usual one — equals the restatement
   (tests/lbvh_ref.py), from the one-workgroup and from the multi-kernel builder;
c. on the reference's trees every ray's record equals the oracle's in all 8 fields, EXACT and FAST, "wide" 1 and 0,
   as closest records, t alone, any-hit and rt_trace_rays;
d. on the six other kernel instances (ROWS 3-8 of tests/test_gpu_ray_query_edges.py) the forms agree with one
   another on every ray, FAST equals EXACT bit for bit where "exact_decisions" is set, and the rays of the regular
   classes and "huge" meet the project tolerance against the oracle;
e. frames of the all-metal scene (normals carried into two more segments): EXACT bit-identical on the reference's
   trees with equal work counters, FAST on LBVH trees within the bar of tests/test_gpu_lbvh.py;
f. every instance changing class every frame through rt_scene_update_instances, through singular transforms and back
   (the schedule's conditions: tests/test_oracle_xform_edges.py): the records of each frame equal a fresh oracle's,
   FAST equals EXACT, and on the reference's trees the hits do.

(c) and (d) also trace 432 rays along the world axes at the quarter- and half-turn classes, whose local directions
have the +-4e-8 components that cos 90 deg leaves, under the reference's 1e-6 "parallel" threshold.

Everything in (a), (c), (f) and on rows 7-8 is an equality of bits.  The only tolerances are the project's: the same
(instance, pindex) on >= 99.9 % of rays with |dt| <= 1e-4 t on those (tests/test_gpu_ray_query_edges.py), and
frac_within >= 0.999 for a frame (tests/test_gpu_lbvh.py::test_lbvh_images_within_tolerance).

Measured on an MI355X (profiles/xform_edges/README.md): rows 3-8 name the oracle's surface on every one of the 19 200
pooled rays, with the oracle's t.
"""
import numpy as np
import pytest

import lbvh_sizes_ref as S
import xform_edges_ref as X
from lbvh_ref import assert_tree_equal, check_tree
from rtamd import Renderer
from test_gpu_lbvh import frac_within
from test_gpu_ray_query import assert_records_equal, closest, occluded
from test_gpu_ray_query_edges import DT_REL, ROWS, SAME_SURFACE, check_all_forms, is_hit

pytestmark = pytest.mark.gpu

BUILD_SEED = 5
THREADS = 16
W, H = X.FRAME
FRAMES = X.FRAMES
FRAME_NEED = 0.999           # tests/test_gpu_lbvh.py::test_lbvh_images_within_tolerance at depth 2


class Case:
    def __init__(self):
        from oracle.oracle import OracleScene
        self.scene = X.scene()
        self.oracle = OracleScene(self.scene, build_seed=BUILD_SEED)
        self.rays, self.aimed = X.rays()
        self.want = self.oracle.trace(self.rays)[0]
        self.want.setflags(write=False)
        group = np.array([X.group_of(d["cls"]) for d in self.scene.instances])[self.aimed]
        cls = np.array([d["cls"] for d in self.scene.instances])[self.aimed]
        self.pooled = (group == "regular") | (cls == "huge")
        self.axis_rays, _ = X.axis_rays()                    # local components of +-4e-8: under the parallel threshold
        self.axis_want = self.oracle.trace(self.axis_rays)[0]
        self.axis_want.setflags(write=False)


@pytest.fixture(scope="module")
def case(gpu_lib, oracle_lib):
    c = Case()
    assert len(c.rays) == 26400 and c.pooled.sum() == 16 * 1200
    assert is_hit(c.want)[c.pooled].mean() > 0.99 and is_hit(c.axis_want).mean() > 0.95
    yield c
    c.oracle.close()


def records(r):
    return r.debug_read("instances").view(np.uint32).reshape(-1, 45)


def built(scene, mode, **options):
    r = Renderer(scene, update=False)
    for k, v in options.items():
        r.set_option(k, v)                                   # raises unless the option is accepted
    return r.build_acceleration_structure(BUILD_SEED, mode=mode).configure_camera(W, H)


# ---- a. records ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,options", [("lbvh", {"group": 0}), ("sah", {"gpu_tlas": 1})])
def test_records_equal_the_oracle(case, mode, options):
    r = built(case.scene, mode, **options)
    r.update(0)
    got, want = records(r), case.oracle.instance_state().view(np.uint32)
    assert got.shape == (66, 45)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [(int(k), case.scene.instances[k]["cls"], np.flatnonzero(got[k] != want[k])) for k in bad[:6]]
    r.cleanup()


# ---- b. TLAS ---------------------------------------------------------------------------------------------------------
def test_tlas_equals_restatement(case):
    r = built(case.scene, "lbvh", group=0)
    out = {}
    for frame, small in enumerate((1, 0)):
        r.set_option("tlas_small", small)
        r.update(1 + frame)
        rec = records(r).view(np.float32)
        assert np.array_equal(rec.view(np.uint32), case.oracle.instance_state().view(np.uint32))
        want, height = S.restate_tlas(rec)
        out[small] = r.export_tlas()
        assert_tree_equal(out[small], want, small)
        assert check_tree(*out[small], rec[:, 36:42], S.TLAS_LEAF) == height == r.info()["tlas_height"]
        assert r.info()["tlas_node_pairs"] == 65
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    r.cleanup()


# ---- c. the reference's trees ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [1, 0])
def test_reference_trees_bit_identical(case, wide):
    r = built(case.scene, "compat", wide=wide)
    for exact in (True, False):
        check_all_forms(r, case.rays, None, case.want, exact, (wide, exact))
        assert_records_equal(r.trace_rays(case.rays, exact=exact), case.want)
        check_all_forms(r, case.axis_rays, None, case.axis_want, exact, (wide, exact, "axis"))
        assert_records_equal(r.trace_rays(case.axis_rays, exact=exact), case.axis_want)
    r.cleanup()


# ---- d. the other kernel instances -----------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [3, 4, 5, 6, 7, 8])
def test_other_kernel_instances(case, row):
    mode, opts = ROWS[row]
    r = built(case.scene, mode, **opts)
    t, h = closest(r, case.rays)
    t_only, _ = closest(r, case.rays, want_hits=False)
    occ = occluded(r, case.rays)
    assert np.array_equal(is_hit(h), np.isfinite(h["t"]))
    assert np.array_equal(occ, np.isfinite(t)), int((occ != np.isfinite(t)).sum())
    assert np.array_equal(t, h["t"]) and np.array_equal(t_only, h["t"])
    if opts.get("exact_decisions"):
        te, he = closest(r, case.rays, exact=True)
        assert_records_equal(h, he)
        assert np.array_equal(t, te)
        assert np.array_equal(occ, occluded(r, case.rays, exact=True))
        assert_records_equal(closest(r, case.axis_rays)[1], closest(r, case.axis_rays, exact=True)[1])
    ha = closest(r, case.axis_rays)[1]
    same_axis = (ha["instance"] == case.axis_want["instance"]) & (ha["pindex"] == case.axis_want["pindex"])
    print(f"row {row}: axis rays, same surface as the oracle {same_axis.mean():.5f}")
    assert same_axis.mean() >= SAME_SURFACE, same_axis.mean()
    want = case.want
    same = (h["instance"] == want["instance"]) & (h["pindex"] == want["pindex"])
    p = case.pooled
    both = same & is_hit(want) & p
    rel = np.abs(h["t"][both] - want["t"][both]) / want["t"][both]
    print(f"row {row}: same surface as the oracle {same[p].mean():.5f} of the pooled rays ({int((~same[p]).sum())} "
          f"other), max |dt|/t {rel.max():.3g}; all classes {same.mean():.5f} ({int((~same).sum())} other)")
    assert same[p].mean() >= SAME_SURFACE, same[p].mean()
    assert np.all(rel <= DT_REL), rel.max()
    assert np.all(h["t"][same & ~is_hit(want) & p] == np.inf)
    r.cleanup()


# ---- e. frames -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def metal_frame(oracle_lib):
    from oracle.oracle import OracleScene
    s = X.scene(metal=True)
    assert s.camera["ray_trace_depth"] == 3 and s.camera["sample_count"] == 1
    o = OracleScene(s, build_seed=BUILD_SEED)
    o.camera(W, H)
    orgb, orgba, ocnt = o.render(threads=THREADS)
    o.close()
    assert ocnt["rays"] > W * H + 2000                       # mirrors in view: their normals aim the next segments
    return s, orgb, orgba, ocnt


@pytest.mark.parametrize("kernel", [1, 0])
def test_exact_frame_bit_identical(gpu_lib, metal_frame, kernel):
    s, orgb, orgba, ocnt = metal_frame
    r = built(s, "compat")
    r.set_option("kernel", kernel)
    _, rgb, st = r.render(0, exact=True, want_rgb=True, count_work=True)
    assert np.array_equal(rgb, orgb), (int((rgb != orgb).any(axis=2).sum()), float(np.abs(rgb - orgb).max()))
    assert st["rays"] == ocnt["rays"] and st["triangle_tests"] == ocnt["triangle_tests"]
    r.cleanup()


def test_fast_frame_on_lbvh_trees(gpu_lib, metal_frame):
    s, _, orgba, _ = metal_frame
    r = built(s, "lbvh")
    rgba, _, _ = r.render(0)
    f, mx = frac_within(rgba, orgba)
    print(f"FAST on LBVH trees: within 1 LSB {f:.5f} (max {mx})")
    assert f >= FRAME_NEED, (f, mx)
    r.cleanup()


# ---- f. moving between classes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["lbvh", "compat"])
def test_moving_between_classes(case, mode):
    from oracle.oracle import OracleScene
    r = built(case.scene, mode, **({"group": 0, "exact_decisions": 1} if mode == "lbvh" else {}))
    for frame in range(FRAMES):
        a = X.assignment(frame)
        r.update_instances(0, X.instance_dicts(a))
        r.update(frame)
        fresh = OracleScene(X.scene(assign=a), build_seed=BUILD_SEED)
        fresh.update(frame)
        if mode == "lbvh":
            got, want = records(r), fresh.instance_state().view(np.uint32)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (frame, [(int(k), X.NAMES[a[k]]) for k in bad[:6]])
            t, h = closest(r, case.rays)
            te, he = closest(r, case.rays, exact=True)
            assert_records_equal(h, he)
            assert np.array_equal(t, te)
            assert is_hit(h).sum() > 5000
        else:
            want = fresh.trace(case.rays)[0]
            assert is_hit(want).sum() > 5000
            assert_records_equal(r.trace_rays(case.rays, exact=True), want)
        fresh.close()
    r.cleanup()
