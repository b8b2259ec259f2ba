"""Traversal-stack paging and the GPU builder on chains and ties, on the two deep scenes of tests/deep_tree_ref.py.

Every trace kernel keeps 16 stack entries per lane in LDS and pages half-windows to scratch (csrc/stack.hpp,
struct Stack: stack_page_out from stack_push and from the quad step's three-entry push, stack_page_in).  On these scenes the GPU-built trees are chains 29 (BLAS)
and 10 + 29 (TLAS + BLAS) levels deep with equal Morton codes in them; tests/test_deep_tree_ref.py shows with a CPU model
that 99 % of the rays page out once, 72 % / 99 % twice or more, 46 % take their closest hit from an entry that came back
through a page-in, and that no kernel form can reach the 64-entry capacity (nothing here may report an overflow).

* builder: the exported BLAS / TLAS equal the numpy restatement (tests/lbvh_ref.py) bit for bit on chains with ties —
  the <= 2048-item LDS path, karras_kernel's tie rule, the one-workgroup TLAS and the multi-kernel TLAS;
* per-ray records of rt_trace_rays and rt_query_rays against the oracle's tree-free trace (brute_force=2), on every
  unambiguous ray (deep_tree_ref.ambiguous: <= 2 % of the rays, asserted on the CPU), through every stack site:
  EXACT binary pairs, FAST binary pairs ("wide" 0), FAST quads with and without "exact_decisions", "fast_math";
* the same comparisons on a "compat" build of the same scene, whose balanced trees never page: a failure on the deep
  build alone is a paging or builder bug, a failure on both is something else;
* frames through the grid and persistent render kernels against the oracle's frame, and byte identity between
  configurations that traverse the same trees with the same arithmetic.
"""
import numpy as np
import pytest

import deep_tree_ref as D
from lbvh_ref import assert_tree_equal, check_tree, lbvh_tree
from rtamd import Renderer, abi
from test_gpu_lbvh import PAIR_DT, QUAD_DT, ROOT_DT, _expected_quads, frac_within
from test_gpu_ray_query import closest, occluded

pytestmark = pytest.mark.gpu

THREADS = 16
SAME_SURFACE = 0.999         # the project tolerance for "fast_math" 1 (tests/test_gpu_ray_query_edges.py)
DT_REL = 1e-4
W, H = 160, 90
IDS = ("instance", "pindex", "ptype", "mtype", "midx")
CASES = ["deep_blas", "deep_two_level"]
# build mode, options set before the build; every option here is accepted on these builds (set_option raises otherwise)
BUILDS = {
    "lbvh-quads": ("lbvh", {"group": 0, "wide": 1, "exact_decisions": 0}),
    "lbvh-quads-exact-decisions": ("lbvh", {"group": 0, "wide": 1, "exact_decisions": 1}),
    "lbvh-pairs": ("lbvh", {"group": 0, "wide": 0}),
    "compat-control": ("compat", {"group": 0}),
}


@pytest.fixture(scope="module", params=CASES)
def case(request, gpu_lib, oracle_lib):
    return D.case(request.param)


def build(case, mode, opts):
    r = Renderer(case.scene)
    for k, v in opts.items():
        r.set_option(k, v)
    return r.build_acceleration_structure(0, mode=mode)


# ---- a. the builder on chains and ties ---------------------------------------------------------------------------------
def test_blas_equals_restatement(case):
    """The soup's BLAS (93 items, 31 distinct Morton codes: the <= 2048-item path) equals lbvh_tree bit for bit — node
    boxes, count / index, leaf order — with the restatement's height, after the build and again after two frames of
    per-frame rebuilds; its quads equal the collapse rule applied to the GPU's own pairs."""
    r = build(case, "lbvh", {"group": 0}).configure_camera(W, H)
    want = case.blas
    height = check_tree(*want, case.boxes, D.BLAS_LEAF)
    assert r.info()["blas_count"] == 1
    for rebuilt in (0, 1):
        if rebuilt:
            r.set_option("rebuild", 1)
            r.render(0)
            r.render(1)
        got = r.export_blas(0)
        assert_tree_equal(got, want, rebuilt)
        assert check_tree(*got, case.boxes, D.BLAS_LEAF) == height
        assert r.info()["blas_height_max"] == height
        pairs = r.debug_read("blas_pairs").view(PAIR_DT)
        quads = r.debug_read("blas_quads").view(QUAD_DT)
        roots = r.debug_read("blas_roots").view(ROOT_DT)
        assert len(roots) == 1 and int(roots[0]["height"]) == height
        expected = _expected_quads(pairs, int(roots[0]["ref"]))
        assert len(expected) >= height // 2
        for q, (box, ref) in expected.items():
            g = quads[q]
            assert list(g["ref"]) == ref, (rebuilt, q)
            for k in range(4):
                have = [g["lo_x"][k], g["hi_x"][k], g["lo_y"][k], g["hi_y"][k], g["lo_z"][k], g["hi_z"][k]]
                assert np.array_equal(np.asarray(have, np.float32), box[k]), (rebuilt, q, k)
    r.cleanup()


def test_tlas_equals_restatement(gpu_lib, oracle_lib):
    """deep_two_level: the GPU TLAS over 12 instances whose centroids form a Morton chain with one tie equals
    lbvh_tree(instance world boxes, centroids, 1) of the GPU's own instance records, with its height, built by one
    workgroup ("tlas_small" 1) and by the multi-kernel builder (0); both exports are identical.

    One instance per leaf, not the reference's two: GPU-built TLASes use the library's fixed setting "tlas_leaf" = 1
    (csrc/scene.hpp: a leaf's instances are entered without a box test of their own, so single-instance leaves
    measured best); TLAS_LEAF_CAP = 2 is the host builders' leaf size.  With 2 the restatement merges the tied pair and
    the chain's last two instances into leaves the GPU tree does not have."""
    c = D.case("deep_two_level")
    r = build(c, "lbvh", {"group": 0}).configure_camera(W, H)
    out = {}
    for small in (1, 0):
        r.set_option("tlas_small", small)
        r.update(small)                                      # the scene is static: another frame number, the same TLAS
        rec = r.debug_read("instances").view(np.float32).reshape(-1, 45)
        assert np.array_equal(rec, c.oracle.instance_state())        # the records the CPU conditions were checked on
        want = lbvh_tree(rec[:, 36:42], rec[:, 42:45], D.TLAS_LEAF)
        height = check_tree(*want, rec[:, 36:42], D.TLAS_LEAF)
        assert height >= 10
        out[small] = r.export_tlas()
        assert_tree_equal(out[small], want, small)
        assert r.info()["tlas_height"] == height
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    r.cleanup()


# ---- b. per-ray records through every stack site -----------------------------------------------------------------------
def same_surface(got, want):
    return (got["instance"] == want["instance"]) & (got["pindex"] == want["pindex"])


def assert_ids(got, want, ok, what):
    for k in IDS:
        bad = ok & (got[k] != want[k])
        assert not bad.any(), (what, k, int(bad.sum()), np.flatnonzero(bad)[:8])


def check_against(got, want, ok, what, bit_equal_t):
    """Records `got` against the oracle's `want` on the rays `ok`: the same surface and material, and t bit-equal."""
    assert_ids(got, want, ok, what)
    assert np.array_equal(np.isfinite(got["t"]), got["instance"] != abi.MISS), what
    if bit_equal_t:
        bad = ok & (got["t"] != want["t"])
        with np.errstate(invalid="ignore"):
            rel = np.abs(got["t"][bad] - want["t"][bad]) / want["t"][bad]
        assert not bad.any(), (what, "t", int(bad.sum()), "largest |dt| / t", float(np.nanmax(rel)))


@pytest.mark.parametrize("name", sorted(BUILDS))
def test_records_equal_tree_free_oracle(case, name):
    """rt_trace_rays (EXACT, FAST) and rt_query_rays (closest records, t-only, any-hit; RT_QUERY_EXACT and not) on one
    build: on every unambiguous ray instance, pindex, ptype and the material equal the oracle's tree-free record, and t
    is bit-equal — EXACT, and FAST with "fast_math" 0 as well (README: correctly rounded arithmetic for every value
    that reaches a hit).  occluded == isfinite(t) on every ray, ambiguous ones included.  Ranged queries: tmax = 2 t
    leaves the record unchanged; tmax = 0.5 t and tmax = 0.999 t (the range that ends a deep traversal with nothing
    found, tests/test_deep_tree_ref.py::test_ranged_rays_still_page) equal the oracle's ranged tree-free trace.
    With "fast_math" 1, t is held to DT_REL = 1e-4 on >= 99.9 % same-surface rays, the project's existing bound.

    "compat-control" runs the same comparisons on balanced trees that never page (module docstring)."""
    mode, opts = BUILDS[name]
    r = build(case, mode, opts)
    rays, want, ok = case.rays, case.want, ~case.ambiguous
    hit = want["instance"] != abi.MISS
    assert hit.mean() >= 0.99 and ok.mean() >= 0.98
    r.set_option("fast_math", 0)
    for exact in (True, False):
        what = (name, "exact" if exact else "fast")
        check_against(r.trace_rays(rays, exact=exact), want, ok, what + ("trace_rays",), True)
        t, h = closest(r, rays, exact=exact)
        check_against(h, want, ok, what + ("query",), True)
        assert np.array_equal(t, h["t"]), what
        t_only, _ = closest(r, rays, exact=exact, want_hits=False)
        assert np.array_equal(t_only, t), what
        assert np.array_equal(occluded(r, rays, exact=exact), np.isfinite(t)), what
        # ranged
        far = np.where(hit, np.float32(2.0) * want["t"], np.float32(10.0)).astype(np.float32)
        t2, h2 = closest(r, rays, far, exact=exact)
        for k in IDS + ("t", "point", "normal"):
            assert np.array_equal(h2[k][ok], h[k][ok]), what + ("tmax = 2 t", k)
        assert np.array_equal(occluded(r, rays, far, exact=exact), np.isfinite(t2)), what
        for f in (0.5, D.NEAR_MISS):
            near = np.where(hit, np.float32(f) * want["t"], np.float32(10.0)).astype(np.float32)
            ranged = case.oracle.trace(rays, brute_force=2, tmax=near)[0]
            assert (ranged["instance"][ok] == abi.MISS).all()        # nothing lies in front of an unambiguous hit
            tn, hn = closest(r, rays, near, exact=exact)
            check_against(hn, ranged, ok, what + (f"tmax = {f} t",), True)
            assert np.array_equal(tn, hn["t"])
            assert np.array_equal(occluded(r, rays, near, exact=exact), np.isfinite(tn)), what
    # the fast-math flavour: the project's tolerance against the oracle
    r.set_option("fast_math", 1)
    got = r.trace_rays(rays)
    t, h = closest(r, rays)
    for g, api in ((got, "trace_rays"), (h, "query")):
        same = same_surface(g, want)
        both = same & ok & hit
        rel = np.abs(g["t"][both] - want["t"][both]) / want["t"][both]
        print(f"{case.name} {name} fast_math {api}: same surface {same[ok].mean():.5f}, max |dt|/t {rel.max():.3g}")
        assert same[ok].mean() >= SAME_SURFACE, (name, api, same[ok].mean())
        assert np.all(rel <= DT_REL), (name, api, float(rel.max()))
        for k in ("ptype", "mtype", "midx"):
            assert np.array_equal(g[k][same & ok], want[k][same & ok]), (name, api, k)
    assert np.array_equal(occluded(r, rays), np.isfinite(t)), name
    r.cleanup()


# ---- c. frames through the render kernels ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_frame(case):
    from oracle.oracle import OracleScene
    o = OracleScene(case.scene, build_seed=0)
    o.camera(W, H)
    _, rgba, cnt = o.render(threads=THREADS)
    rgba.setflags(write=False)
    return rgba, cnt


def test_frames_within_fast_bar(case, oracle_frame):
    """160 x 90, ray_trace_depth 2 (bounce rays start on surfaces inside the overlap), camera on the soup: the grid and
    persistent kernels on binary pairs and quads, EXACT and FAST, stay within the project's FAST bar of the oracle's
    frame — >= 99.9 % of pixels within 1 LSB, the ray count within 0.1 % — and count_work raises on a stack overflow.
    EXACT traverses the binary pairs in both kernels: "kernel" 0 and 1 are byte-identical, whatever "wide" is."""
    orgba, ocnt = oracle_frame
    r = build(case, "lbvh", {"group": 0}).configure_camera(W, H)
    exact_frames = []
    for kernel in (0, 1):
        for wide in (0, 1):
            r.set_option("kernel", kernel).set_option("wide", wide)
            for exact in (True, False):
                rgba, _, st = r.render(0, exact=exact, count_work=True)          # raises RT_ERR_UNSUPPORTED on an overflow
                f, mx = frac_within(rgba, orgba)
                print(f"{case.name} kernel {kernel} wide {wide} exact {exact}: within 1 LSB {f:.5f} (max {mx}), "
                      f"rays {st['rays']} / {ocnt['rays']}")
                assert f >= 0.999, (kernel, wide, exact, f, mx)
                assert abs(st["rays"] - ocnt["rays"]) <= 0.001 * ocnt["rays"], (kernel, wide, exact)
                if exact:
                    exact_frames.append(((kernel, wide), rgba, st["rays"]))
    for key, rgba, n in exact_frames[1:]:
        assert np.array_equal(rgba, exact_frames[0][1]) and n == exact_frames[0][2], key
    r.cleanup()


@pytest.mark.parametrize("exact", [False, True])
def test_schedule_options_byte_identical(case, exact):
    """What changes which wave traces which pixel, not what a pixel computes, stays byte-identical on deep trees too,
    as tests/test_gpu_parity.py asserts on shallow ones: "reorder" 1 against 0 over the launches that record costs and
    the ones that claim in the recorded order, and three overlapped lanes against the serial frames."""
    import torch
    F = 6
    r = build(case, "lbvh", {"group": 0}).configure_camera(W, H)
    r.set_option("reorder", 0)
    ref = [r.render(f, exact=exact, count_work=True) for f in range(F)]
    r.set_option("reorder", 1)
    for f in range(F):
        rgba, _, st = r.render(f, exact=exact, count_work=True)
        assert np.array_equal(rgba, ref[f][0]) and st["rays"] == ref[f][2]["rays"], f
    r.collect()
    r.set_option("overlap", 3)
    lanes = [torch.cuda.Stream() for _ in range(3)]
    bufs = [torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda") for _ in range(F)]
    torch.cuda.synchronize()
    for f in range(F):
        r.render(f, exact=exact, want_rgba=False, rgba8_device=bufs[f].data_ptr(), stream=lanes[f % 3].cuda_stream,
                 sync=False, count_work=True, keep_counters=f > 0)
    acc, _ = r.collect()
    torch.cuda.synchronize()
    for f in range(F):
        assert np.array_equal(bufs[f].cpu().numpy().reshape(H, W, 4), ref[f][0]), f
    assert acc["rays"] == sum(x[2]["rays"] for x in ref)
    r.cleanup()
