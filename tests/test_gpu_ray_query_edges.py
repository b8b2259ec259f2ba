"""rt_query_rays at the places tests/test_gpu_ray_query.py leaves open: range bounds on and around a hit, degenerate
rays, every kernel instance, and the call shapes around the work queue's bands.

The reference everywhere is the oracle on the CPU (oracle.OracleScene.trace, with tmax: oracle_trace_range, pinned by
tests/test_oracle_kat.py), computed once per module.  On the reference's trees (compat build) every comparison is
"all rays, all 8 fields, bit for bit".  The only tolerances in this file are the project's for SAH / LBVH trees against
the oracle, as tests/test_gpu_ray_query.py and tests/test_gpu_parity.py state it — the same (instance, pindex) on
>= 99.9 % of rays and |dt| <= 1e-4 t on those — and the measured "fast_math" bound of test_every_kernel_instance.
"""
import ctypes as C

import numpy as np
import pytest

import ray_query_ref as R
from rtamd import Renderer, abi
from rtamd.renderer import hits_to_numpy
from test_gpu_ray_query import (BUILD_SEED, FIELDS, N_RAYS, ao, assert_records_equal, closest, compat,  # noqa: F401
                                gen_rays, occluded, ref)      # ref, compat, ao: that module's fixtures, one copy here

pytestmark = pytest.mark.gpu

SAME_SURFACE = 0.999         # the project tolerance on SAH / LBVH trees (module docstring)
DT_REL = 1e-4


def is_hit(h):
    return h["instance"] != abi.MISS


def check_all_forms(r, rays, tmax, want, exact, what):
    """Closest records (8 fields), t beside them, t alone and occluded: all equal to the oracle's records `want`."""
    t, h = closest(r, rays, tmax, exact=exact)
    for k in FIELDS:
        assert np.array_equal(h[k], want[k]), (what, k, int((h[k] != want[k]).sum()))
    assert np.array_equal(t, want["t"]), what
    t_only, none = closest(r, rays, tmax, exact=exact, want_hits=False)
    assert none is None and np.array_equal(t_only, want["t"]), what
    assert np.array_equal(occluded(r, rays, tmax, exact=exact), is_hit(want)), what


def slab_keeps(box, ray, tmax):
    """BoundingBox::hit (BoundingBox.cu:34-72) of one box {xmin, xmax, ymin, ymax, zmin, zmax} over [0.001, tmax]."""
    from oracle.oracle import lib
    box, ray = np.ascontiguousarray(box, np.float32), np.ascontiguousarray(ray, np.float32)
    rg, te = np.asarray([0.001, tmax], np.float32), np.zeros(1, np.float32)
    return bool(lib().oracle_hit_aabb(box.ctypes.data, ray.ctypes.data, rg.ctypes.data, te.ctypes.data))


# ---- B1. tmax on, beside, inside and outside the 1e-6 window around a hit -------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
def test_tmax_boundaries(ref, compat, exact):
    """rt.h: the range is "[0.001, tmax[i]] with the reference's range test (Range.cuh:33-43)" — closed, with a 1e-6
    window at both ends — and on the reference's trees the query is bit-identical to the reference.  tmax = t_c, one
    ulp either side, t_c +- 5e-7 (inside the window) and t_c +- 2e-6 (outside), t_c the oracle's closest hit; every ray,
    every field, closest / t-only / any-hit, against the ranged oracle."""
    tc = ref.hits["t"]
    for name, tmax in R.boundary_tmax(tc, ref.hit).items():
        want = ref.oracle.trace(ref.rays, tmax=tmax)[0]
        got = is_hit(want)
        assert not got[~ref.hit].any()
        if name == "minus_5e-7":                 # the window at work: accepted hits beyond tmax
            assert (got & (want["t"] > tmax)).sum() > 1000
        if name == "minus_2e-6":                 # outside the window: misses; where 2e-6 is under half an ulp of t_c,
            assert (ref.hit & ~got).sum() > 1000 and got.sum() > 50      # tmax rounds to t_c and the hit stays
            assert np.all(want["t"][got] <= tmax[got] + np.float32(1e-6))
        if name in ("t_c", "next_up"):           # BoundingBox::hit culls at entry >= tmax what the window would accept
            assert 0 < (ref.hit & ~got).sum() < 100
        check_all_forms(compat, ref.rays, tmax, want, exact, name)


@pytest.mark.parametrize("exact", [True, False])
def test_tmax_boundaries_rays_from_surfaces(ref, compat, ao, exact):
    """The same promise for rays that start on a surface (the ambient-occlusion rays): the boundary set around their
    closest hit, and tmax at the lower end of the range — 0.001 itself is rt.h's "!(tmax > 0.001) is a miss and is not
    traversed", one ulp above it the range is a point with its windows."""
    rays, free = ao
    hit = is_hit(free)
    cases = R.boundary_tmax(free["t"], hit)
    cases.update({"tmin_%d" % i: np.full(len(rays), v, np.float32) for i, v in enumerate(R.TMIN_TMAX)})
    for name, tmax in cases.items():
        want = ref.oracle.trace(rays, tmax=tmax)[0]
        if name == "minus_5e-7":
            assert (is_hit(want) & (want["t"] > tmax)).sum() > 1000
        if name == "tmin_0":
            assert not is_hit(want).any()
        if name == "tmin_3":
            assert is_hit(want).sum() > 10       # hits within a millimetre of the surface the ray left
        check_all_forms(compat, rays, tmax, want, exact, name)


# ---- B2. degenerate rays through TLAS -> instance transform -> BLAS -> primitive ------------------------------------
@pytest.fixture(scope="module")
def degenerate(ref):
    """{class: (rays, oracle records)} — built from gen_rays so that the oracle keeps plenty of hits."""
    o = ref.oracle
    boxes, ci, _ = o.export_tlas()
    leaves = boxes[(ci[:, 0] > 0) & (np.abs(boxes[:, 2:4]).max(1) < 100)]       # instance boxes; not the ground's
    ground = np.asarray([[-4, 4, 0, 0, -4, 4]], np.float32)                     # the ground sphere's top: y = 0
    down = R.down_rays(5000, 21)
    state = o.instance_state()
    fwd = state[:, 12:24].reshape(-1, 3, 4)
    centres = [fwd[i] @ np.asarray(tuple(ref.scene.spheres[d["index"]][2]) + (1.0,), np.float32)
               for i, d in enumerate(ref.scene.instances) if d["type"] == abi.SPHERE]
    pbox = state[[i for i, d in enumerate(ref.scene.instances) if d.get("count", 0) > 1], 36:42]
    cloud = [pbox[:, 0].min(), pbox[:, 1].max(), pbox[:, 2].min(), pbox[:, 3].max(), pbox[:, 4].min(), pbox[:, 5].max()]
    sets = {
        "zero_components": R.zero_component_rays(ref.rays),
        "sub_threshold": R.sub_threshold_rays(ref.rays),
        "straight_down": np.concatenate([down, R.on_box_faces(down, np.concatenate([ground, leaves]))]),
        "unnormalised": R.scaled_rays(ref.rays),
        "inside": R.inside_rays(ref.rays, centres, cloud, ref.hits, ref.hit),
    }
    out = {}
    for k, rays in sets.items():
        want = o.trace(rays)[0]
        want.setflags(write=False)
        out[k] = (rays, want)
    return out


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("cls", ["zero_components", "sub_threshold", "straight_down", "unnormalised", "inside"])
def test_degenerate_rays(compat, degenerate, cls, exact):
    """rt.h: rays are "used as given (not normalised)", hits_device[i] "is exactly the record rt_trace_rays writes",
    and on the reference's trees both are the reference's hit bit for bit — also for the rays tests/test_gpu_box.py
    pins on one box only: zero and sub-1e-6 direction components (BoundingBox.cu's parallel-axis rule), origins exactly
    on box planes, unnormalised directions (t in units of |d|), and origins inside spheres, boxes and meshes."""
    rays, want = degenerate[cls]
    hit = is_hit(want)
    assert len(rays) <= N_RAYS and hit.sum() >= 1000, (cls, int(hit.sum()))
    if cls == "straight_down":
        assert hit[:5000].all() and (want["ptype"][:5000] == abi.TRIANGLE).sum() > 30
        assert hit[5000:].sum() >= 1000                      # the rays that start on a box face
    if cls == "inside":
        a, b = len(rays) // 3, 2 * len(rays) // 3
        assert min(hit[:a].sum(), hit[a:b].sum(), hit[b:].sum()) >= 1000
    if cls == "unnormalised":
        q = len(rays) // 4
        assert min(hit[k * q:(k + 1) * q].sum() for k in range(4)) >= 1000
    check_all_forms(compat, rays, None, want, exact, cls)
    traced = compat.trace_rays(rays, exact=exact)
    assert_records_equal(traced, want)


# ---- B3. every kernel instance --------------------------------------------------------------------------------------
#        row: (build mode, {option: value} set before the build)
ROWS = {
    1: ("compat", {"wide": 1}),
    2: ("compat", {"wide": 0}),
    3: ("sah", {"wide": 1}),
    4: ("sah", {"wide": 0}),
    5: ("lbvh", {"wide": 1, "cold_records": 1, "exact_decisions": 0}),
    6: ("lbvh", {"wide": 1, "cold_records": 0, "exact_decisions": 0}),
    7: ("lbvh", {"wide": 1, "cold_records": 1, "exact_decisions": 1}),
    8: ("lbvh", {"wide": 1, "cold_records": 0, "exact_decisions": 1}),
}
# "fast_math" 1 against "fast_math" 0 on the same trees: the measurement (test_every_kernel_instance's docstring,
# profiles/ray_query/README.md) lies inside the project tolerance, so that is the bound
FM_OTHER_SURFACE = 1.0 - SAME_SURFACE
FM_DT_REL = DT_REL


@pytest.fixture(scope="module")
def instance_rays(ref):
    """6 000 generic rays and 14 000 aimed into the particles' meshes (>= 10 000 triangle hits: the records that read
    the caller's triangles on trees without cold records), and the oracle's records for them."""
    parts = ref.oracle.instance_state()[[i for i, d in enumerate(ref.scene.instances) if d.get("count", 0) > 1], 36:42]
    rays = np.concatenate([ref.rays[:6000], R.aimed_rays(gen_rays(14000, 13), parts)])
    want = ref.oracle.trace(rays)[0]
    want.setflags(write=False)
    assert (want["ptype"][is_hit(want)] == abi.TRIANGLE).sum() >= 10000
    return rays, want


@pytest.fixture(scope="module")
def row_scene(ref):
    built = {}

    def get(row):
        if row not in built:
            mode, opts = ROWS[row]
            r = Renderer(ref.scene)
            for k, v in opts.items():
                r.set_option(k, v)                           # raises unless the option is accepted
            built[row] = r.build_acceleration_structure(BUILD_SEED, mode=mode)
        return built[row]

    yield get
    for r in built.values():
        r.cleanup()


@pytest.mark.parametrize("fast_math", [0, 1])
@pytest.mark.parametrize("row", sorted(ROWS))
def test_every_kernel_instance(ref, instance_rays, row_scene, row, fast_math):
    """rt.h: the query works "on every build mode and option rt_trace_rays works on", "a ray is occluded exactly when
    the closest query with the same flags finds a hit", with "exact_decisions" the FAST kernel equals the EXACT one "bit
    for bit", and "fast_math" selects the fast-math kernel.  One scene per row of ROWS — the (wide, raw) instances
    (3,0), (0,2), (1,0), (0,2), (2,0), (2,1), (3,0), (3,1) of RT_DISPATCH_INSTANCE — each with "fast_math" 0 and 1, in the
    forms closest records, closest t-only and any-hit.

    Exact on every row and ray: occluded == isfinite(t); t-only == the records' t; and a second closest query with
    tmax = nextafter(t, inf) returns the same record, except where the reference's own range test loses the hit:
    BoundingBox::hit drops a box once its entry t >= tmax (no 1e-6 window there, rt.h "Range"), and where a surface
    touches a face of its box that entry t can round to t or above.  Every box of any tree contains the hit
    primitive's own box (in the instance's frame) or the instance's box (in the world), and a slab test never drops a
    box that contains one it keeps, so a ray may change only if the reference drops one of those two: the primitive's
    box, decided by the oracle's tree-free loop (brute_force=2), or the instance's world box, decided by
    oracle_hit_aabb.  Measured: 11 rays of 20 000 on the reference's trees — the ranged oracle loses exactly those, and
    on those rows the second query must equal the ranged oracle bit for bit — 12 on SAH / LBVH trees (their TLAS tests
    the ground sphere's world box alone) and 13 on SAH with "wide" 0 (a hit of the parallelogram outside its q-centred
    box, which the reference does not have at any tmax); at most 20 (0.1 % of the rays) may change.

    "fast_math" 1 against "fast_math" 0 on the same trees, measured on an MI355X (20 000 rays, each of the 8 rows):
    1 ray (0.005 %) with another (instance, pindex), largest |dt| / t on the others 2.02e-5.  Both are inside the
    project tolerance (module docstring), which is the bound asserted (profiles/ray_query/README.md).
    """
    rays, want = instance_rays
    mode, opts = ROWS[row]
    r = row_scene(row)
    instance_boxes = ref.oracle.instance_state()[:, 36:42]       # world boxes
    r.set_option("fast_math", 0)
    _, base = closest(r, rays)
    if fast_math:
        r.set_option("fast_math", 1)
    t, h = closest(r, rays)
    t_only, _ = closest(r, rays, want_hits=False)
    occ = occluded(r, rays)
    hit = is_hit(h)
    # the path: every option above was accepted; the records that read triangles (on rows 6 and 8 the caller's own)
    assert (h["ptype"][hit] == abi.TRIANGLE).sum() >= 10000
    # exact on any tree, every ray
    assert np.array_equal(hit, np.isfinite(h["t"]))
    assert np.array_equal(occ, np.isfinite(t)), int((occ != np.isfinite(t)).sum())
    assert np.array_equal(t, h["t"]) and np.array_equal(t_only, h["t"])
    # tmax just beyond the ray's own t: the same record — unless the reference itself loses the hit there (docstring)
    beyond = np.where(hit, np.nextafter(h["t"], np.float32(np.inf)), R.MISS_TMAX).astype(np.float32)
    _, again = closest(r, rays, beyond)
    lost = np.flatnonzero(np.any([again[k] != h[k] if again[k].ndim == 1 else (again[k] != h[k]).any(1)
                                  for k in FIELDS], axis=0))
    print(f"row {row} fast_math {fast_math}: tmax = nextafter(t) changes {len(lost)} rays", lost)
    assert len(lost) <= 20, len(lost)
    tree_free = ref.oracle.trace(rays[lost], brute_force=2, tmax=beyond[lost])[0]
    kept = (tree_free["instance"] == h["instance"][lost]) & (tree_free["pindex"] == h["pindex"][lost])
    kept &= np.array([slab_keeps(instance_boxes[h["instance"][i]], rays[i], beyond[i]) for i in lost], bool)
    assert not kept.any(), (lost[kept], h["t"][lost[kept]], again["t"][lost[kept]])
    if mode == "compat" and not fast_math:
        ranged = ref.oracle.trace(rays, tmax=beyond)[0]
        assert 0 < (ranged["t"] != want["t"]).sum() <= 20    # the reference's own box culls: not vacuous
        assert_records_equal(again, ranged)
    if not fast_math:
        if mode == "compat":
            assert_records_equal(h, want)
        else:
            same = (h["instance"] == want["instance"]) & (h["pindex"] == want["pindex"])
            both = same & is_hit(want)
            rel = np.abs(h["t"][both] - want["t"][both]) / want["t"][both]
            print(f"row {row}: same surface as the oracle {same.mean():.5f}, max |dt|/t {rel.max():.3g}")
            assert same.mean() >= SAME_SURFACE, same.mean()
            assert np.all(rel <= DT_REL)
            assert np.all(h["t"][same & ~is_hit(want)] == np.inf)
        if opts.get("exact_decisions"):
            te, he = closest(r, rays, exact=True)
            assert_records_equal(h, he)
            assert np.array_equal(t, te)
            assert np.array_equal(occ, occluded(r, rays, exact=True))
    else:
        other = (h["instance"] != base["instance"]) | (h["pindex"] != base["pindex"])
        both = ~other & is_hit(base)
        rel = np.abs(h["t"][both] - base["t"][both]) / base["t"][both]
        print(f"row {row}: fast_math other surface {int(other.sum())} of {len(rays)} ({other.mean():.5f}), "
              f"max |dt|/t {rel.max():.3g}")
        assert (h["t"] != base["t"]).any()                   # the fast-math kernel ran: other roundings somewhere
        assert other.mean() <= FM_OTHER_SURFACE, other.mean()
        assert np.all(rel <= FM_DT_REL), rel.max()
        assert np.all(h["t"][~other & ~is_hit(base)] == np.inf)


# ---- B4. call shapes -------------------------------------------------------------------------------------------------
def raw_query(r, n, rays_ptr, tmax_ptr=None, t_ptr=None, hits_ptr=None, occ_ptr=None, flags=0):
    q = abi.RayQuery()
    q.rays_device, q.tmax_device, q.ray_count, q.flags = rays_ptr, tmax_ptr, n, flags
    q.t_device, q.hits_device, q.occluded_device = t_ptr, hits_ptr, occ_ptr
    abi.check(r.lib, r.lib.rt_query_rays(r.h, C.byref(q)))


def test_hits_without_t(ref, compat):
    """rt.h: a closest query takes "at least one of hits_device / t_device".  hits_device alone: the oracle's records,
    and not a byte around them."""
    import torch
    n, pad = 4097, 64
    d_rays = torch.from_numpy(np.array(ref.rays[:n])).cuda()
    buf = torch.full((n + 2 * pad, 48), 0xAB, dtype=torch.uint8, device="cuda")
    raw_query(compat, n, d_rays.data_ptr(), hits_ptr=buf.data_ptr() + pad * 48)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert np.all(out[:pad] == 0xAB) and np.all(out[pad + n:] == 0xAB)
    assert_records_equal(hits_to_numpy(out[pad:pad + n]), ref.hits[:n])


@pytest.mark.parametrize("n", [448, 512, 513, 575, 576, 577, 4097])
def test_sizes_around_the_bands(ref, compat, n):
    """rt.h promises every ray_count <= 0xFFFFFFFF; the kernel splits the chunks of 64 rays into 8 bands (chunks * part /
    8), so 7, 8 and 9 chunks (448, 512, 513 .. 576 rays) and 10 (577) are where a band is empty, holds one chunk, or the
    last chunk is partial.  Closest (records and t) and any-hit with tmax, into sentinel-padded outputs."""
    import torch
    pad = 70
    want = ref.hits[:n]
    tmax = R.boundary_tmax(ref.hits["t"], ref.hit)["minus_5e-7"][:n]
    want_ranged = ref.oracle.trace(ref.rays[:n], tmax=tmax)[0]
    d_rays = torch.from_numpy(np.array(ref.rays[:n])).cuda()
    d_tmax = torch.from_numpy(tmax).cuda()
    t_buf = torch.full((n + pad,), -7.0, dtype=torch.float32, device="cuda")
    h_buf = torch.full((n + pad, 48), 0xAB, dtype=torch.uint8, device="cuda")
    o_buf = torch.full((n + pad,), 0xAB, dtype=torch.uint8, device="cuda")
    o2_buf = torch.full((n + pad,), 0xAB, dtype=torch.uint8, device="cuda")
    raw_query(compat, n, d_rays.data_ptr(), t_ptr=t_buf.data_ptr(), hits_ptr=h_buf.data_ptr())
    raw_query(compat, n, d_rays.data_ptr(), occ_ptr=o_buf.data_ptr(), flags=abi.RT_QUERY_ANY_HIT)
    raw_query(compat, n, d_rays.data_ptr(), d_tmax.data_ptr(), occ_ptr=o2_buf.data_ptr(), flags=abi.RT_QUERY_ANY_HIT)
    torch.cuda.synchronize()
    t, h, o, o2 = t_buf.cpu().numpy(), h_buf.cpu().numpy(), o_buf.cpu().numpy(), o2_buf.cpu().numpy()
    assert np.all(t[n:] == -7.0) and np.all(h[n:] == 0xAB) and np.all(o[n:] == 0xAB) and np.all(o2[n:] == 0xAB)
    assert np.array_equal(t[:n], want["t"])
    assert_records_equal(hits_to_numpy(h[:n]), want)
    assert np.array_equal(o[:n], is_hit(want).astype(np.uint8))
    assert np.array_equal(o2[:n], is_hit(want_ranged).astype(np.uint8))


def test_naturally_aligned_buffers(ref, compat):
    """rt.h asks nothing of the buffers beyond their element types.  Every buffer one element into a larger allocation
    — rays, tmax and t 4 bytes, hits 48 + 4 bytes, occluded 1 byte — so that none is aligned beyond its scalars (the
    kernel reads rays and tmax as single floats and stores an rt_hit, whose alignment is 4): the aligned run's result,
    which is the ranged oracle's."""
    import torch
    n = 4097
    tmax = R.boundary_tmax(ref.hits["t"], ref.hit)["plus_5e-7"][:n]
    want = ref.oracle.trace(ref.rays[:n], tmax=tmax)[0]
    t0, h0 = closest(compat, ref.rays[:n], tmax)
    o0 = occluded(compat, ref.rays[:n], tmax)
    assert_records_equal(h0, want)

    d_rays = torch.zeros(6 * n + 2, dtype=torch.float32, device="cuda")
    d_rays[1:6 * n + 1] = torch.from_numpy(np.array(ref.rays[:n]).reshape(-1)).cuda()
    d_tmax = torch.zeros(n + 2, dtype=torch.float32, device="cuda")
    d_tmax[1:n + 1] = torch.from_numpy(tmax).cuda()
    t_buf = torch.full((n + 2,), -7.0, dtype=torch.float32, device="cuda")
    h_buf = torch.full(((n + 3) * 48,), 0xAB, dtype=torch.uint8, device="cuda")
    o_buf = torch.full((n + 2,), 0xAB, dtype=torch.uint8, device="cuda")
    for x in (d_rays, d_tmax, t_buf, h_buf, o_buf):
        assert x.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    raw_query(compat, n, d_rays.data_ptr() + 4, d_tmax.data_ptr() + 4, t_ptr=t_buf.data_ptr() + 4,
              hits_ptr=h_buf.data_ptr() + 52)
    raw_query(compat, n, d_rays.data_ptr() + 4, d_tmax.data_ptr() + 4, occ_ptr=o_buf.data_ptr() + 1,
              flags=abi.RT_QUERY_ANY_HIT)
    torch.cuda.synchronize()
    t, h, o = t_buf.cpu().numpy(), h_buf.cpu().numpy(), o_buf.cpu().numpy()
    assert t[0] == -7.0 and t[n + 1] == -7.0 and np.all(h[:52] == 0xAB) and np.all(h[52 + 48 * n:] == 0xAB)
    assert o[0] == 0xAB and o[n + 1] == 0xAB
    assert np.array_equal(t[1:n + 1], t0)
    assert_records_equal(hits_to_numpy(h[52:52 + 48 * n]), h0)
    assert np.array_equal(o[1:n + 1].astype(bool), o0)
