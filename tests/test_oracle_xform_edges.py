"""The oracle against a float64 reference on the instance transforms of tests/xform_edges_ref.py: pivots other than
rotate-x 90's row swap, negative pivots, mirrors, anisotropic scales, scales of 1e-3 and 1e3, and both singular exits of
the reference's elimination.  tests/test_gpu_xform_edges.py compares the GPU with the oracle on the same scene and
rays bit for bit; this file is what says the oracle is right there.  No GPU.

Bounds.  Each is 4 x the largest deviation of the oracle from the float64 reference measured on these inputs (x86-64,
gcc, glibc; the figures below), one set per group — "regular" (15 classes), "tiny", "huge", "stress" (near_singular,
small).  Another libm or compiler moves the last bits of sin / cos and of the elimination; a wrong row, a transpose
for an inverse transpose or a missing flip moves these figures by orders of magnitude (to 1 for most of them).
The record bounds marked * are not 4 x the measurement but the floor of 4 x 2^-24 = 2.4e-07 (below, at BOUNDS): 4 x
those measurements is less than one last bit of a float32 can move a value.

    measured             regular    tiny       huge       stress
    forward  (1)         7.8e-07    1.1e-07    1.0e-07    0
    inverse  (2)         1.3e-06    1.3e-07    7.0e-08    4.1e-08 *
    box      (3)         4.7e-08 *  1.6e-08 *  3.3e-08 *  5.6e-08 *
    |dt| / t             2.8e-04    1.0e-03    3.4e-05    2.2e-04
    point    (4)         1.6e-03    9.6e-06    6.5e-02    5.6e-04
    normal   (5)         1.1e-02    2.6e-02    3.6e-05    1.9e-02
    |dt| / t (6)                                          4.7e-04

    (1) rows of the forward matrix against m64, relative to the largest entry of its 3 x 3 part; the shift column is
        exact.  (2) rows of the inverse against numpy's float64 inverse of m64, relative to its largest entry.  (3) how
        far a face of the transformed box lies outside the float64 image of the local box's corners, relative to the
        largest coordinate of those; by how much it may lie inside is not measured but reasoned: CONTAIN.  (4), (5)
        largest component difference, in world units and of unit vectors, on the rays that are not ambiguous.  (6) on
        the ambiguous rays of "near_singular" (its mesh and sphere, 1e-6 thick): the nearest t, whichever side is named.
    The largest figures come from where the formats say they should: normal of "regular" from "aniso" and "flat" (the
    inverse transpose stretches a local rounding 100-fold), |dt| / t of "regular" from rays that graze
    "mirror_aniso" and "rot_gen", point of "huge" from float32's spacing of 5e-4 at 5000, everything of "tiny" from an
    object 1e-3 wide standing 24 from the origin.

Conditions on the inputs (not tolerances), as measured: no ray of a class other than "near_singular" is ambiguous
(the bound is 2 %); every ray aimed at a regular class but 8 of "aniso" (0.7 %) hits the instance it was aimed at
(the bound is 95 %).  In "near_singular" the mesh and the sphere are 1e-6 thick: their rays meet two surfaces within
1e-4 t and are ambiguous (799 of 800), whatever the rays; its parallelogram's rays carry the 2 % condition and the
per-surface comparison alone, and the 800 are held to the reference's nearest t (6).  No ray hits a singular instance.
"""
import numpy as np
import pytest

import xform_edges_ref as X
from rtamd import abi

U = 2.0 ** -24
# A face of the float32 box may lie inside the float64 image of the corners by float32's rounding of that image, and no
# more: a coordinate is a sum of 4 products of entries that each carry the roundings of sin, cos and two matrix
# products (a few U), so 16 U of the largest coordinate bounds it with a factor 2 to spare.
CONTAIN = 16 * U
MAX_AMBIGUOUS = 0.02
MIN_OWN = 0.95
#        4 x the module docstring's table
BOUNDS = {
    "regular": dict(forward=3.2e-6, inverse=5.2e-6, box=1.9e-7, dt=1.1e-3, point=6.2e-3, normal=4.4e-2),
    "tiny":    dict(forward=4.4e-7, inverse=5.2e-7, box=6.4e-8, dt=4.1e-3, point=3.9e-5, normal=1.03e-1),
    "huge":    dict(forward=4.0e-7, inverse=2.8e-7, box=1.4e-7, dt=1.4e-4, point=2.6e-1, normal=1.5e-4),
    "stress":  dict(forward=0.0,    inverse=1.7e-7, box=2.3e-7, dt=8.5e-4, point=2.3e-3, normal=7.3e-2, dt_thin=1.9e-3),
}
# ... but never under 4 U for a float32 record: one last bit of a sin or cos that another libm rounds the other way
# moves an entry by up to 2 U of itself, and an entry is a sum of such.  "stress" has no rotation: sin 0 and cos 0 are
# exact, its forward rows are products with 0 and 1, and its bound of 0 stands.
for _b in BOUNDS.values():
    for _k in ("forward", "inverse", "box"):
        _b[_k] = max(_b[_k], 4 * U) if _b[_k] else 0.0
INVERTIBLE = [n for n in X.NAMES if X.group_of(n) != "singular"]
SINGULAR = [n for n in X.NAMES if X.group_of(n) == "singular"]


def bound_set(name):
    g = X.group_of(name)
    return name if g == "scaled" else ("regular" if g == "singular" else g)


class Case:
    def __init__(self):
        from oracle.oracle import OracleScene
        self.scene = X.scene()
        self.oracle = OracleScene(self.scene, build_seed=0)
        self.rays, self.aimed = X.rays()
        self.state = self.oracle.instance_state()
        self.got = self.oracle.trace(self.rays)[0]
        self.ref = X.closest64(self.scene, self.rays)

    def of(self, name):
        return np.flatnonzero(self.aimed // X.PER_CLASS == X.NAMES.index(name))


@pytest.fixture(scope="module")
def case(oracle_lib):
    c = Case()
    yield c
    c.oracle.close()


def instances_of(name):
    c = X.NAMES.index(name)
    return range(X.PER_CLASS * c, X.PER_CLASS * (c + 1))


# ---- inputs ----------------------------------------------------------------------------------------------------------
def test_scene_is_the_stated_one(case):
    s = case.scene
    assert len(X.CLASSES) == 22 and len(s.instances) == 66 and s.triangle_count == 1408 and not s.animated
    assert len(case.rays) == 66 * X.N_PER_INSTANCE and case.rays.dtype == np.float32
    assert sorted(X.GRID + ["huge"]) == sorted(X.NAMES)
    meshes = [d for d in s.instances if d["type"] == abi.TRIANGLE]
    assert len({d["index"] for d in meshes}) == 22 and all(d["count"] == 64 and "bounds" in d for d in meshes)
    shifts = np.array([d["shift"] for d in s.instances])
    grid = shifts[[k for k, d in enumerate(s.instances) if d["cls"] != "huge"]]
    assert len({tuple(x) for x in np.round(grid, 6)}) == 63
    cells = (grid - X.OFFSET) / X.PITCH
    assert np.allclose(cells, np.round(cells)) and np.allclose(cells.mean(axis=0), 0)      # centred on the origin
    assert np.all(shifts[[k for k, d in enumerate(s.instances) if d["cls"] == "huge"], 2] == X.HUGE_Z + X.OFFSET[2])
    # the frames' camera sees the whole grid: every instance's centre, and a radius around it, inside 192 x 128
    assert X.FRAME == (192, 128) and s.camera["sample_count"] == 1 and s.camera["ray_trace_depth"] == 3
    for off in ((0, 0, 0), (X.RADIUS, X.RADIUS, 0), (-X.RADIUS, -X.RADIUS, 0)):
        px = X.project(grid + np.asarray(off))
        assert np.all((px[:, 0] > 2) & (px[:, 0] < X.FRAME[0] - 2) & (px[:, 1] > 2) & (px[:, 1] < X.FRAME[1] - 2)), off
    huge = X.project(shifts[[k for k, d in enumerate(s.instances) if d["cls"] == "huge"]])
    assert np.all((huge[:, 1] > 0) & (huge[:, 1] < X.FRAME[1])) and ((huge[:, 0] > 0) & (huge[:, 0] < X.FRAME[0])).any()


def test_assignments_pass_through_singular_transforms():
    """The moving test's schedule (tests/test_gpu_xform_edges.py): every instance changes class every frame, every
    class is taken in every frame, and instances go into singular transforms and come back within the frames."""
    singular = [X.NAMES.index(n) for n in SINGULAR]
    a = np.stack([X.assignment(f) for f in range(X.FRAMES)])
    assert np.all(a[1:] != a[:-1]) and (a[0] != np.arange(X.N_INSTANCES) // X.PER_CLASS).sum() >= 60
    assert all(set(row) == set(range(len(X.NAMES))) for row in a)
    into = np.isin(a[1:], singular) & ~np.isin(a[:-1], singular)
    back = ~np.isin(a[1:], singular) & np.isin(a[:-1], singular)
    assert into.any(axis=0).sum() >= 12 and back.any(axis=0).sum() >= 12
    assert (into.any(axis=0) & back.any(axis=0)).sum() >= 6  # regular -> singular -> regular within the 6 frames


def test_axis_rays_leave_sub_threshold_components(case):
    """X.axis_rays(): in the frame of an instance of a quarter- or half-turn class most of them have a direction
    component that is not 0 and is below the reference's 1e-6 "parallel" threshold (BoundingBox.cu:44-50) — what
    cos 90 deg = -4.4e-8 leaves — and the oracle agrees with float64 on what they hit."""
    rays, aimed = X.axis_rays()
    assert len(rays) == len(X.TURNS) * X.PER_CLASS * X.AXIS_PER_INSTANCE
    inv = case.state[aimed, :12].reshape(-1, 3, 4)
    local = np.abs(np.einsum("rab,rb->ra", inv[:, :, :3], rays[:, 3:]))
    sub = ((local > 0) & (local < X.FZERO)).any(axis=1)
    print(f"axis rays: {int(sub.sum())} of {len(rays)} with a local component in (0, 1e-6)")
    assert sub.sum() >= 0.6 * len(rays)
    got, ref = case.oracle.trace(rays)[0], X.closest64(case.scene, rays)
    clear = ~ref["ambiguous"]
    assert clear.mean() >= 1 - MAX_AMBIGUOUS
    same = (got["instance"] == ref["instance"]) & (got["pindex"] == ref["pindex"])
    assert same[clear].all() and (got["instance"] == aimed).mean() >= MIN_OWN
    both = clear & (ref["instance"] != abi.MISS)
    assert np.all(np.abs(got["t"][both] - ref["t"][both]) <= BOUNDS["regular"]["dt"] * ref["t"][both])


# ---- records ---------------------------------------------------------------------------------------------------------
def record_deviations(case, k):
    """(forward, inverse or None, box out, box in) of instance k; see the module docstring."""
    d = case.scene.instances[k]
    m = X.instance_m64(d)
    inv32, fwd32 = (case.state[k, a:a + 12].reshape(3, 4).astype(np.float64) for a in (0, 12))
    forward = np.abs(fwd32 - m[:3]).max() / max(np.abs(m[:3, :3]).max(), 1e-300)
    inverse = None
    if X.group_of(d["cls"]) != "singular":
        mi = np.linalg.inv(m)
        inverse = np.abs(inv32 - mi[:3]).max() / np.abs(mi[:3]).max()
    c = X.world_corners(case.scene, d)
    lo, hi = c.min(axis=0), c.max(axis=0)
    flat = hi - lo < X.FZERO                                 # BoundingBox's padding of an axis without extent
    lo, hi = np.where(flat, lo - X.FZERO, lo), np.where(flat, hi + X.FZERO, hi)
    box = case.state[k, 36:42].astype(np.float64)
    out = np.concatenate([lo - box[0::2], box[1::2] - hi])   # > 0: the float32 face lies outside
    size = np.abs(c).max()
    return forward, inverse, out.max() / size, (-out).max() / size


@pytest.mark.parametrize("name", X.NAMES)
def test_records(case, name):
    """Forward rows, inverse rows and the transformed box of the class's three instances."""
    b = BOUNDS[bound_set(name)]
    for k in instances_of(name):
        d = case.scene.instances[k]
        forward, inverse, box_out, box_in = record_deviations(case, k)
        print(f"{name} instance {k}: forward {forward:.3g} inverse {inverse if inverse is None else f'{inverse:.3g}'} "
              f"box outside {box_out:.3g} inside {box_in:.3g}")
        assert np.array_equal(case.state[k, 12:24].reshape(3, 4)[:, 3], np.asarray(d["shift"], np.float32))
        assert forward <= b["forward"], (k, forward)
        if inverse is not None:
            assert inverse <= b["inverse"], (k, inverse)
        assert box_in <= CONTAIN, (k, box_in)
        assert box_out <= b["box"], (k, box_out)
        box = case.state[k, 36:42]
        assert np.all(box[1::2] - box[0::2] >= 0)
        q, u, v = (np.asarray(x, np.float32).astype(np.float64) for x in X.QUAD)
        local = {abi.TRIANGLE: d.get("centroid"), abi.SPHERE: (0, 0, 0), abi.PARALLELOGRAM: q + u / 2 + v / 2}
        local = local[d["type"]]
        centroid = X.instance_m64(d)[:3] @ np.append(np.asarray(local, np.float64), 1.0)
        assert np.abs(case.state[k, 42:45] - centroid).max() <= CONTAIN * np.abs(centroid).max()


@pytest.mark.parametrize("name", SINGULAR)
def test_singular_records(case, name):
    """Both exits of the elimination (a pivot below 1e-6 on the way down, Matrix.cu:5-45; a diagonal entry below 1e-6
    on the way up, Matrix.cu:46-68) end in Matrix::inverse returning its argument: inverse rows == forward rows and
    inverse transpose == forward transposed, bit for bit — for a scale of 1e-7 as for 0.  Their boxes are what the
    GPU's TLAS builders must take: BoundingBox pads an axis without extent by 1e-6 (BoundingBox.cuh:24-28), which
    float32 keeps at 0.37 and drops at 32.37, so some of these boxes have no extent at all
    (test_boxes_without_extent)."""
    boxes = case.state[list(instances_of(name)), 36:42]
    extent = boxes[:, 1::2] - boxes[:, 0::2]
    print(f"{name}: smallest box extents {extent.min(axis=1)}")
    assert np.all(extent >= 0) and np.all(extent.min(axis=1) <= np.float32(4e-6))
    for k in instances_of(name):
        inv, fwd, nrm = (case.state[k, a:a + 12].reshape(3, 4) for a in (0, 12, 24))
        assert inv.tobytes() == fwd.tobytes(), k
        full = np.vstack([fwd, np.asarray([[0, 0, 0, 1]], np.float32)])
        assert nrm.tobytes() == np.ascontiguousarray(full.T[:3]).tobytes(), k
    a, b = (case.state[instances_of(n)[0], :36] for n in ("sing_x0", "sing_1e-7"))
    assert np.array_equal(a[:12] == a[12:24], b[:12] == b[12:24]) and np.all(a[:12] == a[12:24])


def test_boxes_without_extent(case):
    """Conditions on the inputs: boxes with an axis of extent exactly 0 are among the records, and one instance's box
    is 1e3 times the usual one and 1e5 times the smallest class's."""
    extent = case.state[:, 37:42:2] - case.state[:, 36:42:2]
    flat = np.flatnonzero((extent == 0).any(axis=1))
    print("boxes without extent on an axis:", [(int(k), case.scene.instances[k]["cls"]) for k in flat])
    assert len(flat) >= 2 and {case.scene.instances[k]["cls"] for k in flat} >= {"sing_all0", "near_singular"}
    size = extent.max(axis=1)
    tiny = size[[k for k, d in enumerate(case.scene.instances) if d["cls"] == "tiny"]]
    print(f"largest box {size.max():.4g}, median {np.median(size):.4g}, tiny's {tiny.max():.4g}")
    assert size.max() >= 1e3 * np.median(size) and size.max() >= 1e5 * tiny.max()


def test_invertible_records_are_inverted(case):
    """... and no other class takes that exit: inverse times forward is the identity to 1e-5 (the largest deviation
    measured: 1.9e-6), "near_singular" (2e-6, 1, 1) included."""
    worst = 0.0
    for name in INVERTIBLE:
        for k in instances_of(name):
            inv, fwd = (np.vstack([case.state[k, a:a + 12].reshape(3, 4).astype(np.float64), [[0, 0, 0, 1]]])
                        for a in (0, 12))
            worst = max(worst, np.abs((inv @ fwd)[:3, :3] - np.eye(3)).max())
    print(f"|inverse forward - 1| <= {worst:.3g}")
    assert worst <= 1e-5


# ---- hits ------------------------------------------------------------------------------------------------------------
def hit_deviations(case, name):
    idx = case.of(name)
    got, ref = case.got[idx], case.ref[idx]
    clear = ~ref["ambiguous"]
    same = (got["instance"] == ref["instance"]) & (got["pindex"] == ref["pindex"]) & (got["ptype"] == ref["ptype"])
    both = clear & same & (ref["instance"] != abi.MISS)
    dt = np.abs(got["t"][both] - ref["t"][both]) / ref["t"][both]
    point = np.abs(got["point"][both] - ref["point"][both]).max(axis=1)
    normal = np.abs(got["normal"][both] - ref["normal"][both]).max(axis=1)
    return idx, clear, same, both, dt, point, normal


def thin_dt(case):
    """|dt| / t on the ambiguous rays of "near_singular" (its mesh and sphere, 1e-6 thick) that hit the instance the
    reference names: whichever side is named, the nearest t is the reference's to within the object's thickness."""
    idx = case.of("near_singular")
    got, ref = case.got[idx], case.ref[idx]
    sel = ref["ambiguous"] & (got["instance"] == ref["instance"]) & (ref["instance"] != abi.MISS)
    return sel, np.abs(got["t"][sel] - ref["t"][sel]) / ref["t"][sel]


@pytest.mark.parametrize("name", INVERTIBLE)
def test_hits(case, name):
    """Every ray of the class that is not ambiguous: the float64 reference's (instance, primitive); t, point and
    normal within the group's bounds; the normal faces the ray."""
    idx, clear, same, both, dt, point, normal = hit_deviations(case, name)
    got = case.got[idx]
    print(f"{name}: {len(idx)} rays, {int((~clear).sum())} ambiguous, {int((clear & ~same).sum())} other surface, "
          f"{int(both.sum())} compared: |dt|/t {dt.max():.3g} point {point.max():.3g} normal {normal.max():.3g}")
    assert not (clear & ~same).any(), np.flatnonzero(clear & ~same)[:8]
    assert both.sum() >= 0.3 * len(idx)
    b = BOUNDS[bound_set(name)]
    assert dt.max() <= b["dt"] and point.max() <= b["point"] and normal.max() <= b["normal"]
    hit = got["instance"] != abi.MISS
    assert np.all((got["normal"][hit].astype(np.float64) * case.rays[idx][hit, 3:]).sum(axis=1) < 0)
    assert np.all(np.abs(np.linalg.norm(got["normal"][hit].astype(np.float64), axis=1) - 1.0) < 1e-6)
    if name == "near_singular":
        sel, thin = thin_dt(case)
        print(f"near_singular: {int(sel.sum())} ambiguous rays on the reference's instance, |dt|/t {thin.max():.3g}")
        assert sel.sum() >= 600      # of 799: on the others float32 finds another instance, or none
        assert thin.max() <= b["dt_thin"]


@pytest.mark.parametrize("name", X.NAMES)
def test_conditions_on_the_inputs(case, name):
    idx = case.of(name)
    amb = case.ref["ambiguous"][idx]
    own = case.got["instance"][idx] == case.aimed[idx]
    print(f"{name}: ambiguous {amb.mean():.4f}, hits the instance aimed at {own.mean():.4f}")
    if name == "near_singular":                              # 1e-6 thick: two surfaces within 1e-4 t (module docstring)
        flat = case.aimed[idx] % X.PER_CLASS != 2
        assert amb[flat].mean() >= 0.99
        amb = amb[~flat]
    assert amb.mean() <= MAX_AMBIGUOUS
    if X.group_of(name) == "regular":
        assert own.mean() >= MIN_OWN
    if X.group_of(name) == "singular":
        assert not own.any()
        assert not np.isin(case.got["instance"], list(instances_of(name))).any()       # nor does any other ray
