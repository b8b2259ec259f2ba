"""rt_accumulate_motion and rt_instance_motion_records (include/rt.h, "Moving instances") restated in numpy, and a
seeded builder of synthetic cases.

carry() is the MOTION kernel's own part in float32 with csrc/accumulate.hip's operation order: a pixel's point and
normal carried to the previous frame by its instance's record, or the pixel marked for reset.  Everything after that
is rt_accumulate's text on the carried point and normal, so accumulate_motion() hands the carried records to
accumulate_ref.accumulate / guided_ref.accumulate_moments (neither file is changed) and gives the kernel's bits.  The
faults of tests/test_motion_ref.py: the translation dropped, the point's linear map used for the normal, the
normalisation skipped, flag 7 handled as static, a record read for an instance id past the records.

records64() restates rt_instance_motion_records in float64 from two float forward matrices, in the header's operation
order.

The cases are accumulate_ref.case's guides with their instance ids (floor 0, sphere 1) assigned to motion classes."""
import numpy as np

import accumulate_ref as A
import guided_ref as G

F32 = np.float32
MISS = A.MISS
STATIC, MOVED, NO_HISTORY = 0, 1, 2
EPS32 = A.EPS32


def motion_dtype():
    from rtamd.renderer import MOTION_DTYPE
    return MOTION_DTYPE


# ---- the kernel's motion step ----------------------------------------------------------------------------------------

def _row(P, c, x):
    return ((P[..., c, 0] * x[..., 0] + P[..., c, 1] * x[..., 1]) + P[..., c, 2] * x[..., 2])


def carry(hits, records, *, fault=None, beyond=None):
    """hits [H, W] rt_hit records, records [n] of MOTION_DTYPE -> a copy of hits with point = xp and normal = np, and
    instance = MISS where the motion resets the pixel (accumulate then resets it: `inst != MISS` is its first test).
    float32, the kernel's operation order.  fault in (None, "no_shift", "normal_A", "no_normalise", "flag7_static",
    "read_beyond"); read_beyond reads `beyond` (one record) for every instance id >= n, what a kernel without the range
    test would find behind the buffer."""
    out = np.array(hits)
    inst = hits["instance"]
    n = len(records)
    hit = inst != MISS
    inside = hit & (inst < n)
    idx = np.where(inside, inst, 0).astype(np.int64)
    rec = records[idx] if n else np.zeros(inst.shape, motion_dtype())
    if fault == "read_beyond":
        past = hit & ~inside
        rec = np.where(past, np.asarray(beyond, motion_dtype()).reshape(()), rec)
        inside = hit
    f = rec["flags"]
    if fault == "flag7_static":
        f = np.where(f == 7, STATIC, f)
    moved = inside & (f == MOVED)
    reset = inside & (f != MOVED) & (f != STATIC)
    x, nrm = hits["point"].astype(F32), hits["normal"].astype(F32)
    P, N = rec["point"].astype(F32), rec["normal"].astype(F32)
    if fault == "normal_A":
        N = P[..., :3]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xp = np.stack([_row(P, c, x) if fault == "no_shift" else _row(P, c, x) + P[..., c, 3] for c in range(3)], axis=-1)
        u = np.stack([_row(N, c, nrm) for c in range(3)], axis=-1)
        l2 = (u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]
        reset = reset | (moved & ~(l2 > 0))
        s = np.sqrt(l2)
        unit = u if fault == "no_normalise" else u / s[..., None]
    assert xp.dtype == F32 and unit.dtype == F32
    keep = moved & ~reset
    out["point"] = np.where(keep[..., None], xp, x)
    out["normal"] = np.where(keep[..., None], unit, nrm)
    out["instance"] = np.where(reset, MISS, inst)
    return out


def accumulate_motion(color, hits, prev_hits, prev_history, view, records, *, albedo=None, prev_moments=None,
                      moments=False, fault=None, beyond=None, **kw):
    """rt_accumulate_motion in float32 -> (history [H, W, 4], moments [H, W, 2] or None, valid [H, W, 4] or None)."""
    H, W = color.shape[:2]
    carried = carry(hits.reshape(H, W), records, fault=fault, beyond=beyond) if prev_history is not None else hits
    if moments:
        h, m = G.accumulate_moments(color, albedo, carried, prev_hits, prev_history, prev_moments, view, dtype=np.float32, **kw)
        return h, m, None
    h, valid = A.accumulate(color, carried, prev_hits, prev_history, view, dtype=np.float32, **kw)
    return h, None, valid


# ---- rt_instance_motion_records in float64 ---------------------------------------------------------------------------

def _cofactor_inverse(L):
    C = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            C[i, j] = L[i1, j1] * L[i2, j2] - L[i1, j2] * L[i2, j1]
    det = (L[0, 0] * C[0, 0] + L[0, 1] * C[0, 1]) + L[0, 2] * C[0, 2]
    if det == 0.0 or not np.isfinite(det):
        return None
    return C.T / det


def _product(X, Y):
    return np.array([[(X[i, 0] * Y[0, j] + X[i, 1] * Y[1, j]) + X[i, 2] * Y[2, j] for j in range(3)] for i in range(3)])


def records64(fp, fc):
    """The record of two forward matrices (rows [3, 4], float32 values), in float64 and the header's order ->
    (flags, point [3, 4] float64, normal [3, 3] float64), the maps before their one rounding to float.  The library's
    extra exit (a matrix its own elimination does not invert) is not restated: callers pass matrices it inverts."""
    fp, fc = np.asarray(fp, F32).astype(np.float64).reshape(3, 4), np.asarray(fc, F32).astype(np.float64).reshape(3, 4)
    Lp, tp, Lc, tc = fp[:, :3], fp[:, 3], fc[:, :3], fc[:, 3]
    zero = (NO_HISTORY, np.zeros((3, 4)), np.zeros((3, 3)))
    with np.errstate(all="ignore"):
        Lpi, Lci = _cofactor_inverse(Lp), _cofactor_inverse(Lc)
        if Lpi is None or Lci is None:
            return zero
        Am, M = _product(Lp, Lci), _product(Lc, Lpi)
        b = np.array([tp[i] - ((Am[i, 0] * tc[0] + Am[i, 1] * tc[1]) + Am[i, 2] * tc[2]) for i in range(3)])
        point = np.concatenate([Am, b[:, None]], axis=1)
        normal = M.T
        if not (np.isfinite(point.astype(F32)).all() and np.isfinite(normal.astype(F32)).all()):
            return zero
    return MOVED, point, normal


# ---- synthetic cases -------------------------------------------------------------------------------------------------

CLASSES = ("static", "translation", "quarter_turn", "scale", "rotation", "no_history", "flag7", "zero_normal", "beyond")
EXACT = ("translation", "quarter_turn", "scale")           # float32 applies these maps without a rounding of the matrix
CARRIED = EXACT + ("rotation",)                             # the classes whose previous records are the carried current ones
LIFT = 0.25                                                 # every map of CARRIED but the rotation raises y by exactly this
INSTANCE_COUNT = 8                                          # records: one per class but "beyond", whose id is past them
BEYOND_IDS = (INSTANCE_COUNT, 0x80000000)                   # the first id past the records, and one whose byte offset passes 2^32
VIEWS = tuple(v for v in A.VIEWS if v != "null")            # the views that have a prev_view
REGIONS = 3                                                 # floor x < 0, floor x >= 0, sphere


def _record(point=None, normal=None, flags=MOVED):
    r = np.zeros((), motion_dtype())
    r["point"] = np.eye(3, 4, dtype=F32) if point is None else np.asarray(point, F32)
    r["normal"] = np.eye(3, dtype=F32) if normal is None else np.asarray(normal, F32)
    r["flags"] = flags
    return r


def class_records():
    """The INSTANCE_COUNT records in CLASSES' order, and the record the read_beyond fault finds behind them.
    translation: powers of two, lifting the surface by 0.25 so the uncompensated plane test fails (tolerance 0.02 t,
    t about 5).  quarter_turn: about the vertical through the sphere's centre, x -> z, z -> -x, entries 0 and +-1, and
    the same lift.  scale: the instance has grown by (2, 1, 0.5) about the origin since the last frame, so the point map
    is diag(0.5, 1, 2) with the lift and the normal map its inverse, diag(2, 1, 0.5), not the point's: where the normal
    looks along z, as in the middle of the sphere, the unnormalised normal is half as long.  rotation: 5 degrees about (1, 2, 3), its matrix rounded to float32: the products round."""
    lift = LIFT
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    c, s = np.cos(np.radians(5.0)), np.sin(np.radians(5.0))
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + s * K + (1 - c) * (K @ K)
    rows = lambda L, b: np.concatenate([np.asarray(L, np.float64), np.asarray(b, np.float64)[:, None]], axis=1)
    turn = [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]
    recs = np.zeros(INSTANCE_COUNT, motion_dtype())
    recs[0] = _record(flags=STATIC)
    recs[1] = _record(rows(np.eye(3), [0.125, lift, -0.0625]))
    recs[2] = _record(rows(turn, [0.0, lift, 0.0]), turn)
    recs[3] = _record(rows(np.diag([0.5, 1.0, 2.0]), [0.0, lift, 0.0]), np.diag([2.0, 1.0, 0.5]))
    recs[4] = _record(rows(R, [0.05, 0.1, -0.05]), R)
    recs[5] = _record(np.zeros((3, 4)), np.zeros((3, 3)), NO_HISTORY)
    recs[6] = _record(flags=7)
    recs[7] = _record(normal=np.zeros((3, 3)))
    recs.setflags(write=False)
    return recs, _record(rows(np.eye(3), [0.125, lift, -0.0625]))


def assignment(width, height, view):
    """The classes (indices into CLASSES) of the case's three regions: every class takes every region over the cases."""
    k = A.SIZES.index((width, height)) * len(VIEWS) + VIEWS.index(view)
    return tuple((k + 3 * r) % len(CLASSES) for r in range(REGIONS))


def _region(rec):
    return np.where(rec["instance"] == 1, 2, np.where(rec["point"][..., 0] < 0, 0, 1))


_cache = {}
KW = G.KW


def case(width, height, view, seed=0):
    """guided_ref.moments_case(width, height, view) with its instance ids assigned to motion classes, computed once and
    shared (read-only).  A hit's id becomes the class index of its region (assignment); class "beyond" takes an id of
    BEYOND_IDS.  Last frame's records keep accumulate_ref's ray cast (ids by their own region) except under the pixels
    of a class of CARRIED: there the previous record is the current one carried by the class's map, in float32 by the
    kernel's expressions, so the carried point meets its own surface in the previous frame; the ray cast's own records
    of such a class, which stand where the instance is now, become sky.  The maps of EXACT raise
    every point by LIFT exactly, so where the normal is (0, 1, 0), the floor, an uncarried point is LIFT off the
    previous surface along its normal, whichever previous pixel it looks at.  -> the inputs, "records", "beyond", "classes" [H, W] (-1 on sky), and the float32 references
    "history32" (no moments), "moments32" = (history, moments) with albedo."""
    key = (width, height, view, seed)
    if key not in _cache:
        g = dict(G.moments_case(width, height, view, seed))
        recs, beyond = class_records()
        cls_of = np.asarray(assignment(width, height, view))
        k = A.SIZES.index((width, height)) * len(VIEWS) + VIEWS.index(view)
        ids = np.arange(len(CLASSES), dtype=np.uint32)
        ids[CLASSES.index("beyond")] = BEYOND_IDS[(k // len(CLASSES)) % 2]

        def relabel(rec):
            rec = np.array(rec)
            cls = cls_of[_region(rec)]
            hit = rec["instance"] != MISS
            rec["instance"] = np.where(hit, ids[cls], MISS)
            return rec, np.where(hit, cls, -1)

        hits, cls = relabel(g["hits"])
        prev, prev_cls = relabel(g["prev_hits"])
        carried_classes = [CLASSES.index(n) for n in CARRIED]
        built = np.isin(cls, carried_classes)
        prev["instance"][np.isin(prev_cls, carried_classes)] = MISS      # no record of such a class but the carried ones
        carried = carry(hits, recs)
        prev[built] = carried[built]
        g.update(hits=hits, prev_hits=prev, records=recs, beyond=beyond, classes=cls)
        args = (g["color"], hits, prev, g["prev_history"], g["view"], recs)
        g["history32"], _, g["valid32"] = accumulate_motion(*args, **KW)
        g["moments32"] = accumulate_motion(*args, albedo=g["albedo"], prev_moments=g["prev_moments"], moments=True, **KW)[:2]
        for arr in g.values():
            for a in (arr if isinstance(arr, tuple) else (arr,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _cache[key] = g
    return _cache[key]
