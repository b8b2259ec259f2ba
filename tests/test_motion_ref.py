"""tests/motion_ref.py and rt_instance_motion_records, without a GPU.

The restatement of the MOTION kernel: with static records it is accumulate_ref / guided_ref bit for bit; on the classes
whose maps float32 applies exactly it keeps what the uncompensated call resets; and each fault a kernel could have
changes its output, so the GPU test's bit comparison would notice it.

The host helper: the bits that depend on no libm (equal transforms, pure shifts, pure axis scales, singular
transforms), and general transforms against the float64 restatement on the oracle's forward matrices."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import accumulate_ref as A
import guided_ref as G
import motion_ref as M
import xform_edges_ref as X
from rtamd import abi, scenes

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(w, h, v) for (w, h) in A.SIZES for v in M.VIEWS]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def static_records(n):
    r = np.zeros(n, M.motion_dtype())
    r["point"], r["normal"], r["flags"] = np.eye(3, 4, dtype=F32), np.eye(3, dtype=F32), M.STATIC
    return r


# ---- the kernel's restatement ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(w, h, v) for (w, h) in A.SIZES for v in A.VIEWS], ids=lambda c: "%dx%d_%s" % c)
def test_static_records_give_the_parents_bits(case):
    g = G.moments_case(*case)
    for records in (static_records(2), static_records(1), static_records(0)):     # the sphere's id in range, past them, none
        h, _, valid = M.accumulate_motion(g["color"], g["hits"], g["prev_hits"], g["prev_history"], g["view"], records, **M.KW)
        assert np.array_equal(bits(h), bits(g["ref32"])) and np.array_equal(valid, g["valid32"])
        h, m, _ = M.accumulate_motion(g["color"], g["hits"], g["prev_hits"], g["prev_history"], g["view"], records,
                                      albedo=g["albedo"], prev_moments=g["prev_moments"], moments=True, **M.KW)
        assert np.array_equal(bits(h), bits(g["with_albedo32"][0])) and np.array_equal(bits(m), bits(g["with_albedo32"][1]))
    first = M.accumulate_motion(g["color"], g["hits"], None, None, g["view"], static_records(2), albedo=g["albedo"],
                                moments=True, **M.KW)
    assert np.array_equal(bits(first[0]), bits(g["first32"][0])) and np.array_equal(bits(first[1]), bits(g["first32"][1]))


def test_exact_classes_keep_with_records_what_resets_without():
    """Over every case: a pixel of an EXACT class on the floor (normal (0, 1, 0), which every such map raises by LIFT
    exactly) whose plane tolerance is below LIFT.  With the records, those whose four taps lie on their instance in the
    previous frame keep their history: all four taps enter the blend and the length is the blended one plus one.
    Without records every one of them resets: whichever previous pixel the uncarried point looks at, a record of its
    instance there is LIFT off its plane."""
    kept = {name: 0 for name in M.EXACT}
    sphere_kept = 0
    for case in CASES:
        g = M.case(*case)
        none = M.accumulate_motion(g["color"], g["hits"], g["prev_hits"], g["prev_history"], g["view"], g["records"][:0], **M.KW)
        tol = F32(A.PLANE_TOLERANCE) * g["hits"]["t"]
        floor = (g["hits"]["normal"] == np.array([0, 1, 0], F32)).all(axis=-1) & (tol < F32(M.LIFT))
        for name in M.EXACT:
            cls = g["classes"] == M.CLASSES.index(name)
            four = cls & floor & g["valid32"].all(axis=-1)
            kept[name] += int(four.sum())
            assert (g["history32"][four][:, 3] > 1.0).all()
            assert not none[2][cls & floor].any(), (case, name)
            assert (none[0][cls & floor][:, 3] == 1.0).all()
            assert np.array_equal(bits(none[0][cls & floor][:, :3]), bits(g["color"][cls & floor]))
            sphere_kept += int((cls & (g["hits"]["normal"][..., 1] != 1) & g["valid32"].any(axis=-1)).sum())
    print("pixels of the exact classes that keep all four taps:", kept, "and on the sphere, any tap:", sphere_kept)
    assert all(n > 0 for n in kept.values()), kept
    assert sphere_kept > 0                                  # normals that the scale's two maps send to different places


@pytest.mark.parametrize("fault", ("no_shift", "normal_A", "no_normalise", "flag7_static", "read_beyond"))
def test_each_fault_changes_some_pixel(fault):
    changed = 0
    for case in CASES:
        g = M.case(*case)
        h, _, _ = M.accumulate_motion(g["color"], g["hits"], g["prev_hits"], g["prev_history"], g["view"], g["records"],
                                      fault=fault, beyond=g["beyond"], **M.KW)
        changed += int((bits(h) != bits(g["history32"])).any(axis=-1).sum())
    print(f"{fault}: {changed} pixels change over the {len(CASES)} cases")
    assert changed > 0


def test_every_class_meets_every_kind_of_region():
    seen = {(c, r) for case in CASES for r, c in enumerate(M.assignment(*case))}
    assert seen == {(c, r) for c in range(len(M.CLASSES)) for r in range(M.REGIONS)}
    for case in CASES:
        assert len(set(M.assignment(*case))) == M.REGIONS         # a case's regions are distinct instances


# ---- rt_instance_motion_records --------------------------------------------------------------------------------------

def xform(shift=(0, 0, 0), rotate=(0, 0, 0), scale=(1, 1, 1)):
    return np.concatenate([np.asarray(v, F32) for v in (shift, rotate, scale)])


def records(lib_path, prev, cur):
    import rtamd
    abi.load_library(lib_path)
    return rtamd.instance_motion(np.asarray(prev, F32).reshape(-1, 9), np.asarray(cur, F32).reshape(-1, 9))


def test_equal_transforms_are_static(rtlib_path):
    xs = [xform((1.5, -2, 3), (10, 20, 30), (1, 2, 0.5)), xform(), xform(scale=(0, 0, 0)), xform(rotate=(np.nan, 0, 0))]
    r = records(rtlib_path, xs, xs)
    assert (r["flags"] == M.STATIC).all() and (r["reserved"] == 0).all()
    assert np.array_equal(r["point"], np.broadcast_to(np.eye(3, 4, dtype=F32), (4, 3, 4)))
    assert np.array_equal(r["normal"], np.broadcast_to(np.eye(3, dtype=F32), (4, 3, 3)))


def test_pure_shifts_subtract_in_double(rtlib_path):
    rng = np.random.default_rng(11)
    sp, sc = rng.uniform(-50, 50, (64, 3)).astype(F32), rng.uniform(-50, 50, (64, 3)).astype(F32)
    sc[:8] = np.nextafter(sp[:8], F32(np.inf))                 # one float apart
    r = records(rtlib_path, [xform(shift=s) for s in sp], [xform(shift=s) for s in sc])
    assert (r["flags"] == M.MOVED).all()
    assert np.array_equal(r["point"][:, :, :3], np.broadcast_to(np.eye(3, dtype=F32), (64, 3, 3)))
    assert np.array_equal(r["normal"], np.broadcast_to(np.eye(3, dtype=F32), (64, 3, 3)))
    assert np.array_equal(bits(r["point"][:, :, 3]), bits((sp.astype(np.float64) - sc.astype(np.float64)).astype(F32)))


def test_pure_axis_scales_divide(rtlib_path):
    rng = np.random.default_rng(12)
    sp, sc = rng.uniform(0.5, 2.0, (64, 3)).astype(F32), rng.uniform(0.5, 2.0, (64, 3)).astype(F32)
    sp[:4], sc[:4] = [(2, 1, 0.5), (3, 1.5, 0.75), (1, 1, 1), (-1, 2, -0.25)], [(1, 1, 1), (0.75, 3, 1.5), (1.25, 5, 0.625), (2, -1, 4)]
    r = records(rtlib_path, [xform(scale=s) for s in sp], [xform(scale=s) for s in sc])
    assert (r["flags"] == M.MOVED).all()
    ratio = (sp.astype(np.float64) / sc.astype(np.float64)).astype(F32)
    inverse = (sc.astype(np.float64) / sp.astype(np.float64)).astype(F32)
    off = ~np.eye(3, dtype=bool)
    assert (r["point"][:, :, :3][:, off] == 0).all() and (r["normal"][:, off] == 0).all() and (r["point"][:, :, 3] == 0).all()
    assert np.array_equal(bits(np.einsum("nii->ni", r["point"][:, :, :3])), bits(ratio))
    assert np.array_equal(bits(np.einsum("nii->ni", r["normal"])), bits(inverse))


def test_singular_transforms_have_no_history(rtlib_path):
    regular = xform((1, 2, 3), (10, 20, 30), (1, 2, 0.5))
    singular = [xform(rotate=X.CLASSES[n][0], scale=X.CLASSES[n][1]) for n in X.NAMES if X.group_of(n) == "singular"]
    singular += [xform(scale=(1, 0, 1)), xform((4, 5, 6), (30, 40, 50), (2, 2, 0)), xform(scale=(np.inf, 1, 1)),
                 xform(shift=(np.nan, 0, 0)), xform(rotate=(np.inf, 0, 0))]
    assert len(singular) == 8
    for prev, cur in ([singular, [regular] * 8], [[regular] * 8, singular]):
        r = records(rtlib_path, prev, cur)
        assert (r["flags"] == M.NO_HISTORY).all(), r["flags"]
        assert (r["point"] == 0).all() and (r["normal"] == 0).all() and (r["reserved"] == 0).all()
    # ... and every other class of tests/xform_edges_ref.py, the stress ones at the reference's thresholds included, moves
    others = [xform(rotate=X.CLASSES[n][0], scale=X.CLASSES[n][1]) for n in X.NAMES if X.group_of(n) != "singular"]
    r = records(rtlib_path, others, [regular] * len(others))
    assert (r["flags"] == M.MOVED).all(), r["flags"]
    r = records(rtlib_path, [regular] * len(others), others)
    assert (r["flags"] == M.MOVED).all(), r["flags"]


def test_null_arguments_and_empty_input(rtlib_path):
    lib = abi.load_library(rtlib_path)
    x, out = (abi.Xform * 2)(), (abi.InstanceMotion * 2)()
    assert lib.rt_instance_motion_records(x, x, 2, out) == abi.RT_OK
    for args in ((None, x, 2, out), (x, None, 2, out), (x, x, 2, None)):
        assert lib.rt_instance_motion_records(*args) == 1
        assert lib.rt_last_error()
    assert lib.rt_instance_motion_records(None, None, 0, None) == abi.RT_OK


N_GENERAL = 48


def general_xforms():
    """Well-conditioned transforms: scales in [0.5, 2], any angle, shifts up to 20."""
    rng = np.random.default_rng(2024)
    make = lambda: [xform(rng.uniform(-20, 20, 3), rng.uniform(-360, 360, 3), rng.uniform(0.5, 2.0, 3)) for _ in range(N_GENERAL)]
    return make(), make()


def oracle_forward(oracle_lib, xs):
    """The forward matrices [n, 3, 4] of the oracle's instances under xs: the suite pins them to the library's bits."""
    inst = [dict(type=abi.SPHERE, index=0, shift=tuple(x[0:3]), rotate=tuple(x[3:6]), scale=tuple(x[6:9])) for x in xs]
    scene = scenes.Scene(spheres=[(abi.ROUGH, 0, (0.0, 0.0, 0.0), 0.5)], parallelograms=[], triangles=np.zeros(0, scenes.TRIANGLE_DTYPE),
                         roughs=[(0.5, 0.5, 0.5)], metals=[], instances=inst, animated=False)
    o = oracle_lib.OracleScene(scene, build_seed=0)
    fwd = o.instance_state()[:, 12:24].reshape(-1, 3, 4).copy()
    o.close()
    return fwd


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(F32)).astype(np.float64)


def test_general_transforms_against_float64(rtlib_path, oracle_lib):
    """Both sides round once a double whose own error is about 1e-16 of its terms: they differ by at most one float32
    rounding, plus 1e-12 of the largest magnitude in the row where cancellation leaves an element near zero."""
    prev, cur = general_xforms()
    r = records(rtlib_path, prev, cur)
    fp, fc = oracle_forward(oracle_lib, prev), oracle_forward(oracle_lib, cur)
    worst = 0.0
    rng = np.random.default_rng(5)
    for i in range(N_GENERAL):
        flags, point, normal = M.records64(fp[i], fc[i])
        assert flags == r["flags"][i] == M.MOVED
        for got, want in ((r["point"][i], point), (r["normal"][i], normal)):
            bound = ulp32(want) + 1e-12 * np.abs(want).max(axis=1, keepdims=True)
            err = np.abs(got.astype(np.float64) - want)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (i, err, bound)
        # consistency: A (Fc p) + b is Fp p for local points p, with the same bound scaled by |p|
        p = rng.uniform(-2, 2, (16, 3))
        Fp, Fc = fp[i].astype(np.float64), fc[i].astype(np.float64)
        world_c, world_p = p @ Fc[:, :3].T + Fc[:, 3], p @ Fp[:, :3].T + Fp[:, 3]
        back = world_c @ r["point"][i][:, :3].astype(np.float64).T + r["point"][i][:, 3].astype(np.float64)
        # four terms per component, each off by at most one rounding of its record element times its factor
        scale = np.abs(r["point"][i]).max() * max(1.0, float(np.abs(world_c).max()))
        assert np.abs(back - world_p).max() <= 4 * (A.EPS32 + 1e-12) * scale, (i, np.abs(back - world_p).max())
    print(f"general transforms: worst error / bound = {worst:.3f}")


def test_stand_alone_program_under_sanitizers_gives_the_librarys_bytes(rtlib_path, tmp_path):
    """csrc/instance_motion.hpp in a host program of its own, built with the address and undefined-behaviour
    sanitizers: every kind of pair above in one run, the records byte for byte the library's; the program also holds
    the helper's singularity test to hm::inverse's exits."""
    exe = str(tmp_path / "instance_motion_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "cpp", "instance_motion_check.cpp")], check=True)
    regular = xform((1, 2, 3), (10, 20, 30), (1, 2, 0.5))
    edge = [xform(rotate=X.CLASSES[n][0], scale=X.CLASSES[n][1], shift=X.OFFSET) for n in X.NAMES]
    edge += [xform(scale=(np.inf, 1, 1)), xform(shift=(np.nan, 0, 0)), xform(rotate=(np.inf, 0, 0)), xform(scale=(1e30, 1e30, 1e30))]
    gp, gc = general_xforms()
    prev = edge + [regular] * len(edge) + edge + gp + [regular]
    cur = [regular] * len(edge) + edge + edge[1:] + edge[:1] + gc + [regular]
    pairs = np.stack([np.asarray(prev, F32), np.asarray(cur, F32)], axis=1)
    src, dst = str(tmp_path / "pairs.f32"), str(tmp_path / "records.bin")
    pairs.tofile(src)
    p = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = np.fromfile(dst, M.motion_dtype())
    want = records(rtlib_path, prev, cur)
    assert len(got) == len(want) == len(prev)
    assert got.tobytes() == want.tobytes()
    assert {int(f) for f in want["flags"]} == {M.STATIC, M.MOVED, M.NO_HISTORY}


def test_import_surface():
    import rtamd
    assert callable(rtamd.instance_motion) and C.sizeof(abi.InstanceMotion) == M.motion_dtype().itemsize == 96
