"""rt_accumulate, rt_accumulate_moments, rt_denoise_guided and rt_denoise on the GPU where they decide
(tests/filter_edges_ref.py; tests/test_filter_edges_ref.py shows on the references what these tests would notice).

A  the reprojection lattice, 24 x 8: the window's ends, floorf's steps, taps of weight exactly 0, the denominator's sign,
   zero, NaN and a float32 denormal.  History, rgb32 and moments equal the float32 restatements bit for bit in both
   pixel mappings; the reset set is the one derived by hand; a +inf history texel reaches the restatement's pixels.
B  steady frames, 35 x 34 and 33 x 18: lengths a float32 step either side of 4, fractional lengths, and requests for the
   spatial variance estimate in some 16 x 16 tiles only, so the tile kernel's vote sends the others home.  Within the
   existing bars of the float64 reference; where N >= 4, v_0 has the float32 restatement's bits.
C  one NaN or +inf colour: exactly the box its taps reach turns non-finite, every other pixel keeps the bits of the
   same call on the clean input.

Every call goes through the guarded buffers of the harnesses of tests/test_gpu_guided.py and tests/test_gpu_denoise.py.
No image is larger than 257 x 34."""
import numpy as np
import pytest

import accumulate_ref as A
import denoise_ref as D
import filter_edges_ref as E
import guided_ref as G
from test_gpu_denoise import denoise
from test_gpu_denoise import upload as upload_denoise
from test_gpu_guided import accumulate, denoise_guided, upload_acc
from test_gpu_guided import upload as upload_guided

pytestmark = pytest.mark.gpu

F32 = np.float32
same_bits = E.same_bits


# ---- A ---------------------------------------------------------------------------------------------------------------

@pytest.fixture
def lattice_thresholds(monkeypatch):
    """The harness takes its thresholds from accumulate_ref; the lattice switches the plane test off."""
    monkeypatch.setattr(A, "PLANE_TOLERANCE", E.KW_A["plane_tolerance"])
    assert (A.MAX_HISTORY, A.NORMAL_COS, A.PLANE_TOLERANCE) == tuple(E.KW_A.values())


@pytest.mark.parametrize("form", ("r", "b"))
def test_reprojection_lattice_bit_for_bit(gpu_lib, monkeypatch, lattice_thresholds, form):
    monkeypatch.setenv("RTAMD_ACCUMULATE_FORM", form)
    g = E.lattice()
    t = upload_acc(g)
    want_reset = E.hand_reset()
    colour = np.array(E.COLOUR, F32)
    for moments in (False, True):
        hist, rgb, mom = accumulate(gpu_lib, t, g["view"], moments=moments)
        wrong = (hist.view(np.uint32) != g["ref32"].view(np.uint32)).any(axis=-1)
        print(f"lattice form={form} moments={moments}: {int(wrong.sum())} of {wrong.size} pixels differ from ref32 "
              f"{np.argwhere(wrong)[:8].tolist()}; {int((hist[..., 3] == 1.0).sum())} reset")
        flat = hist.reshape(-1, 4)
        print(f"  denormal pixel {flat[E.K_DENORMAL]}, plain (3, 2) pixel {flat[E.K_PLAIN]}")
        assert np.array_equal(hist[..., 3] == 1.0, want_reset)
        assert same_bits(hist[want_reset][:, :3], np.tile(colour, (int(want_reset.sum()), 1)))
        assert same_bits(flat[E.K_DENORMAL], flat[E.K_PLAIN])
        assert not wrong.any()
        assert same_bits(rgb, hist[..., :3])
        if moments:
            assert same_bits(mom, g["moments32"][1])
            assert same_bits(mom.reshape(-1, 2)[E.K_DENORMAL], mom.reshape(-1, 2)[E.K_PLAIN])


@pytest.mark.parametrize("form", ("r", "b"))
def test_an_infinite_history_texel_reaches_its_valid_taps(gpu_lib, monkeypatch, lattice_thresholds, form):
    monkeypatch.setenv("RTAMD_ACCUMULATE_FORM", form)
    g = E.lattice(variant=True)
    t = upload_acc(g)
    want = ~np.isfinite(g["ref32"]).all(axis=-1)
    assert int(want.sum()) == 6
    for moments in (False, True):
        hist, rgb, mom = accumulate(gpu_lib, t, g["view"], moments=moments)
        bad = ~np.isfinite(hist).all(axis=-1)
        print(f"variant form={form} moments={moments}: non-finite at {np.argwhere(bad).tolist()}")
        assert np.array_equal(bad, want)
        assert np.array_equal(bad, E.hand_reaches(E.POISONED_TEXEL))
        assert same_bits(hist[~bad], g["ref32"][~bad]) and same_bits(hist[..., 3], g["ref32"][..., 3])
        assert np.array_equal(np.isnan(hist), np.isnan(g["ref32"])) and np.array_equal(np.isinf(hist), np.isinf(g["ref32"]))
        assert same_bits(rgb[~bad], hist[~bad][:, :3]) and np.array_equal(np.isfinite(rgb), np.isfinite(hist[..., :3]))
        if moments:
            assert same_bits(mom, g["moments32"][1])          # the moments' taps read no colour


# ---- B ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(E.STEADY))
def test_steady_frames_fractional_lengths_and_sparse_requests(gpu_lib, monkeypatch, name):
    W, H, it, ask, quiet = E.STEADY[name]
    r = E.steady_reference(name)
    t = upload_guided(r)
    monkeypatch.delenv("RTAMD_GUIDED_PREP", raising=False)
    rgb, rgba, v0 = denoise_guided(gpu_lib, t, it)
    err = float(np.abs(rgb.astype(np.float64) - r["out64"]).max())
    verr = float(np.abs(v0.astype(np.float64) - r["v64"]).max())
    trusted = r["g"]["history"][..., 3] >= 4
    differ = (v0.view(np.uint32) != r["v32"].view(np.uint32)) & trusted
    print(f"steady {name}: max|gpu-ref64|={err:.3g} F={r['F']:.3g} ratio={err / r['F']:.2f} bar={r['bar']:.3g}; v_0: {verr:.3g} "
          f"bar_v={r['barv']:.3g}; {int(differ.sum())} of {int(trusted.sum())} pixels with N >= 4 differ from v32 "
          f"{np.argwhere(differ)[:8].tolist()}")
    for (x, y) in {**ask, **quiet}:
        print(f"  ({x}, {y}): N={r['g']['history'][y, x, 3]!r} v_0 gpu={v0[y, x]:.6g} ref64={r['v64'][y, x]:.6g}")
    assert np.isfinite(rgb).all() and np.isfinite(v0).all()
    assert verr <= r["barv"], (name, verr, r["barv"])
    assert err <= r["bar"], (name, err, r["bar"])
    assert not differ.any()
    assert np.array_equal(rgba, D.quantise(rgb))
    for form in ("t", "d"):
        monkeypatch.setenv("RTAMD_GUIDED_PREP", form)
        rgb_f, _, v0_f = denoise_guided(gpu_lib, t, it)
        assert same_bits(v0_f, v0) and same_bits(rgb_f, rgb), form
        assert same_bits(denoise_guided(gpu_lib, t, it, variance=False)[0], rgb), form


# ---- C ---------------------------------------------------------------------------------------------------------------

def check_poisoned(name, out, clean, want):
    bad = ~np.isfinite(out[0]).all(axis=-1)
    print(f"{name}: {int(bad.sum())} pixels non-finite, the box has {int(want.sum())}")
    assert np.array_equal(bad, want), name
    assert same_bits(out[0][~bad], clean[0][~bad]), name
    with np.errstate(invalid="ignore"):                       # what a NaN quantises to is not pinned
        assert np.array_equal(out[1][~bad], D.quantise(out[0])[~bad]), name


@pytest.mark.parametrize("case", E.POISON_CASES, ids=lambda c: "%dx%d_it%d" % c)
def test_denoise_one_non_finite_colour(gpu_lib, monkeypatch, case):
    W, H, it = case
    g = D.synth(W, H)
    for forms in (None, "ddd", "rrr") if case == (257, 5, 4) else (None,):
        if forms is None:
            monkeypatch.delenv("RTAMD_DENOISE_FORMS", raising=False)
        else:
            monkeypatch.setenv("RTAMD_DENOISE_FORMS", forms)
        clean = denoise(gpu_lib, upload_denoise(g), it)
        assert np.isfinite(clean[0]).all()
        for z in E.positions(g["miss"]):
            for value in E.POISON_VALUES:
                p = dict(g)
                p["color"] = E.poisoned(g["color"], z, value)
                out = denoise(gpu_lib, upload_denoise(p), it)
                check_poisoned("rt_denoise %dx%d it=%d forms=%s z=%s %s" % (W, H, it, forms, z, value), out, clean,
                               E.box(W, H, it, z))


@pytest.mark.parametrize("case", E.POISON_CASES, ids=lambda c: "%dx%d_it%d" % c)
def test_guided_one_non_finite_colour(gpu_lib, case):
    import torch
    W, H, it = case
    r = G.reference(W, H, it)
    t = upload_guided(r)
    clean = denoise_guided(gpu_lib, t, it)
    assert np.isfinite(clean[0]).all()
    for z in E.positions(r["g"]["miss"]):
        for value in E.POISON_VALUES:
            hist = np.array(r["g"]["history"])
            hist[..., :3] = E.poisoned(hist[..., :3], z, value)
            p = dict(t)
            p["history"] = torch.from_numpy(hist).cuda()
            out = denoise_guided(gpu_lib, p, it)
            check_poisoned("rt_denoise_guided %dx%d it=%d z=%s %s" % (W, H, it, z, value), out, clean, E.box(W, H, it, z))
            assert same_bits(out[2], clean[2])                # v_0 reads no colour


def test_accumulate_a_nan_colour_stays_in_its_pixel(gpu_lib):
    import torch
    g = G.moments_case(9, 9, "moved")
    kept = np.argwhere(g["ref32"][..., 3] > 1.0)
    y, x = kept[len(kept) // 2]
    t = upload_acc(g)
    for moments in (False, True):
        clean = accumulate(gpu_lib, t, g["view"], moments=moments)
        color = np.array(g["color"])
        color[y, x, 1] = E.NAN
        p = dict(t)
        p["color"] = torch.from_numpy(color).cuda()
        hist, rgb, mom = accumulate(gpu_lib, p, g["view"], moments=moments)
        bad = ~np.isfinite(hist).all(axis=-1)
        assert int(bad.sum()) == 1 and bad[y, x] and np.isnan(hist[y, x, 1]) and np.isnan(rgb[y, x, 1])
        assert hist[y, x, 3] == g["ref32"][y, x, 3] > 1.0
        assert same_bits(hist[~bad], clean[0][~bad]) and same_bits(rgb[~bad], clean[1][~bad])
        assert same_bits(hist[y, x, [0, 2, 3]], clean[0][y, x, [0, 2, 3]])
        if moments:                                           # the moments are of the luminance, which reads green
            mbad = ~np.isfinite(mom).all(axis=-1)
            assert int(mbad.sum()) == 1 and mbad[y, x] and same_bits(mom[~mbad], clean[2][~mbad])
