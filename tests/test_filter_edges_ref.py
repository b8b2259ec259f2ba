"""tests/filter_edges_ref.py checked without a GPU: the conditions on the references that make
tests/test_gpu_filter_edges.py meaningful, and what each of the faults it is meant to catch would do to the references.

A  the restatement's reset set on the reprojection lattice equals the one derived by hand from the contract; float32
   and float64 take the same taps; a kept pixel's blend is the bilinear value of the tapped columns and rows; a +inf
   history texel reaches exactly the pixels that have it among their valid taps, weight 0 included.
B  the steady frames keep the colour bar sharp (F <= 1e-5) and at every hand-placed pixel the spatial and the temporal
   variance estimates lie at least 100 bar_v apart, so taking the wrong one cannot hide.
C  one non-finite colour turns exactly the box its taps reach non-finite in both float32 restatements and leaves
   every other pixel's bits alone.
Every figure printed here is in profiles/filter_edges/README.md."""
import numpy as np
import pytest

import accumulate_ref as A
import denoise_ref as D
import filter_edges_ref as E
import guided_ref as G

F32 = np.float32


# ---- A ---------------------------------------------------------------------------------------------------------------

def test_lattice_layout():
    pts = E.lattice_points()
    assert len(pts) == E.LW * E.LH == 192 and len(E.axis_values(E.LW)) == 13
    assert sum(p is None for p, _ in pts) == 192 - 169 - len(E.DENOMINATORS) - len(E.PLAIN) == 11
    assert pts[E.K_DENORMAL][1] == (3.0, 2.0) and pts[E.K_PLAIN][1] == (3.0, 2.0)
    z = pts[E.K_DENORMAL][0]
    tiny = float(np.finfo(F32).tiny)
    assert all(type(c) is F32 and 0 < float(c) < tiny for c in z)        # denormal, and exactly (3 Z, 2 Z, Z)
    assert float(z[0]) == 3 * 2.0 ** -130 and float(z[1]) == 2 * 2.0 ** -130 and float(z[2]) == 2.0 ** -130
    for n in (E.LW, E.LH):
        v = [float(x) for x in E.axis_values(n)]
        assert v[0] < -1.0 == v[1] < v[2] < v[3] < v[4] < 0.0 == v[5] == v[6] and np.signbit(E.axis_values(n)[5])
        assert 0.0 < -v[4] < tiny and v[10] == n - 1 and v[11] < n == v[12] and F32(v[11]) == E.axis_values(n)[11]
    hist = E.lattice()["prev_history"][..., 3]
    assert (hist != np.floor(hist)).any() and (hist > E.KW_A["max_history"]).any() and hist.min() >= 1.0


def test_reset_set_is_the_hand_derived_one():
    g, want = E.lattice(), E.hand_reset()
    for key in ("ref32", "ref64"):
        reset = g[key][..., 3] == 1.0
        assert np.array_equal(reset, want), key
        assert np.array_equal(g[key][reset][:, :3], np.tile(np.array(E.COLOUR, g[key].dtype), (int(reset.sum()), 1)))
        tapless = ~g["valid" + key[3:]].any(axis=-1)
        assert reset[tapless].all() and int((reset & ~tapless).sum()) == 21     # -1 on an axis, the other
        # inside the window (11 + 11 - 1 pairs): a valid tap of weight 0, D = 0
    pairs = want.reshape(-1)[:E.N_PAIRS]
    print(f"lattice: {int(want.sum())} of {want.size} pixels reset; {int(pairs.sum())} of the {E.N_PAIRS} pairs")
    # per axis 3 of the 13 values reset (outside below, -1 with D = 0, n outside): 169 - 10 * 10 pairs
    assert int(pairs.sum()) == 69 and int(want.sum()) == 69 + 6 + 11
    flat = want.reshape(-1)
    assert flat[E.N_PAIRS:E.K_DENORMAL].all() and not flat[E.K_DENORMAL] and not flat[E.K_PLAIN]
    assert E.same_bits(g["moments32"][0], g["ref32"])
    assert E.same_bits(g["ref32"].reshape(-1, 4)[E.K_DENORMAL], g["ref32"].reshape(-1, 4)[E.K_PLAIN])
    assert E.same_bits(g["moments32"][1].reshape(-1, 2)[E.K_DENORMAL], g["moments32"][1].reshape(-1, 2)[E.K_PLAIN])


def test_float32_and_float64_take_the_same_taps():
    g = E.lattice()
    assert np.array_equal(g["valid32"], g["valid64"])
    h = E.hand()
    for k, hh in enumerate(h):
        if hh is None:                                      # reset; at -1 the restatement still lists the tap of weight 0
            continue
        taps = [q for q, _ in hh["taps"]]
        want = E.lattice_points()[k][1]
        got = [(int(np.floor(float(want[0]))) + (t & 1), int(np.floor(float(want[1]))) + (t >> 1)) for t in range(4)
               if g["valid32"][k // E.LW, k % E.LW, t]]
        assert got == taps, k
    zero = sum(any(b == 0 for _, b in hh["taps"]) for hh in h if hh is not None)
    print(f"lattice: {zero} kept pixels have a valid tap of weight exactly 0")
    assert zero >= 30


def test_kept_pixels_blend_the_tapped_columns_and_rows():
    """Undo out = Hm + a (c - Hm) with a = 1 / N: Hm.r is the bilinear value of qx + 1 over the inside columns, Hm.g of
    qy + 1 over the inside rows, within accumulate_ref.bound."""
    g, bound = E.lattice(), A.bound(E.LW, E.LH)
    for key in ("ref64", "ref32"):
        out, worst = g[key].astype(np.float64).reshape(-1, 4), 0.0
        for k, hh in enumerate(E.hand()):
            if hh is None:
                continue
            a = 1.0 / out[k, 3]
            assert out[k, 3] >= 2.0
            for ch, name in ((0, "r"), (1, "g")):
                worst = max(worst, abs((out[k, ch] - a * E.COLOUR[ch]) / (1.0 - a) - hh[name]))
        print(f"lattice {key}: max |Hm - bilinear| = {worst:.3g}, bound {bound:.3g}")
        assert worst <= bound


def test_an_infinite_texel_reaches_its_valid_taps_weight_zero_included():
    clean, g = E.lattice(), E.lattice(variant=True)
    assert np.isfinite(clean["ref32"]).all() and np.isfinite(clean["moments32"][1]).all()
    for key in ("ref32", "ref64"):
        bad = ~np.isfinite(g[key]).all(axis=-1)
        assert np.array_equal(bad, E.restatement_reaches(g["valid" + key[3:]], E.POISONED_TEXEL)), key
        assert np.array_equal(bad, E.hand_reaches(E.POISONED_TEXEL)), key
        assert bad.reshape(-1)[E.K_DENORMAL] and bad.reshape(-1)[E.K_PLAIN]          # the fx = 3.0 pixels
    assert E.same_bits(g["ref32"][~bad], clean["ref32"][~bad])
    assert np.array_equal(g["ref32"][..., 3], clean["ref32"][..., 3])                # the length is untouched
    print(f"variant: {int(bad.sum())} pixels non-finite, {int(E.hand_reaches(E.POISONED_TEXEL, skip_zero=True).sum())} "
          "if a tap of weight 0 were skipped")


def test_what_the_faults_would_do_to_the_lattice():
    """`fx > -1.0f` and `fx <= (float)W` change no output: at fx = -1 the only inside tap has weight exactly 0 and at
    fx = W no tap is inside, so D = 0 and the pixel resets with or without the window (the window guards the int cast,
    which the 1e30 pixel pins).  `if (b == 0.0f) continue;` changes the +inf variant's non-finite set."""
    want = E.hand_reset()
    for fault in (dict(lo="gt"), dict(hi="le"), dict(lo="gt", hi="le")):
        assert np.array_equal(E.hand_reset(**fault), want), fault
    assert np.array_equal(E.hand_reset(skip_zero=True), want)
    full, skipped = E.hand_reaches(E.POISONED_TEXEL), E.hand_reaches(E.POISONED_TEXEL, skip_zero=True)
    assert int(full.sum()) == 6 and int(skipped.sum()) == 2 and (full | skipped == full).all()


# ---- B ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(E.STEADY))
def test_steady_frames_meet_their_conditions(name):
    W, H, it, ask, quiet = E.STEADY[name]
    r = E.steady_reference(name)
    g = r["g"]
    N = g["history"][..., 3]
    asks = N < 4
    assert sorted(zip(*np.nonzero(asks.T))) == sorted(ask) and all(N[y, x] == F32(v[1]) for (x, y), v in {**ask, **quiet}.items())
    assert (N[~asks] >= 4).all()
    tiles = {(x // 16, y // 16) for x, y in ask}
    if name == "35x34":
        assert tiles == {(0, 0), (1, 0), (1, 1), (2, 2), (0, 1)} and int((~asks).sum()) == 1183
        assert N[15, 16] == F32(E.ABOVE_4) > 4.0 and N[16, 16] == F32(E.BELOW_4)
    else:
        assert tiles == {(2, 1)} and (W - 1, H - 1) in ask
    spatial, temporal = E.estimates(r)
    gaps = {p: abs(spatial[p[1], p[0]] - temporal[p[1], p[0]]) / r["barv"] for p in {**ask, **quiet}}
    print(f"{name}: F = {r['F']:.3g}, bar = {r['bar']:.3g}, F_v = {r['Fv']:.3g}, bar_v = {r['barv']:.3g}; the smallest gap "
          f"between the estimates at a placed pixel is {min(gaps.values()):.0f} bar_v at {min(gaps, key=gaps.get)}")
    assert r["F"] <= 1e-5
    assert min(gaps.values()) >= 100.0, gaps
    # where N >= 4, v_0 is max(0, m2 - m1 m1) / N in plain float32: restated here once more, on its own
    m = r["moments"]
    own = np.maximum(F32(0), m[..., 1] - m[..., 0] * m[..., 0]) / N
    assert own.dtype == F32 and E.same_bits(own[~asks], r["v32"][~asks])


def test_what_the_pack_kernels_fault_would_do():
    """`hist.w > GD_MIN_LENGTH` is the restatement's threshold one float32 step above 4: the pixels with N = 4.0 exactly
    would take the spatial estimate, at least 100 bar_v from the temporal one."""
    W, H, it, ask, quiet = E.STEADY["35x34"]
    r = E.steady_reference("35x34")
    g = r["g"]
    out, v0 = G.guided(g["history"], r["moments"], g["normal"], g["point"], g["miss"], r["albedo"], dtype=np.float64,
                       threshold=E.ABOVE_4, **r["kw"])
    moved = np.abs(v0 - r["v64"]) / r["barv"]
    at4 = [p for p, v in quiet.items() if v[1] == 4.0]
    assert sorted(zip(*np.nonzero((moved > 0).T))) == sorted(at4) == [(15, 16), (33, 33)]
    print(f"threshold > 4: v_0 moves by {moved[16, 15]:.0f} and {moved[33, 33]:.0f} bar_v at the two pixels with N = 4.0, "
          f"the colour by {np.abs(out - r['out64']).max() / r['bar']:.1f} bars")
    assert min(moved[y, x] for x, y in at4) >= 100.0
    # `hist.w > 3.0f`, which agrees with `>= 4` on every whole length: the threshold one step above 3
    _, v0 = G.guided(g["history"], r["moments"], g["normal"], g["point"], g["miss"], r["albedo"], dtype=np.float64,
                     threshold=float(np.nextafter(F32(3), F32(4))), **r["kw"])
    moved = np.abs(v0 - r["v64"]) / r["barv"]
    between = [p for p, v in ask.items() if 3.0 < v[1] < 4.0]
    assert sorted(zip(*np.nonzero((moved > 0).T))) == sorted(between) == [(16, 16), (32, 32)]
    print(f"threshold > 3: v_0 moves by {moved[16, 16]:.0f} and {moved[32, 32]:.0f} bar_v at the pixels with N = 3.9999998, 3.75")
    assert min(moved[y, x] for x, y in between) >= 100.0


# ---- C ---------------------------------------------------------------------------------------------------------------

def run_denoise(g, color, it):
    with np.errstate(all="ignore"):
        return D.denoise(color, g["normal"], g["point"], g["miss"], g["albedo"], dtype=np.float32, iterations=it,
                         sigma_color=D.SIGMAS[0], sigma_normal=D.SIGMAS[1], sigma_plane=D.SIGMAS[2])


def run_guided(r, history):
    g = r["g"]
    with np.errstate(all="ignore"):
        return G.guided(history, r["moments"], g["normal"], g["point"], g["miss"], r["albedo"], dtype=np.float32, **r["kw"])


@pytest.mark.parametrize("case", E.POISON_CASES, ids=lambda c: "%dx%d_it%d" % c)
def test_one_non_finite_colour_poisons_its_box_and_nothing_else(case):
    W, H, it = case
    g = D.synth(W, H)
    r = G.reference(W, H, it)
    clean_d = run_denoise(g, g["color"], it)
    clean_g, clean_v = run_guided(r, r["g"]["history"])
    assert E.same_bits(clean_d, D.reference(W, H, it)[2]) and E.same_bits(clean_g, r["out32"])
    shares, shielded = [], []
    for z in E.positions(g["miss"]):
        want = E.box(W, H, it, z)
        shares.append(1.0 - want.mean())
        shielded.append(int((want & ~E.shielded(g["miss"], it, z)).sum()))
        assert int(want.sum()) >= 9
        for value in E.POISON_VALUES:
            out = run_denoise(g, E.poisoned(g["color"], z, value), it)
            bad = ~np.isfinite(out).all(axis=-1)
            assert np.array_equal(bad, want), ("rt_denoise", z, value)
            assert E.same_bits(out[~bad], clean_d[~bad])
            hist = np.array(r["g"]["history"])
            hist[..., :3] = E.poisoned(hist[..., :3], z, value)
            out, v0 = run_guided(r, hist)
            bad = ~np.isfinite(out).all(axis=-1)
            assert np.array_equal(bad, want), ("rt_denoise_guided", z, value)
            assert E.same_bits(out[~bad], clean_g[~bad]) and E.same_bits(v0, clean_v)
    z = E.positions(g["miss"])[3]
    assert g["miss"][z[1], z[0]] and not g["miss"][z[1], z[0] - 1]
    print(f"{W}x{H} it={it}: finite share {min(shares):.2f} .. {max(shares):.2f}; a tap that returned early across the "
          f"hit / sky boundary would spare {shielded} pixels of the four boxes")
    assert min(shares) >= 0.5
    assert shielded[3] >= 1            # the boundary position's box crosses the boundary: the fault shows there


def test_a_nan_in_this_frames_colour_stays_in_its_pixel():
    g = G.moments_case(9, 9, "moved")
    kept = np.argwhere(g["ref32"][..., 3] > 1.0)
    y, x = kept[len(kept) // 2]
    color = np.array(g["color"])
    color[y, x, 1] = E.NAN
    out, _ = A.accumulate(color, g["hits"], g["prev_hits"], g["prev_history"], g["view"], dtype=np.float32,
                          max_history=A.MAX_HISTORY, normal_cos=A.NORMAL_COS, plane_tolerance=A.PLANE_TOLERANCE)
    bad = ~np.isfinite(out).all(axis=-1)
    assert bad.sum() == 1 and bad[y, x] and np.isnan(out[y, x, 1]) and np.isfinite(out[y, x, [0, 2, 3]]).all()
    assert out[y, x, 3] == g["ref32"][y, x, 3] > 1.0 and E.same_bits(out[~bad], g["ref32"][~bad])
