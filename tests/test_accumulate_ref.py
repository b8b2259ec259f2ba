"""tests/accumulate_ref.py, the numpy statement of rt_accumulate's filter, checked on its own (CPU): what the filter
must do whatever computes it; that its float32 form, whose bits the GPU test demands of the kernel, agrees with float64
on every GPU case — the same taps on at least 99 % of the hit pixels, and there within accumulate_ref.bound(); and
that leaving out any one tap or dropping any one validity test moves the float64 result by far more than that bound
on some case, so the GPU test cannot miss such a change."""
import numpy as np
import pytest

import accumulate_ref as R
from rtamd import abi, reprojection, scenes
from rtamd.renderer import ACCUMULATE_DEFAULTS

INF = float("inf")
KW = dict(max_history=R.MAX_HISTORY, normal_cos=R.NORMAL_COS, plane_tolerance=R.PLANE_TOLERANCE)
CASES = [(w, h, v) for (w, h) in R.SIZES for v in R.VIEWS]


def run(g, **over):
    kw = dict(KW)
    kw.update(over)
    view = kw.pop("view", g["view"])
    return R.accumulate(g["color"], g["hits"], g["prev_hits"], g["prev_history"], view, **kw)


def test_rows_send_every_pixel_centre_to_itself():
    for centre, target in (R.CAMERA, R.MOVED, R.PAN, R.BEHIND):
        cam = R.derive_camera(centre, target, 96, 64)
        rows = R.reprojection_rows(cam)
        jj, ii = np.mgrid[0:64, 0:96].astype(np.float64)
        x = np.asarray(cam["po"], np.float64) + ii[..., None] * cam["dx"] + jj[..., None] * cam["dy"]
        fx, fy, r2 = R.project(rows, x)
        assert np.abs(r2 - 1.0).max() <= 1e-12                # the image plane is at rw . v = 1
        assert max(np.abs(fx - ii).max(), np.abs(fy - jj).max()) <= 1e-10
        fx, fy, r2 = R.project(rows, 2.0 * np.asarray(cam["centre"], np.float64) - x)
        assert (r2 < 0.0).all()                               # behind the camera


def test_the_generators_camera_is_the_librarys(rtlib_path):
    """accumulate_ref.derive_camera restates rt_camera_set in numpy; rt_camera_reprojection derives its rows from the
    library's own camera.  The two agree where it matters: the library's rows send the pixel centres of the numpy
    camera to themselves within 16 eps32 (W + H) pixels, the bar tests/test_accumulate_abi.py holds them to against the
    oracle's camera."""
    abi.load_library(rtlib_path)
    scene = scenes.demo_scene()
    W, H = 96, 64
    for centre, target in (R.CAMERA, R.MOVED, R.PAN, R.BEHIND):
        cam = R.derive_camera(centre, target, W, H)
        r = reprojection(scene.camera_input(center=centre, target=target, fov=R.FOV, up=R.UP), W, H)
        rows = {k: np.array(list(getattr(r, k)), np.float64) for k in ("centre", "rx", "ry", "rw")}
        jj, ii = np.mgrid[0:H, 0:W].astype(np.float64)
        x = np.asarray(cam["po"], np.float64) + ii[..., None] * cam["dx"] + jj[..., None] * cam["dy"]
        fx, fy, r2 = R.project(rows, x)
        assert (r2 > 0.0).all()
        assert max(np.abs(fx - ii).max(), np.abs(fy - jj).max()) <= 16.0 * R.EPS32 * (W + H)


def test_the_python_defaults_are_valid_thresholds():
    max_history, normal_cos, plane_tolerance = ACCUMULATE_DEFAULTS
    assert max_history >= 1.0 and normal_cos <= 1.0 and plane_tolerance > 0.0
    g = R.case(37, 23, "moved")
    out, valid = run(g, max_history=max_history, normal_cos=normal_cos, plane_tolerance=plane_tolerance)
    assert valid.any() and np.isfinite(out).all() and out[..., 3].max() <= max_history


def test_first_frame_and_sky_reset():
    g = R.case(37, 23, "moved")
    out, valid = R.accumulate(g["color"], g["hits"], None, None, g["view"], **KW)
    assert np.array_equal(out[..., :3], g["color"].astype(np.float64)) and (out[..., 3] == 1.0).all()
    assert not valid.any()
    sky = g["hits"]["instance"] == R.MISS
    assert sky.any() and not sky.all()
    out = g["ref64"]
    assert np.array_equal(out[sky][:, :3], g["color"][sky].astype(np.float64)) and (out[sky][:, 3] == 1.0).all()
    assert (out[~sky][:, 3] > 1.0).any()


def test_max_history_one_returns_the_colour():
    """N = 1, a = 1: out = Hm + (c - Hm), the colour up to the two roundings of that expression — each at most half an
    ulp of the larger of |c| and |Hm|, both below 1.5 here."""
    g = R.case(37, 23, "moved")
    for dtype in (np.float64, np.float32):
        out, valid = run(g, max_history=1.0, dtype=dtype)
        assert valid.any()
        assert (out[..., 3] == 1.0).all()
        assert np.abs(out[..., :3] - g["color"].astype(dtype)).max() <= 2.0 * np.finfo(dtype).eps * 1.5


def test_static_frames_average():
    """Same records, view None, unbounded history: frame k's history is the running mean of the k + 1 colours."""
    rng = np.random.default_rng(3)
    g = R.case(9, 9, "null")
    hits = g["hits"]
    hit = hits["instance"] != R.MISS
    colors = rng.uniform(0.0, 1.0, (6,) + g["color"].shape).astype(np.float32)
    hist = None
    for k in range(6):
        hist, _ = R.accumulate(colors[k], hits, hits if k else None, hist, None, max_history=INF, normal_cos=0.9,
                               plane_tolerance=0.02)
        assert (hist[hit][:, 3] == k + 1).all()
        # the history is stored as float32 between frames: half an ulp of a value below 1 per frame
        assert np.abs(hist[hit][:, :3] - colors[:k + 1].astype(np.float64).mean(axis=0)[hit]).max() <= (k + 1) * R.EPS32 / 2
        hist = hist.astype(np.float32)


def test_behind_resets_everything_and_pan_loses_about_a_third():
    g = R.case(96, 64, "behind")
    assert not g["valid64"].any() and (g["ref64"][..., 3] == 1.0).all()
    g = R.case(96, 64, "pan")
    hit = g["hits"]["instance"] != R.MISS
    fx, fy, r2 = R.project(g["view"], g["hits"]["point"])
    outside = hit & ~((r2 > 0) & (fx >= -1) & (fx < 96) & (fy >= -1) & (fy < 64))
    share = outside.sum() / hit.sum()
    print(f"pan: {share:.2f} of the hit pixels land outside the last frame")
    assert 0.2 <= share <= 0.5
    assert (g["ref64"][outside][:, 3] == 1.0).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_%s" % c)
def test_float32_agrees_with_float64(case):
    W, H, view = case
    g = R.case(W, H, view)
    hit = g["hits"]["instance"] != R.MISS
    differ = (g["valid32"] != g["valid64"]).any(axis=-1)
    assert not differ[~hit].any()
    nhit, ndiff = int(hit.sum()), int(differ.sum())
    err = float(np.abs(g["ref32"].astype(np.float64) - g["ref64"])[~differ].max())
    bar = R.bound(W, H)
    print(f"{W}x{H} {view}: {ndiff} of {nhit} hit pixels differ in their taps; elsewhere max|ref32-ref64|={err:.3g}, "
          f"bound {bar:.3g}")
    assert g["ref32"].dtype == np.float32 and g["valid32"].shape == (H, W, 4)
    assert ndiff <= 0.01 * nhit
    assert err <= bar


CHANGES = [("skip_tap", t) for t in range(4)] + [("drop", d) for d in ("inside", "instance", "normal", "plane")]


@pytest.mark.parametrize("change", CHANGES, ids=lambda c: "%s_%s" % c)
def test_every_tap_and_every_test_moves_the_result(change):
    """Somewhere among the GPU cases the change moves ref64 by at least 100 bounds of that case."""
    best = 0.0
    for W, H, view in CASES:
        g = R.case(W, H, view)
        out, _ = run(g, **{change[0]: change[1]})
        moved = float(np.abs(out - g["ref64"]).max()) / R.bound(W, H)
        best = max(best, moved)
    print(f"{change[0]}={change[1]}: moves ref64 by up to {best:.3g} bounds")
    assert best >= 100.0
