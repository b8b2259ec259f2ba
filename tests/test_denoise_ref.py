"""tests/denoise_ref.py, the numpy statement of rt_denoise's filter, checked on its own (CPU): what the filter must do
whatever computes it, and the condition that keeps the GPU test's bar honest — on every GPU case, leaving any single
tap out of any pass moves the float64 result by at least 10 x that case's bar somewhere, so a kernel that drops, or
doubles, or misplaces one tap cannot pass."""
import numpy as np
import pytest

import denoise_ref as R

INF = float("inf")


def run(g, albedo=None, **kw):
    kw.setdefault("iterations", 3)
    for k, v in zip(("sigma_color", "sigma_normal", "sigma_plane"), R.SIGMAS):
        kw.setdefault(k, v)
    return R.denoise(g["color"], g["normal"], g["point"], g["miss"], albedo, **kw)


def test_constant_image_stays_constant():
    g = dict(R.synth(23, 19))
    g["color"] = np.full_like(g["color"], 0.375)
    for dtype, tol in ((np.float64, 1e-15), (np.float32, 5e-7)):
        out = run(g, iterations=5, dtype=dtype)
        assert out.dtype == dtype
        assert np.abs(out - 0.375).max() <= tol


def test_all_sigmas_off_is_the_b3_convolution():
    g = dict(R.synth(21, 17, seed=2))
    g["miss"] = np.zeros_like(g["miss"])
    out = run(g, iterations=2, sigma_color=INF, sigma_normal=INF, sigma_plane=INF)
    k = np.array(R.K)
    c = g["color"].astype(np.float64)
    for step in (1, 2):                        # interior pixels: every tap inside, so the weights sum to 1
        nxt = np.full_like(c, np.nan)
        m = 2 * step
        for y in range(m, 17 - m):
            for x in range(m, 21 - m):
                win = c[y - m:y + m + 1:step, x - m:x + m + 1:step]
                nxt[y, x] = np.einsum("i,j,ijc->c", k, k, win)
        c = nxt
    inner = ~np.isnan(c[..., 0])
    assert inner.sum() == (17 - 12) * (21 - 12)
    assert np.abs(out[inner] - c[inner]).max() <= 1e-14


def test_hit_miss_boundary_is_never_crossed():
    g = dict(R.synth(24, 16, seed=3))
    assert g["miss"].any() and not g["miss"].all()
    color = np.where(g["miss"][..., None], np.float32(5.0), np.float32(0.25)).astype(np.float32) * np.ones(3, np.float32)
    g["color"] = color
    out = run(g, iterations=5, sigma_color=INF)        # colour term off: only the miss rule separates the two
    assert np.abs(out[g["miss"]] - 5.0).max() <= 1e-12
    assert np.abs(out[~g["miss"]] - 0.25).max() <= 1e-12


def test_normal_step_is_kept():
    H, W = 12, 32
    rng = np.random.default_rng(5)
    normal = np.zeros((H, W, 3), np.float32)
    normal[:, :W // 2] = (0.0, 0.0, 1.0)
    normal[:, W // 2:] = (1.0, 0.0, 0.0)
    level = np.where(np.arange(W) < W // 2, 0.2, 0.8)[None, :, None]
    g = {"color": (level + rng.uniform(-0.05, 0.05, (H, W, 3))).astype(np.float32), "normal": normal,
         "point": np.zeros((H, W, 3), np.float32), "miss": np.zeros((H, W), bool)}
    out = run(g, iterations=4, sigma_color=INF, sigma_normal=0.1, sigma_plane=INF)
    left, right = out[:, :W // 2], out[:, W // 2:]
    assert np.abs(left - 0.2).max() < 0.05 and np.abs(right - 0.8).max() < 0.05      # no bleed across the step
    assert left.std() < 0.5 * g["color"][:, :W // 2].std()                          # yet each side is smoothed
    blurred = run(g, iterations=4, sigma_color=INF, sigma_normal=INF, sigma_plane=INF)
    assert np.abs(blurred[:, W // 2 - 1] - 0.2).max() > 0.1                          # without the term it bleeds


def test_noise_variance_falls_with_every_pass():
    H, W = 48, 48
    rng = np.random.default_rng(9)
    normal = np.zeros((H, W, 3), np.float32)
    normal[..., 2] = 1.0
    g = {"color": (0.5 + rng.uniform(-0.2, 0.2, (H, W, 3))).astype(np.float32), "normal": normal,
         "point": np.zeros((H, W, 3), np.float32), "miss": np.zeros((H, W), bool)}
    var = [float(g["color"].astype(np.float64).var())]
    for it in range(1, 6):
        var.append(float(run(g, iterations=it, sigma_color=4.0).var()))
    assert all(b < a for a, b in zip(var, var[1:])), var


@pytest.mark.parametrize("with_albedo", (True, False), ids=("albedo", "plain"))
@pytest.mark.parametrize("case", R.GPU_CASES, ids=lambda c: "%dx%d_it%d" % c)
def test_every_tap_moves_the_result_by_ten_bars(case, with_albedo):
    W, H, it = case
    g, r64, _, F, bar = R.reference(W, H, it, with_albedo)
    assert F <= 2e-6, F                          # the float32 restatement's own error: what the bar is made of
    alb = g["albedo"] if with_albedo else None
    weakest = INF
    for i in range(it):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if not R.lands(W, H, 1 << i, dx, dy):
                    continue
                out = run(g, alb, iterations=it, skip=(i, dx, dy))
                diff = np.abs(out - r64)
                moved = float(np.nanmax(diff)) if not np.isnan(diff).all() else INF
                if np.isnan(diff).any():        # the only tap of a pixel left out: 0 / 0
                    moved = INF
                weakest = min(weakest, moved)
                assert moved >= 10.0 * bar, (case, (i, dx, dy), moved, bar)
    print(f"{W}x{H} it={it} albedo={with_albedo}: F={F:.3g} bar={bar:.3g} weakest tap moves {weakest:.3g}")
