"""tests/feedback_ref.py pinned without a GPU: on the still-camera sequence (64 x 48, 24 frames, 3 passes, float32)
feeding the first pass's colour back as history lowers the flicker of the guided chain's output to at most 0.92 of the
plain chain's and does not raise the last frame's error.  The reference gives 0.83 - 0.85 and 0.93 - 0.95 for seeds
0 - 3; 0.92 lies halfway between that and "no effect".  Feeding the second pass back instead leaves the flicker where
it is and raises the error by about 1.56: the test notices which pass is fed back."""
import numpy as np
import pytest

import feedback_ref as FB
import guided_ref as G

W, H, FRAMES = 64, 48, 24


def figures(seed, **how):
    s = FB.inputs(W, H, FRAMES, seed)
    miss = s["g"]["miss"]
    out = FB.chain(W, H, FRAMES, seed=seed, **how)
    return FB.flicker(out, miss), FB.rmse(out, s["albedo"], s["truth"], miss)


@pytest.mark.parametrize("seed", (0, 1))
def test_feedback_lowers_the_flicker_and_not_the_accuracy(seed):
    f_plain, e_plain = figures(seed, feedback_on=False)
    f_fb, e_fb = figures(seed, feedback_on=True)
    print(f"seed {seed}: flicker {f_fb:.6f} / {f_plain:.6f} = {f_fb / f_plain:.3f}, RMSE {e_fb:.6f} / {e_plain:.6f} = {e_fb / e_plain:.3f}")
    assert f_fb <= 0.92 * f_plain
    assert e_fb <= e_plain


def test_feeding_back_the_second_pass_is_noticed():
    _, e_plain = figures(0, feedback_on=False)
    f_2, e_2 = figures(0, feedback_on=True, fed_pass=2)
    print(f"pass 2 fed back: RMSE {e_2:.6f} / {e_plain:.6f} = {e_2 / e_plain:.3f}")
    assert not e_2 <= e_plain                                 # the first test's inequality fails; the ratio is 1.56


@pytest.mark.parametrize("with_albedo", (True, False), ids=("albedo", "plain"))
def test_feedback_is_the_first_pass_with_the_historys_length(with_albedo):
    r = G.reference(37, 23, 1, with_albedo=with_albedo)
    g = r["g"]
    kw = {k: v for k, v in r["kw"].items() if k != "iterations"}
    for dtype in (np.float32, np.float64):
        fb = FB.feedback(g["history"], r["moments"], g["normal"], g["point"], g["miss"], r["albedo"], dtype=dtype, **kw)
        assert fb.shape == (23, 37, 4) and fb.dtype == dtype
        assert np.array_equal(fb[..., :3], r["out32" if dtype is np.float32 else "out64"])
        assert np.array_equal(fb[..., 3].astype(np.float32).view(np.uint32), np.ascontiguousarray(g["history"][..., 3]).view(np.uint32))
    assert len(np.unique(g["history"][..., 3])) > 3           # the lengths are not all one value
