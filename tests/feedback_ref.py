"""rt_denoise_guided_feedback (include/rt.h, "History feedback") restated in numpy on tests/guided_ref.py, and the
still-camera sequence on which the feedback's effect is stated: the flicker of the guided chain's output and its error
against the noise-free frame, with the first pass's colour fed back as history and without.

denoise_ref, accumulate_ref and guided_ref are used as they are."""
import numpy as np

import denoise_ref as D
import guided_ref as G

F32 = np.float32
AMP_HIT, AMP_SKY = 0.5, 0.02
PASSES = 3                                                # the chain's filter passes
STRIPE = (0.7, 0.6, 0.5)                                  # replaces D.synth's albedo stripe below the floor


def sigmas():
    from rtamd.renderer import GUIDED_SIGMAS
    return dict(sigma_luminance=GUIDED_SIGMAS[0], sigma_normal=GUIDED_SIGMAS[1], sigma_plane=GUIDED_SIGMAS[2])


def feedback(history, moments, normal, point, miss, albedo=None, *, sigma_luminance, sigma_normal, sigma_plane,
             dtype=np.float64, fed_pass=1):
    """What rt_denoise_guided_feedback writes to feedback_device, [H, W, 4] in `dtype`: guided(..., iterations=1)'s
    image with the history's length appended.  fed_pass = 2, 3: the fault of feeding a later pass back."""
    img, _ = G.guided(history, moments, normal, point, miss, albedo, iterations=fed_pass, sigma_luminance=sigma_luminance,
                      sigma_normal=sigma_normal, sigma_plane=sigma_plane, dtype=dtype)
    length = np.asarray(history, F32)[..., 3:4].astype(dtype)
    out = np.concatenate([img, length], axis=-1)
    assert out.dtype == dtype
    return out


_cache = {}


def inputs(width, height, frames, seed=0):
    """The sequence's inputs, computed once and shared (read-only): guides, albedo, rt_hit records, the noise-free
    demodulated truth and the `frames` one-sample colours."""
    key = (width, height, frames, seed)
    if key not in _cache:
        from rtamd.renderer import HIT_DTYPE
        W, H = width, height
        g = dict(D.synth(W, H, seed))
        albedo = np.array(g["albedo"])
        albedo[albedo[..., 0] < 1e-3] = STRIPE
        g["albedo"] = albedo
        del g["color"]
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        truth = np.stack([0.55 + 0.35 * np.sin(0.03 * xx + 0.7 * ch) * np.cos(0.036 * yy - 0.4 * ch) for ch in range(3)], axis=-1)
        amp = np.where(g["miss"], AMP_SKY, AMP_HIT)[..., None]
        rng = np.random.default_rng(4242 + seed)
        colors = np.stack([(albedo.astype(np.float64) * truth * (1.0 + amp * rng.uniform(-1.0, 1.0, (H, W, 3)))).astype(F32)
                           for _ in range(frames)])
        r = {"g": g, "albedo": albedo, "truth": truth, "colors": colors, "hits": D.hit_records(g, HIT_DTYPE).reshape(H, W)}
        for a in (albedo, truth, colors, r["hits"], *g.values()):
            a.setflags(write=False)
        _cache[key] = r
    return _cache[key]


def chain(width, height, frames, feedback_on, seed=0, dtype=np.float32, fed_pass=1):
    """The still-camera sequence: per frame G.accumulate_moments (prev_hits = hits, view None, G.KW), then G.guided with
    the renderer's GUIDED_SIGMAS and PASSES iterations; with feedback_on the next prev_history is feedback(...) cast to
    float32, else the accumulated history.  -> the guided frames [frames, H, W, 3] in `dtype`."""
    key = (width, height, frames, bool(feedback_on), seed, np.dtype(dtype).name, fed_pass)
    if key not in _cache:
        s = inputs(width, height, frames, seed)
        g, hits, kw = s["g"], s["hits"], sigmas()
        hist, mom, outs = None, None, []
        for k in range(frames):
            first = hist is None
            hist, mom = G.accumulate_moments(s["colors"][k], s["albedo"], hits, None if first else hits, hist, mom, None,
                                             dtype=dtype, **G.KW)
            hist, mom = hist.astype(F32), mom.astype(F32)
            args = (hist, mom, g["normal"], g["point"], g["miss"], s["albedo"])
            outs.append(G.guided(*args, iterations=PASSES, dtype=dtype, **kw)[0])
            if feedback_on:
                hist = feedback(*args, dtype=dtype, fed_pass=fed_pass, **kw).astype(F32)
        out = np.stack(outs)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def flicker(out, miss):
    """Mean over hit pixels and channels of the standard deviation, over the second half of the frames, of
    sqrt(clip(out, 0, 1))."""
    gam = np.sqrt(np.clip(np.asarray(out, np.float64), 0.0, 1.0))
    return float(gam[len(gam) // 2:].std(axis=0)[~miss].mean())


def rmse(out, albedo, truth, miss):
    """The last frame against sqrt(albedo truth) over hit pixels, in gamma space."""
    gam = np.sqrt(np.clip(np.asarray(out[-1], np.float64), 0.0, 1.0))
    want = np.sqrt(np.asarray(albedo, np.float64) * truth)
    return float(np.sqrt(np.mean((gam - want)[~miss] ** 2)))
