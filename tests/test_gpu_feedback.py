"""rt_denoise_guided_feedback on the GPU (include/rt.h, "History feedback").

Over guided_ref.CASES, with and without albedo: the call's outputs are rt_denoise_guided's bit for bit, the feedback's
colour is bit for bit the rgb32 of rt_denoise_guided with one iteration and lies within guided_ref.reference(w, h, 1)'s
bar of the float64 result, its .w lane is the history's; then one pass only, the feedback aliased onto the history,
each output alone, NO_SYNC on a side stream, both forms of the variance kernel, the still-camera chain of
tests/feedback_ref.py run on the GPU, and the Renderer's option.

Every call here goes through buffers with guard bands around the outputs and the scratch, as tests/test_gpu_guided.py's."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as D
import feedback_ref as FB
import guided_ref as G
from rtamd import Renderer, abi, scenes
from rtamd.renderer import GUIDED_SIGMAS, HIT_DTYPE

pytestmark = pytest.mark.gpu

GUARD = 256                                    # bytes kept around every buffer a call writes (a multiple of 16)
FILL = 0xA5
OUTPUTS = (("rgb", 12, "rgb32_device"), ("rgba", 4, "rgba8_device"), ("variance", 4, "variance_device"))


def guarded(nbytes):
    import torch
    return torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")


def inner(buf, dtype, shape):
    return buf[GUARD:buf.numel() - GUARD].view(dtype).reshape(shape)


def guards_intact(bufs):
    for k, b in bufs.items():
        raw = b.cpu().numpy()
        assert (raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all(), f"{k}: bytes beyond the buffer were written"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def upload(r):
    import torch
    g = r["g"]
    H, W = g["miss"].shape
    return {"history": torch.from_numpy(np.array(g["history"])).cuda(), "moments": torch.from_numpy(np.array(r["moments"])).cuda(),
            "hits": torch.from_numpy(D.hit_records(g, HIT_DTYPE).view(np.uint8).reshape(H, W, 48).copy()).cuda(),
            "albedo": torch.from_numpy(np.array(r["albedo"])).cuda() if r["albedo"] is not None else None}


def call(lib, t, iterations, sigmas=G.SIGMAS, *, feedback="own", rgb=True, rgba=True, variance=True, stream=None, flags=0):
    """One call on guarded outputs and scratch -> {"rgb", "rgba", "variance", "feedback"} as numpy arrays (None where
    not asked for).  feedback: None = rt_denoise_guided; "own" = rt_denoise_guided_feedback into a guarded buffer;
    "alias" = into a guarded copy of the history, which is also the call's history_device."""
    import torch
    H, W = t["history"].shape[:2]
    n = W * H
    d = abi.DenoiseGuidedDesc()
    d.width, d.height, d.iterations, d.flags = W, H, iterations, flags
    d.sigma_luminance, d.sigma_normal, d.sigma_plane = sigmas
    bufs = {}
    for name, size, field in OUTPUTS:
        if {"rgb": rgb, "rgba": rgba, "variance": variance}[name]:
            bufs[name] = guarded(size * n)
            setattr(d, field, bufs[name].data_ptr() + GUARD)
    d.scratch_bytes = lib.rt_denoise_guided_scratch_bytes(W, H)
    bufs["scratch"] = guarded(int(d.scratch_bytes))
    d.scratch_device = bufs["scratch"].data_ptr() + GUARD
    d.history_device, d.moments_device, d.hits_device = t["history"].data_ptr(), t["moments"].data_ptr(), t["hits"].data_ptr()
    d.albedo_device = t["albedo"].data_ptr() if t["albedo"] is not None else None
    d.stream = stream.cuda_stream if stream is not None else None
    f = abi.FeedbackDesc()
    if feedback is not None:
        bufs["feedback"] = guarded(16 * n)
        f.feedback_device = bufs["feedback"].data_ptr() + GUARD
        assert f.feedback_device % 16 == 0
        if feedback == "alias":
            inner(bufs["feedback"], torch.float32, (H, W, 4)).copy_(t["history"])
            d.history_device = f.feedback_device
    torch.cuda.synchronize()
    if feedback is None:
        rc = lib.rt_denoise_guided(0, C.byref(d))
    else:
        rc = lib.rt_denoise_guided_feedback(0, C.byref(d), C.byref(f))
    assert rc == abi.RT_OK, lib.rt_last_error()
    if stream is not None:
        stream.synchronize()
    elif flags & abi.RT_DENOISE_NO_SYNC:
        torch.cuda.synchronize()
    guards_intact(bufs)
    got = lambda name, dtype, shape: inner(bufs[name], dtype, shape).cpu().numpy() if name in bufs else None
    return {"rgb": got("rgb", torch.float32, (H, W, 3)), "rgba": got("rgba", torch.uint8, (H, W, 4)),
            "variance": got("variance", torch.float32, (H, W)), "feedback": got("feedback", torch.float32, (H, W, 4))}


def same_outputs(a, b):
    return all((a[k] is None and b[k] is None) or
               (np.array_equal(a[k], b[k]) if k == "rgba" else same_bits(a[k], b[k])) for k in ("rgb", "rgba", "variance"))


def check_feedback(name, fb, one_pass_rgb, history, r1):
    """The feedback against rt_denoise_guided with one iteration, the history's lengths and the float64 reference."""
    assert same_bits(fb[..., :3], one_pass_rgb), name
    assert same_bits(fb[..., 3], history[..., 3]), name
    err = float(np.abs(fb[..., :3].astype(np.float64) - r1["out64"]).max())
    print(f"{name}: feedback max|gpu-ref64|={err:.3g} F={r1['F']:.3g} bar={r1['bar']:.3g}")
    assert np.isfinite(fb).all()
    assert err <= r1["bar"], (name, err, r1["bar"])


@pytest.mark.parametrize("with_albedo", (True, False), ids=("albedo", "plain"))
@pytest.mark.parametrize("case", G.CASES, ids=lambda c: "%dx%d_it%d" % c)
def test_feedback_matches_the_plain_call_and_the_first_pass(gpu_lib, case, with_albedo):
    w, h, it = case
    r = G.reference(w, h, it, with_albedo=with_albedo)
    r1 = G.reference(w, h, 1, with_albedo=with_albedo)
    t = upload(r)
    plain = call(gpu_lib, t, it, feedback=None)
    one = call(gpu_lib, t, 1, feedback=None)
    fed = call(gpu_lib, t, it)
    assert same_outputs(fed, plain), case
    check_feedback("%dx%d it=%d albedo=%s" % (*case, with_albedo), fed["feedback"], one["rgb"], r["g"]["history"], r1)


@pytest.mark.parametrize("size", ((17, 17), (37, 23)), ids=lambda s: "%dx%d" % s)
def test_one_pass_writes_outputs_and_feedback_from_the_same_products(gpu_lib, size):
    for with_albedo in (True, False):
        r1 = G.reference(*size, 1, with_albedo=with_albedo)
        t = upload(r1)
        plain = call(gpu_lib, t, 1, feedback=None)
        fed = call(gpu_lib, t, 1)
        assert same_outputs(fed, plain)
        assert same_bits(fed["feedback"][..., :3], fed["rgb"])
        assert np.array_equal(fed["rgba"], D.quantise(fed["feedback"][..., :3]))
        check_feedback("%dx%d it=1 albedo=%s" % (*size, with_albedo), fed["feedback"], plain["rgb"], r1["g"]["history"], r1)
        err = float(np.abs(fed["rgb"].astype(np.float64) - r1["out64"]).max())
        assert err <= r1["bar"], (size, err, r1["bar"])


@pytest.mark.parametrize("case", ((17, 17, 2), (96, 64, 5)), ids=lambda c: "%dx%d_it%d" % c)
def test_feedback_may_be_the_history_itself(gpu_lib, case):
    w, h, it = case
    r = G.reference(w, h, it)
    t = upload(r)
    kept = t["history"].clone()
    apart = call(gpu_lib, t, it)
    aliased = call(gpu_lib, t, it, feedback="alias")           # its history_device is the returned feedback buffer
    assert same_outputs(aliased, apart), case
    assert same_bits(aliased["feedback"], apart["feedback"]), case   # afterwards the history buffer holds the feedback
    assert same_bits(t["history"].cpu().numpy(), kept.cpu().numpy())
    assert not same_bits(aliased["feedback"][..., :3], kept.cpu().numpy()[..., :3])


def test_each_output_alone_with_the_feedback(gpu_lib):
    r = G.reference(37, 23, 5)
    t = upload(r)
    full = call(gpu_lib, t, 5)
    only_rgb = call(gpu_lib, t, 5, rgba=False, variance=False)
    only_rgba = call(gpu_lib, t, 5, rgb=False, variance=False)
    assert same_bits(only_rgb["rgb"], full["rgb"]) and only_rgb["rgba"] is None
    assert np.array_equal(only_rgba["rgba"], full["rgba"]) and only_rgba["rgb"] is None
    assert same_bits(only_rgb["feedback"], full["feedback"]) and same_bits(only_rgba["feedback"], full["feedback"])
    full1 = call(gpu_lib, t, 1)                                # ... and where the first pass is the last
    a, b = call(gpu_lib, t, 1, rgba=False, variance=False), call(gpu_lib, t, 1, rgb=False, variance=False)
    assert same_bits(a["rgb"], full1["rgb"]) and np.array_equal(b["rgba"], full1["rgba"])
    assert same_bits(a["feedback"], full1["feedback"]) and same_bits(b["feedback"], full1["feedback"])


def test_no_sync_on_a_side_stream(gpu_lib):
    import torch
    r = G.reference(96, 64, 5)
    t = upload(r)
    a = call(gpu_lib, t, 5)
    s = torch.cuda.Stream()
    for how in (dict(stream=s, flags=abi.RT_DENOISE_NO_SYNC), dict(stream=s), dict(flags=abi.RT_DENOISE_NO_SYNC)):
        b = call(gpu_lib, t, 5, **how)
        assert same_outputs(a, b) and same_bits(a["feedback"], b["feedback"]), how


@pytest.mark.parametrize("form", ("t", "d"))
def test_both_forms_of_the_variance_kernel_give_the_same_feedback(gpu_lib, monkeypatch, form):
    cases = [G.reference(*c) for c in ((1, 1, 1), (7, 1, 3), (17, 17, 2), (257, 5, 4), (96, 64, 5))]
    cases.append(G.reference(37, 23, 5, lengths="first"))      # every pixel takes the spatial estimate
    for r in cases:
        t = upload(r)
        monkeypatch.delenv("RTAMD_GUIDED_PREP", raising=False)
        a = call(gpu_lib, t, r["kw"]["iterations"])
        monkeypatch.setenv("RTAMD_GUIDED_PREP", form)
        b = call(gpu_lib, t, r["kw"]["iterations"])
        assert same_outputs(a, b) and same_bits(a["feedback"], b["feedback"]), (form, r["g"]["miss"].shape)


def test_inaccessible_feedback_buffer_is_rejected(gpu_lib):
    import torch
    r = G.reference(16, 16, 2)
    t = upload(r)
    n = 256
    host = np.zeros(16 * n + 64, np.uint8)
    d = abi.DenoiseGuidedDesc()
    d.width, d.height, d.iterations = 16, 16, 2
    d.sigma_luminance, d.sigma_normal, d.sigma_plane = G.SIGMAS
    out = {k: torch.zeros(size * n, dtype=torch.uint8, device="cuda") for k, size in (("rgb32_device", 12), ("scratch_device", 64))}
    d.rgb32_device, d.scratch_device, d.scratch_bytes = out["rgb32_device"].data_ptr(), out["scratch_device"].data_ptr(), 64 * n
    d.history_device, d.moments_device, d.hits_device = t["history"].data_ptr(), t["moments"].data_ptr(), t["hits"].data_ptr()
    f = abi.FeedbackDesc()
    f.feedback_device = host.ctypes.data // 16 * 16 + 16        # pageable host memory
    assert gpu_lib.rt_denoise_guided_feedback(0, C.byref(d), C.byref(f)) == 1
    assert b"accessible" in gpu_lib.rt_last_error()
    fb = torch.zeros((16, 16, 4), device="cuda")
    f.feedback_device = fb.data_ptr()
    current = torch.cuda.current_device()
    assert gpu_lib.rt_denoise_guided_feedback(0, C.byref(d), C.byref(f)) == abi.RT_OK
    assert torch.cuda.current_device() == current
    assert gpu_lib.rt_denoise_guided_feedback(gpu_lib.rt_device_count(), C.byref(d), C.byref(f)) == 1


# ---- the chain ---------------------------------------------------------------------------------------------------------

def gpu_chain(lib, s, feedback_on):
    """feedback_ref.chain on the GPU: rt_accumulate_moments, then rt_denoise_guided_feedback (or rt_denoise_guided), per
    frame; with feedback_on the feedback is the next frame's prev_history."""
    import torch
    H, W = s["g"]["miss"].shape
    hits = torch.from_numpy(np.ascontiguousarray(s["hits"]).view(np.uint8).reshape(H, W, 48).copy()).cuda()
    albedo = torch.from_numpy(np.array(s["albedo"])).cuda()
    colors = torch.from_numpy(np.array(s["colors"])).cuda()
    scratch = torch.empty(int(lib.rt_denoise_guided_scratch_bytes(W, H)), dtype=torch.uint8, device="cuda")
    prev_h, prev_m, outs = None, None, []
    for k in range(colors.shape[0]):
        hist, mom = torch.empty((H, W, 4), device="cuda"), torch.empty((H, W, 2), device="cuda")
        a = abi.AccumulateDesc()
        a.width, a.height = W, H
        a.max_history, a.normal_cos, a.plane_tolerance = G.KW["max_history"], G.KW["normal_cos"], G.KW["plane_tolerance"]
        a.color_device, a.hits_device, a.history_device = colors[k].data_ptr(), hits.data_ptr(), hist.data_ptr()
        m = abi.MomentsDesc()
        m.albedo_device, m.moments_device = albedo.data_ptr(), mom.data_ptr()
        if prev_h is not None:
            a.prev_hits_device, a.prev_history_device, m.prev_moments_device = hits.data_ptr(), prev_h.data_ptr(), prev_m.data_ptr()
        assert lib.rt_accumulate_moments(0, C.byref(a), C.byref(m)) == abi.RT_OK, lib.rt_last_error()
        d = abi.DenoiseGuidedDesc()
        d.width, d.height, d.iterations = W, H, FB.PASSES
        d.sigma_luminance, d.sigma_normal, d.sigma_plane = GUIDED_SIGMAS
        d.history_device, d.moments_device, d.hits_device, d.albedo_device = hist.data_ptr(), mom.data_ptr(), hits.data_ptr(), albedo.data_ptr()
        out = torch.empty((H, W, 3), device="cuda")
        d.rgb32_device, d.scratch_device, d.scratch_bytes = out.data_ptr(), scratch.data_ptr(), scratch.numel()
        prev_h, prev_m = hist, mom
        if feedback_on:
            f = abi.FeedbackDesc()
            prev_h = torch.empty((H, W, 4), device="cuda")
            f.feedback_device = prev_h.data_ptr()
            assert lib.rt_denoise_guided_feedback(0, C.byref(d), C.byref(f)) == abi.RT_OK, lib.rt_last_error()
        else:
            assert lib.rt_denoise_guided(0, C.byref(d)) == abi.RT_OK, lib.rt_last_error()
        outs.append(out)
    return torch.stack(outs).cpu().numpy()


def test_the_chain_on_the_gpu(gpu_lib):
    """tests/test_feedback_ref.py's two inequalities on the GPU's own outputs (64 x 48, 24 frames, seed 0).  The largest
    deviation of the GPU chain's frames from the float32 reference chain is printed and not asserted: a chained bar
    cannot be derived from the reference alone (profiles/feedback/README.md records the figure)."""
    W, H, FRAMES = 64, 48, 24
    s = FB.inputs(W, H, FRAMES, 0)
    miss = s["g"]["miss"]
    plain, fed = gpu_chain(gpu_lib, s, False), gpu_chain(gpu_lib, s, True)
    for name, got, on in (("plain", plain, False), ("feedback", fed, True)):
        ref = FB.chain(W, H, FRAMES, on, 0)
        print(f"{name} chain: max |gpu - ref32| over {FRAMES} frames = {float(np.abs(got - ref).max()):.3g}")
    f_plain, f_fb = FB.flicker(plain, miss), FB.flicker(fed, miss)
    e_plain, e_fb = FB.rmse(plain, s["albedo"], s["truth"], miss), FB.rmse(fed, s["albedo"], s["truth"], miss)
    print(f"gpu: flicker {f_fb:.6f} / {f_plain:.6f} = {f_fb / f_plain:.3f}, RMSE {e_fb:.6f} / {e_plain:.6f} = {e_fb / e_plain:.3f}")
    assert np.isfinite(fed).all() and np.isfinite(plain).all()
    assert f_fb <= 0.92 * f_plain
    assert e_fb <= e_plain


def test_renderer_feedback_loop(gpu_lib):
    """The demo scene at 160 x 96 (tests/test_gpu_guided.py's end-to-end scene), 4 one-sample frames through render ->
    query_camera -> accumulate(prev) -> denoise_guided(feedback=True) with prev = res["prev"]."""
    import torch
    W, H, SEED = 160, 96, 0xACC0
    scene = scenes.demo_with_particles(6)
    r = Renderer(scene).build_acceleration_structure(7)
    r.configure_camera(W, H, ray_trace_depth=2, sample_count=1)
    prev = None
    for k in range(4):
        noisy = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        r.render(0, frame_seed=SEED + k, want_rgba=False, rgb32_device=noisy.data_ptr())
        q = r.query_camera(first_sample=True, frame_seed=SEED + k, want_t=False, want_hits=True, want_albedo=True)
        acc = r.accumulate(noisy, q["hits"], prev, albedo=q["albedo"], moments=True)     # res["prev"] is accepted
        before = {key: v.clone() for key, v in acc.items()}
        plain = r.denoise_guided(acc, q["albedo"], want_rgba=True, want_variance=True)
        res = r.denoise_guided(acc, q["albedo"], want_rgba=True, want_variance=True, feedback=True)
        assert set(acc) == set(before) and all(torch.equal(acc[key], before[key]) for key in acc)
        assert "history" not in plain and "prev" not in plain
        for key in ("rgb", "rgba", "variance"):
            assert torch.equal(res[key].view(torch.uint8), plain[key].view(torch.uint8)), (k, key)
        assert res["history"].shape == (H, W, 4) and res["history"].data_ptr() != acc["history"].data_ptr()
        assert res["prev"]["history"] is res["history"]
        assert all(res["prev"][key] is acc[key] for key in acc if key != "history")
        assert torch.equal(res["history"][..., 3], acc["history"][..., 3])
        one = r.denoise_guided(acc, q["albedo"], iterations=1)
        assert torch.equal(res["history"][..., :3].contiguous().view(torch.uint8), one["rgb"].view(torch.uint8)), k
        if k:
            assert float(acc["history"][..., 3].max()) == k + 1    # the fed-back lengths carried the history on
        prev = res["prev"]
    r.cleanup()
