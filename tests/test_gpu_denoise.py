"""rt_denoise on the GPU against tests/denoise_ref.py.

Synthetic guides (denoise_ref.synth) are uploaded as tensors, the rt_hit records built in numpy with hits_to_numpy's
layout.  The sizes (denoise_ref.GPU_CASES) sit where the kernels can go wrong: 1 x 1 (only the centre tap), 7 x 1 and
1 x 7 (a whole tap axis outside), 16 x 16 and 17 x 17 (one LDS tile exactly, and one pixel more), 64 x 9 and 65 x 9 (a
wave's row of the direct form exactly, and one more), 37 x 23 (steps 8 and 16 leave the image from most pixels),
96 x 64 (halos span several tiles on every path) and 65 x 33.

The bar, per case: max |gpu - ref64| <= 4 F + 4 eps32 max |color| with F = max |ref32 - ref64|, computed from the
reference alone.  The kernels differ from the float32 restatement only in their expf, a rounding-sized effect that is
amplified exactly as float32's own rounding is; tests/test_denoise_ref.py shows that a single missing tap moves the
result by at least 10 bars.  Each test prints its measured ratio max |gpu - ref64| / F (profiles/denoise/README.md).

Every call here goes through buffers with guard bands around the outputs and the scratch."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as R
from rtamd import Renderer, abi, scenes
from rtamd.renderer import DENOISE_SIGMAS, HIT_DTYPE, hits_to_numpy

pytestmark = pytest.mark.gpu

INVALID = 1
GUARD = 256                                    # bytes kept around every buffer the call writes (a multiple of 16)
FILL = 0xA5
INF = float("inf")
CASE_IDS = ["%dx%d_it%d" % c for c in R.GPU_CASES]


def upload(g, with_albedo=True):
    import torch
    H, W = g["miss"].shape
    t = {"color": torch.from_numpy(np.array(g["color"])).cuda(),
         "hits": torch.from_numpy(R.hit_records(g, HIT_DTYPE).view(np.uint8).reshape(H, W, 48).copy()).cuda(),
         "albedo": torch.from_numpy(np.array(g["albedo"])).cuda() if with_albedo else None}
    return t


def guarded(nbytes):
    import torch
    return torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")


def inner(buf, dtype, shape):
    return buf[GUARD:buf.numel() - GUARD].view(dtype).reshape(shape)


def denoise(lib, t, iterations, sigmas=R.SIGMAS, *, rgb=True, rgba=True, in_place=False, stream=None, flags=0, device=0):
    """One rt_denoise call.  Returns (rgb float32 [H, W, 3] | None, rgba uint8 [H, W, 4] | None) as numpy arrays after
    checking that every guard band kept its fill.  in_place: the colour is copied into the guarded output buffer and
    that buffer is both color_device and rgb32_device."""
    import torch
    H, W = t["color"].shape[:2]
    n = W * H
    d = abi.DenoiseDesc()
    d.width, d.height, d.iterations, d.flags = W, H, iterations, flags
    d.sigma_color, d.sigma_normal, d.sigma_plane = sigmas
    bufs = {}
    if rgb:
        bufs["rgb"] = guarded(12 * n)
        d.rgb32_device = bufs["rgb"].data_ptr() + GUARD
    if rgba:
        bufs["rgba"] = guarded(4 * n)
        d.rgba8_device = bufs["rgba"].data_ptr() + GUARD
    d.scratch_bytes = lib.rt_denoise_scratch_bytes(W, H)
    assert d.scratch_bytes == 64 * n
    bufs["scratch"] = guarded(int(d.scratch_bytes))
    d.scratch_device = bufs["scratch"].data_ptr() + GUARD
    assert d.scratch_device % 16 == 0
    d.color_device = t["color"].data_ptr()
    if in_place:
        inner(bufs["rgb"], torch.float32, (H, W, 3)).copy_(t["color"])
        d.color_device = d.rgb32_device
    d.hits_device = t["hits"].data_ptr()
    d.albedo_device = t["albedo"].data_ptr() if t["albedo"] is not None else None
    d.stream = stream.cuda_stream if stream is not None else None
    torch.cuda.synchronize()
    rc = lib.rt_denoise(device, C.byref(d))
    assert rc == abi.RT_OK, lib.rt_last_error()
    if stream is not None:
        stream.synchronize()
    elif flags & abi.RT_DENOISE_NO_SYNC:
        torch.cuda.synchronize()
    for k, b in bufs.items():
        raw = b.cpu().numpy()
        assert (raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all(), f"{k}: bytes beyond the buffer were written"
    out_rgb = inner(bufs["rgb"], torch.float32, (H, W, 3)).cpu().numpy() if rgb else None
    out_rgba = inner(bufs["rgba"], torch.uint8, (H, W, 4)).cpu().numpy() if rgba else None
    return out_rgb, out_rgba


def check_against_reference(name, out, r64, F, bar):
    err = float(np.abs(out.astype(np.float64) - r64).max())
    print(f"{name}: max|gpu-ref64|={err:.3g} F={F:.3g} ratio={err / F if F else 0.0:.2f} bar={bar:.3g}")
    assert np.isfinite(out).all()
    assert err <= bar, (name, err, F, bar)


@pytest.mark.parametrize("with_albedo", (True, False), ids=("albedo", "plain"))
@pytest.mark.parametrize("case", R.GPU_CASES, ids=CASE_IDS)
def test_matches_reference(gpu_lib, case, with_albedo):
    W, H, it = case
    g, r64, _, F, bar = R.reference(W, H, it, with_albedo)
    rgb, rgba = denoise(gpu_lib, upload(g, with_albedo), it)
    check_against_reference("%dx%d it=%d albedo=%s" % (W, H, it, with_albedo), rgb, r64, F, bar)
    assert np.array_equal(rgba, R.quantise(rgb))           # bit for bit, of the same call's rgb32


@pytest.mark.parametrize("off", (0, 1, 2), ids=("color_off", "normal_off", "plane_off"))
def test_each_sigma_switched_off(gpu_lib, off):
    W, H, it = 65, 33, 4
    sigmas = tuple(INF if k == off else s for k, s in enumerate(R.SIGMAS))
    g, r64, _, F, bar = R.reference(W, H, it, True, sigmas)
    rgb, rgba = denoise(gpu_lib, upload(g), it, sigmas)
    check_against_reference("65x33 it=4 sigmas=%s" % (sigmas,), rgb, r64, F, bar)
    assert np.array_equal(rgba, R.quantise(rgb))
    # the term is off, not merely weak: the result differs from the one with every term on
    assert np.abs(rgb - R.reference(W, H, it, True)[2]).max() > 10 * bar


# 256 x 3 and 257 x 5: one workgroup of the row form exactly, and one pixel more; 530 x 4: three of them per row
FORM_CASES = ((96, 64, 5), (37, 23, 5), (65, 33, 4), (256, 3, 5), (257, 5, 5), (530, 4, 4))


@pytest.mark.parametrize("forms", ("ddd", "rrr", "tdr", "trd"))
def test_every_form_of_the_wide_passes(gpu_lib, monkeypatch, forms):
    """The passes of step 4, 8 and 16 have up to three forms each (csrc/denoise.hip, DN_FORMS: LDS tile, direct, rows);
    scripts/denoise_bench.py switches between them through RTAMD_DENOISE_FORMS, read per call.  Every combination
    meets the bar and gives the bits of the default (same taps, same order)."""
    for W, H, it in FORM_CASES:
        g, r64, _, F, bar = R.reference(W, H, it, True)
        t = upload(g)
        monkeypatch.delenv("RTAMD_DENOISE_FORMS", raising=False)
        default, _ = denoise(gpu_lib, t, it)
        monkeypatch.setenv("RTAMD_DENOISE_FORMS", forms)
        rgb, _ = denoise(gpu_lib, t, it)
        check_against_reference("%dx%d it=%d forms=%s" % (W, H, it, forms), rgb, r64, F, bar)
        assert np.array_equal(rgb, default)
    monkeypatch.setenv("RTAMD_DENOISE_FORMS", "xyz")          # not three valid letters: ignored
    assert np.array_equal(denoise(gpu_lib, t, it)[0], default)


@pytest.mark.parametrize("case", ((1, 1, 1), (17, 17, 1), (17, 17, 2), (96, 64, 5)), ids=lambda c: "%dx%d_it%d" % c)
def test_in_place_equals_out_of_place(gpu_lib, case):
    W, H, it = case
    t = upload(R.synth(W, H, seed=4))
    a, a8 = denoise(gpu_lib, t, it)
    b, b8 = denoise(gpu_lib, t, it, in_place=True)
    assert np.array_equal(a, b) and np.array_equal(a8, b8)


def test_no_sync_on_a_side_stream_equals_the_synchronous_call(gpu_lib):
    import torch
    t = upload(R.synth(96, 64, seed=5))
    a, a8 = denoise(gpu_lib, t, 5)
    s = torch.cuda.Stream()
    b, b8 = denoise(gpu_lib, t, 5, stream=s, flags=abi.RT_DENOISE_NO_SYNC)
    assert np.array_equal(a, b) and np.array_equal(a8, b8)
    c, c8 = denoise(gpu_lib, t, 5, stream=s)                 # synchronous on the side stream
    assert np.array_equal(a, c) and np.array_equal(a8, c8)


def test_two_runs_are_identical_and_outputs_are_optional(gpu_lib):
    t = upload(R.synth(65, 33, seed=6))
    a, a8 = denoise(gpu_lib, t, 4)
    b, b8 = denoise(gpu_lib, t, 4)
    assert np.array_equal(a, b) and np.array_equal(a8, b8)
    only_rgb, none = denoise(gpu_lib, t, 4, rgba=False)
    assert none is None and np.array_equal(only_rgb, a)
    none, only_rgba = denoise(gpu_lib, t, 4, rgb=False)
    assert none is None and np.array_equal(only_rgba, a8)


def test_inaccessible_buffer_and_device_are_rejected(gpu_lib):
    import torch
    W, H = 8, 4
    t = upload(R.synth(W, H))
    host = np.zeros(W * H * 3, np.float32)
    d = abi.DenoiseDesc()
    d.width, d.height, d.iterations = W, H, 2
    d.sigma_color, d.sigma_normal, d.sigma_plane = R.SIGMAS
    out = torch.zeros((H, W, 3), device="cuda")
    scratch = torch.zeros(64 * W * H, dtype=torch.uint8, device="cuda")
    d.color_device, d.hits_device = t["color"].data_ptr(), t["hits"].data_ptr()
    d.rgb32_device, d.scratch_device, d.scratch_bytes = out.data_ptr(), scratch.data_ptr(), scratch.numel()
    assert gpu_lib.rt_denoise(0, C.byref(d)) == abi.RT_OK
    for field in ("color_device", "albedo_device", "rgb32_device"):
        keep = getattr(d, field)
        setattr(d, field, host.ctypes.data)                   # pageable host memory
        assert gpu_lib.rt_denoise(0, C.byref(d)) == INVALID, field
        assert b"accessible" in gpu_lib.rt_last_error()
        setattr(d, field, keep)
    assert gpu_lib.rt_denoise(gpu_lib.rt_device_count(), C.byref(d)) == INVALID
    assert gpu_lib.rt_denoise(-1, C.byref(d)) == INVALID
    current = torch.cuda.current_device()
    assert gpu_lib.rt_denoise(0, C.byref(d)) == abi.RT_OK
    assert torch.cuda.current_device() == current


def gamma_rmse(a, b):
    ga, gb = np.sqrt(np.clip(a, 0.0, 1.0)), np.sqrt(np.clip(b, 0.0, 1.0))
    return float(np.sqrt(np.mean((ga.astype(np.float64) - gb) ** 2)))


def test_render_query_denoise_on_one_stream(gpu_lib):
    """The demo scene at 160 x 96, depth 2: render(sample_count=1) -> query_camera(hits, albedo) -> denoise, all
    sync=False on one torch stream.  The result is within the bar of the reference on the downloaded inputs, and nearer
    to the converged frame (256 samples) than the noisy one in gamma space."""
    import torch
    W, H, SEED = 160, 96, 0xD15EA5E
    scene = scenes.demo_with_particles(6)
    r = Renderer(scene).build_acceleration_structure(7).configure_camera(W, H, ray_trace_depth=2, sample_count=1)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        noisy = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    r.render(0, frame_seed=SEED, want_rgba=False, rgb32_device=noisy.data_ptr(), stream=s.cuda_stream, sync=False)
    q = r.query_camera(first_sample=True, frame_seed=SEED, want_t=False, want_hits=True, want_albedo=True, stream=s,
                       sync=False)
    out = r.denoise(noisy, q["hits"], q["albedo"], want_rgba=True, stream=s, sync=False)
    s.synchronize()
    r.synchronize()
    rgb, rgba = out["rgb"].cpu().numpy(), out["rgba"].cpu().numpy()
    color, albedo = noisy.cpu().numpy(), q["albedo"].cpu().numpy()
    hits = hits_to_numpy(q["hits"]).reshape(H, W)
    miss = hits["instance"] == abi.MISS
    assert miss.any() and not miss.all()
    kw = dict(iterations=5, sigma_color=DENOISE_SIGMAS[0], sigma_normal=DENOISE_SIGMAS[1], sigma_plane=DENOISE_SIGMAS[2])
    r64 = R.denoise(color, hits["normal"], hits["point"], miss, albedo, dtype=np.float64, **kw)
    r32 = R.denoise(color, hits["normal"], hits["point"], miss, albedo, dtype=np.float32, **kw)
    F = float(np.abs(r32 - r64).max())
    bar = 4.0 * F + 4.0 * float(np.finfo(np.float32).eps) * float(np.abs(color).max())
    check_against_reference("demo 160x96 end to end", rgb, r64, F, bar)
    assert np.array_equal(rgba, R.quantise(rgb))
    # the converged frame: the same camera with 256 samples per pixel
    r.configure_camera(W, H, ray_trace_depth=2, sample_count=256)
    _, converged, _ = r.render(0, frame_seed=SEED, want_rgba=False, want_rgb=True)
    r.cleanup()
    e_noisy, e_denoised = gamma_rmse(color, converged), gamma_rmse(rgb, converged)
    print(f"gamma-space RMSE against 256 spp: noisy {e_noisy:.4f}, denoised {e_denoised:.4f}, "
          f"ratio {e_denoised / e_noisy:.3f}")
    assert e_denoised < e_noisy
