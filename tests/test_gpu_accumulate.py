"""rt_accumulate on the GPU against tests/accumulate_ref.py, bit for bit.

Synthetic guides (accumulate_ref.case) are uploaded as tensors.  The sizes sit where the kernels can go wrong: 1 x 1
(every tap but one lies outside), 7 x 1 and 1 x 7 (a whole tap axis outside), 8 x 8 and 9 x 9 (one block of the blocks
mapping exactly, and one pixel more), 64 x 2 and 65 x 2 (a wave's row of the rows mapping exactly, and one more),
37 x 23 (partial edges on every side) and 96 x 64 (several tiles on every path); each with the five views of
accumulate_ref.VIEWS.  The kernel uses no operation that numpy's float32 rounds differently, so history and rgb32 must
equal the float32 restatement exactly; tests/test_accumulate_ref.py pins that restatement against float64 and shows
that a missing tap or validity test could not hide.

Every call here goes through buffers with guard bands around the outputs."""
import ctypes as C

import numpy as np
import pytest

import accumulate_ref as R
from rtamd import Renderer, abi, scenes
from rtamd.renderer import DENOISE_SIGMAS, hits_to_numpy

pytestmark = pytest.mark.gpu

INVALID = 1
GUARD = 256                                    # bytes kept around every buffer the call writes (a multiple of 16)
FILL = 0xA5
INF = float("inf")
KW = dict(max_history=R.MAX_HISTORY, normal_cos=R.NORMAL_COS, plane_tolerance=R.PLANE_TOLERANCE)
CASES = [(w, h, v) for (w, h) in R.SIZES for v in R.VIEWS]


def upload(g):
    import torch
    H, W = g["color"].shape[:2]
    rec = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(H, W, 48).copy()).cuda()
    return {"color": torch.from_numpy(np.array(g["color"])).cuda(), "hits": rec(g["hits"]),
            "prev_hits": rec(g["prev_hits"]), "prev_history": torch.from_numpy(np.array(g["prev_history"])).cuda()}


def rows_struct(view):
    if view is None:
        return None
    r = abi.Reprojection()
    for k in ("centre", "rx", "ry", "rw"):
        for a in range(3):
            getattr(r, k)[a] = float(view[k][a])
    return r


def guarded(nbytes):
    import torch
    return torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")


def inner(buf, dtype, shape):
    return buf[GUARD:buf.numel() - GUARD].view(dtype).reshape(shape)


def accumulate(lib, t, view, *, first=False, rgb=True, in_place=False, stream=None, flags=0, device=0, **over):
    """One rt_accumulate call.  Returns (history float32 [H, W, 4], rgb float32 [H, W, 3] | None) as numpy arrays after
    checking that every guard band kept its fill.  in_place: the colour is copied into the guarded output buffer and
    that buffer is both color_device and rgb32_device.  first: no previous frame."""
    import torch
    H, W = t["color"].shape[:2]
    n = W * H
    kw = dict(KW)
    kw.update(over)
    d = abi.AccumulateDesc()
    d.width, d.height, d.flags = W, H, flags
    d.max_history, d.normal_cos, d.plane_tolerance = kw["max_history"], kw["normal_cos"], kw["plane_tolerance"]
    rows = rows_struct(view)
    if rows is not None:
        d.prev_view = C.pointer(rows)
    bufs = {"history": guarded(16 * n)}
    d.history_device = bufs["history"].data_ptr() + GUARD
    assert d.history_device % 16 == 0
    if rgb or in_place:
        bufs["rgb"] = guarded(12 * n)
        d.rgb32_device = bufs["rgb"].data_ptr() + GUARD
    d.color_device = t["color"].data_ptr()
    if in_place:
        inner(bufs["rgb"], torch.float32, (H, W, 3)).copy_(t["color"])
        d.color_device = d.rgb32_device
    d.hits_device = t["hits"].data_ptr()
    if not first:
        d.prev_hits_device, d.prev_history_device = t["prev_hits"].data_ptr(), t["prev_history"].data_ptr()
    d.stream = stream.cuda_stream if stream is not None else None
    torch.cuda.synchronize()
    rc = lib.rt_accumulate(device, C.byref(d))
    assert rc == abi.RT_OK, lib.rt_last_error()
    if stream is not None:
        stream.synchronize()
    elif flags & abi.RT_ACCUMULATE_NO_SYNC:
        torch.cuda.synchronize()
    for k, b in bufs.items():
        raw = b.cpu().numpy()
        assert (raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all(), f"{k}: bytes beyond the buffer were written"
    history = inner(bufs["history"], torch.float32, (H, W, 4)).cpu().numpy()
    out_rgb = inner(bufs["rgb"], torch.float32, (H, W, 3)).cpu().numpy() if "rgb" in bufs else None
    return history, out_rgb


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_is_reference(name, history, rgb, ref32):
    wrong = (history.view(np.uint32) != np.ascontiguousarray(ref32).view(np.uint32)).any(axis=-1)
    err = float(np.abs(history.astype(np.float64) - ref32).max())
    print(f"{name}: {int(wrong.sum())} of {wrong.size} pixels differ from ref32, max |gpu - ref32| = {err:.3g}")
    assert not wrong.any(), (name, int(wrong.sum()), err)
    if rgb is not None:
        assert same_bits(rgb, history[..., :3])


def ref32(g, view="case", **over):
    kw = dict(KW)
    kw.update(over)
    return R.accumulate(g["color"], g["hits"], g["prev_hits"], g["prev_history"], g["view"] if view == "case" else view,
                        dtype=np.float32, **kw)[0]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_%s" % c)
def test_matches_reference_bit_for_bit(gpu_lib, case):
    W, H, view = case
    g = R.case(W, H, view)
    history, rgb = accumulate(gpu_lib, upload(g), g["view"])
    assert_is_reference("%dx%d %s" % case, history, rgb, g["ref32"])


@pytest.mark.parametrize("off", (dict(normal_cos=-INF), dict(plane_tolerance=INF), dict(max_history=INF)),
                         ids=("normal_off", "plane_off", "history_unbounded"))
def test_each_test_switched_off(gpu_lib, off):
    g = R.case(96, 64, "moved")
    history, rgb = accumulate(gpu_lib, upload(g), g["view"], **off)
    assert_is_reference("96x64 moved %s" % (off,), history, rgb, ref32(g, **off))
    # the test is off, not merely weak: the result differs from the one with every test on
    assert np.abs(history - g["ref32"]).max() > 100.0 * R.bound(96, 64)


def test_first_frame_resets_every_pixel(gpu_lib):
    g = R.case(37, 23, "moved")
    history, rgb = accumulate(gpu_lib, upload(g), g["view"], first=True)
    assert same_bits(rgb, g["color"]) and same_bits(history[..., :3], g["color"]) and (history[..., 3] == 1.0).all()
    history, rgb = accumulate(gpu_lib, upload(g), None, first=True)
    assert same_bits(rgb, g["color"]) and (history[..., 3] == 1.0).all()


def test_max_history_one_returns_the_colour(gpu_lib):
    """N = 1, a = 1: Hm + (c - Hm), the colour up to two roundings (tests/test_accumulate_ref.py has the bound)."""
    g = R.case(37, 23, "moved")
    history, rgb = accumulate(gpu_lib, upload(g), g["view"], max_history=1.0)
    assert_is_reference("37x23 moved max_history=1", history, rgb, ref32(g, max_history=1.0))
    assert (history[..., 3] == 1.0).all()
    assert np.abs(rgb - g["color"]).max() <= 2.0 * R.EPS32 * 1.5


def test_a_band_of_changed_instances_resets_exactly_those_pixels(gpu_lib):
    """Static camera, last frame's records equal to this frame's but for rows 5 .. 9, whose instance ids changed."""
    g = dict(R.case(37, 23, "null"))
    prev = np.array(g["hits"])
    band = np.zeros(prev.shape, bool)
    band[5:10] = True
    prev["instance"][band & (prev["instance"] != R.MISS)] += 5
    g["prev_hits"] = prev
    history, rgb = accumulate(gpu_lib, upload(g), None)
    assert_is_reference("37x23 band", history, rgb, ref32(g, view=None))
    hit = g["hits"]["instance"] != R.MISS
    assert (band & hit).any() and (~band & hit).any()
    reset = history[..., 3] == 1.0
    assert np.array_equal(reset, band | ~hit)
    assert same_bits(history[reset][:, :3], g["color"][reset])
    expect = np.minimum(g["prev_history"][..., 3] + 1.0, R.MAX_HISTORY)
    assert np.array_equal(history[~reset][:, 3], expect[~reset])


@pytest.mark.parametrize("case", ((1, 1, "same"), (9, 9, "moved"), (65, 2, "pan"), (96, 64, "moved")), ids=lambda c: "%dx%d_%s" % c)
def test_in_place_equals_out_of_place(gpu_lib, case):
    g = R.case(*case)
    t = upload(g)
    a, a_rgb = accumulate(gpu_lib, t, g["view"])
    b, b_rgb = accumulate(gpu_lib, t, g["view"], in_place=True)
    assert same_bits(a, b) and same_bits(a_rgb, b_rgb)
    c, none = accumulate(gpu_lib, t, g["view"], rgb=False)     # rgb32_device is optional
    assert none is None and same_bits(a, c)


def test_two_runs_are_identical(gpu_lib):
    g = R.case(96, 64, "moved")
    t = upload(g)
    a, a_rgb = accumulate(gpu_lib, t, g["view"])
    b, b_rgb = accumulate(gpu_lib, t, g["view"])
    assert same_bits(a, b) and same_bits(a_rgb, b_rgb)


@pytest.mark.parametrize("form", ("r", "b"))
def test_both_mappings_give_the_same_bits(gpu_lib, monkeypatch, form):
    """csrc/accumulate.hip maps pixels to lanes by rows or by 8 x 8 blocks; scripts/accumulate_bench.py switches
    between them through RTAMD_ACCUMULATE_FORM, read per call."""
    for W, H, view in ((1, 1, "same"), (7, 1, "moved"), (1, 7, "moved"), (8, 8, "same"), (9, 9, "pan"), (64, 2, "moved"),
                       (65, 2, "moved"), (37, 23, "null"), (37, 23, "pan"), (96, 64, "moved")):
        g = R.case(W, H, view)
        t = upload(g)
        monkeypatch.setenv("RTAMD_ACCUMULATE_FORM", form)
        history, rgb = accumulate(gpu_lib, t, g["view"])
        assert_is_reference("%dx%d %s form=%s" % (W, H, view, form), history, rgb, g["ref32"])
    monkeypatch.setenv("RTAMD_ACCUMULATE_FORM", "rows")       # not one valid letter: ignored
    assert same_bits(accumulate(gpu_lib, t, g["view"])[0], history)
    monkeypatch.delenv("RTAMD_ACCUMULATE_FORM")
    assert same_bits(accumulate(gpu_lib, t, g["view"])[0], history)


def test_no_sync_on_a_side_stream_equals_the_synchronous_call(gpu_lib):
    import torch
    g = R.case(96, 64, "moved")
    t = upload(g)
    a, a_rgb = accumulate(gpu_lib, t, g["view"])
    s = torch.cuda.Stream()
    b, b_rgb = accumulate(gpu_lib, t, g["view"], stream=s, flags=abi.RT_ACCUMULATE_NO_SYNC)
    assert same_bits(a, b) and same_bits(a_rgb, b_rgb)
    c, c_rgb = accumulate(gpu_lib, t, g["view"], stream=s)     # synchronous on the side stream
    assert same_bits(a, c) and same_bits(a_rgb, c_rgb)
    e, e_rgb = accumulate(gpu_lib, t, g["view"], flags=abi.RT_ACCUMULATE_NO_SYNC)      # the null stream
    assert same_bits(a, e) and same_bits(a_rgb, e_rgb)


def test_overlap_inaccessible_buffer_and_device_are_rejected(gpu_lib):
    import torch
    W, H = 8, 4
    g = R.case(8, 8, "same")
    t = {k: v[:H].contiguous() for k, v in upload(g).items()}
    host = np.zeros(W * H * 12, np.float32)
    d = abi.AccumulateDesc()
    d.width, d.height = W, H
    d.max_history, d.normal_cos, d.plane_tolerance = R.MAX_HISTORY, R.NORMAL_COS, R.PLANE_TOLERANCE
    history = torch.zeros((2 * H, W, 4), device="cuda")      # room for a shifted, overlapping pair
    rgb = torch.zeros((H, W, 3), device="cuda")
    d.color_device, d.hits_device = t["color"].data_ptr(), t["hits"].data_ptr()
    d.prev_hits_device, d.prev_history_device = t["prev_hits"].data_ptr(), t["prev_history"].data_ptr()
    d.history_device, d.rgb32_device = history.data_ptr(), rgb.data_ptr()
    assert gpu_lib.rt_accumulate(0, C.byref(d)) == abi.RT_OK
    before = history.cpu().numpy().copy()
    # an overlapping history pair: the same buffer, and one shifted by a row
    for prev in (history.data_ptr(), history.data_ptr() + 16 * W):
        d.prev_history_device = prev
        assert gpu_lib.rt_accumulate(0, C.byref(d)) == INVALID
        assert b"overlap" in gpu_lib.rt_last_error()
    d.prev_history_device = history.data_ptr() + 16 * W * H   # back to back is fine
    assert gpu_lib.rt_accumulate(0, C.byref(d)) == abi.RT_OK
    d.prev_history_device = t["prev_history"].data_ptr()
    for field in ("color_device", "hits_device", "prev_hits_device", "prev_history_device", "history_device", "rgb32_device"):
        keep = getattr(d, field)
        setattr(d, field, host.ctypes.data // 16 * 16 + 16)   # pageable host memory
        assert gpu_lib.rt_accumulate(0, C.byref(d)) == INVALID, field
        assert b"accessible" in gpu_lib.rt_last_error()
        setattr(d, field, keep)
    assert gpu_lib.rt_accumulate(gpu_lib.rt_device_count(), C.byref(d)) == INVALID
    assert gpu_lib.rt_accumulate(-1, C.byref(d)) == INVALID
    current = torch.cuda.current_device()
    assert gpu_lib.rt_accumulate(0, C.byref(d)) == abi.RT_OK
    assert torch.cuda.current_device() == current
    assert np.array_equal(history.cpu().numpy()[:H], before[:H])          # the same inputs, the same result


# ---- end to end ------------------------------------------------------------------------------------------------------

def gamma_rmse(a, b):
    ga, gb = np.sqrt(np.clip(a, 0.0, 1.0)), np.sqrt(np.clip(b, 0.0, 1.0))
    return float(np.sqrt(np.mean((ga.astype(np.float64) - gb) ** 2)))


def rows_dict(r):
    return None if r is None else {k: np.array(list(getattr(r, k)), np.float32) for k in ("centre", "rx", "ry", "rw")}


@pytest.mark.parametrize("dolly", (False, True), ids=("static", "dolly"))
def test_render_query_accumulate_on_one_stream(gpu_lib, dolly):
    """The demo scene at 160 x 96, depth 2, frame 0 every time so nothing moves: eight one-sample frames with
    different seeds through render -> query_camera -> accumulate, all sync=False on one torch stream, the camera
    still or dollying forward a little each frame (prev_view = rtamd.reprojection of the previous camera).  Every
    frame's history equals the float32 reference on the downloaded inputs bit for bit; the last accumulated frame is
    nearer to the converged one (256 samples at the last camera) than the last noisy frame in gamma space, and nearer
    still after rt_denoise."""
    import torch
    import rtamd
    W, H, FRAMES, SEED = 160, 96, 8, 0xACC0
    scene = scenes.demo_with_particles(6)
    r = Renderer(scene).build_acceleration_structure(7)
    base = np.array(scene.camera["center"], np.float64)
    toward = np.array(scene.camera["target"], np.float64) - base
    toward /= np.linalg.norm(toward)
    s = torch.cuda.Stream()
    frames, prev, prev_camera = [], None, None
    for k in range(FRAMES):
        center = tuple(float(v) for v in base + (0.03 * k if dolly else 0.0) * toward)
        r.configure_camera(W, H, ray_trace_depth=2, sample_count=1, center=center)
        with torch.cuda.stream(s):
            noisy = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        r.render(0, frame_seed=SEED + k, want_rgba=False, rgb32_device=noisy.data_ptr(), stream=s.cuda_stream, sync=False)
        q = r.query_camera(first_sample=True, frame_seed=SEED + k, want_t=False, want_hits=True, want_albedo=True,
                           stream=s, sync=False)
        view = rtamd.reprojection(prev_camera, W, H) if dolly and prev_camera is not None else None
        prev = r.accumulate(noisy, q["hits"], prev, prev_view=view, stream=s, sync=False)
        frames.append({"color": noisy, "hits": q["hits"], "albedo": q["albedo"], "view": view, "out": prev})
        prev_camera = r.camera
    last = frames[-1]
    # rt_denoise has no variance guidance: its colour sigma is the caller's statement of the noise level, and the
    # default is the one-sample frame's.  The mean of FRAMES samples has 1 / sqrt(FRAMES) of that noise.
    denoised_1spp_sigma = r.denoise(last["out"]["rgb"], last["hits"], last["albedo"], stream=s, sync=False)
    denoised = r.denoise(last["out"]["rgb"], last["hits"], last["albedo"], sigma_color=DENOISE_SIGMAS[0] / FRAMES ** 0.5,
                         stream=s, sync=False)
    s.synchronize()
    r.synchronize()
    # the float32 reference, frame by frame on the downloaded inputs with Renderer.accumulate's defaults
    from rtamd.renderer import ACCUMULATE_DEFAULTS
    kw = dict(max_history=ACCUMULATE_DEFAULTS[0], normal_cos=ACCUMULATE_DEFAULTS[1], plane_tolerance=ACCUMULATE_DEFAULTS[2])
    ref, prev_hits = None, None
    for k, f in enumerate(frames):
        hits = hits_to_numpy(f["hits"]).reshape(H, W)
        ref, _ = R.accumulate(f["color"].cpu().numpy(), hits, prev_hits, ref, rows_dict(f["view"]), dtype=np.float32, **kw)
        assert_is_reference("demo 160x96 %s frame %d" % ("dolly" if dolly else "static", k),
                            f["out"]["history"].cpu().numpy(), f["out"]["rgb"].cpu().numpy(), ref)
        prev_hits = hits
    miss = hits["instance"] == abi.MISS
    assert miss.any() and not miss.all()
    length = ref[..., 3]
    assert (length[miss] == 1.0).all() and length.max() >= FRAMES - 1e-3   # some pixel kept every frame
    print(f"history length after {FRAMES} frames: mean over hits {float(length[~miss].mean()):.2f}")
    # the converged frame: the last camera with 256 samples per pixel
    r.configure_camera(W, H, ray_trace_depth=2, sample_count=256, center=center)
    _, converged, _ = r.render(0, frame_seed=SEED, want_rgba=False, want_rgb=True)
    r.cleanup()
    e_noisy = gamma_rmse(last["color"].cpu().numpy(), converged)
    e_acc = gamma_rmse(last["out"]["rgb"].cpu().numpy(), converged)
    e_den = gamma_rmse(denoised["rgb"].cpu().numpy(), converged)
    e_den_1spp = gamma_rmse(denoised_1spp_sigma["rgb"].cpu().numpy(), converged)
    print(f"gamma-space RMSE against 256 spp: noisy {e_noisy:.4f}, accumulated {e_acc:.4f}, accumulated and denoised "
          f"{e_den:.4f} (with the one-sample frame's colour sigma: {e_den_1spp:.4f})")
    assert e_acc < e_noisy
    assert e_den < e_acc
