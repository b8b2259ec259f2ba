"""rt_accumulate_moments and rt_denoise_guided on the GPU against tests/guided_ref.py.

rt_accumulate_moments over accumulate_ref.SIZES x VIEWS: history and rgb32 bit-identical to rt_accumulate on the same
inputs, moments bit-identical to the float32 restatement (the kernel uses no operation numpy's float32 rounds
differently), with and without albedo, on a first frame and in both pixel mappings.

rt_denoise_guided over guided_ref.CASES — 1 x 1, 7 x 1 and 1 x 7 (the 7 x 7 window's radius and whole tap axes
outside), 4 x 4, 16 x 16 and 17 x 17 (the LDS tile's edge), 65 x 9 and 257 x 5 (the row form's 256-pixel chunk at steps
4 and 8, and one pixel more), 37 x 23 and 96 x 64 (all five steps) — within the bar 4 F + 4 eps32 max |colour| of the
float64 reference, F = max |ref32 - ref64| from the reference alone, and v_0 within the same form of bar;
tests/test_guided_ref.py shows what that bar would notice.

Every call here goes through buffers with guard bands around the outputs and the scratch."""
import ctypes as C

import numpy as np
import pytest

import accumulate_ref as A
import denoise_ref as D
import guided_ref as G
from rtamd import Renderer, abi, scenes
from rtamd.renderer import ACCUMULATE_DEFAULTS, DENOISE_SIGMAS, GUIDED_SIGMAS, HIT_DTYPE, hits_to_numpy

pytestmark = pytest.mark.gpu

INVALID = 1
GUARD = 256                                    # bytes kept around every buffer a call writes (a multiple of 16)
FILL = 0xA5
INF = float("inf")
ACC_CASES = [(w, h, v) for (w, h) in A.SIZES for v in A.VIEWS]


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


# ---- rt_accumulate_moments -------------------------------------------------------------------------------------------

def upload_acc(g):
    import torch
    H, W = g["color"].shape[:2]
    rec = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(H, W, 48).copy()).cuda()
    t = {k: torch.from_numpy(np.array(g[k])).cuda() for k in ("color", "prev_history", "prev_moments", "albedo")}
    t["hits"], t["prev_hits"] = rec(g["hits"]), rec(g["prev_hits"])
    return t


def rows_struct(view):
    if view is None:
        return None
    r = abi.Reprojection()
    for k in ("centre", "rx", "ry", "rw"):
        for a in range(3):
            getattr(r, k)[a] = float(view[k][a])
    return r


def accumulate(lib, t, view, *, moments=True, albedo=True, first=False, stream=None, flags=0):
    """One rt_accumulate_moments (or, moments=False, rt_accumulate) call on guarded outputs -> (history, rgb, moments |
    None) as numpy arrays."""
    import torch
    H, W = t["color"].shape[:2]
    n = W * H
    d = abi.AccumulateDesc()
    d.width, d.height, d.flags = W, H, flags
    d.max_history, d.normal_cos, d.plane_tolerance = A.MAX_HISTORY, A.NORMAL_COS, A.PLANE_TOLERANCE
    rows = rows_struct(view)
    if rows is not None:
        d.prev_view = C.pointer(rows)
    bufs = {"history": guarded(16 * n), "rgb": guarded(12 * n)}
    d.history_device = bufs["history"].data_ptr() + GUARD
    d.rgb32_device = bufs["rgb"].data_ptr() + GUARD
    d.color_device, d.hits_device = t["color"].data_ptr(), t["hits"].data_ptr()
    if not first:
        d.prev_hits_device, d.prev_history_device = t["prev_hits"].data_ptr(), t["prev_history"].data_ptr()
    d.stream = stream.cuda_stream if stream is not None else None
    torch.cuda.synchronize()
    if moments:
        m = abi.MomentsDesc()
        bufs["moments"] = guarded(8 * n)
        m.moments_device = bufs["moments"].data_ptr() + GUARD
        assert m.moments_device % 8 == 0
        m.albedo_device = t["albedo"].data_ptr() if albedo else None
        m.prev_moments_device = None if first else t["prev_moments"].data_ptr()
        rc = lib.rt_accumulate_moments(0, C.byref(d), C.byref(m))
    else:
        rc = lib.rt_accumulate(0, C.byref(d))
    assert rc == abi.RT_OK, lib.rt_last_error()
    if stream is not None:
        stream.synchronize()
    elif flags & abi.RT_ACCUMULATE_NO_SYNC:
        torch.cuda.synchronize()
    guards_intact(bufs)
    return (inner(bufs["history"], torch.float32, (H, W, 4)).cpu().numpy(),
            inner(bufs["rgb"], torch.float32, (H, W, 3)).cpu().numpy(),
            inner(bufs["moments"], torch.float32, (H, W, 2)).cpu().numpy() if moments else None)


def check_moments(name, lib, g, t, **how):
    plain_h, plain_rgb, _ = accumulate(lib, t, g["view"], moments=False, first=how.get("first", False))
    h, rgb, mom = accumulate(lib, t, g["view"], **how)
    key = "first32" if how.get("first") else ("with_albedo32" if how.get("albedo", True) else "without_albedo32")
    wrong = (mom.view(np.uint32) != np.ascontiguousarray(g[key][1]).view(np.uint32)).any(axis=-1)
    print(f"{name} {how}: {int(wrong.sum())} of {wrong.size} pixels' moments differ from ref32")
    assert same_bits(h, plain_h) and same_bits(rgb, plain_rgb), name
    assert same_bits(h, g[key][0])
    assert not wrong.any(), (name, int(wrong.sum()))


@pytest.mark.parametrize("case", ACC_CASES, ids=lambda c: "%dx%d_%s" % c)
def test_accumulate_moments_bit_for_bit(gpu_lib, case):
    g = G.moments_case(*case)
    t = upload_acc(g)
    name = "%dx%d %s" % case
    check_moments(name, gpu_lib, g, t)
    check_moments(name, gpu_lib, g, t, albedo=False)
    check_moments(name, gpu_lib, g, t, first=True)


@pytest.mark.parametrize("form", ("r", "b"))
def test_accumulate_moments_both_mappings(gpu_lib, monkeypatch, form):
    monkeypatch.setenv("RTAMD_ACCUMULATE_FORM", form)
    for case in ((1, 1, "same"), (7, 1, "moved"), (1, 7, "moved"), (8, 8, "same"), (9, 9, "pan"), (64, 2, "moved"),
                 (65, 2, "moved"), (37, 23, "null"), (37, 23, "pan"), (96, 64, "moved")):
        g = G.moments_case(*case)
        check_moments("%dx%d %s form=%s" % (*case, form), gpu_lib, g, upload_acc(g))


def test_accumulate_moments_no_sync_on_a_side_stream(gpu_lib):
    import torch
    g = G.moments_case(96, 64, "moved")
    t = upload_acc(g)
    a = accumulate(gpu_lib, t, g["view"])
    s = torch.cuda.Stream()
    b = accumulate(gpu_lib, t, g["view"], stream=s, flags=abi.RT_ACCUMULATE_NO_SYNC)
    c = accumulate(gpu_lib, t, g["view"], flags=abi.RT_ACCUMULATE_NO_SYNC)
    for x, y, z in zip(a, b, c):
        assert same_bits(x, y) and same_bits(x, z)


# ---- rt_denoise_guided -----------------------------------------------------------------------------------------------

def upload(r):
    import torch
    g = r["g"]
    H, W = g["miss"].shape
    return {"history": torch.from_numpy(np.array(g["history"])).cuda(), "moments": torch.from_numpy(np.array(r["moments"])).cuda(),
            "hits": torch.from_numpy(D.hit_records(g, HIT_DTYPE).view(np.uint8).reshape(H, W, 48).copy()).cuda(),
            "albedo": torch.from_numpy(np.array(r["albedo"])).cuda() if r["albedo"] is not None else None}


def denoise_guided(lib, t, iterations, sigmas=G.SIGMAS, *, rgb=True, rgba=True, variance=True, stream=None, flags=0):
    """One rt_denoise_guided call on guarded outputs and scratch -> (rgb | None, rgba | None, v_0 | None)."""
    import torch
    H, W = t["history"].shape[:2]
    n = W * H
    d = abi.DenoiseGuidedDesc()
    d.width, d.height, d.iterations, d.flags = W, H, iterations, flags
    d.sigma_luminance, d.sigma_normal, d.sigma_plane = sigmas
    bufs = {}
    for name, want, size, field in (("rgb", rgb, 12, "rgb32_device"), ("rgba", rgba, 4, "rgba8_device"),
                                    ("variance", variance, 4, "variance_device")):
        if want:
            bufs[name] = guarded(size * n)
            setattr(d, field, bufs[name].data_ptr() + GUARD)
    d.scratch_bytes = lib.rt_denoise_guided_scratch_bytes(W, H)
    assert d.scratch_bytes == 64 * n
    bufs["scratch"] = guarded(int(d.scratch_bytes))
    d.scratch_device = bufs["scratch"].data_ptr() + GUARD
    assert d.scratch_device % 16 == 0
    d.history_device, d.moments_device, d.hits_device = t["history"].data_ptr(), t["moments"].data_ptr(), t["hits"].data_ptr()
    d.albedo_device = t["albedo"].data_ptr() if t["albedo"] is not None else None
    d.stream = stream.cuda_stream if stream is not None else None
    torch.cuda.synchronize()
    rc = lib.rt_denoise_guided(0, C.byref(d))
    assert rc == abi.RT_OK, lib.rt_last_error()
    if stream is not None:
        stream.synchronize()
    elif flags & abi.RT_DENOISE_NO_SYNC:
        torch.cuda.synchronize()
    guards_intact(bufs)
    return (inner(bufs["rgb"], torch.float32, (H, W, 3)).cpu().numpy() if rgb else None,
            inner(bufs["rgba"], torch.uint8, (H, W, 4)).cpu().numpy() if rgba else None,
            inner(bufs["variance"], torch.float32, (H, W)).cpu().numpy() if variance else None)


def check_against_reference(name, rgb, v0, r):
    err = float(np.abs(rgb.astype(np.float64) - r["out64"]).max())
    verr = float(np.abs(v0.astype(np.float64) - r["v64"]).max())
    print(f"{name}: max|gpu-ref64|={err:.3g} F={r['F']:.3g} bar={r['bar']:.3g}; v_0: {verr:.3g} F_v={r['Fv']:.3g} bar_v={r['barv']:.3g}")
    assert np.isfinite(rgb).all() and np.isfinite(v0).all()
    assert verr <= r["barv"], (name, verr, r["barv"])
    assert err <= r["bar"], (name, err, r["bar"])


@pytest.mark.parametrize("with_albedo", (True, False), ids=("albedo", "plain"))
@pytest.mark.parametrize("case", G.CASES, ids=lambda c: "%dx%d_it%d" % c)
def test_guided_matches_reference(gpu_lib, case, with_albedo):
    r = G.reference(*case, with_albedo=with_albedo)
    rgb, rgba, v0 = denoise_guided(gpu_lib, upload(r), case[2])
    check_against_reference("%dx%d it=%d albedo=%s" % (*case, with_albedo), rgb, v0, r)
    assert np.array_equal(rgba, D.quantise(rgb))           # bit for bit, of the same call's rgb32


@pytest.mark.parametrize("off", (0, 1, 2), ids=("luminance_off", "normal_off", "plane_off"))
def test_guided_each_sigma_switched_off(gpu_lib, off):
    W, H, it = 65, 33, 4
    sigmas = tuple(INF if k == off else s for k, s in enumerate(G.SIGMAS))
    r = G.reference(W, H, it, True, sigmas)
    rgb, _, v0 = denoise_guided(gpu_lib, upload(r), it, sigmas)
    check_against_reference("65x33 it=4 sigmas=%s" % (sigmas,), rgb, v0, r)
    # the term is off, not merely weak: the result differs from the one with every term on
    assert np.abs(rgb - G.reference(W, H, it, True)["out32"]).max() > 10 * r["bar"]


def test_guided_first_frame_takes_the_spatial_estimate_everywhere(gpu_lib):
    r = G.reference(37, 23, 5, lengths="first")
    assert (r["g"]["history"][..., 3] == 1).all()
    rgb, _, v0 = denoise_guided(gpu_lib, upload(r), 5)
    check_against_reference("37x23 it=5 first frame", rgb, v0, r)


def test_guided_constant_image_with_zero_variance(gpu_lib):
    r = G.reference(37, 23, 5, with_albedo=False, lengths="constant")
    rgb, _, v0 = denoise_guided(gpu_lib, upload(r), 5)
    check_against_reference("37x23 it=5 constant", rgb, v0, r)
    assert (v0 == 0).all()
    assert np.abs(rgb - r["g"]["history"][..., :3]).max() <= r["bar"] + 8 * G.EPS32


@pytest.mark.parametrize("form", ("t", "d"))
def test_guided_both_forms_of_the_variance_kernel(gpu_lib, monkeypatch, form):
    """csrc/guided.hip computes the spatial variance estimate from an LDS tile or by direct loads;
    scripts/guided_bench.py switches between them through RTAMD_GUIDED_PREP, read per call.  Both give the default's
    bits (and so lie within the bar): compared here on the variance and on the filtered frame."""
    cases = [G.reference(*c) for c in ((1, 1, 1), (7, 1, 3), (1, 7, 3), (16, 16, 2), (17, 17, 2), (257, 5, 4), (96, 64, 5))]
    cases.append(G.reference(37, 23, 5, lengths="first"))
    for r in cases:
        t = upload(r)
        monkeypatch.delenv("RTAMD_GUIDED_PREP", raising=False)
        a = denoise_guided(gpu_lib, t, r["kw"]["iterations"])
        monkeypatch.setenv("RTAMD_GUIDED_PREP", form)
        b = denoise_guided(gpu_lib, t, r["kw"]["iterations"])
        assert same_bits(a[2], b[2]) and same_bits(a[0], b[0]), (form, r["g"]["miss"].shape)
        check_against_reference("%s form=%s" % (r["g"]["miss"].shape, form), b[0], b[2], r)
    monkeypatch.setenv("RTAMD_GUIDED_PREP", "tile")           # not one valid letter: ignored
    assert same_bits(denoise_guided(gpu_lib, t, 5)[0], a[0])


def test_guided_two_runs_outputs_optional_and_no_sync(gpu_lib):
    import torch
    r = G.reference(96, 64, 5)
    t = upload(r)
    a = denoise_guided(gpu_lib, t, 5)
    b = denoise_guided(gpu_lib, t, 5)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2])
    s = torch.cuda.Stream()
    for how in (dict(stream=s, flags=abi.RT_DENOISE_NO_SYNC), dict(stream=s), dict(flags=abi.RT_DENOISE_NO_SYNC)):
        c = denoise_guided(gpu_lib, t, 5, **how)
        assert same_bits(a[0], c[0]) and np.array_equal(a[1], c[1]) and same_bits(a[2], c[2]), how
    only_rgb = denoise_guided(gpu_lib, t, 5, rgba=False, variance=False)
    only_rgba = denoise_guided(gpu_lib, t, 5, rgb=False, variance=False)
    assert same_bits(a[0], only_rgb[0]) and np.array_equal(a[1], only_rgba[1])


def test_guided_inaccessible_buffer_and_device_are_rejected(gpu_lib):
    import torch
    r = G.reference(16, 16, 2)
    t = upload(r)
    W = H = 16
    n = W * H
    host = np.zeros(64 * n + 64, np.uint8)
    d = abi.DenoiseGuidedDesc()
    d.width, d.height, d.iterations = W, H, 2
    d.sigma_luminance, d.sigma_normal, d.sigma_plane = G.SIGMAS
    out = {k: torch.zeros(size * n, dtype=torch.uint8, device="cuda") for k, size in
           (("rgb32_device", 12), ("rgba8_device", 4), ("variance_device", 4), ("scratch_device", 64))}
    for k, v in out.items():
        setattr(d, k, v.data_ptr())
    d.scratch_bytes = 64 * n
    d.history_device, d.moments_device, d.hits_device = t["history"].data_ptr(), t["moments"].data_ptr(), t["hits"].data_ptr()
    d.albedo_device = t["albedo"].data_ptr()
    assert gpu_lib.rt_denoise_guided(0, C.byref(d)) == abi.RT_OK
    before = out["rgb32_device"].cpu().numpy().copy()
    for field in ("history_device", "moments_device", "hits_device", "albedo_device", "rgb32_device", "rgba8_device",
                  "variance_device", "scratch_device"):
        keep = getattr(d, field)
        setattr(d, field, host.ctypes.data // 16 * 16 + 16)   # pageable host memory
        assert gpu_lib.rt_denoise_guided(0, C.byref(d)) == INVALID, field
        assert b"accessible" in gpu_lib.rt_last_error()
        setattr(d, field, keep)
    d.rgb32_device = d.history_device                         # an output on an input
    assert gpu_lib.rt_denoise_guided(0, C.byref(d)) == INVALID
    assert b"overlap" in gpu_lib.rt_last_error()
    d.rgb32_device = out["rgb32_device"].data_ptr()
    assert gpu_lib.rt_denoise_guided(gpu_lib.rt_device_count(), C.byref(d)) == INVALID
    assert gpu_lib.rt_denoise_guided(-1, C.byref(d)) == INVALID
    current = torch.cuda.current_device()
    assert gpu_lib.rt_denoise_guided(0, C.byref(d)) == abi.RT_OK
    assert torch.cuda.current_device() == current
    assert np.array_equal(out["rgb32_device"].cpu().numpy(), before)
    # rt_accumulate_moments: the same two rejections
    g = G.moments_case(8, 8, "same")
    ta = upload_acc(g)
    a = abi.AccumulateDesc()
    a.width, a.height = 8, 8
    a.max_history, a.normal_cos, a.plane_tolerance = A.MAX_HISTORY, A.NORMAL_COS, A.PLANE_TOLERANCE
    hist, mom = torch.zeros((8, 8, 4), device="cuda"), torch.zeros((8, 8, 2), device="cuda")
    a.color_device, a.hits_device, a.history_device = ta["color"].data_ptr(), ta["hits"].data_ptr(), hist.data_ptr()
    a.prev_hits_device, a.prev_history_device = ta["prev_hits"].data_ptr(), ta["prev_history"].data_ptr()
    m = abi.MomentsDesc()
    m.albedo_device, m.prev_moments_device, m.moments_device = ta["albedo"].data_ptr(), ta["prev_moments"].data_ptr(), mom.data_ptr()
    assert gpu_lib.rt_accumulate_moments(0, C.byref(a), C.byref(m)) == abi.RT_OK
    for field in ("albedo_device", "prev_moments_device", "moments_device"):
        keep = getattr(m, field)
        setattr(m, field, host.ctypes.data // 16 * 16 + 16)
        assert gpu_lib.rt_accumulate_moments(0, C.byref(a), C.byref(m)) == INVALID, field
        assert b"accessible" in gpu_lib.rt_last_error()
        setattr(m, field, keep)
    assert gpu_lib.rt_accumulate_moments(gpu_lib.rt_device_count(), C.byref(a), C.byref(m)) == INVALID
    assert gpu_lib.rt_accumulate_moments(-1, C.byref(a), C.byref(m)) == INVALID


# ---- end to end ------------------------------------------------------------------------------------------------------

def gamma_rmse(a, b):
    ga, gb = np.sqrt(np.clip(a, 0.0, 1.0)), np.sqrt(np.clip(b, 0.0, 1.0))
    return float(np.sqrt(np.mean((ga.astype(np.float64) - gb) ** 2)))


def rows_dict(r):
    return None if r is None else {k: np.array(list(getattr(r, k)), np.float32) for k in ("centre", "rx", "ry", "rw")}


@pytest.mark.parametrize("dolly", (False, True), ids=("static", "dolly"))
def test_render_query_accumulate_guided_on_one_stream(gpu_lib, dolly):
    """tests/test_gpu_accumulate.py's end-to-end harness with the guided chain: the demo scene at 160 x 96, eight
    one-sample frames through render -> query_camera -> accumulate(moments=True) -> denoise_guided, all sync=False on
    one stream, every call with its defaults and nothing scaled per frame.  Every frame's history and moments equal the
    float32 restatement bit for bit and its guided frame lies within the bar of the float64 reference; at frame 1 and
    at frame 8 the guided frame is nearer to the converged one (256 samples) than its own input in gamma space."""
    import torch
    import rtamd
    W, H, FRAMES, SEED = 160, 96, 8, 0xACC0
    scene = scenes.demo_with_particles(6)
    r = Renderer(scene).build_acceleration_structure(7)
    base = np.array(scene.camera["center"], np.float64)
    toward = np.array(scene.camera["target"], np.float64) - base
    toward /= np.linalg.norm(toward)
    s = torch.cuda.Stream()
    frames, prev, prev_camera, centers = [], None, None, []
    for k in range(FRAMES):
        center = tuple(float(v) for v in base + (0.03 * k if dolly else 0.0) * toward)
        centers.append(center)
        r.configure_camera(W, H, ray_trace_depth=2, sample_count=1, center=center)
        with torch.cuda.stream(s):
            noisy = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        r.render(0, frame_seed=SEED + k, want_rgba=False, rgb32_device=noisy.data_ptr(), stream=s.cuda_stream, sync=False)
        q = r.query_camera(first_sample=True, frame_seed=SEED + k, want_t=False, want_hits=True, want_albedo=True,
                           stream=s, sync=False)
        view = rtamd.reprojection(prev_camera, W, H) if dolly and prev_camera is not None else None
        prev = r.accumulate(noisy, q["hits"], prev, prev_view=view, stream=s, sync=False, albedo=q["albedo"], moments=True)
        guided = r.denoise_guided(prev, q["albedo"], want_variance=True, stream=s, sync=False)
        frames.append({"color": noisy, "hits": q["hits"], "albedo": q["albedo"], "view": view, "out": prev, "guided": guided})
        prev_camera = r.camera
    # the hand-scaled rt_denoise of tests/test_gpu_accumulate.py, for the record
    first, last = frames[0], frames[-1]
    hand_1 = r.denoise(first["out"]["rgb"], first["hits"], first["albedo"], stream=s, sync=False)
    hand_8 = r.denoise(last["out"]["rgb"], last["hits"], last["albedo"], sigma_color=DENOISE_SIGMAS[0] / FRAMES ** 0.5,
                       stream=s, sync=False)
    s.synchronize()
    r.synchronize()
    kw = dict(max_history=ACCUMULATE_DEFAULTS[0], normal_cos=ACCUMULATE_DEFAULTS[1], plane_tolerance=ACCUMULATE_DEFAULTS[2])
    gkw = dict(iterations=5, sigma_luminance=GUIDED_SIGMAS[0], sigma_normal=GUIDED_SIGMAS[1], sigma_plane=GUIDED_SIGMAS[2])
    ref, ref_m, prev_hits = None, None, None
    name = "dolly" if dolly else "static"
    for k, f in enumerate(frames):
        hits = hits_to_numpy(f["hits"]).reshape(H, W)
        albedo = f["albedo"].cpu().numpy()
        ref, ref_m = G.accumulate_moments(f["color"].cpu().numpy(), albedo, hits, prev_hits, ref, ref_m, rows_dict(f["view"]),
                                          dtype=np.float32, **kw)
        assert same_bits(f["out"]["history"].cpu().numpy(), ref), (name, k)
        assert same_bits(f["out"]["moments"].cpu().numpy(), ref_m), (name, k)
        assert same_bits(f["out"]["rgb"].cpu().numpy(), ref[..., :3]), (name, k)
        prev_hits = hits
        miss = hits["instance"] == abi.MISS
        args = (ref, ref_m, hits["normal"], hits["point"], miss, albedo)
        o64, v64 = G.guided(*args, dtype=np.float64, **gkw)
        o32, v32 = G.guided(*args, dtype=np.float32, **gkw)
        F, Fv = float(np.abs(o32 - o64).max()), float(np.abs(v32 - v64).max())
        bar = 4.0 * F + 4.0 * G.EPS32 * float(np.abs(ref[..., :3]).max())
        barv = 4.0 * Fv + 4.0 * G.EPS32 * float(v64.max())
        err = float(np.abs(f["guided"]["rgb"].cpu().numpy() - o64).max())
        verr = float(np.abs(f["guided"]["variance"].cpu().numpy() - v64).max())
        print(f"demo 160x96 {name} frame {k}: max|gpu-ref64|={err:.3g} F={F:.3g} bar={bar:.3g}; v_0: {verr:.3g} bar_v={barv:.3g}")
        assert verr <= barv, (name, k, verr, barv)
        assert err <= bar, (name, k, err, bar)
    assert miss.any() and not miss.all()
    # the converged frames: the first and the last camera with 256 samples per pixel
    figures = {}
    for k, f, hand in ((0, first, hand_1), (FRAMES - 1, last, hand_8)):
        r.configure_camera(W, H, ray_trace_depth=2, sample_count=256, center=centers[k])
        _, converged, _ = r.render(0, frame_seed=SEED, want_rgba=False, want_rgb=True)
        figures[k] = (gamma_rmse(f["out"]["rgb"].cpu().numpy(), converged), gamma_rmse(f["guided"]["rgb"].cpu().numpy(), converged),
                      gamma_rmse(hand["rgb"].cpu().numpy(), converged))
        print(f"{name} frame {k + 1}: gamma-space RMSE against 256 spp: input {figures[k][0]:.4f}, guided {figures[k][1]:.4f}, "
              f"hand-scaled rt_denoise {figures[k][2]:.4f}")
    r.cleanup()
    for k, (e_in, e_guided, _) in figures.items():
        assert e_guided < e_in, (name, k + 1, e_guided, e_in)
