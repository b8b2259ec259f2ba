#!/usr/bin/env python3
"""rt_denoise timings on the C2 scene's own guides (profiles/denoise/README.md).

Per shape (1920x1080 and 3840x2160 by default): one 1-spp frame of C2's scene is rendered into device memory,
rt_query_camera writes its hit records and albedo, and rt_denoise runs on them with 5 iterations, albedo on, rgb32 and
rgba8 out, into buffers allocated once.  Timed with device events around batches of calls on one stream, after a
warm-up of every shape and of every form of the passes of step 4, 8 and 16; the forms (--forms: one letter per such
pass, t = LDS tile (step 4 only), d = direct, r = rows; RTAMD_DENOISE_FORMS, read by the library per call) alternate
batch by batch in this one process.

Reported per shape and form: ms per call (mean and spread over the batches); the time of a call with k = 1..5
iterations and the increments T(k) - T(k-1), i.e. what the pass of step 2^(k-1) adds (T(1) is the pack pass plus one
last pass; an increment is a pass that writes a colour plane instead of the outputs); and the achieved rate on the
compulsory bytes, as a share of the 6.3 TB/s of HBM bandwidth that is achievable on an MI355X.  That share is a
whole-call figure (launch gaps included), not one kernel's.

Compulsory bytes per pixel: pack pass 72 read (12 colour + 12 albedo + 48 rt_hit) + 48 written; a filter pass 48 read
+ 16 written; the last pass 48 read + 12 + 4 written.  So a call of k iterations moves 120 + 64 k bytes per pixel.

One JSON line per measurement on stdout; --out also writes them to a file.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "real-time-gpu-ray-tracer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ACHIEVABLE_TBS = 6.3
ENV = "RTAMD_DENOISE_FORMS"


def bytes_per_pixel(iterations):
    pack = 72 + 48
    middle = (iterations - 1) * (48 + 16)
    last = 48 + 12 + 4
    return pack + middle + last


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="1920x1080,3840x2160")
    ap.add_argument("--forms", default="tdd,ddd,rdd,trd,tdr,trr,rrr", help="the form strings to alternate")
    ap.add_argument("--batches", type=int, default=10, help="timed batches per form (alternating)")
    ap.add_argument("--calls", type=int, default=40, help="calls per batch")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.batches * a.calls >= 200, "at least 200 timed calls per form"

    import torch
    from rtamd import Renderer, abi, scenes
    from rtamd.renderer import DENOISE_SIGMAS
    assert torch.cuda.is_available(), "needs a GPU: no timing is taken without one"
    lib = abi.load_library()
    cfg = scenes.CONFIGS["C2"]
    r = Renderer(scenes.config_scene(cfg)).build_acceleration_structure(0, mode="sah")
    stream = torch.cuda.Stream()
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    c2_ms = None
    try:
        with open(os.path.join(REPO, "profiles", "r06_final", "bench_C2_sah.json")) as f:
            c2_ms = json.load(f).get("ms_per_step")
    except OSError:
        pass

    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    jobs = []
    for W, H in shapes:
        r.configure_camera(W, H, ray_trace_depth=cfg.depth, sample_count=1)
        with torch.cuda.stream(stream):
            noisy = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            out = torch.empty_like(noisy)
            rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
            scratch = torch.empty(lib.rt_denoise_scratch_bytes(W, H), dtype=torch.uint8, device="cuda")
        r.render(0, want_rgba=False, rgb32_device=noisy.data_ptr(), stream=stream.cuda_stream, sync=False)
        q = r.query_camera(first_sample=True, want_t=False, want_hits=True, want_albedo=True, stream=stream, sync=False)
        stream.synchronize()
        d = abi.DenoiseDesc()
        d.width, d.height, d.iterations, d.flags = W, H, 5, abi.RT_DENOISE_NO_SYNC
        d.sigma_color, d.sigma_normal, d.sigma_plane = DENOISE_SIGMAS
        d.color_device, d.hits_device, d.albedo_device = noisy.data_ptr(), q["hits"].data_ptr(), q["albedo"].data_ptr()
        d.rgb32_device, d.rgba8_device = out.data_ptr(), rgba.data_ptr()
        d.scratch_device, d.scratch_bytes = scratch.data_ptr(), scratch.numel()
        d.stream = stream.cuda_stream
        jobs.append((W, H, d, (noisy, out, rgba, scratch, q)))

    def batch(d, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            abi.check(lib, lib.rt_denoise(0, C.byref(d)))
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    forms = a.forms.split(",")
    for W, H, d, _ in jobs:                       # warm-up: every shape, every iteration count, every form
        for form in forms:
            os.environ[ENV] = form
            for k in range(1, 6):
                d.iterations = k
                batch(d, a.warmup)
    for W, H, d, _ in jobs:
        npix = W * H
        d.iterations = 5
        ms = {form: [] for form in forms}
        for _ in range(a.batches):                # alternating
            for form in forms:
                os.environ[ENV] = form
                ms[form].append(batch(d, a.calls))
        for form in forms:
            mean = statistics.fmean(ms[form])
            rate = bytes_per_pixel(5) * npix / (mean * 1e-3) / 1e12
            emit(what="call", shape=f"{W}x{H}", iterations=5, forms=form,
                 ms_per_call=round(mean, 4), ms_min=round(min(ms[form]), 4), ms_max=round(max(ms[form]), 4),
                 calls=a.batches * a.calls, bytes_per_pixel=bytes_per_pixel(5), compulsory_TB_per_s=round(rate, 3),
                 share_of_achievable_6_3_TB_per_s=round(rate / ACHIEVABLE_TBS, 3), c2_frame_ms_r06_final=c2_ms)
        for form in forms:                        # per pass: calls of 1..5 iterations
            os.environ[ENV] = form
            t = []
            for k in range(1, 6):
                d.iterations = k
                t.append(statistics.fmean(batch(d, a.calls) for _ in range(max(1, a.batches // 2))))
            emit(what="passes", shape=f"{W}x{H}", forms=form,
                 ms_by_iterations=[round(v, 4) for v in t],
                 ms_added_by_step={str(1 << k): round(t[k] - t[k - 1], 4) for k in range(1, 5)},
                 ms_pack_plus_last_pass=round(t[0], 4))
    os.environ.pop(ENV, None)
    r.cleanup()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
