#!/usr/bin/env python3
"""rt_accumulate timings on the C2 scene's own frames (profiles/accumulate/README.md).

Per shape (1920x1080 and 3840x2160 by default) two 1-spp frames of C2's scene are rendered into device memory with
their rt_query_camera records: the last frame and this one, from the same camera ("static", prev_view NULL: one tap
per pixel) and from a camera that has strafed and turned a little ("moving", prev_view = rt_camera_reprojection of the
last camera: four taps).  The last frame's history comes from a first-frame call.  rt_accumulate then runs with
Renderer.accumulate's default thresholds, history and rgb32 out, into buffers allocated once.  Timed with device events
around batches of calls on one stream, after a warm-up of every shape, camera and mapping; the two pixel-to-lane
mappings (r = rows, b = blocks; RTAMD_ACCUMULATE_FORM, read by the library per call) alternate batch by batch in this
one process.

Reported per shape, camera and mapping: ms per call (mean and spread over the batches), the share of pixels that
kept their history, and the achieved rate on the compulsory bytes as a share of the 6.3 TB/s of HBM bandwidth that is
achievable on an MI355X.  Compulsory bytes per pixel: 12 colour + 48 rt_hit + 48 of last frame's records (which
neighbouring lanes' taps share) + 16 history in + 16 history out + 12 rgb out = 152.  The share is a whole-call figure
(launch gaps included), and it counts 152 bytes for every pixel although a sky pixel moves 88: the share of pixels
that kept their history says how far that is off.  A call's buffers are 315 MB at 1080p and 1.26 GB at 4K; --spread N
rotates each batch over N copies of them so that no call finds its data in the 256 MiB Infinity Cache.

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
BYTES_PER_PIXEL = 12 + 48 + 48 + 16 + 16 + 12
ENV = "RTAMD_ACCUMULATE_FORM"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="1920x1080,3840x2160")
    ap.add_argument("--forms", default="r,b", help="the mappings to alternate")
    ap.add_argument("--batches", type=int, default=10, help="timed batches per mapping (alternating)")
    ap.add_argument("--calls", type=int, default=40, help="calls per batch")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--spread", type=int, default=4, help="copies of the buffers a batch rotates over (1: one set)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.batches * a.calls >= 200, "at least 200 timed calls per mapping"

    import torch
    import rtamd
    from rtamd import Renderer, abi, scenes
    from rtamd.renderer import ACCUMULATE_DEFAULTS
    assert torch.cuda.is_available(), "needs a GPU: no timing is taken without one"
    lib = abi.load_library()
    cfg = scenes.CONFIGS["C2"]
    scene = scenes.config_scene(cfg)
    r = Renderer(scene).build_acceleration_structure(0, mode="sah")
    stream = torch.cuda.Stream()
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    centre = [float(v) for v in scene.camera["center"]]
    target = [float(v) for v in scene.camera["target"]]
    reach = sum((t - c) ** 2 for c, t in zip(centre, target)) ** 0.5
    # the last frame's camera of the "moving" case: a strafe of 1 % and a turn of 2 % of the distance to the target
    last_camera = dict(center=(centre[0] - 0.01 * reach, centre[1], centre[2]), target=(target[0] - 0.02 * reach, target[1], target[2]))

    def frame(W, H, seed, **camera):
        r.configure_camera(W, H, ray_trace_depth=cfg.depth, sample_count=1, **camera)
        with torch.cuda.stream(stream):
            noisy = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        r.render(0, frame_seed=seed, want_rgba=False, rgb32_device=noisy.data_ptr(), stream=stream.cuda_stream, sync=False)
        q = r.query_camera(first_sample=True, frame_seed=seed, want_t=False, want_hits=True, want_albedo=False,
                           stream=stream, sync=False)
        stream.synchronize()
        return noisy, q["hits"], r.camera

    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    jobs = []
    for W, H in shapes:
        for name, camera in (("static", {}), ("moving", last_camera)):
            last_rgb, last_hits, last_ci = frame(W, H, 0x5EED + 1, **camera)
            rgb, hits, _ = frame(W, H, 0x5EED)
            first = r.accumulate(last_rgb, last_hits, None, stream=stream)
            view = rtamd.reprojection(last_ci, W, H) if name == "moving" else None
            sets = []
            for _ in range(max(1, a.spread)):
                with torch.cuda.stream(stream):
                    t = {"rgb": rgb.clone(), "hits": hits.clone(), "prev_hits": last_hits.clone(),
                         "prev_history": first["history"].clone(), "history": torch.empty_like(first["history"]),
                         "out": torch.empty_like(rgb)}
                d = abi.AccumulateDesc()
                d.width, d.height, d.flags = W, H, abi.RT_ACCUMULATE_NO_SYNC
                d.max_history, d.normal_cos, d.plane_tolerance = ACCUMULATE_DEFAULTS
                if view is not None:
                    d.prev_view = C.pointer(view)
                d.color_device, d.hits_device = t["rgb"].data_ptr(), t["hits"].data_ptr()
                d.prev_hits_device, d.prev_history_device = t["prev_hits"].data_ptr(), t["prev_history"].data_ptr()
                d.history_device, d.rgb32_device = t["history"].data_ptr(), t["out"].data_ptr()
                d.stream = stream.cuda_stream
                sets.append((d, t))
            stream.synchronize()
            jobs.append((W, H, name, sets, view))

    def batch(sets, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for k in range(calls):
            abi.check(lib, lib.rt_accumulate(0, C.byref(sets[k % len(sets)][0])))
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    forms = a.forms.split(",")
    for W, H, name, sets, _ in jobs:              # warm-up: every shape, camera and mapping
        for form in forms:
            os.environ[ENV] = form
            batch(sets, a.warmup)
    for W, H, name, sets, _ in jobs:
        npix = W * H
        ms = {form: [] for form in forms}
        for _ in range(a.batches):                # alternating
            for form in forms:
                os.environ[ENV] = form
                ms[form].append(batch(sets, a.calls))
        kept = float((sets[0][1]["history"][..., 3] > 1.0).float().mean())
        for form in forms:
            mean = statistics.fmean(ms[form])
            rate = BYTES_PER_PIXEL * npix / (mean * 1e-3) / 1e12
            emit(what="call", shape=f"{W}x{H}", camera=name, form=form, buffer_sets=len(sets),
                 ms_per_call=round(mean, 4), ms_median=round(statistics.median(ms[form]), 4), ms_min=round(min(ms[form]), 4),
                 ms_max=round(max(ms[form]), 4), calls=a.batches * a.calls, pixels_keeping_history=round(kept, 3),
                 bytes_per_pixel=BYTES_PER_PIXEL, compulsory_TB_per_s=round(rate, 3),
                 share_of_achievable_6_3_TB_per_s=round(rate / ACHIEVABLE_TBS, 3))
    os.environ.pop(ENV, None)
    r.cleanup()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
