#!/usr/bin/env python3
"""rt_accumulate_moments against rt_accumulate and rt_denoise_guided against rt_denoise, on the C2 scene's own frames
(profiles/guided/README.md), in scripts/denoise_bench.py's manner: device events around batches of calls on one stream,
the candidates alternated batch by batch in this one process after a warm-up of each, every batch rotating over
--spread copies of its buffers so that no call finds its data in the 256 MiB Infinity Cache.

Per shape (1920x1080 and 3840x2160 by default) --history one-sample frames of C2's scene from a still camera are
accumulated with rt_accumulate_moments, which gives the steady state (every hit pixel --history frames long, sky 1);
the first of them alone gives the first frame (every pixel 1 long, so rt_denoise_guided's spatial variance estimate
runs everywhere).  A second pair of frames from a camera that strafed and turned a little times the four-tap case
of the accumulation (scripts/accumulate_bench.py's "moving").

Reported: ms per call (mean, min and max over the batches) of rt_accumulate and rt_accumulate_moments, static and
moving; of rt_denoise, rt_denoise_guided on the first frame and in the steady state, 5 iterations, with each form of
its variance kernel (--prep-forms: t = LDS tile, d = direct; RTAMD_GUIDED_PREP, read by the library per call); and the
same with 1..5 iterations, so that the difference per pass can be read off.  rt_accumulate_moments moves 28 more compulsory
bytes per kept pixel than rt_accumulate's 152: 12 albedo, 8 moments in, 8 moments out.

One JSON line per measurement on stdout; --out also writes them to a file."""
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


PREP_ENV = "RTAMD_GUIDED_PREP"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="1920x1080,3840x2160")
    ap.add_argument("--history", type=int, default=8)
    ap.add_argument("--batches", type=int, default=10, help="timed batches per candidate (alternating)")
    ap.add_argument("--calls", type=int, default=20, help="calls per batch")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--prep-forms", default="t,d", help="the variance kernel's forms to alternate (RTAMD_GUIDED_PREP)")
    ap.add_argument("--spread", type=int, default=4, help="copies of the buffers a batch rotates over")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.batches * a.calls >= 200, "at least 200 timed calls per candidate"

    import torch
    import rtamd
    from rtamd import Renderer, abi, scenes
    from rtamd.renderer import ACCUMULATE_DEFAULTS, DENOISE_SIGMAS, GUIDED_SIGMAS
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
    last_camera = dict(center=(centre[0] - 0.01 * reach, centre[1], centre[2]), target=(target[0] - 0.02 * reach, target[1], target[2]))

    def frame(W, H, seed, **camera):
        r.configure_camera(W, H, ray_trace_depth=cfg.depth, sample_count=1, **camera)
        with torch.cuda.stream(stream):
            noisy = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        r.render(0, frame_seed=seed, want_rgba=False, rgb32_device=noisy.data_ptr(), stream=stream.cuda_stream, sync=False)
        q = r.query_camera(first_sample=True, frame_seed=seed, want_t=False, want_hits=True, want_albedo=True, stream=stream,
                           sync=False)
        stream.synchronize()
        return noisy, q["hits"], q["albedo"], r.camera

    def copies(tensors):
        with torch.cuda.stream(stream):
            return [{k: v.clone() for k, v in tensors.items()} for _ in range(max(1, a.spread))]

    def accumulate_descs(W, H, cur, prev, view):
        """(rt_accumulate descs, rt_accumulate_moments (desc, moments) pairs), one per buffer set."""
        plain, with_moments = [], []
        for t in copies({"rgb": cur[0], "hits": cur[1], "albedo": cur[2], "prev_hits": prev["hits"], "prev_history": prev["history"],
                         "prev_moments": prev["moments"], "history": torch.empty_like(prev["history"]),
                         "out": torch.empty_like(cur[0]), "moments": torch.empty_like(prev["moments"])}):
            d = abi.AccumulateDesc()
            d.width, d.height, d.flags = W, H, abi.RT_ACCUMULATE_NO_SYNC
            d.max_history, d.normal_cos, d.plane_tolerance = ACCUMULATE_DEFAULTS
            if view is not None:
                d.prev_view = C.pointer(view)
            d.color_device, d.hits_device = t["rgb"].data_ptr(), t["hits"].data_ptr()
            d.prev_hits_device, d.prev_history_device = t["prev_hits"].data_ptr(), t["prev_history"].data_ptr()
            d.history_device, d.rgb32_device = t["history"].data_ptr(), t["out"].data_ptr()
            d.stream = stream.cuda_stream
            m = abi.MomentsDesc()
            m.albedo_device, m.prev_moments_device, m.moments_device = (t["albedo"].data_ptr(), t["prev_moments"].data_ptr(),
                                                                        t["moments"].data_ptr())
            plain.append((d, t))
            with_moments.append((d, m, t))
        return plain, with_moments

    def filter_descs(W, H, acc, noisy, albedo):
        """(rt_denoise descs on the noisy frame, rt_denoise_guided descs on `acc`), one per buffer set."""
        n_scratch = int(lib.rt_denoise_guided_scratch_bytes(W, H))
        plain, guided = [], []
        for t in copies({"noisy": noisy, "history": acc["history"], "moments": acc["moments"], "hits": acc["hits"], "albedo": albedo,
                         "out": torch.empty_like(noisy), "rgba": torch.empty((H, W, 4), dtype=torch.uint8, device="cuda"),
                         "scratch": torch.empty(n_scratch, dtype=torch.uint8, device="cuda")}):
            d = abi.DenoiseDesc()
            d.width, d.height, d.iterations, d.flags = W, H, 5, abi.RT_DENOISE_NO_SYNC
            d.sigma_color, d.sigma_normal, d.sigma_plane = DENOISE_SIGMAS
            d.color_device, d.hits_device, d.albedo_device = t["noisy"].data_ptr(), t["hits"].data_ptr(), t["albedo"].data_ptr()
            g = abi.DenoiseGuidedDesc()
            g.width, g.height, g.iterations, g.flags = W, H, 5, abi.RT_DENOISE_NO_SYNC
            g.sigma_luminance, g.sigma_normal, g.sigma_plane = GUIDED_SIGMAS
            g.history_device, g.moments_device = t["history"].data_ptr(), t["moments"].data_ptr()
            g.hits_device, g.albedo_device = t["hits"].data_ptr(), t["albedo"].data_ptr()
            for x in (d, g):
                x.rgb32_device, x.rgba8_device = t["out"].data_ptr(), t["rgba"].data_ptr()
                x.scratch_device, x.scratch_bytes = t["scratch"].data_ptr(), n_scratch
                x.stream = stream.cuda_stream
            plain.append((d, t))
            guided.append((g, t))
        return plain, guided

    def batch(call, sets, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for k in range(calls):
            call(sets[k % len(sets)])
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    def acc_plain(s):
        abi.check(lib, lib.rt_accumulate(0, C.byref(s[0])))

    def acc_moments(s):
        abi.check(lib, lib.rt_accumulate_moments(0, C.byref(s[0]), C.byref(s[1])))

    def den_plain(s):
        abi.check(lib, lib.rt_denoise(0, C.byref(s[0])))

    def den_guided(s):
        abi.check(lib, lib.rt_denoise_guided(0, C.byref(s[0])))

    def guided_with(form):                        # the variance kernel's form: t = LDS tile, d = direct (read per call)
        def call(s):
            os.environ[PREP_ENV] = form
            den_guided(s)
        return call

    def compare(what, shape, candidates, **extra):
        """candidates: {name: (call, sets)}: warm-up of each, then alternating batches."""
        for call, sets in candidates.values():
            batch(call, sets, a.warmup)
        ms = {name: [] for name in candidates}
        for _ in range(a.batches):
            for name, (call, sets) in candidates.items():
                ms[name].append(batch(call, sets, a.calls))
        for name in candidates:
            emit(what=what, shape=shape, candidate=name, ms_per_call=round(statistics.fmean(ms[name]), 4),
                 ms_median=round(statistics.median(ms[name]), 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                 calls=a.batches * a.calls, buffer_sets=len(candidates[name][1]), **extra)

    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    for W, H in shapes:
        shape = f"{W}x{H}"
        # the steady state and the first frame, from a still camera
        acc, first = None, None
        for k in range(a.history):
            cur = frame(W, H, 0x5EED + k)
            prev = acc
            acc = r.accumulate(cur[0], cur[1], acc, albedo=cur[2], moments=True, stream=stream)
            first = first or acc
        kept = float((acc["history"][..., 3] > 1.0).float().mean())
        plain, with_moments = accumulate_descs(W, H, cur, prev, None)
        compare("accumulate", shape, {"rt_accumulate": (acc_plain, plain), "rt_accumulate_moments": (acc_moments, with_moments)},
                camera="static", pixels_keeping_history=round(kept, 3))
        del plain, with_moments
        # four taps: the last frame from a camera that strafed and turned a little
        last = frame(W, H, 0x5EED + 100, **last_camera)
        cur2 = frame(W, H, 0x5EED + 101)
        prev2 = r.accumulate(last[0], last[1], None, albedo=last[2], moments=True, stream=stream)
        plain, with_moments = accumulate_descs(W, H, cur2, prev2, rtamd.reprojection(last[3], W, H))
        compare("accumulate", shape, {"rt_accumulate": (acc_plain, plain), "rt_accumulate_moments": (acc_moments, with_moments)},
                camera="moving")
        del plain, with_moments, last, cur2, prev2
        # the filters
        d_plain, g_steady = filter_descs(W, H, acc, cur[0], cur[2])
        _, g_first = filter_descs(W, H, first, cur[0], cur[2])
        stream.synchronize()
        cands = {"rt_denoise": (den_plain, d_plain)}
        for form in a.prep_forms.split(","):
            cands[f"rt_denoise_guided_first_frame_prep_{form}"] = (guided_with(form), g_first)
            cands[f"rt_denoise_guided_steady_prep_{form}"] = (guided_with(form), g_steady)
        compare("filter", shape, cands, iterations=5, share_below_4_steady=round(float((acc["history"][..., 3] < 4).float().mean()), 4))
        by_iter = {name: [] for name in cands}
        for k in range(1, 6):
            for name, (call, sets) in cands.items():
                for s in sets:
                    s[0].iterations = k
                batch(call, sets, a.warmup)
            t = {name: [] for name in cands}
            for _ in range(max(1, a.batches // 2)):
                for name, (call, sets) in cands.items():
                    t[name].append(batch(call, sets, a.calls))
            for name in cands:
                by_iter[name].append(statistics.fmean(t[name]))
        for name in cands:
            t = by_iter[name]
            emit(what="passes", shape=shape, candidate=name, ms_by_iterations=[round(v, 4) for v in t],
                 ms_added_by_step={str(1 << k): round(t[k] - t[k - 1], 4) for k in range(1, 5)},
                 ms_prep_plus_last_pass=round(t[0], 4))
        del d_plain, g_steady, g_first, cands, acc, first, cur, prev
        torch.cuda.empty_cache()
    os.environ.pop(PREP_ENV, None)
    r.cleanup()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
