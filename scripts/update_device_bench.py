#!/usr/bin/env python3
"""Cost of handing a deforming scene's triangles to the library, host path against device path.

At --config's scene (default C5: 10 M particle triangles) built as bench.py builds it with --build lbvh --rebuild, in
one process, alternating the three and repeating each --reps times after warm-up:

  (a) rt_scene_update_triangles over all particle triangles from a host array;
  (b) rt_scene_update_triangles_device with normals over the same range;
  (b') (b) with RT_TRI_UPDATE_BOUNDS: the device also derives the particle instances' bounds (csrc/inst_bounds.hip reads
      36 B per triangle more).  The library releases the caller's stream behind the write kernel, before those kernels,
      so events on that stream do not see them: (b') is timed on the host clock, against "b_wall";
  (c) a plain device-to-device hipMemcpyAsync (torch copy_) that moves the bytes (b) must move, read plus write:
      72 B read + 112 B written per triangle = a copy of 92 B per triangle.  The yardstick for (b)'s kernel.
  (d) what per-frame bounds cost without the flag: (b) plus rt_scene_update_instances for every particle instance
      (descriptions prepared once), host clock.  It runs last, after the frames: it breaks the particles' group for good.

(b) and (c) are timed by events on the caller's stream around the call (the library makes that stream wait for its
kernel, so the stop event falls behind it).  (a) has no device bracket: most of it is host work (the material walk, two
memcpys) before its copy reaches the scene's stream, so (a) is timed on the host from the call to rt_synchronize's
return, and so is (b) a second time ("b_wall") to compare the two in one measure.

Then frames with the per-frame rebuild, pipelined on the library's lanes as bench.py's, each frame preceded by (a) or
by (b) without waiting: ms per frame on the host clock over --frames frames; then --pairs alternating pairs of such
runs with (b') and with (b) ("frame_pairs_ms").

Each step runs under a time limit of its own (--step-timeout seconds, SIGALRM): a step that exceeds it ends the
process.  Prints one JSON line per step and a summary line."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "real-time-gpu-ray-tracer_amd"))


class step:
    """with step(name, seconds): the body under a time limit of its own."""

    def __init__(self, name, limit):
        self.name, self.limit = name, limit

    def _expired(self, *_):
        print(json.dumps({"step": self.name, "error": f"exceeded {self.limit} s"}), flush=True)
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.limit)
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        signal.alarm(0)
        print(json.dumps({"step": self.name, "seconds": round(time.perf_counter() - self.t0, 3)}), flush=True)


def spread(ms):
    s = sorted(ms)
    return {"median": round(statistics.median(s), 4), "min": round(s[0], 4), "max": round(s[-1], 4),
            "p10": round(s[len(s) // 10], 4), "p90": round(s[(9 * len(s)) // 10], 4), "n": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--pre-opt", action="append", default=[], help="rt_scene_set_option key=value before the build")
    a = ap.parse_args()
    import ctypes as C

    import numpy as np
    import torch
    from rtamd import Renderer, abi, scenes

    cfg = scenes.CONFIGS[a.config]
    n_p = cfg.particles * 1024
    with step("build", a.step_timeout):
        scene = scenes.config_scene(cfg)
        r = Renderer(scene)
        r.set_option("rebuild", 1)                       # before the build, as bench.py --rebuild
        for kv in a.pre_opt:
            k, v = kv.split("=")
            r.set_option(k, int(v, 0))
        r.build_acceleration_structure(0, mode="lbvh").configure_camera(cfg.width, cfg.height)
        r.set_option("overlap", -1)
        tris = np.ascontiguousarray(scene.triangles[:n_p])
        verts = torch.from_numpy(np.ascontiguousarray(tris["vertex"]).reshape(-1)).cuda()
        norms = torch.from_numpy(np.ascontiguousarray(tris["normal"]).reshape(-1)).cuda()
        copy_src = torch.empty(92 * n_p, dtype=torch.uint8, device="cuda")
        copy_dst = torch.empty_like(copy_src)
        first_inst = len(scene.instances) - cfg.particles
        inst_descs = scenes.instance_desc_array(scene.instances[first_inst:])
        frame_bufs = [torch.zeros(cfg.width * cfg.height * 4, dtype=torch.uint8, device="cuda") for _ in range(8)]
        st = torch.cuda.Stream()
        torch.cuda.synchronize()

    def timed_on_stream(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def host_update():
        t0 = time.perf_counter()
        r.update_triangles(0, tris)
        r.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def device_update_wall(bounds=False):
        t0 = time.perf_counter()
        r.update_triangles_device(0, verts, norms, stream=st, bounds=bounds)
        r.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def memcpy():
        with torch.cuda.stream(st):
            copy_dst.copy_(copy_src, non_blocking=True)

    def device_plus_instances_wall():
        t0 = time.perf_counter()
        r.update_triangles_device(0, verts, norms, stream=st, sync=False)
        abi.check(r.lib, r.lib.rt_scene_update_instances(r.h, first_inst, cfg.particles, inst_descs))
        r.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ms = {"a_host_wall": [], "b_device_events": [], "b2_device_bounds_wall": [], "b_device_wall": [], "c_memcpy_events": []}
    with step("updates", a.step_timeout):
        for k in range(a.warmup + a.reps):
            row = {"a_host_wall": host_update(),
                   "b_device_events": timed_on_stream(lambda: r.update_triangles_device(0, verts, norms, stream=st, sync=False)),
                   "b2_device_bounds_wall": device_update_wall(bounds=True),
                   "c_memcpy_events": timed_on_stream(memcpy),
                   "b_device_wall": device_update_wall()}
            r.synchronize()
            if k >= a.warmup:
                for key, v in row.items():
                    ms[key].append(v)

    def frames(update):
        for f in range(a.warmup + a.frames):
            if f == a.warmup:
                r.synchronize()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            update()
            r.render(f, want_rgba=False, rgba8_device=frame_bufs[f % 8].data_ptr(), sync=False)
        r.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.frames

    frame_ms = {}
    with step("frames_host_update", a.step_timeout):
        frame_ms["a_host"] = round(frames(lambda: r.update_triangles(0, tris)), 4)
    with step("frames_device_update", a.step_timeout):
        frame_ms["b_device"] = round(frames(lambda: r.update_triangles_device(0, verts, norms, stream=st, sync=False)), 4)
    with step("frames_no_update", a.step_timeout):
        frame_ms["none"] = round(frames(lambda: None), 4)

    pairs = {"b2_device_bounds": [], "b_device": []}
    with step("frame_pairs", a.step_timeout):
        for _ in range(a.pairs):
            pairs["b2_device_bounds"].append(round(frames(
                lambda: r.update_triangles_device(0, verts, norms, stream=st, sync=False, bounds=True)), 4))
            pairs["b_device"].append(round(frames(
                lambda: r.update_triangles_device(0, verts, norms, stream=st, sync=False)), 4))
    ms["d_device_plus_instances_wall"] = []
    with step("device_plus_instances", a.step_timeout):
        for k in range(a.warmup + a.reps):
            v = device_plus_instances_wall()
            if k >= a.warmup:
                ms["d_device_plus_instances_wall"].append(v)

    out = {"config": a.config, "opts": a.pre_opt, "triangles": n_p, "update_ms": {k: spread(v) for k, v in ms.items()},
           "bytes_moved_b": 184 * n_p, "frame_ms": frame_ms, "frame_pairs_ms": pairs, "frames": a.frames,
           "device": torch.cuda.get_device_name(0)}
    b, c = out["update_ms"]["b_device_events"]["median"], out["update_ms"]["c_memcpy_events"]["median"]
    out["b_GBps"] = round(184 * n_p / (b * 1e6), 1)
    out["c_GBps"] = round(184 * n_p / (c * 1e6), 1)
    out["b_over_c"] = round(b / c, 3)
    out["b2_minus_b_wall_ms"] = round(out["update_ms"]["b2_device_bounds_wall"]["median"] -
                                      out["update_ms"]["b_device_wall"]["median"], 4)
    print(json.dumps(out), flush=True)
    r.cleanup()


if __name__ == "__main__":
    main()
