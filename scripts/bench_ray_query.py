#!/usr/bin/env python3
"""rt_query_rays on a benchmark config's scene (default C2: SAH trees, frame 0): device time of closest hit with
records, closest hit with t only and any-hit, on

  (a) the camera's primary rays through the pixel centres (RenderPin.cu:73-95, no jitter), and
  (b) ambient-occlusion rays: origins at (a)'s hit points, directions uniform on the hit normal's hemisphere
      (fixed seed), tmax = 2.0 — incoherent rays;

as the median of --launches launches after --warmup warm-ups, timed with torch CUDA events on the query's stream.
The closest-t run on (b) is repeated three times: the spread is what "any-hit is not slower than closest-t" is held
to.  Next to them: the wall time of rt_trace_rays (host rays, the one-thread-per-ray kernel) on the same rays, and
set (a) made by the library itself (a_camera_query: rt_query_camera, centre rays, t only, three runs).
The refill threshold is a compile-time constant (RT_QUERY_THRESHOLD, csrc/ray_query.hpp): for a sweep, build variants
with scripts/build_variant.sh and run this script per library through RTAMD_LIB.

  --trace-once     only: one rt_trace_rays call on set (b), then one closest query with records on it with the same
                   range and one with tmax = 2.0, for a kernel trace that lists trace_rays_kernel's device time next
                   to ray_query_kernel's (rocprofv3 --kernel-trace --stats -- python scripts/bench_ray_query.py
                   --trace-once; the first ray_query_kernel dispatch is set (a), which makes set (b))
  --camera         instead: rt_query_camera (centre rays; t only, records + albedo, rays only) against rt_query_rays on
                   set (a) in a buffer, in row order and in 8x8-tile order, and against the torch expression that
                   produces that buffer on the device; the variants alternated --repeats times in one process
  --out FILE       write the JSON there as well as to stdout
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "real-time-gpu-ray-tracer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def camera_frame(ci, w, h):
    """(centre, pixel origin, dx, dy) of the camera's pixel grid (RenderPin.cu:73-95), float64."""
    v = lambda a: np.asarray([a.x, a.y, a.z], np.float64)
    center, target, up = v(ci.center), v(ci.target), v(ci.up)
    unit = lambda a: a / np.linalg.norm(a)
    fd = np.linalg.norm(target - center)
    vw = 2.0 * np.tan(np.radians(ci.fov) / 2.0) * fd
    vh = vw / (w / h)
    W = unit(target - center)
    U = unit(np.cross(W, up))
    V = unit(np.cross(U, W))
    dx, dy = U * vw / w, V * vh / h
    po = center + W * fd - U * vw * 0.5 - V * vh * 0.5 + dx * 0.5 + dy * 0.5
    return center, po, dx, dy


def primary_rays(ci, w, h):
    center, po, dx, dy = camera_frame(ci, w, h)
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    d = po[None, None, :] + px[..., None] * dx + py[..., None] * dy - center
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(center, d.shape)
    return np.concatenate([o, d], -1).reshape(-1, 6).astype(np.float32)


def hemisphere_rays(points, normals, seed):
    g = np.random.default_rng(seed)
    d = g.normal(size=points.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.where((d * normals).sum(1) < 0, -1.0, 1.0)[:, None]
    return np.concatenate([points, d], 1).astype(np.float32)


def setup(config):
    import torch
    from rtamd import Renderer, scenes
    from rtamd.renderer import hits_to_numpy
    cfg = scenes.CONFIGS[config]
    scene = scenes.config_scene(cfg)
    r = Renderer(scene).build_acceleration_structure(0, mode="sah").configure_camera(cfg.width, cfg.height)
    a = primary_rays(r.camera, cfg.width, cfg.height)
    d_a = torch.from_numpy(a).cuda()
    _, hits = r.query_rays(d_a)
    h = hits_to_numpy(hits)
    hit = h["instance"] != 0xFFFFFFFF
    b = hemisphere_rays(h["point"][hit], h["normal"][hit], 7)
    return r, a, b, float(hit.mean())


def timed_call(enqueue, n, launches, warmup):
    """enqueue(): one launch (or torch expression) on torch's current stream, without a host wait."""
    import torch
    st = torch.cuda.Stream()
    # every launch is enqueued before the first wait: the host runs ahead of the device, so an interval holds the
    # head reset, the kernel and the event records, not the host's enqueue of the call
    ev = []
    with torch.cuda.stream(st):
        for i in range(warmup + launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            enqueue()
            e1.record(st)
            ev.append((e0, e1))
    st.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in ev[warmup:]]
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "Mrays_s": round(n / med / 1e3, 1)}


def timed(r, rays, tmax, launches, warmup, **kw):
    return timed_call(lambda: r.query_rays(rays, tmax, sync=False, **kw), len(rays), launches, warmup)


def primary_rays_device(ci, w, h):
    """primary_rays as a torch expression on the device (float32): the producer of the buffer a caller without
    rt_query_camera has to run before rt_query_rays.  The camera frame's nine vectors are host values."""
    import torch
    center, po, dx, dy = camera_frame(ci, w, h)
    dev = lambda a: torch.tensor(a, dtype=torch.float32, device="cuda")
    t_po, t_dx, t_dy, t_c = dev(po - center), dev(dx), dev(dy), dev(center)
    xs = torch.arange(w, dtype=torch.float32, device="cuda")
    ys = torch.arange(h, dtype=torch.float32, device="cuda")

    def produce():
        d = t_po + xs[None, :, None] * t_dx + ys[:, None, None] * t_dy
        d = d * torch.rsqrt((d * d).sum(-1, keepdim=True))
        return torch.cat([t_c.expand(h, w, 3), d], -1).reshape(-1, 6)
    return produce


def measure_camera(args):
    """rt_query_camera (centre rays) against rt_query_rays on the same rays held in a buffer, in one process, the
    variants alternated --repeats times after one pass that warms every shape (profiles/camera_query/README.md)."""
    import torch
    r, a, _, hit_frac = setup(args.config)
    w, h = r.width, r.height
    n = w * h
    tiles = np.arange(n).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1)
    d_rows = torch.from_numpy(a).cuda()
    d_tiles = torch.from_numpy(a[tiles]).cuda()
    produce = primary_rays_device(r.camera, w, h)
    variants = {
        "camera_t": lambda: r.query_camera(sync=False),
        "camera_hits_albedo": lambda: r.query_camera(want_t=False, want_hits=True, want_albedo=True, sync=False),
        "camera_rays_only": lambda: r.query_camera(want_t=False, want_rays=True, sync=False),
        "a_primary": lambda: r.query_rays(d_rows, None, want_hits=False, sync=False),
        "a_primary_8x8_tiles": lambda: r.query_rays(d_tiles, None, want_hits=False, sync=False),
        "a_primary_records": lambda: r.query_rays(d_rows, None, sync=False),
        "producer_torch": produce,
    }
    # the camera query's t against the buffer query's on the script's own rays (float64-built, so not bit-equal rays)
    t_cam = r.query_camera()["t"].reshape(-1)
    t_buf, _ = r.query_rays(d_rows, None, want_hits=False)
    same = float(((t_cam == t_buf) | ((t_cam - t_buf).abs() <= 1e-4 * t_buf.abs())).float().mean())
    out = {"config": args.config, "build": "sah", "width": w, "height": h, "launches": args.launches,
           "warmup": args.warmup, "repeats": args.repeats, "primary_hit_fraction": round(hit_frac, 4),
           "t_agree_fraction": round(same, 6), "lib": os.path.basename(os.environ.get("RTAMD_LIB", "librtamd.so"))}
    for fn in variants.values():                          # warm every shape first
        timed_call(fn, n, 3, 2)
    res = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            res[k].append(timed_call(fn, n, args.launches, args.warmup)["ms_median"])
    for k, v in res.items():
        out[k] = {"ms_medians": v, "ms_median": round(statistics.median(v), 4), "spread": round(max(v) - min(v), 4)}
    r.cleanup()
    return out


def measure(args):
    import torch
    r, a, b, hit_frac = setup(args.config)
    out = {"config": args.config, "build": "sah",
           "launches": args.launches, "warmup": args.warmup, "primary_hit_fraction": round(hit_frac, 4)}
    # (a) again with each chunk of 64 rays an 8x8 pixel tile (the render kernel's unit) instead of 64 pixels of a row
    cfg_w, cfg_h = r.width, r.height
    tiles = np.arange(cfg_w * cfg_h).reshape(cfg_h // 8, 8, cfg_w // 8, 8).transpose(0, 2, 1, 3).reshape(-1)
    sets = {"a_primary": (a, None), "a_primary_8x8_tiles": (a[tiles], None), "b_ambient_occlusion": (b, 2.0)}
    for name, (rays, tm) in sets.items():
        d = torch.from_numpy(rays).cuda()
        t = None if tm is None else torch.full((len(rays),), tm, dtype=torch.float32, device="cuda")
        res = {"rays": len(rays), "tmax": tm}
        res["closest_records"] = timed(r, d, t, args.launches, args.warmup)
        res["closest_t"] = [timed(r, d, t, args.launches, args.warmup, want_hits=False) for _ in range(3)]
        res["any_hit"] = timed(r, d, t, args.launches, args.warmup, any_hit=True)
        occ = r.query_rays(d, t, any_hit=True)
        res["occluded_fraction"] = round(float(occ.float().mean()), 4)
        w = []
        for _ in range(3):
            t0 = time.perf_counter()
            r.trace_rays(rays)
            w.append((time.perf_counter() - t0) * 1e3)
        res["rt_trace_rays_wall_ms"] = round(min(w), 3)
        out[name] = res
    # set (a) made by the library itself: rt_query_camera, centre rays, t only (--camera has the full comparison)
    n = cfg_w * cfg_h
    out["a_camera_query"] = {"rays": n, "closest_t": [timed_call(lambda: r.query_camera(sync=False), n, args.launches,
                                                                 args.warmup) for _ in range(3)]}
    r.cleanup()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="C2")
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--trace-once", action="store_true")
    p.add_argument("--camera", action="store_true")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--out")
    args = p.parse_args()
    if args.trace_once:
        import torch
        r, a, b, _ = setup(args.config)                  # dispatch 1 of ray_query_kernel: set (a), records
        h = r.trace_rays(b)                              # trace_rays_kernel: set (b), range [0.001, inf)
        d = torch.from_numpy(b).cuda()
        r.query_rays(d)                                  # dispatch 2: set (b), records, the same range
        r.query_rays(d, torch.full((len(b),), 2.0, dtype=torch.float32, device="cuda"))   # dispatch 3: tmax = 2.0
        print(json.dumps({"rays": len(b), "hit_fraction": round(float((h["instance"] != 0xFFFFFFFF).mean()), 4)}))
        r.cleanup()
        return
    out = measure_camera(args) if args.camera else measure(args)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
