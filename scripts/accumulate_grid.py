#!/usr/bin/env python3
"""Renderer.accumulate's default thresholds: a small grid over max_history, normal_cos and plane_tolerance on C2's
scene with a moving camera.  --frames one-sample frames (a seed each, scene frame 0 every time, so only the camera
moves) are rendered at --size with their rt_query_camera records while the camera strafes sideways by --step of its
distance to the target per frame, still looking at the target; every grid point then accumulates the same frames, with
prev_view = rt_camera_reprojection of the previous camera.  Scored as the denoiser's sigma grid was: RMSE in gamma
space (sqrt of the colour clamped to [0, 1], the framebuffer's encoding) of the last accumulated frame against the
last camera's frame rendered with sample_count = 1024.  Prints one JSON line per grid point, then the best point and,
there, what each test is worth and what rt_denoise adds; profiles/accumulate/README.md keeps the table,
rtamd.renderer.ACCUMULATE_DEFAULTS the choice."""
import argparse
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "real-time-gpu-ray-tracer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def floats(s):
    return tuple(float(v) for v in s.split(","))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--step", type=float, default=0.002)
    ap.add_argument("--converged", type=int, default=1024)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED)
    ap.add_argument("--max-history", type=floats, default=(8.0, 16.0, 32.0, 64.0, 128.0))
    ap.add_argument("--normal-cos", type=floats, default=(0.5, 0.8, 0.9, 0.95, 0.99))
    ap.add_argument("--plane-tolerance", type=floats, default=(0.002, 0.005, 0.01, 0.02, 0.05, 0.1))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import rtamd
    from rtamd import Renderer, scenes
    assert torch.cuda.is_available(), "needs a GPU"
    W, H = (int(v) for v in a.size.split("x"))
    cfg = scenes.CONFIGS["C2"]
    scene = scenes.config_scene(cfg)
    r = Renderer(scene).build_acceleration_structure(0, mode="sah")
    stream = torch.cuda.current_stream()
    centre = [float(v) for v in scene.camera["center"]]
    target = [float(v) for v in scene.camera["target"]]
    reach = sum((t - c) ** 2 for c, t in zip(centre, target)) ** 0.5

    def camera(k):
        return dict(center=(centre[0] + a.step * reach * (k - a.frames + 1), centre[1], centre[2]))   # the last one: the scene's

    frames = []
    for k in range(a.frames):
        r.configure_camera(W, H, ray_trace_depth=cfg.depth, sample_count=1, **camera(k))
        noisy = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.render(0, frame_seed=a.seed + k, want_rgba=False, rgb32_device=noisy.data_ptr(), stream=stream.cuda_stream,
                 skip_update=k > 0)
        q = r.query_camera(first_sample=True, frame_seed=a.seed + k, want_t=False, want_hits=True, want_albedo=k == a.frames - 1)
        view = rtamd.reprojection(frames[-1]["camera"], W, H) if frames else None
        frames.append({"rgb": noisy, "hits": q["hits"], "albedo": q.get("albedo"), "camera": r.camera, "view": view})
    converged = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.configure_camera(W, H, ray_trace_depth=cfg.depth, sample_count=a.converged, **camera(a.frames - 1))
    r.render(0, frame_seed=a.seed + a.frames, want_rgba=False, rgb32_device=converged.data_ptr(), stream=stream.cuda_stream,
             skip_update=True)

    def score(img):
        g = torch.sqrt(torch.clamp(img, 0.0, 1.0)) - torch.sqrt(torch.clamp(converged, 0.0, 1.0))
        return float(torch.sqrt(torch.mean(g.double() ** 2)))

    def run(**kw):
        prev = None
        for f in frames:
            prev = r.accumulate(f["rgb"], f["hits"], prev, prev_view=f["view"], **kw)
        return prev

    last = frames[-1]
    lines = [{"what": "noisy", "size": a.size, "frames": a.frames, "step": a.step, "converged_spp": a.converged,
              "rmse_gamma": round(score(last["rgb"]), 5)}]
    print(json.dumps(lines[0]), flush=True)
    best = None
    for mh, nc, pt in itertools.product(a.max_history, a.normal_cos, a.plane_tolerance):
        out = run(max_history=mh, normal_cos=nc, plane_tolerance=pt)
        hit_len = out["history"][..., 3]
        ln = {"what": "grid", "max_history": mh, "normal_cos": nc, "plane_tolerance": pt,
              "rmse_gamma": round(score(out["rgb"]), 5), "mean_length": round(float(hit_len.mean()), 2)}
        lines.append(ln)
        print(json.dumps(ln), flush=True)
        if best is None or ln["rmse_gamma"] < best["rmse_gamma"]:
            best = ln
    inf = float("inf")
    at_best = dict(max_history=best["max_history"], normal_cos=best["normal_cos"], plane_tolerance=best["plane_tolerance"])
    for name, kw in (("no_normal", dict(normal_cos=-inf)), ("no_plane", dict(plane_tolerance=inf)),
                     ("unbounded_history", dict(max_history=inf))):
        args = dict(at_best)
        args.update(kw)
        ln = {"what": name, "rmse_gamma": round(score(run(**args)["rgb"]), 5)}
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    acc = run(**at_best)
    # rt_denoise after it: with Renderer.denoise's colour sigma (the one-sample frame's noise level), and with that
    # sigma scaled by 1 / sqrt(max_history), the noise level of a mean of that many samples
    from rtamd.renderer import DENOISE_SIGMAS
    scaled = DENOISE_SIGMAS[0] / best["max_history"] ** 0.5
    for name, img, sigma in (("denoised_noisy", last["rgb"], DENOISE_SIGMAS[0]), ("denoised_accumulated", acc["rgb"], DENOISE_SIGMAS[0]),
                             ("denoised_accumulated_scaled_sigma", acc["rgb"], scaled)):
        out = r.denoise(img, last["hits"], last["albedo"], sigma_color=sigma)
        ln = {"what": name, "sigma_color": round(sigma, 4), "rmse_gamma": round(score(out["rgb"]), 5)}
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    edges = [k for k, grid in (("max_history", a.max_history), ("normal_cos", a.normal_cos), ("plane_tolerance", a.plane_tolerance))
             if best[k] in (min(grid), max(grid))]
    lines.append(dict(best, what="best", on_the_edge_of=edges))
    print(json.dumps(lines[-1]), flush=True)
    r.cleanup()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
