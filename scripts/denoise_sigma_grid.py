#!/usr/bin/env python3
"""Renderer.denoise's default sigmas: a small grid on C2's scene at 1080p, 1 sample per pixel, scored by the RMSE in
gamma space (sqrt of the colour clamped to [0, 1], the framebuffer's encoding) against the same frame rendered with
sample_count = 1024.  Prints one JSON line per grid point, then the best point; profiles/denoise/README.md keeps the
table, rtamd.renderer.DENOISE_SIGMAS the choice."""
import argparse
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "real-time-gpu-ray-tracer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIGMA_COLOR = (0.5, 1.0, 1.5, 2.0, 3.0, 4.0)
SIGMA_NORMAL = (0.025, 0.05, 0.1, 0.25, 0.5)
SIGMA_PLANE = (0.02, 0.1, 0.5, 2.0)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--converged", type=int, default=1024)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from rtamd import Renderer, scenes
    assert torch.cuda.is_available(), "needs a GPU"
    W, H = (int(v) for v in a.size.split("x"))
    cfg = scenes.CONFIGS["C2"]
    r = Renderer(scenes.config_scene(cfg)).build_acceleration_structure(0, mode="sah")
    stream = torch.cuda.current_stream()
    noisy = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    converged = torch.zeros_like(noisy)
    torch.cuda.synchronize()
    r.configure_camera(W, H, ray_trace_depth=cfg.depth, sample_count=a.converged)
    r.render(0, frame_seed=a.seed + 1, want_rgba=False, rgb32_device=converged.data_ptr(), stream=stream.cuda_stream)
    r.configure_camera(W, H, ray_trace_depth=cfg.depth, sample_count=1)
    r.render(0, frame_seed=a.seed, want_rgba=False, rgb32_device=noisy.data_ptr(), stream=stream.cuda_stream, skip_update=True)
    q = r.query_camera(first_sample=True, frame_seed=a.seed, want_t=False, want_hits=True, want_albedo=True)

    def score(img):
        g = torch.sqrt(torch.clamp(img, 0.0, 1.0)) - torch.sqrt(torch.clamp(converged, 0.0, 1.0))
        return float(torch.sqrt(torch.mean(g.double() ** 2)))

    lines = [{"what": "noisy", "size": a.size, "converged_spp": a.converged, "rmse_gamma": round(score(noisy), 5)}]
    print(json.dumps(lines[0]), flush=True)
    best = None
    for sc, sn, sp in itertools.product(SIGMA_COLOR, SIGMA_NORMAL, SIGMA_PLANE):
        for alb in (True, False) if (sc, sn, sp) == (SIGMA_COLOR[0], SIGMA_NORMAL[0], SIGMA_PLANE[0]) else (True,):
            out = r.denoise(noisy, q["hits"], q["albedo"] if alb else None, sigma_color=sc, sigma_normal=sn, sigma_plane=sp)
            ln = {"what": "grid", "sigma_color": sc, "sigma_normal": sn, "sigma_plane": sp, "albedo": alb,
                  "rmse_gamma": round(score(out["rgb"]), 5)}
            lines.append(ln)
            print(json.dumps(ln), flush=True)
            if alb and (best is None or ln["rmse_gamma"] < best["rmse_gamma"]):
                best = ln
    # the guides alone: how much each one is worth at the best point
    inf = float("inf")
    for name, kw in (("no_normal", dict(sigma_normal=inf)), ("no_plane", dict(sigma_plane=inf)),
                     ("no_color", dict(sigma_color=inf)), ("no_albedo", dict())):
        args = dict(sigma_color=best["sigma_color"], sigma_normal=best["sigma_normal"], sigma_plane=best["sigma_plane"])
        args.update(kw)
        out = r.denoise(noisy, q["hits"], None if name == "no_albedo" else q["albedo"], **args)
        ln = {"what": name, "rmse_gamma": round(score(out["rgb"]), 5)}
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    lines.append(dict(best, what="best"))
    print(json.dumps(lines[-1]), flush=True)
    r.cleanup()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
