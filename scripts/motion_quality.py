#!/usr/bin/env python3
"""What rt_accumulate_motion gains on a scene whose instances move (profiles/motion/README.md).

C2's scene at --size with its demo animation running (rt_demo_update: scene frame k for frame k), --frames one-sample
frames with a seed each, from a still camera and from scripts/guided_grid.py's strafing one (sideways by --step of the
distance to the target per frame, the last frame from the scene's own camera).  Every frame is rendered and queried
once and accumulated twice on the same inputs: by rt_accumulate_moments (the still camera with prev_view NULL, as its
callers do) and by rt_accumulate_motion with the records of rt_instance_motion_records from the previous and the
current frame's transforms and the previous camera's rows; the last accumulated frame of each goes through
rt_denoise_guided with the defaults.

Reported per camera and chain: RMSE in gamma space (sqrt of the colour clamped to [0, 1]) against the last frame —
scene frame, camera — with sample_count = --converged, over the whole frame and over the pixels of the instances whose
transform changed between the last two frames; and the mean history length on those pixels.

One JSON line per measurement on stdout; --out also writes them to a file.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "real-time-gpu-ray-tracer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def demo_xforms(lib, scene, frame):
    """The scene's rt_xform array after rt_demo_update for `frame`, as floats [n, 9]."""
    from rtamd import abi
    rows = np.asarray([tuple(d.get("shift", (0, 0, 0))) + tuple(d.get("rotate", (0, 0, 0))) + tuple(d.get("scale", (1, 1, 1)))
                       for d in scene.instances], np.float32)
    lib.rt_demo_update(None, C.cast(rows.ctypes.data, C.POINTER(abi.Xform)), len(rows), frame)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--step", type=float, default=0.002)
    ap.add_argument("--converged", type=int, default=1024)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import rtamd
    from rtamd import Renderer, abi, scenes
    assert torch.cuda.is_available(), "needs a GPU"
    W, H = (int(v) for v in a.size.split("x"))
    cfg = scenes.CONFIGS["C2"]
    scene = scenes.config_scene(cfg)
    assert scene.animated
    lib = abi.load_library()
    r = Renderer(scene).build_acceleration_structure(0, mode="sah")
    stream = torch.cuda.current_stream()
    centre = [float(v) for v in scene.camera["center"]]
    target = [float(v) for v in scene.camera["target"]]
    reach = sum((t - c) ** 2 for c, t in zip(centre, target)) ** 0.5
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def gamma(img):
        return torch.sqrt(torch.clamp(img, 0.0, 1.0))

    last = a.frames - 1
    moved = np.flatnonzero((demo_xforms(lib, scene, last - 1) != demo_xforms(lib, scene, last)).any(axis=1))
    emit(what="scene", config="C2", size=a.size, frames=a.frames, instances=len(scene.instances),
         instances_moving_in_the_last_frame=[int(i) for i in moved])
    for path, step in (("still", 0.0), ("strafe", a.step)):
        def camera(k):
            return dict(center=(centre[0] + step * reach * (k - last), centre[1], centre[2]))   # the last one: the scene's

        acc = {"accumulate_moments": None, "accumulate_motion": None}
        prev_camera = None
        for k in range(a.frames):
            r.configure_camera(W, H, ray_trace_depth=cfg.depth, sample_count=1, **camera(k))
            noisy = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            r.render(k, frame_seed=a.seed + k, want_rgba=False, rgb32_device=noisy.data_ptr(), stream=stream.cuda_stream, sync=False)
            q = r.query_camera(first_sample=True, frame_seed=a.seed + k, want_t=False, want_hits=True, want_albedo=True,
                               stream=stream, sync=False)
            rows = rtamd.reprojection(prev_camera, W, H) if prev_camera is not None else None
            records = rtamd.instance_motion(demo_xforms(lib, scene, k - 1), demo_xforms(lib, scene, k)) if k else None
            acc["accumulate_moments"] = r.accumulate(noisy, q["hits"], acc["accumulate_moments"], prev_view=rows if step else None,
                                                     albedo=q["albedo"], moments=True, stream=stream, sync=False)
            acc["accumulate_motion"] = r.accumulate(noisy, q["hits"], acc["accumulate_motion"], prev_view=rows, motion=records,
                                                    albedo=q["albedo"], moments=True, stream=stream, sync=False)
            prev_camera = r.camera
        filtered = {c: r.denoise_guided(p, q["albedo"])["rgb"] for c, p in acc.items()}
        converged = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        r.configure_camera(W, H, ray_trace_depth=cfg.depth, sample_count=a.converged, **camera(last))
        r.render(last, frame_seed=a.seed + a.frames, want_rgba=False, rgb32_device=converged.data_ptr(), stream=stream.cuda_stream)
        torch.cuda.synchronize()
        inst = q["hits"].view(torch.int32)[..., 1]                                  # rt_hit.instance
        on_moved = torch.isin(inst, torch.as_tensor(moved, dtype=torch.int32, device="cuda"))
        want = gamma(converged)

        def rmse(img, mask=None):
            e = ((gamma(img) - want).double() ** 2).mean(dim=-1)
            return float(torch.sqrt((e if mask is None else e[mask]).mean()))

        emit(what="noisy", camera=path, rmse_gamma=round(rmse(noisy), 5), rmse_gamma_moving_instances=round(rmse(noisy, on_moved), 5),
             pixels_on_moving_instances=int(on_moved.sum()), share_of_frame=round(float(on_moved.float().mean()), 4))
        for c in acc:
            length = acc[c]["history"][..., 3]
            emit(what="chain", camera=path, chain=c + " + denoise_guided", rmse_gamma=round(rmse(filtered[c]), 5),
                 rmse_gamma_moving_instances=round(rmse(filtered[c], on_moved), 5),
                 rmse_gamma_accumulated_only=round(rmse(acc[c]["rgb"]), 5),
                 rmse_gamma_accumulated_only_moving_instances=round(rmse(acc[c]["rgb"], on_moved), 5),
                 mean_history_moving_instances=round(float(length[on_moved].mean()), 3),
                 mean_history_all_hits=round(float(length[inst != -1].mean()), 3))
    r.cleanup()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
