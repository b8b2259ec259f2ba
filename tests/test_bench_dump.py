"""bench.py --dump-outputs: the frame the last timed step rendered, written so two builds can be compared.

CPU: the writer itself (whole frame, and the seeded pixel sample of a frame above the size cap).
GPU: a plain run of the smallest config (C1, 256x256) in this process — the result line's headline fields, --steps as
the number of timed frames, two runs writing identical files, and the dumped frame equal to a synchronous rt_render
of the same frame of the same scene.
"""
import json
import os
import sys

import numpy as np
import pytest

STEPS, WARMUP = 5, 2
ARGS = ["--gpus", "1", "--config", "C1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--clock-warmup", "0"]


def test_dump_writer_whole_frame_and_seeded_sample(tmp_path, monkeypatch):
    import torch
    import bench
    w, h = 64, 48
    frame = torch.arange(w * h * 4, dtype=torch.int64).remainder(251).to(torch.uint8)
    want = frame.numpy().reshape(h * w, 4).astype(np.float32)

    bench.dump_outputs(str(tmp_path / "whole"), frame, w, h)
    assert sorted(os.listdir(tmp_path / "whole")) == ["frame_rgba8.npy"]
    a = np.load(tmp_path / "whole" / "frame_rgba8.npy")
    assert a.dtype == np.float32 and np.array_equal(a, want)

    monkeypatch.setattr(bench, "DUMP_MAX_PIXELS", 1000)
    for name in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / name), frame, w, h)
    idx = np.load(tmp_path / "s1" / "frame_pixel_index.npy")
    px = np.load(tmp_path / "s1" / "frame_rgba8.npy")
    assert idx.dtype == np.float64 and idx.shape == (1000,) and px.dtype == np.float32 and px.shape == (1000, 4)
    i = idx.astype(np.int64)
    assert np.all(np.diff(i) > 0) and i[0] >= 0 and i[-1] < w * h          # distinct pixels of the frame, in order
    assert np.array_equal(px, want[i])
    for f in ("frame_pixel_index.npy", "frame_rgba8.npy"):                 # the same sample every run
        assert np.array_equal(np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f))


def run_bench(monkeypatch, capsys, extra):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + ARGS + extra)
    capsys.readouterr()
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_frame(gpu_lib, tmp_path, monkeypatch, capsys):
    from rtamd import Renderer, scenes
    d = [run_bench(monkeypatch, capsys, ["--dump-outputs", str(tmp_path / n)]) for n in ("a", "b")]
    for line in d:
        assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["full"] is False
        assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["ms_per_step"] > 0 and line["value"] > 0
        # value and ms_per_step are the same timed region: rays of the STEPS timed frames over their elapsed time
        assert line["value"] == pytest.approx(line["rays_per_frame"] / (line["ms_per_step"] * 1e-3) / 1e6, rel=0.01)
        assert "roofline" not in line and "cpu_baseline" not in line and "frame_latency_ms_median" not in line
    assert d[0]["rays_per_frame"] == d[1]["rays_per_frame"]
    a, b = (np.load(tmp_path / n / "frame_rgba8.npy") for n in ("a", "b"))
    assert a.dtype == np.float32 and a.shape == (256 * 256, 4) and np.array_equal(a, b)

    cfg = scenes.CONFIGS["C1"]
    r = Renderer(scenes.config_scene(cfg)).build_acceleration_structure(0, mode="sah").configure_camera(cfg.width, cfg.height)
    r.set_option("kernel", 1)
    rgba, _, st = r.render(WARMUP + STEPS - 1)             # the last timed frame, one synchronous launch
    r.cleanup()
    assert np.array_equal(a.reshape(cfg.height, cfg.width, 4), rgba.astype(np.float32))
    # a picture, not the cleared buffer bench.py starts from (zeros): every pixel written (alpha 255), not one colour
    assert (a[:, 3] == 255).all() and len(np.unique(a, axis=0)) > 1
