"""Edge cases of the trace path through the C ABI: ragged frame sizes (partial 8x8 units and 64x64
tiles, single rows / columns, one pixel), scenes of a single primitive (one-leaf BLAS, one-record
TLAS, mostly sky), and tiny frames on overlapped lanes across a heaviest-first reorder.

The oracle (tests only) traverses the reference-order compat trees; EXACT frames on those trees are
bit-identical in float RGB.  Single-primitive scenes have no hit ties, so every
builder (compat / SAH / GPU LBVH) must give the oracle's bits there too.
"""
import os

import numpy as np
import pytest

from rtamd import Renderer, abi, scenes

pytestmark = pytest.mark.gpu

THREADS = 16


def _oracle(scene, w, h, seed=0, **cam):
    from oracle.oracle import OracleScene
    o = OracleScene(scene, build_seed=seed)
    o.camera(w, h, **cam)
    return o


def _single(kind):
    """One instance of one primitive above no ground (Main.cu's materials): the BLAS is one leaf."""
    s = scenes.demo_scene()
    s.animated = False
    if kind == "sphere":
        s.instances = [dict(type=abi.SPHERE, index=1, shift=(0.5, 0.2, 0.0))]
    elif kind == "parallelogram":
        s.instances = [dict(type=abi.PARALLELOGRAM, index=0, rotate=(0.0, 35.0, 0.0))]
    else:
        s.instances = [dict(type=abi.TRIANGLE, index=0, scale=(2.0, 2.0, 2.0))]
    return s


@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (65, 33), (130, 1), (1, 97), (9, 200)])
def test_ragged_frame_sizes_exact(gpu_lib, w, h):
    """Frames whose sides are not multiples of the 8x8 scheduling unit: every pixel written once,
    float RGB bit-identical to the oracle, same ray count; a repeated render (after the reorder pass
    has costed the frame) gives the same bytes."""
    s = scenes.demo_with_particles(4)
    r = Renderer(s).build_acceleration_structure(0).configure_camera(w, h, ray_trace_depth=3)
    o = _oracle(s, w, h, 0, ray_trace_depth=3)
    orgb, orgba, ocnt = o.render(threads=THREADS)
    first = None
    for rep in range(10):                       # reorder_period 8: launches 0 and 8 rebuild the order
        rgba, rgb, st = r.render(0, exact=True, want_rgb=True, count_work=True)
        assert st["pixels"] == w * h
        assert (rgb != orgb).any(axis=2).sum() == 0, rep
        assert st["rays"] == ocnt["rays"]
        if first is None:
            first = rgba
        assert np.array_equal(rgba, first), rep
    d = np.abs(first.astype(np.int32) - orgba.astype(np.int32)).max()
    assert d <= 1


@pytest.mark.parametrize("w,h", [(7, 5), (65, 33)])
def test_ragged_frame_sizes_fast_kernels_agree(gpu_lib, w, h):
    """FAST mode on ragged frames: the persistent kernel (quads, binary pairs) and the grid kernel give the same
    bytes on the reference's trees (every box decision the reference's), equal to the oracle's float frame."""
    s = scenes.demo_with_particles(4)
    r = Renderer(s).build_acceleration_structure(0).configure_camera(w, h, ray_trace_depth=2, sample_count=4)
    o = _oracle(s, w, h, 0, ray_trace_depth=2, sample_count=4)
    orgb, orgba, _ = o.render(threads=THREADS)
    for kernel, wide in ((1, 1), (1, 0), (0, 1)):
        r.set_option("kernel", kernel).set_option("wide", wide)
        rgba, rgb, st = r.render(0, want_rgb=True)
        assert np.array_equal(rgb, orgb), (kernel, wide)
        d = np.abs(rgba.astype(np.int32) - orgba.astype(np.int32)).max(axis=-1)
        assert (d <= 1).all(), (kernel, wide)


@pytest.mark.parametrize("kind", ["sphere", "parallelogram", "triangle"])
@pytest.mark.parametrize("mode", ["compat", "sah", "lbvh"])
def test_single_primitive_scene(gpu_lib, kind, mode):
    """One instance of one primitive: a one-leaf BLAS under a one-record TLAS (host-built or GPU
    LBVH).  EXACT float RGB equals the oracle bit for bit and the work counters match (no ties, so
    the builder cannot change which surface is hit)."""
    s = _single(kind)
    W, H = 96, 64
    r = Renderer(s, update=False).build_acceleration_structure(0, mode=mode).configure_camera(W, H, ray_trace_depth=4)
    o = _oracle(s, W, H, 0, ray_trace_depth=4)
    orgb, orgba, ocnt = o.render(threads=THREADS)
    rgba, rgb, st = r.render(0, exact=True, want_rgb=True, count_work=True)
    assert (rgb != orgb).any(axis=2).sum() == 0
    assert st["rays"] == ocnt["rays"]
    if mode == "compat":
        assert st["instance_visits"] == ocnt["instance_visits"]
        assert st["triangle_tests"] == ocnt["triangle_tests"]
        assert st["sphere_quad_tests"] == ocnt["sphere_quad_tests"]
    # the primitive is hit and the rest is sky: both kinds of pixel are present
    assert 0 < st["hits"] < st["rays"]
    rgba_f, rgb_f, _ = r.render(0, want_rgb=True)
    if mode == "compat":                             # FAST on the reference's trees: bit-identical
        assert (rgb_f != orgb).any(axis=2).sum() == 0
    d = np.abs(rgba_f.astype(np.int32) - orgba.astype(np.int32)).max(axis=-1)
    assert (d <= 1).mean() >= (1.0 if mode == "compat" else 0.999)


@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (17, 9)])
def test_tiny_frames_on_overlapped_lanes(gpu_lib, w, h):
    """Frames smaller than one scheduling unit on three overlapped lanes, over more launches than
    the reorder period: every frame's bytes equal its synchronous render."""
    import torch
    s = scenes.demo_with_particles(6)
    F = 12
    r = Renderer(s).build_acceleration_structure(0, mode="sah").configure_camera(w, h, ray_trace_depth=2)
    ref = [r.render(f)[0] for f in range(F)]
    r.collect()
    r.set_option("overlap", 3)
    lanes = [torch.cuda.Stream() for _ in range(3)]
    bufs = [torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda") for _ in range(F)]
    torch.cuda.synchronize()
    for f in range(F):
        r.render(f, want_rgba=False, rgba8_device=bufs[f].data_ptr(), stream=lanes[f % 3].cuda_stream, sync=False)
    _, kms = r.collect()
    torch.cuda.synchronize()
    for f in range(F):
        assert np.array_equal(bufs[f].cpu().numpy(), ref[f].reshape(-1)), f
    assert len(kms) == F
    r.set_option("overlap", 0)


@pytest.mark.parametrize("lanes", [0, 3])
def test_null_stream_device_outputs_ordered(gpu_lib, lanes):
    """rt_render with device outputs and no stream (opts.stream NULL) runs on a non-blocking stream of the scene; it
    is ordered after the caller's null-stream work enqueued before the call and, without "overlap", before the null
    stream's work after it (render.cpp order_null), as a drop-in caller of the reference's render-into-my-surface
    loop (Renderer.cu:305-317) expects.  Each iteration queues a long fill on torch's default (null) stream, a fill
    of the output with junk, the frame with RT_RENDER_NO_SYNC and no stream, and a copy of the output — no host
    synchronisation anywhere — and every copy equals the synchronously rendered frame byte for byte.  With
    "overlap" the frames run side by side on the scene's own lanes and are read after rt_synchronize."""
    import torch
    s = scenes.demo_with_particles(10)
    W, H = 320, 184
    r = Renderer(s).build_acceleration_structure(0, mode="sah").configure_camera(W, H, ray_trace_depth=2)
    ref = [r.render(f)[0] for f in range(4)]
    if lanes:
        r.set_option("overlap", lanes)
    big = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    out = torch.empty(W * H * 4, dtype=torch.uint8, device="cuda")
    copies = []
    for it in range(24):
        big.fill_(float(it))                         # keeps the null stream busy for a while
        if lanes:
            # frames on the scene's own lane streams run side by side: each waits for the caller's null-stream work
            # before the call (the junk fill), and its output is complete once rt_synchronize returns
            o = torch.empty(W * H * 4, dtype=torch.uint8, device="cuda")
            o.fill_(0x5A)
            r.render(it % 4, want_rgba=False, rgba8_device=o.data_ptr(), sync=False)
            copies.append(o)
        else:
            out.fill_(0x5A)
            r.render(it % 4, want_rgba=False, rgba8_device=out.data_ptr(), sync=False)
            copies.append(out.clone())
    if lanes:
        r.synchronize()
    for it, c in enumerate(copies):
        assert np.array_equal(c.cpu().numpy().reshape(H, W, 4), ref[it % 4]), it
    r.cleanup()


@pytest.mark.parametrize("build", ["sah", "lbvh"])
def test_lane_priority_change_after_library_lane_frames(gpu_lib, build):
    """Option "lane_priority" destroys the scene's lane streams (recreated at the next frame).  After frames on those
    lanes (overlap, opts.stream NULL, NO_SYNC), nothing may keep a handle to them: rt_synchronize (drain() waits on the
    last frame's stream) and the next frames (GPU-built frames compare the frame block's chain stream) must work and
    render the same frames (a stale last_stream made that drain wait on a destroyed stream)."""
    import torch
    s = scenes.demo_with_particles(10)
    W, H = 160, 96
    r = Renderer(s).build_acceleration_structure(0, mode=build).configure_camera(W, H, ray_trace_depth=2)
    ref = [r.render(f)[0] for f in range(6)]
    r.set_option("overlap", 3)
    for value in (0, 1, 0):
        outs = []
        for f in range(6):
            o = torch.empty(W * H * 4, dtype=torch.uint8, device="cuda")
            r.render(f, want_rgba=False, rgba8_device=o.data_ptr(), sync=False)
            outs.append(o)
        r.set_option("lane_priority", value)       # drains, then destroys the lane streams the frames ran on
        r.synchronize()
        for f, o in enumerate(outs):
            assert np.array_equal(o.cpu().numpy().reshape(H, W, 4), ref[f]), (value, f)
    assert np.array_equal(r.render(3)[0], ref[3])
    r.cleanup()


def test_synchronous_frame_after_pipelined_frames(gpu_lib):
    """A synchronous call behind NO_SYNC frames still in flight on the scene's own lanes (auto overlap): every frame
    equals its single-launch render, three bursts in a row."""
    import torch
    s = scenes.demo_with_particles(10)
    W, H = 320, 184
    r = Renderer(s).build_acceleration_structure(0, mode="sah").configure_camera(W, H, ray_trace_depth=2)
    ref = [r.render(f)[0] for f in range(6)]
    r.set_option("overlap", -1)
    outs = [torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda") for _ in range(6)]
    for it in range(3):
        for f in range(6):
            r.render(f, want_rgba=False, rgba8_device=outs[f].data_ptr(), sync=(f == 5))
        r.synchronize()
        for f in range(6):
            assert np.array_equal(outs[f].cpu().numpy().reshape(H, W, 4), ref[f]), (it, f)
    r.cleanup()


DOCUMENTED_OPTIONS = {"overlap": -1, "stage_depth": 8, "lane_priority": 1, "grid_pct": 0, "rebuild": 0, "cold_records": -1,
                      "blas_double": 1, "blas_sets": 3, "tlas_small": 1, "exact_decisions": 0, "group": 1, "gpu_tlas": 0,
                      "tlas_sah": 1, "kernel": 1, "wide": 1, "fast_math": 0, "reorder": 1, "timeline": 0, "costmap": 0}
REMOVED_OPTIONS = ("threshold", "leaf_early", "queue_parts", "grab", "supertile", "merge", "split", "reorder_period",
                   "reserve", "lds_scene", "lds_blas", "inst_by_slot", "blas_leaf", "tlas_leaf", "tlas_median_leaf",
                   "variant", "nt_store", "cost_max", "tlas_classes", "wide_merge", "scene_priority")


def test_option_surface_is_the_documented_one(gpu_lib):
    """rt_scene_set_option accepts exactly the 19 keys include/rt.h documents (verdict r5 item 7: the A/B-only and
    measured-negative switches are gone) and rejects the removed ones and bad values with RT_ERR_INVALID_ARGUMENT."""
    import re
    from rtamd import abi
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt.h")).read()
    block = hdr[hdr.index("/* Scene options"):hdr.index("rt_status rt_scene_set_option(")]
    documented = set(re.findall(r'^ \*   "(\w+)"', block, re.M))
    assert documented == set(DOCUMENTED_OPTIONS), documented ^ set(DOCUMENTED_OPTIONS)
    assert len(documented) <= 20
    r = Renderer(scenes.demo_scene())
    for k, v in DOCUMENTED_OPTIONS.items():
        r.set_option(k, v)
    for k in REMOVED_OPTIONS:
        with pytest.raises(abi.RtError, match="RT_ERR_INVALID_ARGUMENT"):
            r.set_option(k, 0)
    for k in ("tlas_sah", "exact_decisions", "lane_priority", "reorder"):
        with pytest.raises(abi.RtError, match="RT_ERR_INVALID_ARGUMENT"):
            r.set_option(k, 2)
    r.cleanup()
