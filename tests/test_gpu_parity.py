"""HIP path (librtamd.so via the C ABI) vs the oracle on the same seeded inputs.

Tolerances:
  * EXACT mode (IEEE division, no FMA contraction) on identical trees: float RGB bit-identical,
    RGBA8 within 1 LSB (the GPU applies gamma with sqrtf, the reference with powf(x, 0.5)),
    identical work counters (rays, instance visits, primitive tests).
  * FAST mode (default: quad traversal with reciprocal slab culls whose marginal decisions are re-taken with the
    reference's slab, the reference's arithmetic for every value that reaches a hit or a pixel): on identical trees
    bit-identical like EXACT (full frames: tests/test_gpu_parity_full.py; the crops, the C3-settings frame and the
    20k closest hits below); on other trees (SAH / LBVH: ties in the 1e-6 window) RGBA8 |d| <= 1 on
    >= 99.9 % of pixels at depth 1-2 and >= 99.5 % at depth >= 4 on these small scenes; per-ray closest hit
    identical on >= 99.9 % of rays with |dt| <= 1e-4 * t.  Option "fast_math" (hardware reciprocals, FMA) is
    held to the same small-scene tolerance.
"""
import numpy as np
import pytest

from rtamd import Renderer, scenes

pytestmark = pytest.mark.gpu

THREADS = 16


def pair(scene, seed, w, h, **cam):
    from oracle.oracle import OracleScene
    r = Renderer(scene).build_acceleration_structure(seed).configure_camera(w, h, **cam)
    o = OracleScene(scene, build_seed=seed)
    o.camera(w, h, **cam)
    return r, o


def frac_within(a, b, lsb=1):
    d = np.abs(a.astype(np.int32) - b.astype(np.int32)).max(axis=-1)
    return float((d <= lsb).mean()), int(d.max())


def test_trees_identical_to_oracle(gpu_lib):
    s = scenes.demo_with_particles(6)
    r, o = pair(s, 11, 64, 64)
    assert r.info()["blas_count"] == o.blas_count() == 5 + 6 - 1   # sphere 1 shared by 2 instances
    for b in range(o.blas_count()):
        for x, y in zip(r.export_blas(b), o.export_blas(b)):
            assert np.array_equal(x, y), f"BLAS {b}"
    for frame in (0, 37):
        r.update(frame)
        o.update(frame)
        for x, y in zip(r.export_tlas(), o.export_tlas()):
            assert np.array_equal(x, y), f"TLAS frame {frame}"


@pytest.mark.parametrize("depth", [1, 2, 10])
def test_exact_mode_bit_identical_demo(gpu_lib, depth):
    r, o = pair(scenes.demo_scene(), 3, 240, 160, ray_trace_depth=depth)
    rgba, rgb, st = r.render(0, exact=True, want_rgb=True, count_work=True)
    orgb, orgba, ocnt = o.render(threads=THREADS)
    mism = (rgb != orgb).any(axis=2)
    assert mism.sum() == 0, f"{mism.sum()} pixels differ, max |d| {np.abs(rgb - orgb).max()}"
    f, _ = frac_within(rgba, orgba)
    assert f == 1.0
    assert st["rays"] == ocnt["rays"]
    assert st["instance_visits"] == ocnt["instance_visits"]
    assert st["triangle_tests"] == ocnt["triangle_tests"]
    assert st["sphere_quad_tests"] == ocnt["sphere_quad_tests"]


@pytest.mark.parametrize("kernel", [1, 0])
def test_c1_exact_256_depth10(gpu_lib, kernel):
    """BASELINE.json configs[0] (C1) at its own workload: the demo scene, 256x256, 1 spp, depth 10.  EXACT on the
    reference's trees is bit-identical to the oracle's BVH frame (persistent and grid kernels) with equal work
    counters, and within SURVEY 8(c)'s depth-10 bar (<= 0.05 % of pixels beyond 1 LSB) of the oracle's
    brute-force loops (tests/test_oracle_kat.py::test_c1_bvh_equals_brute_force_256 pins BVH vs loops)."""
    r, o = pair(scenes.demo_scene(), 0, 256, 256, ray_trace_depth=10)
    r.set_option("kernel", kernel)
    rgba, rgb, st = r.render(0, exact=True, want_rgb=True, count_work=True)
    orgb, orgba, ocnt = o.render(threads=THREADS)
    assert (rgb != orgb).any(axis=2).sum() == 0, float(np.abs(rgb - orgb).max())
    assert frac_within(rgba, orgba)[0] == 1.0
    for k in ("rays", "instance_visits", "triangle_tests", "sphere_quad_tests"):
        assert st[k] == ocnt[k], k
    _, brgba, _ = o.render(threads=THREADS, brute_force=2)
    bad = int((np.abs(rgba.astype(np.int32) - brgba.astype(np.int32)).max(axis=2) > 1).sum())
    assert bad <= 0.0005 * 256 * 256, bad
    fast, _, _ = r.render(0)
    assert int((np.abs(fast.astype(np.int32) - orgba.astype(np.int32)).max(axis=2) > 1).sum()) <= 0.0005 * 256 * 256


def test_exact_mode_particles_and_animation(gpu_lib):
    s = scenes.demo_with_particles(12)
    r, o = pair(s, 5, 200, 120, ray_trace_depth=2)
    for frame in (0, 37):
        o.update(frame)
        rgba, rgb, st = r.render(frame, exact=True, want_rgb=True, count_work=True)
        orgb, orgba, ocnt = o.render(threads=THREADS)
        assert (rgb != orgb).any(axis=2).sum() == 0
        assert st["rays"] == ocnt["rays"] and st["triangle_tests"] == ocnt["triangle_tests"]


@pytest.mark.parametrize("depth,need", [(1, 0.999), (2, 0.999), (10, 0.995)])
def test_fast_mode_within_tolerance_demo(gpu_lib, depth, need):
    """The default FAST kernel on the reference's trees is bit-identical to the oracle (its arithmetic is the
    reference's wherever a value reaches a hit or a pixel); option "fast_math" is held to its tolerance."""
    r, o = pair(scenes.demo_scene(), 3, 240, 160, ray_trace_depth=depth)
    rgba, rgb, _ = r.render(0, want_rgb=True)
    orgb, orgba, _ = o.render(threads=THREADS)
    assert (rgb != orgb).any(axis=2).sum() == 0, float(np.abs(rgb - orgb).max())
    assert frac_within(rgba, orgba)[0] == 1.0
    r.set_option("fast_math", 1)
    rgba, rgb, _ = r.render(0, want_rgb=True)
    f, mx = frac_within(rgba, orgba)
    assert f >= need, (f, mx)
    assert np.abs(rgb - orgb).mean() < 2e-3


def test_fast_mode_c2_crop(gpu_lib):
    """C2 (1080p, 1 spp, depth 2, 68 particles) on the reference's trees: the FAST frame's float RGB equals the
    oracle's on the particle crop and a ground/sky crop (round 5: marginal box decisions re-taken exactly)."""
    cfg = scenes.CONFIGS["C2"]
    s = scenes.config_scene(cfg)
    r, o = pair(s, 0, cfg.width, cfg.height)
    rgba, rgb, st = r.render(0, want_rgb=True)
    assert st["pixels"] == cfg.width * cfg.height
    for x0, y0, w, h in ((800, 620, 320, 160), (0, 0, 256, 128)):
        orgb, orgba, _ = o.render(region=(x0, y0, w, h), threads=THREADS)
        crop = rgb[y0:y0 + h, x0:x0 + w]
        assert (crop != orgb).any(axis=2).sum() == 0, float(np.abs(crop - orgb).max())
        assert frac_within(rgba[y0:y0 + h, x0:x0 + w], orgba)[0] == 1.0


def test_c3_settings_spp4_depth4_crop(gpu_lib):
    s = scenes.demo_with_particles(24)
    r, o = pair(s, 1, 320, 180, sample_count=4, ray_trace_depth=4)
    rgba, rgb, st = r.render(0, want_rgb=True)
    orgb, orgba, ocnt = o.render(threads=THREADS)
    assert (rgb != orgb).any(axis=2).sum() == 0, float(np.abs(rgb - orgb).max())   # FAST on the reference's trees
    assert frac_within(rgba, orgba)[0] == 1.0
    rgba_e, rgb_e, st_e = r.render(0, exact=True, want_rgb=True)
    assert (rgb_e != orgb).any(axis=2).sum() == 0
    assert st_e["rays"] == ocnt["rays"]


def test_sample_count_floor_sqrt(gpu_lib):
    s = scenes.demo_scene()
    r, o = pair(s, 0, 96, 64, sample_count=8, ray_trace_depth=2)    # floor(sqrt(8)) = 2 -> 4 samples
    assert r.info()["sqrt_sample_count"] == 2
    rgba, rgb, st = r.render(0, exact=True, want_rgb=True)
    orgb, _, ocnt = o.render(threads=THREADS)
    assert (rgb != orgb).any(axis=2).sum() == 0 and st["rays"] == ocnt["rays"]


def test_defocus_rng_consumption(gpu_lib):
    r, o = pair(scenes.demo_scene(), 0, 96, 64, focus_disk_radius=0.3, ray_trace_depth=3)
    rgba, rgb, _ = r.render(0, exact=True, want_rgb=True)
    orgb, _, _ = o.render(threads=THREADS)
    assert (rgb != orgb).any(axis=2).sum() == 0


def test_metal_fuzz(gpu_lib):
    s = scenes.demo_with_particles(6)
    s.metals = [((0.8, 0.85, 0.88), 0.3)]
    r, o = pair(s, 2, 160, 90, ray_trace_depth=3)
    rgba, rgb, _ = r.render(0, exact=True, want_rgb=True)
    orgb, _, _ = o.render(threads=THREADS)
    assert (rgb != orgb).any(axis=2).sum() == 0


def _camera_rays(n, seed):
    g = np.random.default_rng(seed)
    o = np.stack([g.uniform(-3, 3, n), g.uniform(0.5, 6, n), g.uniform(4, 12, n)], 1)
    tgt = np.stack([g.uniform(-4, 4, n), g.uniform(-1, 5, n), g.uniform(-4, 4, n)], 1)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], 1).astype(np.float32)


def test_trace_rays_exact_and_fast(gpu_lib):
    s = scenes.demo_with_particles(16)
    r, o = pair(s, 9, 64, 64)
    rays = _camera_rays(20000, 4)
    oh, _ = o.trace(rays)
    eh = r.trace_rays(rays, exact=True)
    for k in ("t", "instance", "pindex", "ptype", "mtype", "midx"):
        assert np.array_equal(eh[k], oh[k]), k
    assert np.array_equal(eh["point"], oh["point"]) and np.array_equal(eh["normal"], oh["normal"])
    fh = r.trace_rays(rays)                   # FAST on the reference's trees: the same closest hits, bit for bit
    for k in ("t", "instance", "pindex", "ptype", "mtype", "midx"):
        assert np.array_equal(fh[k], oh[k]), k
    assert np.array_equal(fh["point"], oh["point"]) and np.array_equal(fh["normal"], oh["normal"])


def test_tile_shards_assemble_to_full_frame(gpu_lib):
    """Multi-GPU data path on one GPU: each 'rank' renders its interleaved tiles into a slab,
    the slabs are concatenated (what the RCCL gather produces) and assembled on the GPU; the
    result is byte-identical to the single-launch frame because the RNG is keyed by the global
    padded pixel index."""
    import torch
    s = scenes.demo_with_particles(10)
    W, H = 400, 232
    r = Renderer(s).build_acceleration_structure(0).configure_camera(W, H, ray_trace_depth=2)
    full, _, _ = r.render(0)
    for count, tw, th in ((2, 64, 64), (3, 64, 32), (8, 32, 32)):
        slab_tiles = max(r.tiles_for_rank(tw, th, k, count) for k in range(count))
        slab_px = slab_tiles * tw * th
        gathered = torch.zeros(count * slab_px * 4, dtype=torch.uint8, device="cuda")
        for k in range(count):
            r.render(0, tiles=(tw, th, k, count), rgba8_device=gathered.data_ptr() + k * slab_px * 4,
                     skip_update=True, want_rgba=False)
        frame = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
        r.assemble_tiles(gathered.data_ptr(), slab_tiles, tw, th, count, frame.data_ptr())
        assert np.array_equal(frame.cpu().numpy().reshape(H, W, 4), full), (count, tw, th)


def test_stack_depth_of_large_blas(gpu_lib):
    """A single 65k-triangle BLAS (depth ~15) plus the TLAS stays within the reference's 64-entry
    stack and matches the oracle exactly."""
    tris, inst = scenes.synth_particles(64, 1024, seed=3)
    s = scenes.demo_scene()
    s.triangles = np.concatenate([tris, s.triangles])
    for d in s.instances:
        if d["type"] == 2:
            d["index"] += tris.shape[0]
    lo = np.minimum.reduce([np.asarray(d["bounds"][0::2]) for d in inst])
    hi = np.maximum.reduce([np.asarray(d["bounds"][1::2]) for d in inst])
    s.instances.append(dict(type=2, index=0, count=tris.shape[0],
                            bounds=(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]), centroid=tuple((lo + hi) / 2),
                            shift=(0.0, 4.0, 0.0), rotate=(90.0, 0.0, 0.0), scale=(3.0, 3.0, 3.0)))
    r, o = pair(s, 4, 200, 120, ray_trace_depth=2)
    rgba, rgb, st = r.render(0, exact=True, want_rgb=True, count_work=True)
    orgb, _, ocnt = o.render(threads=THREADS)
    assert (rgb != orgb).any(axis=2).sum() == 0
    assert st["triangle_tests"] == ocnt["triangle_tests"]


@pytest.mark.parametrize("exact", [True, False])
def test_persistent_kernel_equals_grid_kernel(gpu_lib, exact):
    """The persistent-wave megakernel (lane refill, interleaved shading) and the one-thread-per-
    pixel grid kernel consume each pixel's RNG identically: same bytes, same ray count."""
    s = scenes.demo_with_particles(10)
    r = Renderer(s).build_acceleration_structure(2).configure_camera(320, 180, ray_trace_depth=3, sample_count=4)
    out = {}
    for kernel in (0, 1):
        r.set_option("kernel", kernel)
        out[kernel] = [r.render(0, exact=exact, want_rgb=True, count_work=True) for _ in range(2)]
    ref = out[0][0]
    for kernel, runs in out.items():
        for rgba, rgb, st in runs:
            # EXACT: no contraction, every kernel shape computes the same bits.  FAST on the reference's trees: the
            # grid kernel's binary pairs and the persistent kernel's pair-order quads both take the reference's box
            # decisions (exact-decision instances) with the reference's arithmetic: the same bits too
            assert np.array_equal(rgb, ref[1]) and np.array_equal(rgba, ref[0]), kernel
            for k in (("rays", "pixels", "triangle_tests", "instance_visits", "hits") if exact else ("rays", "pixels")):
                assert st[k] == ref[2][k], (kernel, k)


@pytest.mark.parametrize("depth,need", [(1, 0.999), (2, 0.999), (4, 0.995)])
def test_sah_trees_within_tolerance(gpu_lib, depth, need):
    """RT_BUILD_SAH builds different (better) trees than the reference's median split; hits can
    differ only where two surfaces tie within the 1e-6 window, so both kernels stay within the
    FAST tolerance of the oracle (which traverses the reference-order compat trees)."""
    from oracle.oracle import OracleScene
    s = scenes.demo_with_particles(16)
    r = Renderer(s).build_acceleration_structure(0, mode="sah").configure_camera(320, 180, ray_trace_depth=depth)
    o = OracleScene(s, build_seed=0)
    o.camera(320, 180, ray_trace_depth=depth)
    orgb, orgba, ocnt = o.render(threads=THREADS)
    for exact in (True, False):
        rgba, rgb, st = r.render(0, exact=exact, want_rgb=True, count_work=True)
        f, mx = frac_within(rgba, orgba)
        assert f >= need, (exact, f, mx)
        assert abs(st["rays"] - ocnt["rays"]) <= 0.001 * ocnt["rays"]


def test_pipelined_frames_collect(gpu_lib):
    """NO_SYNC frames with accumulated counters == the sum of synchronous frames; one kernel time
    per frame is collected from the event ring."""
    s = scenes.demo_with_particles(8)
    r = Renderer(s).build_acceleration_structure(0, mode="sah").configure_camera(256, 144, ray_trace_depth=2)
    rays = [r.render(f)[2]["rays"] for f in range(5)]
    r.collect()
    for f in range(5):
        r.render(f, sync=False, keep_counters=f > 0, want_rgba=False)
    acc, kms = r.collect()
    assert acc["rays"] == sum(rays) and len(kms) == 5 and all(k > 0 for k in kms)


def _sched_class(c):
    """layout.hpp cost_class: 0 = heaviest (half-octaves of the mean traversal steps per pixel)."""
    x = c.astype(np.uint64) + 64
    k = np.array([int(v * v).bit_length() - 1 - 12 for v in x.tolist()], np.int64)
    return 15 - np.clip(k, 0, 15)


# the claim-order settings the library fixes (scene.hpp; options until round 5): 8 XCD bands, heavy units in quarters
# from class level 12 (no halves), two adjacent units below level 6 merged into one item, costs recorded on one launch
# in 8 and the order rebuilt on the next
PARTS, K_HALF, K_QUARTER, K_MERGE, PERIOD, SCHED_THREADS = 8, 12, 12, 6, 8, 256


def expected_order(cost, ux, rows):
    """numpy restatement of schedule_kernel's order (csrc/schedule.hip): per band, the 256 threads' even ranges walked in
    screen order — a light pair (both below level K_MERGE) becomes one item (u << 4 | 3) in the pair's heavier class,
    else 1 << split_log2 pieces (u << 4 | piece << 2 | log2 pieces) — then the items class-major (heaviest first),
    thread order inside a class.  Returns {band: items}."""
    cls = _sched_class(cost)
    light = lambda c: 15 - c < K_MERGE
    split = lambda c: 2 if 15 - c >= K_QUARTER else (1 if 15 - c >= K_HALF else 0)
    out = {}
    for p in range(PARTS):
        b0, b1 = rows * p // PARTS * ux, rows * (p + 1) // PARTS * ux
        n = b1 - b0
        per = ((n + SCHED_THREADS - 1) // SCHED_THREADS + 1) & ~1
        by_class = [[] for _ in range(16)]
        for t in range(SCHED_THREADS):
            u, hi = b0 + min(n, t * per), b0 + min(n, (t + 1) * per)
            while u < hi:
                c = int(cls[u])
                if u + 1 < hi and light(c) and light(int(cls[u + 1])):
                    by_class[min(c, int(cls[u + 1]))].append((u << 4) | 3)
                    u += 2
                    continue
                ls = split(c)
                by_class[c].extend((u << 4) | (k << 2) | ls for k in range(1 << ls))
                u += 1
        out[p] = np.asarray([x for c in by_class for x in c], np.int64)
    return out


@pytest.mark.parametrize("exact", [False, True])
def test_reorder_schedule_is_byte_identical(gpu_lib, exact):
    """Option "reorder" (claims ordered heaviest-unit-first from a previous launch's unit costs, csrc/schedule.hip)
    changes only which wave traces which pixel: every frame is byte-identical to the screen-order walk (whole frame
    and a tile shard), and each rebuilt order equals a numpy restatement of the schedule kernel applied to the costs
    it read (light pairs merged, heavy units in quarters, class-major, screen order inside a class), reused until
    the next recording launch."""
    s = scenes.demo_with_particles(12)
    W, H = 480, 272
    F = PERIOD + 2                                    # launch 0 records, 1 orders, 2..8 reuse (8 records), 9 orders
    r = Renderer(s).build_acceleration_structure(0, mode="sah").configure_camera(W, H, ray_trace_depth=2)
    ref = {}
    r.set_option("reorder", 0)
    for f in range(F):
        ref[f] = r.render(f, exact=exact, want_rgb=True)
    tref = r.render(3, exact=exact, tiles=(64, 64, 1, 3), skip_update=True)[0]
    r.set_option("reorder", 1)
    ux, rows = W // 8, H // 8
    last = None
    checked = 0
    for f in range(F):
        rgba, rgb, st = r.render(f, exact=exact, want_rgb=True)
        assert np.array_equal(rgba, ref[f][0]) and np.array_equal(rgb, ref[f][1]), f
        assert st["rays"] == ref[f][2]["rays"]
        if f == 0:
            continue                                  # first launch of the layout: screen order, records costs
        order = r.debug_read("unit_order").view(np.uint32).astype(np.int64)
        if f % PERIOD == 1:                           # the order was rebuilt from the costs the schedule read
            cost = r.debug_read("unit_cost").view(np.uint32)
            assert (cost > 0).all()                   # every unit's pixels reported
            for p, items in expected_order(cost, ux, rows).items():
                b0 = rows * p // PARTS * ux
                assert np.array_equal(order[4 * b0:4 * b0 + len(items)], items), (f, p)
            checked += 1
        else:
            assert np.array_equal(order, last), f     # reused
        last = order
    assert checked == 2
    for _ in range(2):                                # tile shard: first launch of a layout, then ordered
        assert np.array_equal(r.render(3, exact=exact, tiles=(64, 64, 1, 3), skip_update=True)[0], tref)


@pytest.mark.parametrize("depth,need", [(1, 0.999), (2, 0.999), (4, 0.995)])
def test_wide_trees_within_tolerance(gpu_lib, depth, need):
    """Option "wide" (FAST persistent kernel on the 4-child collapse of the same trees): the leaves and
    boxes are the binary tree's, only the visit order changes, so images stay within the FAST
    tolerance of the oracle and of the binary-tree traversal, with the same number of rays."""
    from oracle.oracle import OracleScene
    s = scenes.demo_with_particles(16)
    o = OracleScene(s, build_seed=0)
    o.camera(320, 180, ray_trace_depth=depth)
    orgb, orgba, ocnt = o.render(threads=THREADS)
    for mode in ("compat", "sah"):
        r = Renderer(s).build_acceleration_structure(0, mode=mode).configure_camera(320, 180, ray_trace_depth=depth)
        out = {}
        for wide in (0, 1):
            r.set_option("wide", wide)
            out[wide] = r.render(0, want_rgb=True, count_work=True)
            f, mx = frac_within(out[wide][0], orgba)
            assert f >= need, (mode, wide, f, mx)
            assert abs(out[wide][2]["rays"] - ocnt["rays"]) <= 0.001 * ocnt["rays"]
        f, _ = frac_within(out[0][0], out[1][0])
        assert f >= need, (mode, f)
        r.cleanup()


def test_wide_large_blas_stack(gpu_lib):
    """A 65k-triangle BLAS under the TLAS through the quad traversal: deep trees push up to 3 entries
    per quad; the result stays within the FAST tolerance of the oracle and never overflows."""
    from oracle.oracle import OracleScene
    tris, inst = scenes.synth_particles(64, 1024, seed=3)
    s = scenes.demo_scene()
    s.triangles = np.concatenate([tris, s.triangles])
    for d in s.instances:
        if d["type"] == 2:
            d["index"] += tris.shape[0]
    lo = np.minimum.reduce([np.asarray(d["bounds"][0::2]) for d in inst])
    hi = np.maximum.reduce([np.asarray(d["bounds"][1::2]) for d in inst])
    s.instances.append(dict(type=2, index=0, count=tris.shape[0],
                            bounds=(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]), centroid=tuple((lo + hi) / 2),
                            shift=(0.0, 4.0, 0.0), rotate=(90.0, 0.0, 0.0), scale=(3.0, 3.0, 3.0)))
    r, o = pair(s, 4, 200, 120, ray_trace_depth=2)
    r.set_option("wide", 1)
    rgba, _, st = r.render(0, count_work=True)          # raises on a stack overflow
    _, orgba, ocnt = o.render(threads=THREADS)
    f, mx = frac_within(rgba, orgba)
    assert f >= 0.999, (f, mx)
    assert abs(st["rays"] - ocnt["rays"]) <= 0.001 * ocnt["rays"]


@pytest.mark.parametrize("opts", [{"grid_pct": 30}, {"stage_depth": 2}, {"stage_depth": 64}, {"lane_priority": 0}])
def test_claim_options_byte_identical(gpu_lib, opts):
    """Options that change how a frame is scheduled, not what it computes (a 30 % grid, the staging depth, normal-priority
    lanes): frames on three overlapped lanes equal the screen-order walk byte for byte, across the launches that
    record costs and the ones that claim in the recorded order, and the work counters equal the serial frames'."""
    import torch
    s = scenes.demo_with_particles(10)
    W, H, F = 360, 200, 20
    r = Renderer(s).build_acceleration_structure(0, mode="sah").configure_camera(W, H, ray_trace_depth=2)
    r.set_option("reorder", 0)
    ref = [r.render(f, count_work=True) for f in range(F)]
    r.set_option("reorder", 1).set_option("overlap", 3)
    for k, v in opts.items():
        r.set_option(k, v)
    streams = [torch.cuda.Stream() for _ in range(3)]
    bufs = [torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda") for _ in range(F)]
    torch.cuda.synchronize()
    for f in range(F):
        r.render(f, want_rgba=False, rgba8_device=bufs[f].data_ptr(), stream=streams[f % 3].cuda_stream, sync=False,
                 count_work=True, keep_counters=f > 0)
    acc, _ = r.collect()
    torch.cuda.synchronize()
    for f in range(F):
        assert np.array_equal(bufs[f].cpu().numpy().reshape(H, W, 4), ref[f][0]), f
    assert acc["rays"] == sum(x[2]["rays"] for x in ref)
    assert acc["pixels"] == F * W * H


@pytest.mark.parametrize("tiles,nl,mode", [(None, 2, "sah"), ((64, 64, 1, 3), 2, "sah"), (None, 3, "sah"),
                                           ((64, 64, 0, 2), 4, "sah"), (None, 2, "lbvh"), (None, 3, "lbvh-rebuild")])
def test_overlap_lanes_byte_identical(gpu_lib, tiles, nl, mode):
    """Option "overlap": frames alternate two library lanes on two caller streams and may run
    concurrently (frame k+1 fills frame k's tail).  Every frame is byte-identical to the serial
    render, the accumulated counters equal the sum of the serial frames', and one kernel time per
    frame is collected."""
    import torch
    s = scenes.demo_with_particles(12)
    W, H, F = 480, 272, 6
    r = Renderer(s).build_acceleration_structure(0, mode=mode.split("-")[0]).configure_camera(W, H, ray_trace_depth=2)
    if mode.endswith("rebuild"):
        r.set_option("rebuild", 1)            # every BLAS rebuilt each frame: waits for every lane's trace
    npix = (r.tiles_for_rank(*tiles) * tiles[0] * tiles[1]) if tiles else W * H
    # zeroed device outputs: a tile slab's pixels outside the frame are never written
    zero = [torch.zeros(npix * 4, dtype=torch.uint8, device="cuda") for _ in range(F)]
    torch.cuda.synchronize()
    ref = [r.render(f, tiles=tiles, rgba8_device=zero[f].data_ptr()) for f in range(F)]
    r.collect()
    r.set_option("overlap", nl)
    lanes = [torch.cuda.Stream() for _ in range(nl)]
    bufs = [torch.zeros(npix * 4, dtype=torch.uint8, device="cuda") for _ in range(F)]
    torch.cuda.synchronize()
    for rep in range(2):                       # second pass: both lanes hold a valid heaviest-first schedule
        for f in range(F):
            r.render(f, want_rgba=False, tiles=tiles, rgba8_device=bufs[f].data_ptr(),
                     stream=lanes[f % nl].cuda_stream, sync=False, keep_counters=True)
        acc, kms = r.collect()
        torch.cuda.synchronize()
        for f in range(F):
            assert np.array_equal(bufs[f].cpu().numpy(), ref[f][0].reshape(-1)), (rep, f)
        assert acc["rays"] == sum(x[2]["rays"] for x in ref)
        assert len(kms) == F and all(k > 0 for k in kms)
    r.set_option("overlap", 0)
    zero[2].zero_()
    torch.cuda.synchronize()
    rgba, _, st = r.render(2, tiles=tiles, rgba8_device=zero[2].data_ptr())
    assert np.array_equal(rgba, ref[2][0]) and st["rays"] == ref[2][2]["rays"]


