"""Leaves postponed where they appear (csrc/traverse.hpp spec_round): in the interior-loop iteration whose node step
produced them, and at the end of the leaf phase when the re-tested successor is one.

Rows of N instances on one line, so that one ray meets 1 .. N TLAS leaves in succession — each postponed right after
the leaf phase of the one before it, with whatever the stack holds:

* "sphere" rows: every instance is one sphere, whose BLAS root is a leaf — the FAST quad kernel chains it into the TLAS
  leaf's phase (RT_CHAIN_ROOT_LEAF) and pops the next leaf after its test;
* "mesh" rows: every instance is a 64-triangle sphere, whose BLAS root is interior — not chained; its leaves are
  postponed in the interior loop and the next TLAS leaf is the successor that survives the re-test;
* the reference's trees (TLAS leaves of two instances: the leaf's remainder entry, entry t -inf, is on the stack when
  the leaf after it is postponed) and host SAH trees (one instance per TLAS leaf); N = 1 is a TLAS whose root is a
  leaf, postponed without a node step before it.

Every comparison is exact: rt_query_rays (closest hit, t only, occlusion) and rt_trace_rays against the oracle's ranged
trace, a third of the rays with a range that ends inside the row; the frame looking down the row against the oracle's,
EXACT with the oracle's work counters.  (The persistent kernel's fixed setting "leaf_early" is no option any more, so
no test can switch it.)
"""
import functools

import numpy as np
import pytest

from rtamd import Renderer, abi, scenes
from test_gpu_ray_query import FIELDS, assert_records_equal, closest, occluded

pytestmark = pytest.mark.gpu

THREADS = 16
SIZES = [1, 2, 3, 5, 17, 40]
KINDS = ["sphere", "mesh"]
PITCH = 1.25                       # distance between two instances of a row (their boxes, 0.8 wide, do not touch)
RADIUS = 0.4
N_RAYS = 384
W = H = 32
SEED = 5


def row_scene(kind, n):
    """n instances of one primitive set along the x axis, at x = 0, PITCH, ..."""
    verts, faces = scenes.uv_sphere_template(64)
    tris = np.zeros(len(faces), dtype=scenes.TRIANGLE_DTYPE)
    tris["vertex"] = (verts[faces] * RADIUS).astype(np.float32)
    tris["material_type"] = abi.ROUGH
    tris["material_index"] = np.arange(len(faces)) % 4
    if kind == "sphere":
        inst = [dict(type=abi.SPHERE, index=0, shift=(PITCH * i, 0.0, 0.0)) for i in range(n)]
    else:
        inst = [dict(type=abi.TRIANGLE, index=0, count=len(faces), shift=(PITCH * i, 0.0, 0.0)) for i in range(n)]
    demo = scenes.demo_scene()
    camera = dict(scenes.DEMO_CAMERA, center=(-12.0, 0.3, 0.25), target=(PITCH * n, 0.0, 0.0), fov=6.0)
    return scenes.Scene(spheres=[(abi.ROUGH, 1, (0.0, 0.0, 0.0), RADIUS)], parallelograms=demo.parallelograms,
                        triangles=tris, roughs=demo.roughs, metals=demo.metals, instances=inst, animated=False,
                        camera=camera)


def row_rays(n, seed):
    """Rays along the row, from before its first instance or (a quarter) from behind its last one backwards, offset
    from the axis by up to 1.2 radii on y and z with a small tilt: some hit the first sphere they meet, many pass
    through the corners of box after box without touching what is inside.  A third have a range that ends inside
    the row."""
    g = np.random.default_rng(seed)
    length = PITCH * (n - 1)
    back = g.random(N_RAYS) < 0.25
    o = np.stack([np.where(back, length + 2.0, -2.0), g.uniform(-1.2, 1.2, N_RAYS) * RADIUS,
                  g.uniform(-1.2, 1.2, N_RAYS) * RADIUS], 1)
    d = np.stack([np.where(back, -1.0, 1.0), g.normal(0.0, 0.02, N_RAYS), g.normal(0.0, 0.02, N_RAYS)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmax = np.full(N_RAYS, np.inf, np.float32)
    ranged = np.arange(N_RAYS) % 3 == 0
    tmax[ranged] = g.uniform(1.0, length + 4.0, int(ranged.sum())).astype(np.float32)
    return np.concatenate([o, d], 1).astype(np.float32), tmax


class Row:
    """One row: its scene, rays, and the oracle's answers (computed once)."""

    def __init__(self, kind, n):
        from oracle.oracle import OracleScene
        self.scene = row_scene(kind, n)
        self.oracle = OracleScene(self.scene, build_seed=SEED)
        self.rays, self.tmax = row_rays(n, 100 * n + (kind == "mesh"))
        self.want = self.oracle.trace(self.rays, tmax=self.tmax)[0]
        self.want_open = self.oracle.trace(self.rays)[0]
        self.oracle.camera(W, H, ray_trace_depth=2)
        self.orgb, self.orgba, self.ocnt = self.oracle.render(threads=THREADS)
        for a in (self.rays, self.want, self.want_open, self.orgb, self.orgba):     # (tmax goes to torch as it is)
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def row(kind, n):
    return Row(kind, n)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["compat", "sah"])
def test_rows_of_tlas_leaves(gpu_lib, oracle_lib, mode, kind, n):
    """384 rays down a row of n instances: the closest-hit records, t alone, occlusion (the ranged rays and all of
    them with the open range) and rt_trace_rays equal the oracle's, EXACT and FAST."""
    c = row(kind, n)
    hit = c.want["instance"] != abi.MISS
    cut = (c.want_open["instance"] != abi.MISS) & ~hit                    # the range ended before the hit
    assert hit.sum() >= N_RAYS // 8 and (~hit).sum() >= N_RAYS // 8, (hit.sum(), N_RAYS)
    if n > 1:
        assert cut.sum() > 0
    r = Renderer(c.scene).build_acceleration_structure(SEED, mode=mode)
    for exact in (True, False):
        what = (mode, kind, n, "exact" if exact else "fast")
        t, h = closest(r, c.rays, c.tmax, exact=exact)
        assert_records_equal(h, c.want, FIELDS)
        assert np.array_equal(t, c.want["t"]), what
        t_only, _ = closest(r, c.rays, c.tmax, exact=exact, want_hits=False)
        assert np.array_equal(t_only, c.want["t"]), what
        assert np.array_equal(occluded(r, c.rays, c.tmax, exact=exact), hit), what
        _, h_open = closest(r, c.rays, exact=exact)
        assert_records_equal(h_open, c.want_open, FIELDS)
        assert np.array_equal(occluded(r, c.rays, exact=exact), c.want_open["instance"] != abi.MISS), what
        traced = r.trace_rays(c.rays, exact=exact)
        assert_records_equal(traced, c.want_open, FIELDS)
    r.cleanup()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_row_frames_and_work_counters(gpu_lib, oracle_lib, kind, n):
    """32 x 32 down the row, depth 2, on the reference's trees (TLAS leaves of two instances): the persistent EXACT
    frame is the oracle's bit for bit with the oracle's work counters; the persistent FAST frame and both grid frames
    are the same frame."""
    c = row(kind, n)
    r = Renderer(c.scene).build_acceleration_structure(SEED).configure_camera(W, H, ray_trace_depth=2)
    if n > 2:
        _, ci, _ = r.export_tlas()
        assert (ci[:, 0] == 2).sum() >= 1, ci[:, 0]                       # leaves of two instances
    rgba, rgb, st = r.render(0, exact=True, want_rgb=True, count_work=True)
    print(kind, n, {k: (st[k], c.ocnt[k]) for k in ("rays", "instance_visits", "triangle_tests", "sphere_quad_tests")})
    assert np.array_equal(rgb, c.orgb), int((rgb != c.orgb).any(axis=2).sum())
    assert np.array_equal(rgba, c.orgba)
    for k in ("rays", "instance_visits", "triangle_tests", "sphere_quad_tests"):
        assert st[k] == c.ocnt[k], (k, st[k], c.ocnt[k])
    assert st["instance_visits"] >= W * H // 4                            # the frame does look down the row
    for kernel, exact in ((1, False), (0, True), (0, False)):
        r.set_option("kernel", kernel)
        rgba2, rgb2, st2 = r.render(0, exact=exact, want_rgb=True, count_work=True)
        assert np.array_equal(rgb2, c.orgb) and np.array_equal(rgba2, c.orgba), (kernel, exact)
        assert st2["rays"] == c.ocnt["rays"], (kernel, exact)
    r.cleanup()


def test_demo_frame_work_counters(gpu_lib, oracle_lib):
    """96 x 64 of the demo scene plus 6 particles, depth 2 (tests/test_gpu_last_segment.py's frame): EXACT work counters
    equal the oracle's."""
    from oracle.oracle import OracleScene
    s = scenes.demo_with_particles(6)
    r = Renderer(s).build_acceleration_structure(7).configure_camera(96, 64, ray_trace_depth=2)
    o = OracleScene(s, build_seed=7)
    o.camera(96, 64, ray_trace_depth=2)
    orgb, _, ocnt = o.render(threads=THREADS)
    _, rgb, st = r.render(0, exact=True, want_rgb=True, count_work=True)
    r.cleanup()
    assert np.array_equal(rgb, orgb)
    for k in ("rays", "instance_visits", "triangle_tests", "sphere_quad_tests"):
        assert st[k] == ocnt[k], (k, st[k], ocnt[k])
