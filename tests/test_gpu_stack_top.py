"""The traversal stack's register-held top entry (csrc/stack.hpp, Stack::top_ref / top_tn) at every stack depth.

The newest stack entry stays in two VGPRs and goes to the LDS window only when another entry is pushed on top of it,
so every paging condition of the window (stack_push: sp == LDS_DEPTH; the quad step's stack_push3: sp > LDS_DEPTH - 3;
stack_pop: sp == 0 with spilled > 0; empty()) is now met with and without a held entry above it.  The scenes of
tests/test_gpu_deep_stack.py have trees of one depth (29 and 10 + 29 levels); here the depth is swept, so that the
held entry meets each condition at every residue of the window arithmetic.

* chains of 1 .. 40 levels, GPU-built over clustered centroids as tests/deep_tree_ref.py builds its 29-level soup: a
  soup of `level` + 1 clusters for 1 .. 29 levels (one code bit peeled per level), and for 30 .. 40 levels the
  29-level soup under a TLAS chain of level - 29 levels (deep_two_level's construction, without its tied pair);
* a TLAS leaf of two instances on the reference's trees: spec_leaf_phase pushes the speculative successor and then
  the leaf's resume entry on top of it;
* rt_query_rays on the same chains, with ranges that end between the first and the second hit.
"""
import functools

import numpy as np
import pytest

import deep_tree_ref as D
from lbvh_ref import check_tree, lbvh_tree
from rtamd import Renderer, abi, scenes
from test_gpu_deep_stack import check_against
from test_gpu_lbvh import frac_within
from test_gpu_ray_query import closest, occluded

pytestmark = pytest.mark.gpu

THREADS = 16
LEVELS = list(range(1, 41))
BLAS_MAX = 29                      # levels of the deepest single chain: 30 code bits, the last two clusters share a node
W = H = 32
N_RAYS = 4096


# ---- the chains ----------------------------------------------------------------------------------------------------------
def soup(bits, seed=11):
    """deep_tree_ref.soup_triangles with `bits` chain clusters (+ the far corner's) instead of all 30."""
    g = np.random.default_rng(seed)
    pts = D.chain_points(bits)
    n = len(pts) * D.PER_CLUSTER
    t = np.zeros(n, dtype=scenes.TRIANGLE_DTYPE)
    for i in range(n):
        off = g.normal(0.0, D.SIGMA, (3, 3))
        off -= off.mean(axis=0)
        t["vertex"][i] = (pts[i // D.PER_CLUSTER] + off).astype(D.F32)
        t["material_type"][i] = abi.ROUGH if i % 3 else abi.METAL
        t["material_index"][i] = (i // 3) % 4 if i % 3 == 0 else i % 7
    return t


def chain_scene(level):
    """(scene, BLAS levels, TLAS levels) of a chain `level` levels deep in all."""
    blas, tlas = min(level, BLAS_MAX), max(level - BLAS_MAX, 0)
    tris = soup(blas)
    n = len(tris)
    if tlas == 0:
        inst = [dict(type=abi.TRIANGLE, index=0, count=n)]
    else:
        g = np.random.default_rng(23)
        v = tris["vertex"].astype(D.F32)
        local = (((v[:, 0] + v[:, 1]) + v[:, 2]) / D.F32(3.0)).astype(np.float64).mean(axis=0)
        inst = []
        for p in D.chain_points(tlas, D.TLAS_EXTENT):        # tlas + 1 instances: one centroid code peeled per level
            rot = g.uniform(-20.0, 20.0, 3)
            sc = g.uniform(0.8, 1.25, 3)
            shift = p - (D._rotation(rot) @ np.diag(sc)) @ local
            inst.append(dict(type=abi.TRIANGLE, index=0, count=n, shift=tuple(float(x) for x in shift),
                             rotate=tuple(float(x) for x in rot), scale=tuple(float(x) for x in sc)))
    demo = scenes.demo_scene()
    scene = scenes.Scene(spheres=demo.spheres, parallelograms=demo.parallelograms, triangles=tris,
                         roughs=list(D.ROUGHS), metals=list(D.METALS), instances=inst, animated=False,
                         camera=dict(D.CAMERA))
    return scene, blas, tlas


class Chain:
    """One chain: its scene, its oracle, the restated heights, the oracle's 32 x 32 depth-1 frame (computed once)."""

    def __init__(self, level):
        from oracle.oracle import OracleScene
        self.level = level
        self.scene, self.blas_levels, self.tlas_levels = chain_scene(level)
        self.oracle = OracleScene(self.scene, build_seed=0)
        boxes, cents = D.triangle_items(self.scene)
        assert check_tree(*lbvh_tree(boxes, cents, D.BLAS_LEAF), boxes, D.BLAS_LEAF) == self.blas_levels
        if self.tlas_levels:
            st = self.oracle.instance_state()
            tree = lbvh_tree(st[:, 36:42], st[:, 42:45], D.TLAS_LEAF)
            assert check_tree(*tree, st[:, 36:42], D.TLAS_LEAF) == self.tlas_levels
        self.oracle.camera(W, H, ray_trace_depth=1)
        _, self.orgba, self.ocnt = self.oracle.render(threads=THREADS)
        self.orgba.setflags(write=False)

    def renderer(self):
        r = Renderer(self.scene).set_option("group", 0).build_acceleration_structure(0, mode="lbvh")
        info = r.info()
        assert info["blas_height_max"] == self.blas_levels, (self.level, info["blas_height_max"])
        if self.tlas_levels:
            assert info["tlas_height"] == self.tlas_levels, (self.level, info["tlas_height"])
        return r


@functools.lru_cache(maxsize=None)
def chain(level):
    return Chain(level)


# ---- 1. every stack depth across both paging sites -----------------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
def test_chain_frames_every_depth(gpu_lib, oracle_lib, level):
    """32 x 32, ray_trace_depth 1, count_work on (an overflow raises): the FAST persistent kernel on quads (stack_push3
    and its sp > LDS_DEPTH - 3 page-out) and on binary pairs (stack_push and its sp == LDS_DEPTH page-out), the FAST
    grid kernel and EXACT in both kernels.

    * the FAST persistent frames are byte-identical to the FAST grid frame, and EXACT's two kernels to each other;
    * the EXACT frame is bit-identical to the oracle's.  The oracle traverses its own (median-split) trees of the same
      scene, not the chain: the two can differ only where two hits lie within the reference's 1e-6 window of each
      other, which decides by visit order — no pixel of these 40 frames holds such a pair;
    * the FAST frames meet test_gpu_deep_stack.py's bar against the oracle: >= 99.9 % of pixels within 1 LSB and the
      ray count within 0.1 %."""
    c = chain(level)
    r = c.renderer().configure_camera(W, H, ray_trace_depth=1)
    frames = {}
    for name, kernel, wide, exact in (("fast persistent quads", 1, 1, False), ("fast persistent pairs", 1, 0, False),
                                      ("fast grid", 0, 1, False), ("exact persistent", 1, 0, True),
                                      ("exact grid", 0, 0, True)):
        r.set_option("kernel", kernel).set_option("wide", wide)
        rgba, _, st = r.render(0, exact=exact, count_work=True)              # raises RT_ERR_UNSUPPORTED on an overflow
        f, mx = frac_within(rgba, c.orgba)
        print(f"level {level} {name}: within 1 LSB {f:.5f} (max {mx}), differing pixels "
              f"{int((rgba != c.orgba).any(axis=2).sum())}, rays {st['rays']} / {c.ocnt['rays']}")
        frames[name] = (rgba, st["rays"], f)
    r.cleanup()
    grid = frames["fast grid"]
    for name in ("fast persistent quads", "fast persistent pairs"):
        assert np.array_equal(frames[name][0], grid[0]) and frames[name][1] == grid[1], (level, name)
    assert np.array_equal(frames["exact persistent"][0], frames["exact grid"][0]), level
    assert frames["exact persistent"][1] == frames["exact grid"][1], level
    assert np.array_equal(frames["exact persistent"][0], c.orgba), level
    assert frames["exact persistent"][1] == c.ocnt["rays"], level
    for name, (rgba, rays, f) in frames.items():
        assert f >= 0.999, (level, name, f)
        assert abs(rays - c.ocnt["rays"]) <= 0.001 * c.ocnt["rays"], (level, name)


# ---- 2. a resume entry above a held successor ----------------------------------------------------------------------------
def test_resume_entry_above_held_successor(gpu_lib, oracle_lib):
    """The reference's trees of the demo scene plus 4 particles of 64 triangles: 9 instances under TLAS leaves of two,
    so a postponed TLAS leaf pushes its speculative successor and then the resume entry for its second instance on top
    of it (spec_leaf_phase) — the held successor goes down into LDS and the resume entry is held.  64 x 64,
    ray_trace_depth 4: the FAST persistent frame is bit-identical to the oracle's (mode 3), and so is
    the EXACT frame, with the oracle's ray count."""
    from oracle.oracle import OracleScene
    s = scenes.demo_with_particles(4, T=64)
    r = Renderer(s).build_acceleration_structure(7).configure_camera(64, 64, ray_trace_depth=4)
    _, ci, _ = r.export_tlas()
    assert (ci[:, 0] == 2).sum() >= 2, ci[:, 0]                             # leaves of two instances
    o = OracleScene(s, build_seed=7)
    o.camera(64, 64, ray_trace_depth=4)
    orgb, orgba, ocnt = o.render(threads=THREADS)
    for exact in (False, True):
        rgba, rgb, st = r.render(0, exact=exact, want_rgb=True, count_work=True)
        assert np.array_equal(rgb, orgb), (exact, int((rgb != orgb).any(axis=2).sum()), float(np.abs(rgb - orgb).max()))
        assert np.array_equal(rgba, orgba), exact
        assert st["rays"] == ocnt["rays"], (exact, st["rays"], ocnt["rays"])
    r.cleanup()


# ---- 3. ray queries on the same chains -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def query_rays(two_level):
    rays = D.aimed_rays(N_RAYS, 303 + two_level, (0.3, 0.3, 0.3), 70.0 if two_level else 60.0, 2.0)
    rays.setflags(write=False)
    return rays


@pytest.mark.parametrize("level", LEVELS)
def test_ray_queries_every_depth(gpu_lib, oracle_lib, level):
    """4 096 seeded rays through rt_query_rays, EXACT and FAST: closest records, t-only and occlusion.  The even rays
    have the range [0.001, inf); an odd ray that hits has a finite tmax halfway between its first and its second hit
    (twice its first when there is no second; float64 Moeller-Trumbore over every triangle, deep_tree_ref.all_hits),
    so its traversal ends with the closest hit found and entries still stacked.  Compared as
    tests/test_gpu_deep_stack.py compares: on every unambiguous ray the surface and material equal the oracle's
    tree-free ranged trace and t is bit-equal; occluded == isfinite(t) on every ray."""
    c = chain(level)
    rays = query_rays(c.tlas_levels > 0)
    state = c.oracle.instance_state()
    t, u, v = D.all_hits(c.scene, rays, state[:, :12].reshape(-1, 3, 4))
    with np.errstate(invalid="ignore"):                  # rays that miss everything: inf - inf
        ok = ~D.ambiguous(t, u, v)
    two =np.sort(t.reshape(len(rays), -1), axis=1)[:, :2]
    first, second = two[:, 0], two[:, 1]
    between = np.where(np.isfinite(second), 0.5 * (first + second), 2.0 * first)
    tmax = np.full(len(rays), np.inf, np.float32)
    odd = (np.arange(len(rays)) % 2 == 1) & np.isfinite(first)
    tmax[odd] = between[odd].astype(np.float32)
    want = c.oracle.trace(rays, brute_force=2, tmax=tmax)[0]
    hit = want["instance"] != abi.MISS
    assert ok.mean() >= 0.95 and hit.mean() >= 0.5 and odd.sum() >= N_RAYS // 4, (ok.mean(), hit.mean(), odd.sum())
    r = c.renderer()
    r.set_option("fast_math", 0)
    for exact in (True, False):
        what = (level, "exact" if exact else "fast")
        tq, h = closest(r, rays, tmax, exact=exact)
        check_against(h, want, ok, what + ("query",), True)
        assert np.array_equal(tq, h["t"]), what
        t_only, _ = closest(r, rays, tmax, exact=exact, want_hits=False)
        assert np.array_equal(t_only, tq), what
        assert np.array_equal(occluded(r, rays, tmax, exact=exact), np.isfinite(tq)), what
    r.cleanup()
