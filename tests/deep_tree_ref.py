"""Deep-tree scenes and a CPU model of the trace kernels' traversal stack — TEST INFRASTRUCTURE ONLY.

Every trace kernel keeps a per-lane stack window of 16 entries in LDS and pages half-windows of 8 entries out to and
back from scratch (csrc/stack.hpp, struct Stack).  Balanced trees never fill the window, so the paging code runs
only on deep trees.  This module makes such trees on purpose and says, per ray, how deep the stack gets:

* `deep_blas()` / `deep_two_level()`: two fixed scenes whose GPU-built (RT_BUILD_LBVH) trees are chains.  The triangle
  soup has one cluster of 3 triangles per bit b of the 30-bit Morton code, at the centroid whose code is 1 << b, and one
  cluster at (1, 1, 1) that pins the centroid bounds: 31 distinct codes, each shared by 3 triangles, and a radix tree
  that peels one code off per level (height 29 with 4-triangle leaves).  The triangles are large (vertex offsets with
  sigma 6 around centroids inside the unit cube), so every box of the chain overlaps every other and a ray through the
  soup pushes the far child at nearly every level.  `deep_two_level` instances the soup about a dozen times, with the
  instance centroids on a Morton chain of their own and two of them in one cell.
* `StackModel`: the binary traversal of trav_step (near child next, far child pushed with its entry t, a popped entry
  re-tested as entry t < closest t, TLAS leaves push their remainder, BLAS leaf primitives in order) over trees in the
  exported node form, with the kernel's window arithmetic (page-out of the bottom 8 entries at a push into a full
  window, page-in of 8 at a pop from an empty one).  Boxes are tested by the oracle's BoundingBox::hit
  (oracle_hit_aabb); the primitives' t come from a float64 Moeller-Trumbore over all (ray, instance, triangle), which
  also decides which rays are ambiguous (`ambiguous`).  The model is a yardstick for the inputs — how many rays page,
  how often, and whether the closest hit is found below an entry that went through scratch — not a reference for hits:
  those are the oracle's tree-free trace (OracleScene.trace(..., brute_force=2)).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from lbvh_ref import lbvh_tree
from rtamd import abi, scenes

F32 = np.float32
LDS_DEPTH, HALF = 16, 8            # csrc/trace_kernel.hip, csrc/stack.hpp: the window and the half-page
TMIN = F32(0.001)
CODE_BITS = 30
PER_CLUSTER = 3
SIGMA = 6.0
N_RAYS_BLAS = 3072
N_RAYS_TWO_LEVEL = 2048
TLAS_CHAIN = 10                    # instance centroids at the codes 1 << b, b < TLAS_CHAIN
TLAS_LEAF = 1                      # instances per GPU-built TLAS leaf: the library's fixed setting "tlas_leaf"
                                   # (csrc/scene.hpp; 2, the reference's TLAS leaf size, is the host builders')
BLAS_LEAF = 4                      # LBVH_BLAS_LEAF_CAP
TLAS_EXTENT = 48.0                 # world size of the instance centroids' cube
NEAR_MISS = 0.999                  # tmax = NEAR_MISS * t: just in front of the closest hit, 10 x AMBIGUOUS_DT away
AMBIGUOUS_DT = 1e-4                # two nearest hits within 1e-4 t of each other
AMBIGUOUS_EDGE = 1e-5              # the hit within 1e-5 (barycentric) of an edge


def chain_points(bits, extent=1.0):
    """bits + 1 points of [0, extent]^3: point b in the Morton cell (1024 per axis) whose code is 1 << b — axis
    2 - b % 3 (the code interleaves x, y, z from the top), cell 2 ** (b // 3), the cell's middle — and one at the far
    corner, which pins the bounds the codes are quantised in."""
    p = np.zeros((bits + 1, 3))
    for b in range(bits):
        p[b, 2 - b % 3] = (2 ** (b // 3) + 0.5) / 1024.0 * extent
    p[bits] = extent
    return p


def soup_triangles(seed=11):
    """The chain soup: PER_CLUSTER triangles at each of chain_points(30), every triangle's centroid on its cluster's
    point (zero-mean vertex offsets, sigma SIGMA), a different (material type, index) from its neighbours."""
    g = np.random.default_rng(seed)
    pts = chain_points(CODE_BITS)
    n = len(pts) * PER_CLUSTER
    t = np.zeros(n, dtype=scenes.TRIANGLE_DTYPE)
    for i in range(n):
        off = g.normal(0.0, SIGMA, (3, 3))
        off -= off.mean(axis=0)
        t["vertex"][i] = (pts[i // PER_CLUSTER] + off).astype(F32)
        t["material_type"][i] = abi.ROUGH if i % 3 else abi.METAL
        t["material_index"][i] = (i // 3) % 4 if i % 3 == 0 else i % 7
    return t


ROUGHS = [(.65, .05, .05), (.73, .73, .73), (.12, .45, .15), (.70, .60, .50), (.2, .3, .8), (.8, .8, .1), (.5, .1, .6)]
METALS = [((0.8, 0.85, 0.88), 0.0), ((0.9, 0.6, 0.3), 0.0), ((0.6, 0.9, 0.7), 0.1), ((0.7, 0.7, 0.9), 0.0)]
CAMERA = dict(scenes.DEMO_CAMERA, center=(0.4, 0.3, 30.0), target=(0.3, 0.3, 0.3), fov=50.0, ray_trace_depth=2)


def _scene(instances):
    """The soup under `instances`; the demo's spheres and parallelogram stay in the arrays, in no instance."""
    demo = scenes.demo_scene()
    return scenes.Scene(spheres=demo.spheres, parallelograms=demo.parallelograms, triangles=soup_triangles(),
                        roughs=list(ROUGHS), metals=list(METALS), instances=instances, animated=False,
                        camera=dict(CAMERA))


def deep_blas():
    """One triangle-group instance over the chain soup, untransformed."""
    n = len(chain_points(CODE_BITS)) * PER_CLUSTER
    return _scene([dict(type=abi.TRIANGLE, index=0, count=n)])


def deep_two_level():
    """The soup as one shared BLAS under TLAS_CHAIN + 2 instances: instance b < TLAS_CHAIN has its centroid at the code
    1 << b of the cube [0, TLAS_EXTENT]^3, one more shares the cell of instance 3, and one at the far corner pins the
    bounds.  Rotations up to +-20 degrees and scales 0.8 .. 1.25 about the soup's own centroid, so the shift that puts
    the instance centroid (forward matrix times the soup's centroid) on its point is the point minus the rotated and
    scaled centroid.  The chain lies within half a world unit of the origin: the soups overlap one another."""
    g = np.random.default_rng(23)
    tris = soup_triangles()
    n = len(tris)
    v = tris["vertex"].astype(F32)
    local = (((v[:, 0] + v[:, 1]) + v[:, 2]) / F32(3.0)).astype(np.float64).mean(axis=0)
    pts = chain_points(TLAS_CHAIN, TLAS_EXTENT)
    pts = np.concatenate([pts[:TLAS_CHAIN], pts[3:4] + [0.004, 0.0, 0.006], pts[TLAS_CHAIN:]])
    inst = []
    for p in pts:
        rot = g.uniform(-20.0, 20.0, 3)
        sc = g.uniform(0.8, 1.25, 3)
        m = _rotation(rot) @ np.diag(sc)
        shift = p - m @ local
        inst.append(dict(type=abi.TRIANGLE, index=0, count=n, shift=tuple(float(x) for x in shift),
                         rotate=tuple(float(x) for x in rot), scale=tuple(float(x) for x in sc)))
    return _scene(inst)


def _rotation(deg):
    """Rotation part of the project's forward matrix, from the oracle (oracle_instance_matrices)."""
    import ctypes as C

    from oracle.oracle import lib
    out = np.zeros(48, F32)
    x = abi.Xform(abi.Vec3.of((0, 0, 0)), abi.Vec3.of(tuple(float(d) for d in deg)), abi.Vec3.of((1, 1, 1)))
    lib().oracle_instance_matrices(C.byref(x), out.ctypes.data)
    return out[:16].reshape(4, 4)[:3, :3].astype(np.float64)


def aimed_rays(n, seed, centre, radius, spread):
    """n unit rays from a sphere of `radius` around `centre` towards points normal(centre, spread): from outside the
    soup (its vertices lie within ~4 sigma = 24 of the unit cube) through its middle."""
    g = np.random.default_rng(seed)
    o = g.normal(size=(n, 3))
    o = np.asarray(centre) + radius * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = np.asarray(centre) + g.normal(0.0, spread, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], 1).astype(F32)


def deep_blas_rays():
    return aimed_rays(N_RAYS_BLAS, 101, (0.3, 0.3, 0.3), 60.0, 2.0)


def deep_two_level_rays():
    return aimed_rays(N_RAYS_TWO_LEVEL, 202, (0.3, 0.3, 0.3), 70.0, 2.0)


# ---- items, trees ------------------------------------------------------------------------------------------------------
def triangle_items(scene):
    """The builder's items of the scene's triangles: the reference's primitive boxes (oracle_prim_bounds) and
    centroids ((v0 + v1) + v2) / 3 in float32, as tests/test_gpu_lbvh.py prim_items."""
    import ctypes as C

    from oracle.oracle import lib
    n = scene.triangle_count
    boxes = np.zeros((n, 6), F32)
    for k in range(n):
        prim = abi.Triangle.from_buffer_copy(scene.triangles[k].tobytes())
        lib().oracle_prim_bounds(abi.TRIANGLE, C.byref(prim), boxes[k].ctypes.data)
    v = scene.triangles["vertex"].astype(F32)
    return boxes, ((v[:, 0] + v[:, 1]) + v[:, 2]) / F32(3.0)


def tree_height(ci):
    """Interior levels on the longest root-to-leaf path of a tree in node form (count, index)."""
    height, todo = 0, [(0, 0)]
    while todo:
        j, d = todo.pop()
        if ci[j, 0]:
            height = max(height, d)
        else:
            todo += [(int(ci[j, 1]), d + 1), (int(ci[j, 1]) + 1, d + 1)]
    return height


# ---- all (ray, instance, triangle) intersections, float64 -------------------------------------------------------------
def all_hits(scene, rays, inv):
    """t, u, v [rays, instances, triangles] (float64; t = inf on a miss) of the rays taken into each instance's frame
    with `inv` ([instances, 3, 4], the inverse matrices' rows): Moeller-Trumbore as Triangle.cu:4-44, without its
    1e-6 windows."""
    rays = np.asarray(rays, np.float64)
    inv = np.asarray(inv, np.float64)
    o = np.einsum("iab,rb->ria", inv[:, :, :3], rays[:, :3]) + inv[None, :, :, 3]
    d = np.einsum("iab,rb->ria", inv[:, :, :3], rays[:, 3:])
    p = scene.triangles["vertex"].astype(np.float64)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    h = np.cross(d[:, :, None, :], e2[None, None])
    det = (e1[None, None] * h).sum(-1)
    s = o[:, :, None, :] - p[None, None, :, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (s * h).sum(-1) / det
        q = np.cross(s, e1[None, None])
        v = (d[:, :, None, :] * q).sum(-1) / det
        t = (e2[None, None] * q).sum(-1) / det
    ok = (np.abs(det) > 1e-12) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > float(TMIN))
    return np.where(ok, t, np.inf), u, v


def ambiguous(t, u, v):
    """bool [rays]: the two nearest hits lie within AMBIGUOUS_DT * t of each other (the reference accepts a hit within
    1e-6 of the closest so far, so the visit order decides between them), or the nearest hit lies within
    AMBIGUOUS_EDGE of an edge of its triangle (another rounding may miss it)."""
    r = t.shape[0]
    flat = t.reshape(r, -1)
    order = np.argsort(flat, axis=1)[:, :2]
    t0 = np.take_along_axis(flat, order[:, :1], 1)[:, 0]
    t1 = np.take_along_axis(flat, order[:, 1:], 1)[:, 0]
    hit = np.isfinite(t0)
    close = hit & np.isfinite(t1) & (t1 - t0 <= AMBIGUOUS_DT * t0)
    u0 = np.take_along_axis(u.reshape(r, -1), order[:, :1], 1)[:, 0]
    v0 = np.take_along_axis(v.reshape(r, -1), order[:, :1], 1)[:, 0]
    edge = hit & (np.minimum(np.minimum(u0, v0), 1.0 - u0 - v0) < AMBIGUOUS_EDGE)
    return close | edge


# ---- the stack model ---------------------------------------------------------------------------------------------------
@dataclass
class RayStack:
    max_occupancy: int = 0         # most entries on the stack at any time (window + scratch)
    page_outs: int = 0
    page_ins: int = 0
    enter_blas_max: int = 0        # most entries on the stack at the moment a BLAS is entered
    hit_instance: int = -1         # the model's closest hit (-1: miss)
    hit_prim: int = -1
    hit_paged: bool = False        # ... was found below an entry that had been paged out and back in
    tlas_paged_back: int = 0       # TLAS entries (nodes, leaf remainders) that came back through a page-in
    end_spilled: int = 0           # entries left in scratch when the traversal ends (a ranged query may end early)


class StackModel:
    """trav_step's binary traversal of (tlas, blas) with the kernel's stack window; see the module docstring.

    tlas, blas: (node_boxes, count_index, refs) as rt_scene_export_tlas / _blas give them; blas refs are triangle
    indices, tlas refs instance indices; inv [instances, 3, 4] the instances' inverse rows; t [rays, instances,
    triangles] from all_hits (rays in the same order as the ones given to run)."""

    def __init__(self, tlas, blas, inv, t):
        from oracle.oracle import lib
        self.hit_aabb = lib().oracle_hit_aabb
        self.tb, self.tci, self.trefs = (np.ascontiguousarray(tlas[0], F32), np.asarray(tlas[1]).astype(np.int64),
                                         np.asarray(tlas[2]).astype(np.int64))
        self.bb, self.bci, self.brefs = (np.ascontiguousarray(blas[0], F32), np.asarray(blas[1]).astype(np.int64),
                                         np.asarray(blas[2]).astype(np.int64))
        self.inv = np.asarray(inv, F32)
        self.t = np.asarray(t, F32)
        self.wray = np.zeros(6, F32)           # the buffers oracle_hit_aabb reads and writes: the world ray,
        self.lray = np.zeros(6, F32)           # the ray in the current instance's frame,
        self.rg = np.zeros(2, F32)
        self.te = np.zeros(1, F32)             # the range and the entry t
        self.rg[0] = TMIN
        self.addr = {id(a): a.ctypes.data for a in (self.tb, self.bb, self.wray, self.lray, self.rg, self.te)}

    def _box(self, boxes, j, tmax, ray):
        self.rg[1] = tmax
        a = self.addr
        ok = self.hit_aabb(a[id(boxes)] + 24 * j, a[id(ray)], a[id(self.rg)], a[id(self.te)])
        return bool(ok), float(self.te[0])

    def run(self, i, ray, tmax=np.inf, page_in_entries=HALF):
        """Ray i.  page_in_entries < HALF breaks the model on purpose: a page-in then brings back only the newest
        page_in_entries entries of its half-page and the older ones are lost (what a wrong stack_page_in would do)."""
        out = RayStack()
        world = np.asarray(ray, F32)
        tmax = float(F32(tmax))
        stack = []                 # [kind, a, b, entry t, paged]; the top `sp` entries are the LDS window
        sp = 0

        def push(kind, a, b, tn):
            nonlocal sp
            if sp == LDS_DEPTH:                              # stack_page_out: the window's bottom half to scratch
                base = len(stack) - LDS_DEPTH
                for e in stack[base:base + HALF]:
                    e[4] = True
                sp = HALF
                out.page_outs += 1
            stack.append([kind, a, b, tn, False])
            sp += 1
            out.max_occupancy = max(out.max_occupancy, len(stack))

        def pop():
            nonlocal sp
            if sp == 0:                                      # stack_page_in
                sp = page_in_entries
                del stack[len(stack) - HALF:len(stack) - page_in_entries]
                out.page_ins += 1
            sp -= 1
            return stack.pop()

        self.wray[:] = world
        ok, _ = self._box(self.tb, 0, tmax, self.wray)       # trav_init: the root's pop test
        cur = ["T", 0, 0, 0.0, False] if ok else None
        inst = 0
        paged = False                                        # the subtree in hand hangs below a paged-in entry
        while True:
            if cur is None:
                while stack:
                    e = pop()
                    if e[3] < tmax:                          # pop_keep
                        cur, paged = e, e[4]
                        out.tlas_paged_back += e[4] and e[0] in "TL"
                        break
                else:
                    break
                continue
            kind, a, b = cur[0], cur[1], cur[2]
            cur = None
            if kind in "TB":
                # BLAS entries lie above every TLAS entry, so the instance's ray is still the one they were pushed with
                boxes, ci, ray = (self.tb, self.tci, self.wray) if kind == "T" else (self.bb, self.bci, self.lray)
                if ci[a, 0] == 0:                            # interior: both children, the nearer next
                    left = int(ci[a, 1])
                    h0, e0 = self._box(boxes, left, tmax, ray)
                    h1, e1 = self._box(boxes, left + 1, tmax, ray)
                    if h0 and h1:
                        right_near = e0 > e1
                        push(kind, left if right_near else left + 1, 0, e0 if right_near else e1)
                        cur = [kind, left + 1 if right_near else left, 0]
                    elif h0 or h1:
                        cur = [kind, left if h0 else left + 1, 0]
                elif kind == "T":                            # TLAS leaf = its instances in order
                    cur = ["L", int(ci[a, 1]), int(ci[a, 0])]
                else:                                        # BLAS leaf: primitives in leaf order
                    for p in self.brefs[ci[a, 1]:ci[a, 1] + ci[a, 0]]:
                        t = float(self.t[i, inst, p])
                        if abs(t - tmax) < 1e-6 or float(TMIN) < t < tmax:       # Range.cuh:33-43
                            tmax = t
                            out.hit_instance, out.hit_prim, out.hit_paged = inst, int(p), paged
            else:                                            # "L": instance refs [a, a + b) of a TLAS leaf
                if b > 1:
                    push("L", a + 1, b - 1, -np.inf)
                inst = int(self.trefs[a])
                m = self.inv[inst]
                self.lray[:3] = m[:, :3] @ world[:3] + m[:, 3]
                self.lray[3:] = m[:, :3] @ world[3:]
                ok, _ = self._box(self.bb, 0, tmax, self.lray)                   # the BLAS root's pop test
                if ok:
                    out.enter_blas_max = max(out.enter_blas_max, len(stack))
                    cur = ["B", 0, 0]
        out.end_spilled = len(stack) - sp
        return out


# ---- one prepared case per scene, shared by the CPU conditions and the GPU tests ---------------------------------------
@dataclass
class DeepCase:
    name: str
    scene: object
    rays: np.ndarray
    boxes: np.ndarray              # triangle items
    cents: np.ndarray
    blas: tuple                    # lbvh_tree(boxes, cents, BLAS_LEAF)
    tlas: tuple                    # lbvh_tree(instance world boxes, centroids, TLAS_LEAF), the oracle's instance records
    inv: np.ndarray
    t: np.ndarray                  # all_hits
    ambiguous: np.ndarray
    want: np.ndarray               # the oracle's tree-free records
    oracle: object


@functools.lru_cache(maxsize=None)
def case(name):
    from oracle.oracle import OracleScene
    scene, rays = {"deep_blas": (deep_blas, deep_blas_rays), "deep_two_level": (deep_two_level, deep_two_level_rays)}[name]
    scene, rays = scene(), rays()
    o = OracleScene(scene, build_seed=0)
    state = o.instance_state()
    boxes, cents = triangle_items(scene)
    t, u, v = all_hits(scene, rays, state[:, :12].reshape(-1, 3, 4))
    want = o.trace(rays, brute_force=2)[0]
    for a in (rays, want):
        a.setflags(write=False)
    return DeepCase(name, scene, rays, boxes, cents, lbvh_tree(boxes, cents, BLAS_LEAF),
                    lbvh_tree(state[:, 36:42], state[:, 42:45], TLAS_LEAF), state[:, :12].reshape(-1, 3, 4), t,
                    ambiguous(t, u, v), want, o)


@functools.lru_cache(maxsize=None)
def modelled(name):
    """[RayStack] of the case's rays through its restated trees."""
    c = case(name)
    m = StackModel(c.tlas, c.blas, c.inv, c.t)
    return [m.run(i, r) for i, r in enumerate(c.rays)]
