"""Scenes that put the GPU builder (csrc/lbvh.hip, lbvh_*.hpp) on every one of its size thresholds and on degenerate centroid
sets — TEST INFRASTRUCTURE ONLY.  tests/test_lbvh_sizes_ref.py checks on the CPU that the inputs hit what they aim
at; tests/test_gpu_lbvh_sizes.py compares the GPU's trees with tests/lbvh_ref.py on them.

* `forest(kind, order)`: one static scene with a triangle BLAS of every size in SIZES (26 604 triangles), one instance
  and one transform per size, the sizes' triangles back to back in one array: 1 (the m == 1 special cases), 2..4 (one
  leaf, through Karras), around every power of two a bitonic sort pads to, around LOCAL_SORT_MAX = LOCAL_MAX = 2048
  (LDS sort + bottom_up_local_kernel against rocPRIM sort + chunk and top pass), around LDS_FRONT + 1 = 1025 pairs
  (collapse_wide_kernel's frontier in LDS or in scratch), and multiples of LBVH_CHUNK = 1024 plus 0, 1, 2.
  "shuffled" puts the same trees in another order, so their edges meet waves, blocks, KWIN windows and chunks at other
  offsets and small trees sit inside chunks of large ones.
* kinds: "random"; "planar" (every vertex the same z: no extent on one axis); "same" (every triangle of a tree a copy
  of its first: all codes 0); "dup8" (runs of eight copies: ties that cross leaf, wave and chunk edges).
* `aimed_rays()`: rays at points on the "random" forest's triangles, every size aimed at equally often.
* `tlas_scene(K, kind)`: one sphere under K instances, K around SMALL_TLAS_MAX = 512 and LOCAL_MAX = 2048.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np

from deep_tree_ref import METALS, ROUGHS
from lbvh_ref import check_tree, lbvh_tree, morton_codes
from rtamd import abi, scenes

F32 = np.float32
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2050, 3071, 3072,
         3073, 4097]
KINDS = ("random", "planar", "same", "dup8")
ORDERS = ("ascending", "shuffled")
BLAS_LEAF = 4                      # LBVH_BLAS_LEAF_CAP
TLAS_LEAF = 1                      # the library's fixed "tlas_leaf" for GPU-built TLASes (tests/deep_tree_ref.py)
LOCAL_MAX = 2048                   # lbvh_sort.hpp: LOCAL_SORT_MAX = LOCAL_MAX (a static_assert there)
CHUNK = 1024                       # lbvh_hierarchy.hpp: LBVH_CHUNK
HEIGHT_MAX = 20                    # a condition on the inputs (include/rt.h: tlas_height + blas_height_max <= 40)
HALF_EXTENT = 1.0                  # triangle centroids in [-1, 1]^3 of their BLAS's frame
HALF_EDGE = 0.02                   # vertices within +-0.02 of the centroid: an edge ~0.02 of the cloud's extent
PLANE_Z = -0.25
DUP = 8
N_RAYS = 4000
RAY_SEED = 404
RAY_DISTANCE = 9.0                 # ray origins: this far from their target, outside the cloud (radius < 5)
TLAS_SIZES = [2, 3, 511, 512, 513, 2047, 2048, 2049, 2500]
TLAS_KINDS = ("random", "lattice")
TLAS_FRAME_SIZES = (512, 513, 2048, 2049)
SMALL_TLAS_MAX = 512               # lbvh.hpp
CAMERA = dict(scenes.DEMO_CAMERA, center=(0.0, 0.5, 9.0), target=(0.0, 0.0, 0.0), fov=45.0, ray_trace_depth=2)
TLAS_CAMERA = dict(scenes.DEMO_CAMERA, center=(3.0, 5.0, 60.0), target=(0.0, 0.0, 0.0), fov=45.0, ray_trace_depth=2)


# ---- the size-sweep forest ---------------------------------------------------------------------------------------------
def size_order(order):
    if order == "ascending":
        return list(SIZES)
    assert order == "shuffled"
    return [SIZES[k] for k in np.random.default_rng(31).permutation(len(SIZES))]


@functools.lru_cache(maxsize=None)
def tree_triangles(kind, size):
    """The triangles of the BLAS of `size` items (the same in both orders), in the BLAS's own frame."""
    g = np.random.default_rng([17, size])
    cen = g.uniform(-HALF_EXTENT, HALF_EXTENT, (size, 1, 3))
    v = cen + g.uniform(-HALF_EDGE, HALF_EDGE, (size, 3, 3))
    t = np.zeros(size, dtype=scenes.TRIANGLE_DTYPE)
    t["vertex"] = v.astype(F32)
    i = np.arange(size)
    t["material_type"] = np.where(i % 3 == 0, abi.METAL, abi.ROUGH)
    t["material_index"] = np.where(i % 3 == 0, (i // 3) % len(METALS), i % len(ROUGHS))
    if kind == "planar":
        t["vertex"][:, :, 2] = F32(PLANE_Z)
    elif kind == "same":
        t[:] = t[0]
    elif kind == "dup8":
        t = t[i // DUP].copy()
    else:
        assert kind == "random"
    t.setflags(write=False)
    return t


def transform(size):
    """The instance transform of the BLAS of `size` items: different for every size, the same in both orders."""
    g = np.random.default_rng([29, size])
    return dict(shift=tuple(float(x) for x in g.uniform(-1.5, 1.5, 3)),
                rotate=tuple(float(x) for x in g.uniform(-30.0, 30.0, 3)),
                scale=tuple(float(x) for x in g.uniform(0.8, 1.25, 3)))


@dataclass
class Forest:
    kind: str
    order: str
    scene: object
    trees: list                    # (size, first triangle) per instance = per BLAS, in instance order


def _scene(triangles, instances, camera):
    """Triangles under `instances`; the demo's spheres and parallelogram stay in the arrays, in no instance."""
    demo = scenes.demo_scene()
    return scenes.Scene(spheres=demo.spheres, parallelograms=demo.parallelograms, triangles=triangles,
                        roughs=list(ROUGHS), metals=list(METALS), instances=instances, animated=False,
                        camera=dict(camera))


def forest(kind, order):
    """A fresh scene each call (a test may move its triangles)."""
    trees, parts, inst, first = [], [], [], 0
    for size in size_order(order):
        parts.append(tree_triangles(kind, size))
        trees.append((size, first))
        inst.append(dict(type=abi.TRIANGLE, index=first, count=size, **transform(size)))
        first += size
    return Forest(kind, order, _scene(np.concatenate(parts), inst, CAMERA), trees)


def triangle_items(tris):
    """The builder's items: the reference's primitive boxes (oracle_prim_bounds) and centroids ((v0 + v1) + v2) / 3 in
    float32 — what tests/test_gpu_lbvh.py prim_items gives for the same triangles."""
    from oracle.oracle import lib
    n = tris.shape[0]
    boxes = np.zeros((n, 6), F32)
    for k in range(n):
        prim = abi.Triangle.from_buffer_copy(tris[k].tobytes())
        lib().oracle_prim_bounds(abi.TRIANGLE, C.byref(prim), boxes[k].ctypes.data)
    v = tris["vertex"].astype(F32)
    return boxes, ((v[:, 0] + v[:, 1]) + v[:, 2]) / F32(3.0)


@dataclass
class Restated:
    boxes: np.ndarray
    cents: np.ndarray
    tree: tuple                    # lbvh_tree(boxes, cents, BLAS_LEAF): refs are 0-based within the tree
    height: int
    sorted_codes: np.ndarray


def restate(tris):
    boxes, cents = triangle_items(tris)
    tree = lbvh_tree(boxes, cents, BLAS_LEAF)
    return Restated(boxes, cents, tree, check_tree(*tree, boxes, BLAS_LEAF), np.sort(morton_codes(cents), kind="stable"))


@functools.lru_cache(maxsize=None)
def restated(kind, size):
    return restate(tree_triangles(kind, size))


def runs_across(sorted_codes, position):
    """A run of equal codes holds both sorted positions position - 1 and position."""
    return 0 < position < len(sorted_codes) and sorted_codes[position - 1] == sorted_codes[position]


# ---- rays --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def aimed_rays():
    """N_RAYS unit rays, each at a point inside a triangle of the "random" forest — the size drawn uniformly, then the
    triangle, so the small trees are aimed at as often as the large ones — from RAY_DISTANCE away in a random
    direction.  The instance transforms belong to the sizes, so the rays serve both orders; a "dup8" tree holds a subset
    of the "random" tree's triangles."""
    from oracle.oracle import OracleScene
    f = forest("random", "ascending")
    fwd = OracleScene(f.scene).instance_state()[:, 12:24].reshape(-1, 3, 4).astype(np.float64)
    g = np.random.default_rng(RAY_SEED)
    rays = np.zeros((N_RAYS, 6))
    for r in range(N_RAYS):
        k = int(g.integers(len(f.trees)))
        size, first = f.trees[k]
        v = f.scene.triangles["vertex"][first + int(g.integers(size))].astype(np.float64)
        a, b = g.uniform(0.05, 0.95, 2)
        if a + b > 1.0:
            a, b = 1.0 - a, 1.0 - b
        p = v[0] + a * (v[1] - v[0]) + b * (v[2] - v[0])
        target = fwd[k, :, :3] @ p + fwd[k, :, 3]
        d = g.normal(size=3)
        d /= np.linalg.norm(d)
        rays[r, :3] = target - RAY_DISTANCE * d
        rays[r, 3:] = d
    rays = rays.astype(F32)
    rays.setflags(write=False)
    return rays


def tree_free_trace(oracle, rays, threads=8):
    """OracleScene.trace(rays, brute_force=2) — every primitive of every instance, gated by its own box, no tree — with
    the rays split over `threads` (the oracle's trace reads the scene only; ctypes drops the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    parts = np.array_split(np.arange(rays.shape[0]), threads)
    with ThreadPoolExecutor(threads) as pool:
        out = list(pool.map(lambda idx: oracle.trace(rays[idx], brute_force=2)[0], parts))
    return np.concatenate(out)


# ---- TLAS sizes --------------------------------------------------------------------------------------------------------
def tlas_scene(K, kind):
    """One sphere (radius 0.5) under K instances.  "random": distinct shifts in a 40-unit cube, every fifth instance
    with a non-uniform scale and a rotation; "lattice": shifts on a 4 x 4 x 4 grid and one of three uniform scales, so
    centroids are exactly equal in groups of K / 64 while the boxes are not all the same."""
    g = np.random.default_rng([53, K])
    inst = []
    for i in range(K):
        if kind == "random":
            d = dict(shift=tuple(float(x) for x in g.uniform(-20.0, 20.0, 3)))
            if i % 5 == 0:
                d["scale"] = tuple(float(x) for x in g.uniform(0.5, 2.0, 3))
                d["rotate"] = tuple(float(x) for x in g.uniform(-60.0, 60.0, 3))
        else:
            assert kind == "lattice"
            cell = g.integers(0, 4, 3)
            d = dict(shift=tuple(float(x) for x in (cell - 1.5) * 8.0), scale=(float(1 + i % 3),) * 3)
        inst.append(dict(type=abi.SPHERE, index=0, **d))
    demo = scenes.demo_scene()
    return scenes.Scene(spheres=[(abi.ROUGH, 2, (0.0, 0.0, 0.0), 0.5)], parallelograms=demo.parallelograms,
                        triangles=demo.triangles, roughs=list(ROUGHS), metals=list(METALS), instances=inst,
                        animated=False, camera=dict(TLAS_CAMERA))


def restate_tlas(records, active=None):
    """lbvh_tree over instance records (45 floats each: ..., world box at 36:42, centroid at 42:45) and its height."""
    tree = lbvh_tree(records[:, 36:42], records[:, 42:45], TLAS_LEAF, active)
    return tree, check_tree(*tree, records[:, 36:42], TLAS_LEAF)
