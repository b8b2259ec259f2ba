"""The three primitive tests where they decide, and a float64 reference for them — TEST INFRASTRUCTURE ONLY (numpy; no
GPU, no oracle).  tests/test_prim_edges_ref.py holds the oracle to this reference on the CPU; tests/test_gpu_prim_edges.py
holds the GPU to the oracle (reference trees: bit for bit) and to this reference (every other tree).

* `OBJECTS`: 16 objects, each an instance of its own, each twice — under the identity and under GENERAL (a rotation
  about all three axes times an anisotropic scale: local rays that are unnormalised and not axis-aligned): 32 instances,
  142 flat-shaded triangles, 5 spheres, 6 parallelograms, a material index of its own per primitive.  30 of them on a
  6 x 5 grid of pitch 7 with the non-round OFFSET, the objects that decide within a few float32 spacings nearest the
  origin; the two pairs that tie between instances ("co_a" / "co_b", "touch_ball" / "touch_quad") share a cell; the two
  radius-1000 spheres lie below everything (every other ray travels upwards, so that a ray that falls off its target
  meets nothing else).
* `rays()`: the classes of CLASSES, each aimed at both copies of its object; targets are float32 points of the object's
  own frame, directions have lengths in [0.5, 2] in the world (the two threshold classes "sliver_det" and "quad_ndd"
  set theirs in the object's frame).  `Rays.local`: the same rays in the object's own frame, for the conditions
  tests/test_prim_edges_ref.py asserts with the oracle's single-primitive functions.
* `evaluate()`: the three hit functions (csrc/primitives.hpp, oracle/rt_oracle.c: Triangle.cu:4-44, Sphere.cu:4-49,
  Parallelogram.cu:4-46) restated on arrays, in instance-local space, for every (ray, surface) pair — in float64 with
  float64 matrices (xform_edges_ref.m64), and, for the measurement of the margins, in float32 with the oracle's own
  inverse rows in the oracle's order of operations.  A sphere is two surfaces (near and far root).  Per pair: t and
  one slack per deciding quantity, > 0 inside the range without its 1e-6 window:
      det   |e1 . (d x e2)| - 1e-6                    bary  min(u, 1 - u, v, 1 - v, 1 - (u + v)); alpha, beta alike
      ndd   |n . d| - 1e-6                            disc  (b^2 - 4 a c) / (4 a r^2)
      den   |u x v|^2 - 1e-6                          tmin  t - 0.001
      box   the hit's distance inside the q-centred box the parallelogram's leaf is built from (Parallelogram.cu:48-50)
  With a margin m per class and quantity (MARGINS): a surface is *certain* where every slack > m, *possible* where
  every slack but the box's > -(1e-6 + m); the *tie set* of a ray is its possible surfaces with t <= (smallest certain
  t) + 1e-6 + m.  `judge()` holds records to that: a hit names a member of the tie set, a miss has no certain surface.

MARGINS, per class and copy, are 4 x the largest deviation of the float32 restatement from float64 on the pairs of a
class's rays with the instances they were aimed at (one more row, STRAY, for every other pair), measured on the CPU by
tests/test_prim_edges_ref.py::test_margins_are_the_measured_ones (which also holds the restatement's t to the oracle's
bit for bit); profiles/prim_edges/README.md has the measurements.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import deep_tree_ref as D
import xform_edges_ref as X
from rtamd import abi, scenes

F32 = np.float32
FZERO = 1e-6                       # FLOAT_ZERO_VALUE (Global.cuh:147)
TMIN = 0.001                       # Kernel.cu:66
PITCH = 7.0
OFFSET = (0.37, -0.21, 0.13)       # no shift component is a round number
GENERAL = ((33.0, -41.0, 67.0), (1.3, 0.8, 1.1))      # rotate (degrees), scale of every object's second copy
RAY_SEED = 717
BACK = (1.5, 3.0)                  # ray origins: this far (world units) before the target
NEAR_BACK = (0.5, 1.0)             # ... the sheet's: an edge is aimed at to a few 1e-7 of a triangle's width
BIG_R = 1000.0
BIG_TOP = (-12.0, -42.0)           # world z of the top of the two radius-1000 spheres
BIG_BACK = 20.0
QUAD_BOX_MARGIN = 5e-5             # a parallelogram is certain only where the hit lies this far inside its leaf's box
OFFSETS = (0.0, 5e-7, -5e-7, 2e-6, -2e-6)     # around t = TMIN
NEAR = 1e-2                        # deviations are measured on the pairs whose float64 slacks are all > -NEAR
KINDS = ("det", "bary", "ndd", "disc", "den", "tmin")
MOVE = 1000.0                      # the rebuild of tests/test_gpu_prim_edges.py: the sheet at x + 1000


SHEET_HUBS = [i * 9 + j for i in (1, 3, 5, 7) for j in (1, 3, 5, 7)]


# ---- geometry --------------------------------------------------------------------------------------------------------
def _sheet():
    """(vertices [81, 3], faces [128, 3]): a 9 x 9 grid over [-2, 2]^2, gently non-planar; every interior vertex is
    shared by six triangles.  Triangle.cu accepts u and v in [0, 1] with 1e-6 windows but u + v <= 1 sharply, so an
    edge ties reliably only where it is no triangle's v1-v2 edge: the 16 vertices (odd, odd) are "hubs", the first
    vertex of all six triangles around them, and the 96 edges at a hub ("spokes") are u = 0 or v = 0 edges on both
    sides.  Every other interior edge (a "rim") is the sharp edge of at least one of its triangles."""
    g = np.linspace(-2.0, 2.0, 9)
    x, y = np.meshgrid(g, g, indexing="ij")
    z = 0.08 * np.sin(1.15 * x + 0.4) * np.cos(0.85 * y - 0.2)
    v = np.stack([x, y, z], -1).reshape(-1, 3)
    f = []
    for i in range(8):
        for j in range(8):
            a, b, c, d = i * 9 + j, (i + 1) * 9 + j, i * 9 + j + 1, (i + 1) * 9 + j + 1
            f += [(a, b, d), (a, d, c)]
    f = np.asarray(f)
    for h in SHEET_HUBS:
        for k in np.flatnonzero((f == h).any(axis=1)):
            f[k] = np.roll(f[k], -int(np.flatnonzero(f[k] == h)[0]))
    return v.astype(F32), f


def _fan():
    ph = np.arange(6) * np.pi / 3.0 + 0.2
    ring = np.stack([np.cos(ph), np.sin(ph), 0.06 * (-1.0) ** np.arange(6)], 1)
    v = np.concatenate([[[0.013, -0.021, 0.11]], ring])
    return v.astype(F32), np.asarray([(0, 1 + k, 1 + (k + 1) % 6) for k in range(6)])


def _twins():
    """Two triangles on the same vertices with opposite winding and a third, coplanar, across them."""
    a, b, c = (-0.9, -0.6, 0.0), (0.8, -0.5, 0.34), (0.1, 0.9, 0.02)
    a, b, c = (np.asarray(p) for p in (a, b, c))
    e1, e2 = b - a, c - a
    third = [a + 0.6 * e1 - 0.3 * e2, a + 0.7 * e1 + 0.6 * e2, a - 0.3 * e1 + 0.5 * e2]
    v = np.stack([a, b, c] + third)
    return v.astype(F32), np.asarray([(0, 1, 2), (0, 2, 1), (3, 4, 5)])


SLIVER = 2e-3                      # |e1 x e2| = 4e-6: det = 4e-6 |d| cos


def _sliver():
    o = np.asarray([0.011, 0.023, 0.004])
    v = np.stack([o, o + [SLIVER, 0, 0], o + [0, SLIVER, 0], o + [SLIVER, SLIVER, 2e-4], o + [-SLIVER, 0, 1e-4]])
    return v.astype(F32), np.asarray([(0, 1, 2), (1, 3, 2), (0, 2, 4), (0, 4, 1)])


def _tmin_tri():
    v = np.asarray([(-0.2, -0.15, 0.02), (0.22, -0.1, -0.03), (0.01, 0.21, 0.05)])
    return v.astype(F32), np.asarray([(0, 1, 2)])


MESHES = {"sheet": _sheet, "fan": _fan, "twins": _twins, "sliver": _sliver, "tmin_tri": _tmin_tri}
#          centre, radius
SPHERES = {"ball": ((0.1, -0.2, 0.05), 1.3), "co_a": ((0.0, 0.1, 0.0), 0.9), "co_b": ((0.0, 0.1, 0.0), 0.9),
           "big": ((0.0, 0.0, 0.0), BIG_R), "touch_ball": ((-0.5, -0.5, 0.5), 0.5)}
#          q, u, v
QUADS = {"touch_quad": ((-1.0, -1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0)),
         "quad": ((-0.6, -0.5, 0.05), (1.1, 0.2, 0.1), (-0.1, 0.9, 0.25)),
         "degenerate": ((-0.3, 0.1, 0.0), (0.6, 0.2, 0.1), (0.3, 0.1, 0.05)),
         "thin_out": ((-0.25, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.9e-3, 0.0)),       # |u x v|^2 = 8.1e-7
         "thin_in": ((-0.25, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.1e-3, 0.0)),        # 1.21e-6
         "tmin_quad": ((-0.2, -0.2, 0.01), (0.4, 0.05, 0.02), (-0.03, 0.4, -0.01))}
# the objects in the order of their cells, nearest the origin first; a pair in one tuple shares a cell
CELLS = [("tmin_tri",), ("ball",), ("tmin_quad",), ("sliver",), ("thin_out",), ("thin_in",), ("quad",), ("twins",),
         ("fan",), ("sheet",), ("co_a", "co_b"), ("touch_ball", "touch_quad"), ("degenerate",)]
OBJECTS = [n for cell in CELLS for n in cell] + ["big"]
TRI_FIRST, SPHERE_INDEX, QUAD_INDEX = {}, {n: i for i, n in enumerate(SPHERES)}, {n: i for i, n in enumerate(QUADS)}
_n = 0
for _name, _f in MESHES.items():
    TRI_FIRST[_name] = _n
    _n += len(_f()[1])
N_TRIANGLES = _n


def _cells():
    """The 30 cell centres of the grid, nearest the origin first (ties: by x, then y)."""
    c = [(i * PITCH, j * PITCH) for i in range(-2, 4) for j in range(-2, 3)]
    return sorted(c, key=lambda p: (p[0] * p[0] + p[1] * p[1], p))


def place(name, copy):
    """World shift of the copy (0: identity, 1: GENERAL) of an object."""
    if name == "big":
        s = GENERAL[1] if copy else (1.0, 1.0, 1.0)
        return ((-40.0, 40.0)[copy] + OFFSET[0], OFFSET[1], BIG_TOP[copy] - BIG_R * max(s) + OFFSET[2])
    k = [i for i, cell in enumerate(CELLS) if name in cell][0]
    x, y = _cells()[2 * k + copy]
    return (x + OFFSET[0], y + OFFSET[1], OFFSET[2])


def triangles(move=0.0):
    """The scene's 142 triangles; move: the sheet's vertices at x + move (float32)."""
    t = np.zeros(N_TRIANGLES, dtype=scenes.TRIANGLE_DTYPE)
    for name, f in MESHES.items():
        v, faces = f()
        if name == "sheet" and move:
            v = (v + np.asarray([move, 0, 0], F32)).astype(F32)
        a = TRI_FIRST[name]
        t["vertex"][a:a + len(faces)] = v[faces]
    i = np.arange(N_TRIANGLES)
    t["material_type"] = np.where(i % 3 == 0, abi.METAL, abi.ROUGH)
    t["material_index"] = np.where(i % 3 == 0, (i // 3) % len(D.METALS), i % len(D.ROUGHS))
    t["has_normals"] = 0
    return t


def instance_dicts(move=0.0):
    out = []
    tris = triangles(move)
    for name in OBJECTS:
        for copy in (0, 1):
            rot, scale = GENERAL if copy else ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
            d = dict(shift=tuple(float(F32(x)) for x in place(name, copy)), rotate=rot, scale=scale, obj=name,
                     copy=copy)
            if name in MESHES:
                a, n = TRI_FIRST[name], len(MESHES[name]()[1])
                v = tris["vertex"][a:a + n].reshape(-1, 3)
                lo, hi = v.min(axis=0), v.max(axis=0)
                cen = v.astype(np.float64).mean(axis=0).astype(F32)
                d.update(type=abi.TRIANGLE, index=a, count=n, centroid=tuple(float(x) for x in cen),
                         bounds=tuple(float(x) for x in (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])))
            elif name in SPHERES:
                d.update(type=abi.SPHERE, index=SPHERE_INDEX[name])
            else:
                d.update(type=abi.PARALLELOGRAM, index=QUAD_INDEX[name])
            out.append(d)
    return out


FRAME = (128, 96)
CAMERA = dict(scenes.DEMO_CAMERA, center=(7.0, 4.0, 26.0), target=(7.0, 10.0, 0.0), fov=50.0, ray_trace_depth=3,
              sample_count=4)


def scene(move=0.0):
    """A fresh static scene (build it with update=False)."""
    sph = [(abi.ROUGH if i % 2 else abi.METAL, i % 4, c, r) for i, (c, r) in enumerate(SPHERES.values())]
    quads = [(abi.ROUGH, (i + 2) % len(D.ROUGHS)) + q for i, q in enumerate(QUADS.values())]
    return scenes.Scene(spheres=sph, parallelograms=quads, triangles=triangles(move), roughs=list(D.ROUGHS),
                        metals=list(D.METALS), instances=instance_dicts(move), animated=False, camera=dict(CAMERA))


def instance_of(name, copy):
    return 2 * OBJECTS.index(name) + copy


# ---- rays ------------------------------------------------------------------------------------------------------------
#          class: (object, rays per copy)
CLASSES = {
    "sheet_edge": ("sheet", 1000), "sheet_vertex": ("sheet", 500), "sheet_rim": ("sheet", 500),
    "sheet_boundary": ("sheet", 500),
    "fan_hub": ("fan", 500), "fan_spoke": ("fan", 500), "twins": ("twins", 400), "sliver_det": ("sliver", 800),
    "tri_tmin": ("tmin_tri", 600),
    "sph_tangent": ("ball", 800), "sph_inside": ("ball", 400), "sph_surface": ("ball", 720),
    "sph_coincident": ("co_a", 400), "sph_big": ("big", 600), "contact": ("touch_ball", 600),
    "quad_edge": ("quad", 800), "quad_ndd": ("quad", 800), "quad_boxface": ("quad", 400),
    "quad_degenerate": ("degenerate", 300), "quad_thin_out": ("thin_out", 300), "quad_thin_in": ("thin_in", 300),
    "quad_tmin": ("tmin_quad", 600),
}
NAMES = list(CLASSES)
SHEET_CLASSES = NAMES[:4]


def _unit(g, n):
    d = g.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _steep(g, normal, lo, hi=1.0):
    """Unit directions whose |cos| to the unit vectors `normal` [n, 3] is uniform in [lo, hi]."""
    n = len(normal)
    c = g.uniform(lo, hi, n)
    a = _unit(g, n)
    a -= (a * normal).sum(1, keepdims=True) * normal
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    return c[:, None] * normal + np.sqrt(1.0 - c * c)[:, None] * a


def _f32(p):
    return np.asarray(p, F32).astype(np.float64)


def sheet_edges():
    """(spokes [96, 2 vertices], their two faces [96, 2], rims [80, 2], boundary edges [32, 2])."""
    _, f = _sheet()
    faces_of = {}
    for k, tri in enumerate(f):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            faces_of.setdefault(tuple(sorted((int(tri[a]), int(tri[b])))), []).append(k)
    inner = sorted(e for e, v in faces_of.items() if len(v) == 2 and (e[0] in SHEET_HUBS or e[1] in SHEET_HUBS))
    rims = sorted(e for e, v in faces_of.items() if len(v) == 2 and e not in inner)
    outer = sorted(e for e, v in faces_of.items() if len(v) == 1)
    return np.asarray(inner), np.asarray([faces_of[e] for e in inner]), np.asarray(rims), np.asarray(outer)


def _quad_n(name):
    q, u, v = (_f32(x) for x in QUADS[name])
    n = np.cross(u, v)
    return q, u, v, n / np.linalg.norm(n)


def _class_targets(name, g, n, general, move=0.0):
    """One class in its object's own frame -> dict(p, u[, t | o], hint...): rays through the float32 points p along the
    unit directions u, from BACK before them (or, with t, from p - t d for the final d; or, with o, from o)."""
    z = np.asarray([0.0, 0.0, 1.0])
    if name.startswith("sheet"):
        v, f = _sheet()
        v = (v + np.asarray([move, 0, 0], F32)).astype(F32).astype(np.float64)     # the vertices the scene holds
        inner, inner_faces, rims, outer = sheet_edges()
        if name in ("sheet_edge", "sheet_rim"):
            inner = inner if name == "sheet_edge" else rims
            k = g.integers(len(inner), size=n)
            s = g.uniform(0.05, 0.95, (n, 1))
            p = v[inner[k, 0]] + s * (v[inner[k, 1]] - v[inner[k, 0]])
            hint = k                                                              # the edge, of sheet_edges()
        elif name == "sheet_vertex":
            hint = np.asarray(SHEET_HUBS)[g.integers(len(SHEET_HUBS), size=n)]
            p = v[hint]
        else:
            k = g.integers(len(outer), size=n)
            s = g.uniform(0.0, 1.0, (n, 1))
            s[: n // 5] = np.round(s[: n // 5])                                # a fifth at the edges' ends: corners too
            p = v[outer[k, 0]] + s * (v[outer[k, 1]] - v[outer[k, 0]])
            corner = np.asarray([0, 8, 72, 80])
            p[: n // 10] = v[corner[g.integers(4, size=n // 10)]]
            hint = k
        return dict(p=p, u=_steep(g, np.broadcast_to(z, (n, 3)), 0.3), hint=hint, back=NEAR_BACK)
    if name.startswith("fan"):
        v, _ = _fan()
        v = v.astype(np.float64)
        if name == "fan_hub":
            p, hint = np.broadcast_to(v[0], (n, 3)).copy(), np.zeros(n, int)
        else:
            hint = g.integers(6, size=n)
            p = v[0] + g.uniform(0.05, 0.95, (n, 1)) * (v[1 + hint] - v[0])
        return dict(p=p, u=_steep(g, np.broadcast_to(z, (n, 3)), 0.3), hint=hint)
    if name == "twins":
        v, _ = _twins()
        a, b, c = v[:3].astype(np.float64)
        ab = g.uniform(0.0, 1.0, (n, 2))
        ab = np.where((ab.sum(1) > 1.0)[:, None], 1.0 - ab, ab)
        p = a + ab[:, :1] * (b - a) + ab[:, 1:] * (c - a)
        nrm = np.cross(b - a, c - a)
        return dict(p=p, u=_steep(g, np.broadcast_to(nrm / np.linalg.norm(nrm), (n, 3)), 0.3))
    if name == "sliver_det":
        # det of triangle 0 = 4e-6 |d| cos: |d| cos log-uniform over [0.05, 1.25] puts det across [2e-7, 5e-6]; the
        # length is the ray's (`len`), the cosine the direction's
        v, _ = _sliver()
        a, b, c = v[:3].astype(np.float64)
        ab = g.uniform(0.25, 0.5, (n, 2)) * 0.9
        p = a + ab[:, :1] * (b - a) + ab[:, 1:] * (c - a)
        want = np.exp(g.uniform(np.log(0.05), np.log(1.25), n))
        length = np.maximum(g.uniform(0.5, 2.0, n), np.minimum(want * 1.05, 2.0))
        cos = np.minimum(want / length, 1.0)
        nrm = np.cross(b - a, c - a)
        nrm = np.broadcast_to(nrm / np.linalg.norm(nrm), (n, 3))
        return dict(p=p, u=_steep(g, nrm, cos, cos), local_len=length)
    if name == "tri_tmin":
        v, _ = _tmin_tri()
        a, b, c = v.astype(np.float64)
        ab = g.uniform(0.2, 0.4, (n, 2))
        p = a + ab[:, :1] * (b - a) + ab[:, 1:] * (c - a)
        nrm = np.cross(b - a, c - a)
        t = np.asarray([0.0] + [TMIN + o for o in OFFSETS])[np.arange(n) % 6]      # hint 0: from the surface itself
        return dict(p=p, u=_steep(g, np.broadcast_to(nrm / np.linalg.norm(nrm), (n, 3)), 0.7), t=t, hint=np.arange(n) % 6)
    if name == "quad_tmin":
        q, u, v, nrm = _quad_n("tmin_quad")
        ab = g.uniform(0.1, 0.4, (n, 2))
        t = np.asarray([0.0] + [TMIN + o for o in OFFSETS])[np.arange(n) % 6]
        return dict(p=q + ab[:, :1] * u + ab[:, 1:] * v, u=_steep(g, np.broadcast_to(nrm, (n, 3)), 0.7), t=t,
                    hint=np.arange(n) % 6)
    if name.startswith("sph") or name == "contact":
        obj = CLASSES[name][0]
        c, r = np.asarray(SPHERES[obj][0], np.float64), SPHERES[obj][1]
        nh = _unit(g, n)
        if name == "sph_tangent":
            return dict(p=c + r * nh, u=_steep(g, nh, 0.0, 0.0))
        if name == "sph_inside":
            return dict(o=c + r * g.uniform(0.0, 0.95, (n, 1)) * nh, u=_unit(g, n), p=None)
        if name == "sph_surface":
            # hint k: t = (0, TMIN + OFFSETS)[k % 6]; k // 6 = 0: from outside inwards, 1: from inside outwards
            k = np.arange(n) % 12
            t = np.asarray([0.0] + [TMIN + o for o in OFFSETS])[k % 6]
            u = _steep(g, nh, 0.4) * np.where(k // 6 == 0, -1.0, 1.0)[:, None]
            return dict(p=c + r * nh, u=u, t=t, hint=k, keep_side=True)
        if name == "sph_coincident":
            return dict(p=c + r * g.uniform(0.0, 0.98, (n, 1)) * nh, u=_unit(g, n))
        if name == "sph_big":
            # tangent at the top of the sphere as the world sees it, passing BIG_R + h from the centre, |h| <= 0.01
            m = X.m64((0, 0, 0), *(GENERAL if general else ((0, 0, 0), (1, 1, 1))))[:3, :3]
            top = m.T @ z
            top /= np.linalg.norm(top)
            nh = top + 0.004 * _unit(g, n)
            nh /= np.linalg.norm(nh, axis=1, keepdims=True)
            h = g.uniform(-0.01, 0.01, (n, 1))
            return dict(p=c + (r + h) * nh, u=_steep(g, nh, 0.0, 0.0), back=(BIG_BACK, BIG_BACK), any_side=True)
        # contact: at the point where the ball rests on the parallelogram, and within 0.03 of it
        touch = c - [0.0, 0.0, r]
        p = touch + np.concatenate([g.normal(0.0, 0.01, (n, 2)), np.zeros((n, 1))], 1)
        p[: n // 4] = touch
        return dict(p=p, u=_steep(g, np.broadcast_to(z, (n, 3)), 0.2))
    obj = CLASSES[name][0]
    q, u, v, nrm = _quad_n(obj) if obj != "degenerate" else (*(_f32(x) for x in QUADS[obj]), z)
    nb = np.broadcast_to(nrm, (n, 3))
    if name == "quad_edge":
        # hint 0-3: the edges alpha = 0, alpha = 1, beta = 0, beta = 1; 4-7: the corners
        k = np.arange(n) % 8
        s = g.uniform(0.02, 0.98, n)
        al = np.select([k == 0, k == 1, k == 4, k == 5, k == 6, k == 7], [0.0, 1.0, 0.0, 1.0, 0.0, 1.0], s)
        be = np.select([k == 2, k == 3, k == 4, k == 5, k == 6, k == 7], [0.0, 1.0, 0.0, 0.0, 1.0, 1.0], s)
        return dict(p=q + al[:, None] * u + be[:, None] * v, u=_steep(g, nb, 0.3), hint=k)
    if name == "quad_ndd":
        # n . d = |d| cos, log-uniform over [2e-7, 5e-6]; through points of the part of the parallelogram inside its box
        ab = g.uniform(0.1, 0.35, (n, 2))
        want = np.exp(g.uniform(np.log(2e-7), np.log(5e-6), n))
        length = g.uniform(0.5, 2.0, n)
        return dict(p=q + ab[:, :1] * u + ab[:, 1:] * v, u=_steep(g, nb, want / length, want / length),
                    local_len=length, back=(0.3, 0.3))
    if name == "quad_boxface":
        # on the face x = q.x + |u + v|.x / 2 of the q-centred box: alpha u.x + beta v.x = the half width
        half = 0.5 * abs(u[0] + v[0])
        be = g.uniform(0.05, 0.5, n)
        al = (half - be * v[0]) / u[0]
        return dict(p=q + al[:, None] * u + be[:, None] * v, u=_steep(g, nb, 0.3))
    if name == "quad_degenerate":
        s = g.uniform(-0.2, 1.7, (n, 1))
        return dict(p=q + s * u + g.normal(0.0, 0.01, (n, 3)), u=_unit(g, n))
    ab = np.stack([g.uniform(0.05, 0.45, n), g.uniform(0.15, 0.35, n)], 1)          # the thin pair
    return dict(p=q + ab[:, :1] * u + ab[:, 1:] * v, u=_steep(g, nb, 0.5))


@dataclass
class Rays:
    world: np.ndarray              # [R, 6] float32
    local: np.ndarray              # [R, 6] float32: the same rays in the aimed object's own frame
    cls: np.ndarray                # [R] index in NAMES
    copy: np.ndarray               # [R] 0: the identity copy, 1: the GENERAL one
    hint: np.ndarray               # [R] what the class says of its ray (see _class_targets)

    def of(self, name, copy=None):
        m = self.cls == NAMES.index(name)
        return np.flatnonzero(m if copy is None else m & (self.copy == copy))


def _rays(move, seed):
    world, local, cls, copy, hint = [], [], [], [], []
    for ci, (name, (obj, n)) in enumerate(CLASSES.items()):
        for cp in (0, 1):
            g = np.random.default_rng([seed, sum(name.encode()), cp])           # a stream of its own per class and copy
            c = _class_targets(name, g, n, cp, move)
            shift = _f32(place(obj, cp))
            m = X.m64(shift, *(GENERAL if cp else ((0, 0, 0), (1, 1, 1))))
            lin = m[:3, :3]
            u = c["u"]
            # at x + 1000 a point of an edge is no float32 point (the spacing there is 6e-5): aimed at as it is
            p = None if c["p"] is None else (c["p"] if move and obj == "sheet" else _f32(c["p"]))
            dw = u @ lin.T
            up = np.where(dw[:, 2] < 0.0, -1.0, 1.0)[:, None]                    # every ray travels upwards
            if c.get("keep_side"):                                              # ... a sphere's: mirrored in its centre
                cen = np.asarray(SPHERES[obj][0], np.float64)
                p = _f32(cen + (p - cen) * up)
            if "o" in c:
                up = 1.0
            if c.get("any_side"):
                up = 1.0
            u, dw = u * up, dw * up
            if "local_len" in c:
                d_l = u * c["local_len"][:, None]
            else:
                d_l = u * (g.uniform(0.5, 2.0, (n, 1)) / np.linalg.norm(dw, axis=1, keepdims=True))
            if "o" in c:
                o_l = c["o"]
            elif "t" in c:
                o_l = p - c["t"][:, None] * d_l
            else:
                back = c.get("back")
                dist = g.uniform(*(BACK if back is None else back), (n, 1))
                o_l = p - dist * d_l / np.linalg.norm(d_l @ lin.T, axis=1, keepdims=True)
            world.append(np.concatenate([o_l @ lin.T + m[:3, 3], d_l @ lin.T], 1))
            local.append(np.concatenate([o_l, d_l], 1))
            cls.append(np.full(n, ci))
            copy.append(np.full(n, cp))
            hint.append(np.asarray(c.get("hint", np.zeros(n, int))).reshape(n, -1)[:, 0])
    out = Rays(np.concatenate(world).astype(F32), np.concatenate(local).astype(F32), np.concatenate(cls),
               np.concatenate(copy), np.concatenate(hint))
    for a in (out.world, out.local, out.cls, out.copy, out.hint):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rays(move=0.0, seed=RAY_SEED):
    """Every class at both copies of its object: 24 640 rays (Rays).  move: the sheet at x + move."""
    return _rays(move, seed)


# ---- the hit functions on arrays -------------------------------------------------------------------------------------
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]      # Vec3.cuh:113-119, in its order


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


@dataclass
class Surfaces:
    """Surface s of a scene: its instance, primitive type and index, and 1 for a sphere's far root."""
    inst: np.ndarray
    ptype: np.ndarray
    pindex: np.ndarray
    far: np.ndarray


def surfaces(sc):
    inst, ptype, pindex, far = [], [], [], []
    for k, d in enumerate(sc.instances):
        n = d.get("count", 1) if d["type"] == abi.TRIANGLE else 1
        for rep in range(2 if d["type"] == abi.SPHERE else 1):
            inst += [k] * n
            ptype += [d["type"]] * n
            pindex += list(range(d["index"], d["index"] + n))
            far += [rep] * n
    return Surfaces(*(np.asarray(x) for x in (inst, ptype, pindex, far)))


@dataclass
class Evaluation:
    surf: Surfaces
    t: np.ndarray                  # [R, S] float64 (nan or inf where the arithmetic gives no t)
    certain: np.ndarray            # [R, S]
    possible: np.ndarray           # [R, S]
    m_t: np.ndarray                # [R, S]: the margin of t of the pair
    deviation: dict                # with the oracle's state: {class: {kind, "t": largest |float32 - float64|}}
    t32: np.ndarray                # with the oracle's state: the float32 restatement's t [R, S]


def _local(rays, inv, dtype):
    """Origins and directions [R, 3] of `rays` in the frame whose inverse rows are inv [3, 4] (Instance.cu:19-27), in
    the oracle's order of operations."""
    r = rays.astype(dtype)
    o = np.stack([inv[i, 0] * r[:, 0] + inv[i, 1] * r[:, 1] + inv[i, 2] * r[:, 2] + inv[i, 3] for i in range(3)], 1)
    d = np.stack([inv[i, 0] * r[:, 3] + inv[i, 1] * r[:, 4] + inv[i, 2] * r[:, 5] for i in range(3)], 1)
    return o, d


def _instance(sc, d, o, dr, dtype):
    """(t [R, n], slacks {kind: [R, n]}) of one instance's n surfaces for local rays (o, dr) of `dtype`."""
    one, tmin, fz = dtype(1.0), dtype(TMIN), dtype(FZERO)
    with np.errstate(all="ignore"):
        if d["type"] == abi.TRIANGLE:
            v = sc.triangles["vertex"][d["index"]:d["index"] + d["count"]].astype(dtype)
            e1, e2, v0 = (v[:, 1] - v[:, 0])[None], (v[:, 2] - v[:, 0])[None], v[None, :, 0]
            dd, oo = dr[:, None, :], o[:, None, :]
            h = _cross(dd, e2)
            det = _dot(e1, h)
            s = oo - v0
            u = _dot(s, h) / det
            q = _cross(s, e1)
            vv = _dot(dd, q) / det
            t = _dot(e2, q) / det
            bary = np.minimum(np.minimum(np.minimum(u, one - u), np.minimum(vv, one - vv)), one - (u + vv))
            return t, dict(det=np.abs(det) - fz, bary=bary, tmin=t - tmin)
        if d["type"] == abi.SPHERE:
            _, _, c, r = sc.spheres[d["index"]]
            c, r = np.asarray(c, F32).astype(dtype), dtype(F32(r))
            cq = c[None] - o
            a = _dot(dr, dr)
            b = dtype(-2.0) * _dot(cq, dr)
            cc = _dot(cq, cq) - r * r
            delta = b * b - dtype(4.0) * a * cc
            sq = np.sqrt(np.maximum(delta, dtype(0.0)))                      # below 0: the tangent point (disc decides)
            t = np.stack([(-b - sq) / (a * dtype(2.0)), (-b + sq) / (a * dtype(2.0))], 1)
            disc = (delta.astype(np.float64) / (4.0 * a.astype(np.float64) * float(r) ** 2))[:, None]
            return t, dict(disc=np.concatenate([disc, disc], 1), tmin=t - tmin)
        _, _, q, u, v = sc.parallelograms[d["index"]]
        q, u, v = (np.asarray(x, F32).astype(dtype) for x in (q, u, v))
        cr = _cross(u, v)
        den = _dot(cr, cr)
        n = cr * (one / np.sqrt(den))                                             # Parallelogram.cuh:26-39, vunit
        gd = n[0] * q[0] + n[1] * q[1] + n[2] * q[2]
        ndd = _dot(n[None], dr)
        ndp = n[0] * o[:, 0] + n[1] * o[:, 1] + n[2] * o[:, 2]
        t = (gd - ndp) / ndd
        p = (o + dr * t[:, None]) - q[None]
        al = _dot(_cross(p, v[None]), cr[None]) / den
        be = _dot(_cross(u[None], p), cr[None]) / den
        bary = np.minimum(np.minimum(al, one - al), np.minimum(be, one - be))
        half = np.abs((u + v) * dtype(0.5))
        box = np.where(half[None] > 0, half[None] - np.abs(p), np.inf).min(axis=1)  # the flat axes: by the hit itself
        return t[:, None], dict(ndd=(np.abs(ndd) - fz)[:, None], bary=bary[:, None], tmin=(t - tmin)[:, None],
                                den=(np.abs(den) - fz) * np.ones((len(o), 1)), box=box[:, None])


def own_instances(r):
    """[R, instances] bool: the instances ray r was aimed at — its class's object, and the one that shares its cell, in
    the ray's copy.  Every other instance is a stray's: judged with the margins of STRAY."""
    own = np.zeros((len(r.cls), 2 * len(OBJECTS)), bool)
    for ci, name in enumerate(NAMES):
        cell = [c for c in CELLS + [("big",)] if CLASSES[name][0] in c][0]
        for cp in (0, 1):
            sel = (r.cls == ci) & (r.copy == cp)
            for obj in cell:
                own[sel, instance_of(obj, cp)] = True
    return own


STRAY = "stray"


def evaluate(sc, r, margins=None, state=None, chunk=4096):
    """The Evaluation of the Rays `r` against every surface of the scene.  state: the oracle's instance_state(); with it
    the float32 restatement runs beside float64 and its deviations are measured (margins may then be all zero)."""
    margins = MARGINS if margins is None else margins
    world, cls = r.world, r.cls
    surf = surfaces(sc)
    S, R = len(surf.inst), len(world)
    own = own_instances(r)
    m_own = {k: np.asarray([[margins[n][cp][k] for cp in (0, 1)] for n in NAMES])[cls, r.copy] for k in KINDS + ("t",)}
    inv64 = [np.linalg.inv(X.instance_m64(d))[:3] for d in sc.instances]
    t_all = np.full((R, S), np.inf)
    m_t = np.zeros((R, S))
    t32_all = np.full((R, S), np.inf, F32) if state is not None else None
    certain, possible = np.zeros((R, S), bool), np.zeros((R, S), bool)
    dev = {n: [dict.fromkeys(KINDS + ("t",), 0.0) for _ in (0, 1)] for n in NAMES}
    dev[STRAY] = dict.fromkeys(KINDS + ("t",), 0.0)
    for a in range(0, R, chunk):
        w = world[a:a + chunk]
        col = 0
        for k, d in enumerate(sc.instances):
            o, dr = _local(w, inv64[k], np.float64)
            t, sl = _instance(sc, d, o, dr, np.float64)
            n = t.shape[1]
            mine = own[a:a + chunk, k]
            cer, pos = np.ones(t.shape, bool), np.ones(t.shape, bool)
            with np.errstate(invalid="ignore"):
                for kind, s in sl.items():
                    if kind == "box":
                        cer &= s > QUAD_BOX_MARGIN
                        continue
                    mk = np.where(mine, m_own[kind][a:a + chunk], margins[STRAY][kind])[:, None]
                    cer &= s > mk
                    pos &= s > -(FZERO + mk)
            t_all[a:a + chunk, col:col + n] = t
            m_t[a:a + chunk, col:col + n] = np.where(mine, m_own["t"][a:a + chunk], margins[STRAY]["t"])[:, None]
            certain[a:a + chunk, col:col + n] = cer
            possible[a:a + chunk, col:col + n] = pos
            if state is not None:
                o32, d32 = _local(w, state[k, :12].reshape(3, 4).astype(F32), F32)
                t32, sl32 = _instance(sc, d, o32, d32, F32)
                t32_all[a:a + chunk, col:col + n] = t32
                with np.errstate(invalid="ignore"):
                    near = np.all([s > -NEAR for kind, s in sl.items() if kind != "box"], axis=0)
                    for kind in list(sl) + ["t"]:
                        if kind == "box":
                            continue
                        x64, x32 = (t, t32) if kind == "t" else (sl[kind], sl32[kind])
                        diff = np.where(near, np.abs(x32.astype(np.float64) - x64), 0.0)
                        diff = np.where(np.isfinite(diff), diff, 0.0).max(axis=1)
                        if (~mine).any():
                            dev[STRAY][kind] = max(dev[STRAY][kind], float(diff[~mine].max()))
                        for ci in np.unique(cls[a:a + chunk][mine]):
                            for cp in (0, 1):
                                sel = mine & (cls[a:a + chunk] == ci) & (r.copy[a:a + chunk] == cp)
                                if sel.any():
                                    dev[NAMES[ci]][cp][kind] = max(dev[NAMES[ci]][cp][kind], float(diff[sel].max()))
            col += n
    return Evaluation(surf, t_all, certain, possible, m_t, dev, t32_all)


def record64(sc, world, ev, chosen):
    """(point [R, 3], normal [R, 3]) in the world of surface chosen[r] of ray r, float64: the point on the ray at the
    surface's t; the flat, radial or plane normal, turned to face the local ray (Triangle.cu:36-42, Sphere.cu:40-46,
    Parallelogram.cu:38-44), under the instance's inverse transpose, unit (Instance.cu:40-48)."""
    world = np.asarray(world, np.float64)
    point, normal = np.zeros((len(world), 3)), np.zeros((len(world), 3))
    for k, d in enumerate(sc.instances):
        sel = np.flatnonzero(ev.surf.inst[chosen] == k)
        if not len(sel):
            continue
        fwd = X.instance_m64(d)
        inv = np.linalg.inv(fwd)
        o, dr = _local(world[sel], inv[:3], np.float64)
        pl = o + dr * ev.t[sel, chosen[sel]][:, None]
        if d["type"] == abi.TRIANGLE:
            v = sc.triangles["vertex"][ev.surf.pindex[chosen[sel]]].astype(np.float64)
            n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        elif d["type"] == abi.SPHERE:
            n = pl - np.asarray(sc.spheres[d["index"]][2], F32).astype(np.float64)
        else:
            _, _, q, u, v = sc.parallelograms[d["index"]]
            n = np.broadcast_to(np.cross(_f32(u), _f32(v)), pl.shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            n = n / np.linalg.norm(n, axis=1, keepdims=True)
            n = np.where(((dr * n).sum(1) < 0.0)[:, None], n, -n)
            nw = n @ inv[:3, :3]                                                  # rows: (M^-T n)^T = n^T M^-1
            normal[sel] = nw / np.linalg.norm(nw, axis=1, keepdims=True)
        point[sel] = pl @ fwd[:3, :3].T + fwd[:3, 3]
    return point, normal


@dataclass
class Verdict:
    ok: np.ndarray                 # [R]: a hit names a member of the tie set; a miss has no certain surface
    chosen: np.ndarray             # [R]: the named member whose t64 is nearest the record's t (-1: none, or a miss)
    tie: np.ndarray                # [R, S]
    may_miss: np.ndarray           # [R]


def judge(ev, got):
    """Records `got` (rt_hit fields) against the Evaluation's tie sets."""
    rr = np.arange(len(ev.t))
    with np.errstate(invalid="ignore"):
        tcs = np.where(ev.certain, ev.t, np.inf)
        first = np.argmin(tcs, axis=1)
        tie = ev.possible & (ev.t <= (tcs[rr, first] + FZERO + ev.m_t[rr, first])[:, None] + ev.m_t)
    may_miss = ~ev.certain.any(axis=1)
    hit = got["instance"] != abi.MISS
    s = ev.surf
    named = (got["instance"][:, None] == s.inst[None]) & (got["ptype"][:, None] == s.ptype[None]) & \
        (got["pindex"][:, None] == s.pindex[None]) & tie
    with np.errstate(invalid="ignore"):
        gap = np.where(named, np.abs(ev.t - got["t"].astype(np.float64)[:, None]), np.inf)
    chosen = np.where(named.any(axis=1), np.argmin(gap, axis=1), -1)
    ok = np.where(hit, chosen >= 0, may_miss)
    return Verdict(ok, np.where(hit, chosen, -1), tie, may_miss)


# 4 x the measurements of tests/test_prim_edges_ref.py::test_margins_are_the_measured_ones (profiles/prim_edges/README.md),
# per class [identity copy, GENERAL copy]; STRAY: the pairs of a ray with an instance it was not aimed at
MARGIN_KEYS = KINDS + ("t", "point", "normal")
#                      det      bary     ndd      disc     den      tmin     t        point    normal
_TABLE = {
    "sheet_edge": [(2e-07, 1.2e-06, 1e-08, 1e-08, 1e-08, 1.2e-06, 1e-06, 2.5e-06, 3.9e-07),
                   (4.3e-07, 3.5e-05, 1e-08, 1e-08, 1e-08, 2.8e-05, 2.7e-05, 1.8e-05, 6.5e-07)],
    "sheet_vertex": [(2.1e-07, 1.1e-06, 1e-08, 1e-08, 1e-08, 1.7e-06, 1.5e-06, 2.4e-06, 4.2e-07),
                     (4.8e-07, 4.9e-05, 1e-08, 1e-08, 1e-08, 2.4e-05, 2.4e-05, 1.8e-05, 5.2e-07)],
    "sheet_rim": [(1.7e-07, 1.6e-06, 1e-08, 1e-08, 1e-08, 9.9e-07, 8.9e-07, 2.5e-06, 4.1e-07),
                  (4.9e-07, 3.9e-05, 1e-08, 1e-08, 1e-08, 2.3e-05, 2.3e-05, 1.6e-05, 6.5e-07)],
    "sheet_boundary": [(1.9e-07, 1.3e-06, 1e-08, 1e-08, 1e-08, 1.4e-06, 1.6e-06, 2.5e-06, 4.4e-07),
                       (4.3e-07, 3.3e-05, 1e-08, 1e-08, 1e-08, 2.1e-05, 2.1e-05, 1.6e-05, 5.2e-07)],
    "fan_hub": [(1.1e-06, 4.1e-06, 1e-08, 1e-08, 1e-08, 5.1e-06, 5.4e-06, 3.6e-06, 3.6e-07),
                (1.4e-06, 2.1e-05, 1e-08, 1e-08, 1e-08, 2e-05, 1.9e-05, 1.3e-05, 5.2e-07)],
    "fan_spoke": [(9.9e-07, 2.6e-06, 1e-08, 1e-08, 1e-08, 3.3e-06, 3.6e-06, 3.3e-06, 3.8e-07),
                  (1.2e-06, 2e-05, 1e-08, 1e-08, 1e-08, 1.9e-05, 1.8e-05, 1.3e-05, 6.3e-07)],
    "twins": [(2.5e-06, 1.3e-06, 1e-08, 1e-08, 1e-08, 4.6e-06, 4.3e-06, 2.9e-06, 4.2e-07),
              (3.3e-06, 9e-06, 1e-08, 1e-08, 1e-08, 1.6e-05, 1.5e-05, 1.3e-05, 5.7e-07)],
    "sliver_det": [(1e-08, 0.0041, 1e-08, 1e-08, 1e-08, 3.3e-06, 3e-06, 2.6e-06, 1e-08),
                   (1e-08, 0.026, 1e-08, 1e-08, 1e-08, 3e-05, 3e-05, 8.1e-06, 3.7e-07)],
    "tri_tmin": [(2.2e-07, 7.3e-07, 1e-08, 1e-08, 1e-08, 2.6e-08, 2.6e-08, 7e-08, 1.7e-07),
                 (1.8e-07, 8.1e-06, 1e-08, 1e-08, 1e-08, 5.3e-06, 5.3e-06, 2.7e-06, 4.4e-07)],
    "sph_tangent": [(1e-08, 1e-08, 1e-08, 8.6e-06, 1e-08, 0.0076, 0.0076, 0.005, 8),
                    (1e-08, 1e-08, 1e-08, 1.2e-05, 1e-08, 0.012, 0.012, 0.0078, 8)],
    "sph_inside": [(1e-08, 1e-08, 1e-08, 7e-07, 1e-08, 1.4e-06, 1.3e-06, 2.3e-06, 8.4e-07),
                   (1e-08, 1e-08, 1e-08, 3.7e-06, 1e-08, 6.9e-06, 7e-06, 6.4e-06, 4.2e-06)],
    "sph_surface": [(1e-08, 1e-08, 1e-08, 1.1e-06, 1e-08, 3.2e-06, 2.9e-06, 2.6e-06, 8.8e-07),
                    (1e-08, 1e-08, 1e-08, 4.3e-06, 1e-08, 9.6e-06, 9.6e-06, 6.1e-06, 4.8e-06)],
    "sph_coincident": [(1e-08, 1e-08, 1e-08, 1.6e-05, 1e-08, 1.3e-05, 1.2e-05, 8.2e-06, 5.8e-06),
                       (1e-08, 1e-08, 1e-08, 1.9e-05, 1e-08, 2.7e-05, 2.7e-05, 1.6e-05, 1.9e-05)],
    "sph_big": [(1e-08, 1e-08, 1e-08, 4.4e-07, 1e-08, 0.65, 0.65, 1.1, 0.0011),
                (1e-08, 1e-08, 1e-08, 1.1e-06, 1e-08, 1.8, 1.8, 1.4, 0.0018)],
    "contact": [(1e-08, 4.3e-07, 1.9e-07, 4e-05, 1.9e-07, 2.9e-05, 3e-05, 1.1e-05, 2.5e-05),
                (1e-08, 9.3e-06, 1.2e-06, 5.3e-05, 1.9e-07, 5.1e-05, 5.2e-05, 4.3e-05, 0.00013)],
    "quad_edge": [(1e-08, 1.9e-06, 6.7e-07, 1e-08, 2.3e-08, 3e-06, 2.8e-06, 2.8e-06, 4e-07),
                  (1e-08, 1.6e-05, 1.1e-06, 1e-08, 2.3e-08, 1.9e-05, 1.9e-05, 1.3e-05, 2.2e-07)],
    "quad_ndd": [(1e-08, 0.66, 2.8e-07, 1e-08, 2.3e-08, 0.58, 0.58, 0.13, 4e-07),
                 (1e-08, 24, 7.5e-07, 1e-08, 2.3e-08, 21, 21, 3.4, 2.2e-07)],
    "quad_boxface": [(1e-08, 2e-06, 5.8e-07, 1e-08, 2.3e-08, 2.6e-06, 2.3e-06, 3.3e-06, 4e-07),
                     (1e-08, 1.8e-05, 9.9e-07, 1e-08, 2.3e-08, 1.8e-05, 1.8e-05, 1.3e-05, 2.2e-07)],
    "quad_degenerate": [(1e-08, 1e-08, 1e-08, 1e-08, 1e-08, 1e-08, 1e-08, 1e-08, 1e-08),
                        (1e-08, 1e-08, 1e-08, 1e-08, 1e-08, 1e-08, 1e-08, 1e-08, 1e-08)],
    "quad_thin_out": [(1e-08, 0.00072, 2.9e-07, 1e-08, 1e-08, 2.4e-06, 2.2e-06, 1e-08, 1e-08),
                      (1e-08, 0.022, 1.4e-06, 1e-08, 1e-08, 1.6e-05, 1.6e-05, 1e-08, 1e-08)],
    "quad_thin_in": [(1e-08, 0.00044, 1.9e-07, 1e-08, 1e-08, 2.1e-06, 1.8e-06, 2.2e-06, 1e-08),
                     (1e-08, 0.011, 9.4e-07, 1e-08, 1e-08, 6.6e-06, 6.3e-06, 1.1e-05, 3.7e-07)],
    "quad_tmin": [(1e-08, 2.4e-07, 7.2e-07, 1e-08, 1e-08, 1.7e-08, 1.7e-08, 9.8e-07, 7e-08),
                  (1e-08, 9.8e-06, 1e-06, 1e-08, 1e-08, 7.6e-06, 7.6e-06, 3.7e-06, 5.5e-07)],
    STRAY: (1.4e-06, 3e-05, 6.5e-07, 0.00085, 1.9e-07, 0.021, 0.021, 0.00075, 0.00033),
}
_TABLE_MOVED = {               # the sheet's classes with the sheet at x + MOVE
    "sheet_edge": [(2e-07, 5.4e-05, 1e-08, 1e-08, 1e-08, 7.3e-06, 7.4e-06, 0.00012, 4.3e-07),
                   (4.3e-07, 0.0026, 1e-08, 1e-08, 1e-08, 0.002, 0.002, 0.0015, 6.5e-07)],
    "sheet_vertex": [(2.1e-07, 5.2e-05, 1e-08, 1e-08, 1e-08, 7.9e-06, 8.1e-06, 0.00012, 4.2e-07),
                     (4.8e-07, 0.0034, 1e-08, 1e-08, 1e-08, 0.0025, 0.0025, 0.0011, 6.5e-07)],
    "sheet_rim": [(1.7e-07, 4.9e-05, 1e-08, 1e-08, 1e-08, 8.3e-06, 8.5e-06, 0.00012, 4.3e-07),
                  (4.9e-07, 0.0031, 1e-08, 1e-08, 1e-08, 0.0018, 0.0018, 0.001, 5.3e-07)],
    "sheet_boundary": [(1.9e-07, 4.6e-05, 1e-08, 1e-08, 1e-08, 6.7e-06, 6.6e-06, 0.00012, 4.3e-07),
                       (4.3e-07, 0.0022, 1e-08, 1e-08, 1e-08, 0.0016, 0.0016, 0.00088, 4.8e-07)],
}
MARGINS = {n: [dict(zip(MARGIN_KEYS, row)) for row in rows] for n, rows in _TABLE.items() if n != STRAY}
MARGINS[STRAY] = dict(zip(MARGIN_KEYS, _TABLE[STRAY]))
MARGINS_MOVED = {n: [dict(zip(MARGIN_KEYS, row)) for row in rows] for n, rows in _TABLE_MOVED.items()}


def margins(move=0.0):
    return dict(MARGINS, **MARGINS_MOVED) if move else MARGINS
