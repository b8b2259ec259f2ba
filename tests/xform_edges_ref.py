"""Instance transforms at their edges, and a float64 reference for them — TEST INFRASTRUCTURE ONLY (numpy; no GPU, no
oracle).  tests/test_oracle_xform_edges.py holds the oracle to this reference on the CPU; tests/test_gpu_xform_edges.py
holds the GPU to the oracle.

* `CLASSES`: 22 transforms (rotate in degrees, scale) in four groups.  "regular": identity, quarter and half turns
  (axis components that cos(90 deg) leaves at +-4e-8, pivot patterns other than rotate-x 90's one row swap, negative
  pivots), wrapped and generic angles, three mirrors (determinant < 0), two anisotropic scales (an inverse transpose
  that is no rotation times a scalar).  "scaled": uniform 1e-3 and 1e3 (local directions of length 1e3 and 1e-3).
  "stress": still inverted, but at the reference's absolute 1e-6 thresholds.  "singular": both exits of the reference's
  elimination (Matrix.cu:5-68; a pivot below 1e-6), after which Matrix::inverse returns the matrix itself.
* `scene()`: per class one mesh (a 64-triangle UV sphere of radius 0.5 — two stacks: a double cone — with vertex
  normals and given bounds / centroid, its own copy of the triangles and so its own BLAS), one sphere and one
  parallelogram under that transform: 66 instances, 1 408 triangles.  63 of them side by side on a 9 x 7 grid of pitch 8
  centred on the origin, in the plane z = 0.13, a class's three in one row with its mesh in the middle; "huge" alone at
  z = -5000.  The classes whose objects are only some float32 spacings wide stand in the row through the origin.
* `rays()`: 400 per instance, each through the world image of a point inside the instance's primitive (inside the
  mesh, inside the ball, on the parallelogram inside its q-centred box), in a uniformly random direction, from 4 x the
  instance's world extent away.  Only "tiny", "small" and "near_singular" (NARROW) are aimed more closely — inside a
  triangle, 0.15 (barycentric) from its edges, meeting the surface at |cos| >= 0.2: aimed freely, 1 % of the rays at
  scale 1e-3 and 29 % at 1e-4 (a mesh 50 float32 spacings wide) fall on the other side of an edge in float32 than in
  float64, which says nothing about a transform.
* `axis_rays()`: rays along the world axes at the quarter- and half-turn classes: in the instance's frame they have
  the components of +-4e-8 (or 1e-7) that cos 90 deg leaves, under the reference's 1e-6 "parallel" threshold.
* `m64()`, `closest64()`: the forward matrix and the closest hit in float64, from the float32 inputs, with the
  acceptance rules of the reference's primitives (csrc/primitives.hpp, oracle/rt_oracle.c: absolute 1e-6 windows,
  range [0.001, inf)), singular instances left out; `ambiguous` marks rays another rounding may decide otherwise.
"""
from __future__ import annotations

import functools

import numpy as np

import deep_tree_ref as D
from rtamd import abi, scenes

F32 = np.float32
FZERO = 1e-6                       # FLOAT_ZERO_VALUE (Global.cuh:147)
TMIN = 0.001                       # Kernel.cu:66
PITCH = 8.0
OFFSET = (0.37, -0.21, 0.13)       # no shift component is a round number
HUGE_Z = -5000.0
HUGE_PITCH = 2000.0
RADIUS = 0.5
MESH_TRIANGLES = 64
N_PER_INSTANCE = 400
RAY_SEED = 606
FAR = 4.0                          # ray origins: FAR x the instance's world extent from the target ...
EXTENT_FLOOR = 0.0025              # ... and never nearer than 10 TMIN (the classes of scale <= 1e-3)
NARROW = ("tiny", "small", "near_singular")     # objects a few float32 spacings wide where they stand: aimed closely
EDGE_MARGIN = 0.15                 # their mesh targets: this far (barycentric) from their triangle's edges
GRAZE = 0.2                        # |cos| between their rays and the normal of the surface aimed at: at least this
QUAD = ((-0.3, -0.25, 0.05), (0.9, 0.1, 0.1), (0.2, 0.7, -0.2))    # q, u, v; its box is q +- (0.55, 0.4, 0.05)
QUAD_BOX_MARGIN = 1e-4             # a hit this near a face of the q-centred box (Parallelogram.cu:48-50) is ambiguous
CAMERA = dict(scenes.DEMO_CAMERA, center=(0.3, 0.2, 75.0), target=(0.0, 0.0, 0.0), fov=60.0, ray_trace_depth=3)
FRAME = (192, 128)                 # fov is the horizontal one: +-43.3 by +-28.9 in the grid's plane
FRAMES = 6                         # of instances moving between classes


def _3(x):
    return tuple(float(v) for v in (x if isinstance(x, tuple) else (x, x, x)))


#         name            rotate (degrees)          scale               group
CLASSES = {
    "identity":      ((0, 0, 0),                1,                  "regular"),
    "rot90y":        ((0, 90, 0),               1,                  "regular"),
    "rot90z":        ((0, 0, 90),               1,                  "regular"),
    "rot90xyz":      ((90, 90, 90),             1,                  "regular"),
    "rot180x":       ((180, 0, 0),              1,                  "regular"),
    "rot270y":       ((0, 270, 0),              1,                  "regular"),
    "rotm90x":       ((-90, 0, 0),              1,                  "regular"),
    "rot45":         ((45, 45, 45),             1,                  "regular"),
    "rot_wrap":      ((720.5, -360, 1e-5),      1,                  "regular"),
    "rot_gen":       ((123.4, -77.7, 201.3),    1,                  "regular"),
    "mirror_x":      ((0, 0, 0),                (-1, 1, 1),         "regular"),
    "mirror_all":    ((10, 20, 30),             (-1, -1, -1),       "regular"),
    "mirror_aniso":  ((30, 40, 50),             (1, -2, 0.5),       "regular"),
    "aniso":         ((30, 40, 50),             (10, 0.1, 1),       "regular"),
    "flat":          ((0, 0, 0),                (1, 0.01, 1),       "regular"),
    "tiny":          ((20, 30, 40),             1e-3,               "scaled"),
    "huge":          ((20, 30, 40),             1e3,                "scaled"),
    "near_singular": ((0, 0, 0),                (2e-6, 1, 1),       "stress"),
    "small":         ((0, 0, 0),                1e-4,               "stress"),
    "sing_x0":       ((0, 0, 0),                (0, 1, 1),          "singular"),
    "sing_1e-7":     ((0, 0, 0),                (1e-7, 1, 1),       "singular"),
    "sing_all0":     ((0, 0, 0),                (0, 0, 0),          "singular"),
}
CLASSES = {k: (_3(tuple(r)), _3(s), g) for k, (r, s, g) in CLASSES.items()}
NAMES = list(CLASSES)
GROUPS = ("regular", "scaled", "stress", "singular")
PER_CLASS = 3                      # mesh, sphere, parallelogram
N_INSTANCES = PER_CLASS * len(NAMES)


def group_of(name):
    return CLASSES[name][2]


# the grid's 7 rows of three classes, bottom to top: the classes whose objects are a few float32 spacings wide where
# they stand ("tiny", "small", "near_singular") in the row through the origin, where the spacing is smallest
GRID = [n for n in CLASSES if CLASSES[n][2] == "regular"]
GRID = GRID[:9] + ["tiny", "small", "near_singular"] + GRID[9:] + [n for n in CLASSES if CLASSES[n][2] == "singular"]
CELL = (1, 0, 2)                   # within a class's three cells: the mesh in the middle


def place(k):
    """The shift of instance k (its class's slot: instance k // 3 of NAMES, primitive k % 3)."""
    c, j = divmod(k, PER_CLASS)
    if NAMES[c] == "huge":
        return ((CELL[j] - 1) * HUGE_PITCH + OFFSET[0], OFFSET[1], HUGE_Z + OFFSET[2])
    g = GRID.index(NAMES[c])
    row, col = g // 3, (g % 3) * PER_CLASS + CELL[j]
    return ((col - 4) * PITCH + OFFSET[0], (row - 3) * PITCH + OFFSET[1], OFFSET[2])


@functools.lru_cache(maxsize=None)
def mesh():
    """(vertices [V, 3] float32, faces [64, 3], vertex normals [V, 3] float32) of the local mesh."""
    verts, faces = scenes.uv_sphere_template(MESH_TRIANGLES)
    vn = scenes._vertex_normals(verts, faces)
    return (verts * RADIUS).astype(F32), faces, vn.astype(F32)


def instance_dicts(assign=None):
    """The 66 instance descriptions; assign[k] (default k // 3) is the index in NAMES of the class whose rotation and
    scale instance k takes.  Primitive and shift belong to k."""
    verts, faces, _ = mesh()
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    cen = verts.astype(np.float64).mean(axis=0).astype(F32)
    out = []
    for k in range(N_INSTANCES):
        name = NAMES[k // PER_CLASS if assign is None else int(assign[k])]
        rot, scale, _ = CLASSES[name]
        d = dict(shift=place(k), rotate=rot, scale=scale, cls=name)
        if k % PER_CLASS == 0:
            d.update(type=abi.TRIANGLE, index=(k // PER_CLASS) * MESH_TRIANGLES, count=MESH_TRIANGLES,
                     bounds=tuple(float(x) for x in (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])),
                     centroid=tuple(float(x) for x in cen))
        else:
            d.update(type=abi.SPHERE if k % PER_CLASS == 1 else abi.PARALLELOGRAM, index=0)
        out.append(d)
    return out


def scene(metal=False, assign=None):
    """A fresh scene.  metal: every surface a mirror (frames then carry the normals on into the next segments)."""
    verts, faces, vn = mesh()
    one = np.zeros(MESH_TRIANGLES, dtype=scenes.TRIANGLE_DTYPE)
    one["vertex"] = verts[faces]
    one["normal"] = vn[faces]
    one["has_normals"] = 1
    tris = np.tile(one, len(NAMES))
    i = np.arange(len(tris))
    tris["material_type"] = abi.METAL if metal else abi.ROUGH
    tris["material_index"] = i % (len(D.METALS) if metal else len(D.ROUGHS))
    mt = abi.METAL if metal else abi.ROUGH
    return scenes.Scene(spheres=[(mt, 1, (0.0, 0.0, 0.0), RADIUS)], parallelograms=[(mt, 2) + QUAD], triangles=tris,
                        roughs=list(D.ROUGHS), metals=list(D.METALS), instances=instance_dicts(assign), animated=False,
                        camera=dict(CAMERA))


# ---- float64 matrices ------------------------------------------------------------------------------------------------
def m64(shift, rot, scale):
    """The forward matrix shift * rotate-x * rotate-y * rotate-z * scale (Instance.cu:4-17, Matrix.cu:183-249), 4 x 4 in
    float64, of inputs rounded to float32 first (what the library is given)."""
    sh, ro, sc = (np.asarray(x, F32).astype(np.float64) for x in (shift, rot, scale))
    c, s = np.cos(ro * np.pi / 180.0), np.sin(ro * np.pi / 180.0)
    rx = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]])
    ry = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
    rz = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]])
    m = np.eye(4)
    m[:3, :3] = rx @ ry @ rz @ np.diag(sc)
    m[:3, 3] = sh
    return m


def instance_m64(d):
    return m64(d["shift"], d["rotate"], d["scale"])


def local_box(sc, d):
    """[lo, hi] (2 x 3, float64) of the instance's box in its own frame: the given bounds, the sphere's box, or the
    parallelogram's q-centred box (Parallelogram.cu:48-50), before BoundingBox's 1e-6 padding of flat axes."""
    if d["type"] == abi.TRIANGLE:
        b = np.asarray(d["bounds"], np.float64)
        return np.stack([b[0::2], b[1::2]])
    if d["type"] == abi.SPHERE:
        _, _, c, r = sc.spheres[d["index"]]
        c = np.asarray(c, np.float64)
        return np.stack([c - r, c + r])
    _, _, q, u, v = sc.parallelograms[d["index"]]
    q, u, v = (np.asarray(x, F32).astype(np.float64) for x in (q, u, v))
    h = np.abs((u + v) * 0.5)
    return np.stack([q - h, q + h])


def world_corners(sc, d):
    """The float64 images [8, 3] of the corners of the instance's local box."""
    b = local_box(sc, d)
    m = instance_m64(d)
    corners = np.array([[b[i, 0], b[j, 1], b[k, 2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    return corners @ m[:3, :3].T + m[:3, 3]


# ---- rays ------------------------------------------------------------------------------------------------------------
def _targets(g, d, n):
    """(n points inside the instance's primitive, in its own frame; the surface's normals there [n, 3] each, or none).
    Mesh: inside the double cone |z| + r / cos(pi / 32) <= RADIUS, within 0.9 of it; for a class of NARROW, inside a
    triangle drawn uniformly, EDGE_MARGIN (barycentric) from its edges, with the outward normal and the interpolated
    vertex normal (the one the reference turns to face the ray).  Sphere: inside the ball, within 0.9 of its radius.
    Parallelogram: on it, inside its q-centred box, 0.01 from the box's faces (with its normal, for NARROW)."""
    narrow = d["cls"] in NARROW
    if d["type"] == abi.TRIANGLE and not narrow:
        z = g.uniform(-0.9, 0.9, n) * RADIUS
        r = 0.9 * np.cos(np.pi / 32) * (RADIUS - np.abs(z)) * np.sqrt(g.uniform(0, 1, n))
        ph = g.uniform(0, 2 * np.pi, n)
        return np.stack([r * np.cos(ph), r * np.sin(ph), z], 1), []
    if d["type"] == abi.TRIANGLE:
        verts, faces, vn = mesh()
        f = faces[g.integers(len(faces), size=n)]
        p = verts[f].astype(np.float64)
        ab = g.uniform(0.0, 1.0, (n, 2))
        ab = np.where((ab.sum(1) > 1.0)[:, None], 1.0 - ab, ab)
        ab = EDGE_MARGIN + (1.0 - 3.0 * EDGE_MARGIN) * ab                      # u, v and 1 - u - v all >= EDGE_MARGIN
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        nrm = np.cross(e1, e2)
        nrm *= np.sign((nrm * p.mean(axis=1)).sum(1))[:, None]                 # outward: the mesh surrounds its origin
        w = np.stack([1.0 - ab.sum(1), ab[:, 0], ab[:, 1]], 1)
        return p[:, 0] + ab[:, :1] * e1 + ab[:, 1:] * e2, [nrm, (vn[f].astype(np.float64) * w[:, :, None]).sum(1)]
    if d["type"] == abi.SPHERE:
        p = g.normal(size=(n, 3))
        p /= np.linalg.norm(p, axis=1, keepdims=True)
        return p * (0.9 * RADIUS * np.cbrt(g.uniform(0, 1, n)))[:, None], []
    q, u, v = (np.asarray(x, np.float64) for x in QUAD)
    h = np.abs(u + v) * 0.5
    out = np.zeros((0, 3))
    while len(out) < n:
        ab = g.uniform(0.05, 0.95, (4 * n, 2))
        p = ab[:, :1] * u + ab[:, 1:] * v
        out = np.concatenate([out, q + p[np.all(np.abs(p) <= h - 0.01, axis=1)]])
    return out[:n], [np.broadcast_to(np.cross(u, v), (n, 3))] if narrow else []


def rays(n_per_instance=N_PER_INSTANCE, seed=RAY_SEED):
    """(rays [66 n, 6] float32, aimed [66 n]: the instance each ray was aimed at).  Ray r of instance k goes through the
    world image (m64) of a point of `_targets`, from FAR x the half-diagonal of the instance's world box before it, in
    a uniformly random direction.  For the classes of NARROW the direction is uniformly random among those that meet the
    target's surface at |cos| >= GRAZE to its world normals (the inverse transpose's images of the local ones) — from
    outside, for the mesh: there the object is a few float32 spacings wide, and at any angle through any point inside
    it the hit falls on the other side of an edge, or the normal faces the ray, by a rounding of the ray's origin."""
    sc = scene()
    g = np.random.default_rng(seed)
    out, aimed = [], []
    for k, d in enumerate(sc.instances):
        m = instance_m64(d)
        local, normals = _targets(g, d, n_per_instance)
        target = local @ m[:3, :3].T + m[:3, 3]
        corners = world_corners(sc, d)
        extent = 0.5 * np.linalg.norm(corners.max(axis=0) - corners.min(axis=0))
        dirs = g.normal(size=(n_per_instance, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        if normals:
            nw = [nrm @ np.linalg.inv(m[:3, :3]) for nrm in normals]           # rows: (M^-T n)^T = n^T M^-1
            nw = [x / np.linalg.norm(x, axis=1, keepdims=True) for x in nw]
            while True:
                c = [(dirs * x).sum(1) for x in nw]
                bad = (c[0] > -GRAZE) | (c[1] > -GRAZE) if d["type"] == abi.TRIANGLE else (np.abs(c[0]) < GRAZE)
                if not bad.any():
                    break
                fresh = g.normal(size=(int(bad.sum()), 3))
                dirs[bad] = fresh / np.linalg.norm(fresh, axis=1, keepdims=True)
        out.append(np.concatenate([target - FAR * max(extent, EXTENT_FLOOR) * dirs, dirs], 1))
        aimed.append(np.full(n_per_instance, k))
    out = np.concatenate(out).astype(F32)
    out.setflags(write=False)
    return out, np.concatenate(aimed)


TURNS = ("rot90y", "rot90z", "rot90xyz", "rot180x", "rot270y", "rotm90x")
AXIS_PER_INSTANCE = 24


def axis_rays(seed=RAY_SEED + 1):
    """(rays [6 x 3 x 24, 6] float32, aimed): through points of `_targets` of the instances of TURNS, along +-x, +-y
    and +-z of the world (exact zeros in two components), from FAR x the world extent away."""
    sc = scene()
    g = np.random.default_rng(seed)
    out, aimed = [], []
    for k, d in enumerate(sc.instances):
        if d["cls"] not in TURNS:
            continue
        m = instance_m64(d)
        local, _ = _targets(g, d, AXIS_PER_INSTANCE)
        target = local @ m[:3, :3].T + m[:3, 3]
        corners = world_corners(sc, d)
        extent = 0.5 * np.linalg.norm(corners.max(axis=0) - corners.min(axis=0))
        dirs = np.zeros((AXIS_PER_INSTANCE, 3))
        j = np.arange(AXIS_PER_INSTANCE)
        dirs[j, j % 3] = np.where(j % 6 < 3, 1.0, -1.0)
        out.append(np.concatenate([target - FAR * extent * dirs, dirs], 1))
        aimed.append(np.full(AXIS_PER_INSTANCE, k))
    out = np.concatenate(out).astype(F32)
    out.setflags(write=False)
    return out, np.concatenate(aimed)


def assignment(frame):
    """The class (index in NAMES) instance k takes in frame `frame` of the moving test: (k + frame) mod 22."""
    return (np.arange(N_INSTANCES) + frame) % len(NAMES)


def project(points):
    """Pixel coordinates [n, 2] (x in [0, 192), y in [0, 128) inside the frame) of world points through CAMERA, whose
    fov is the horizontal one (RenderPin.cu:73-95) and which looks along -z."""
    c = np.asarray(CAMERA["center"], np.float64)
    assert tuple(CAMERA["target"][:2]) == (0.0, 0.0) and CAMERA["up"] == (0.0, 1.0, 0.0)
    fwd = np.asarray(CAMERA["target"], np.float64) - c
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    p = np.asarray(points, np.float64) - c
    depth = p @ fwd
    half_w = np.tan(np.radians(CAMERA["fov"]) / 2.0)
    half_h = half_w * FRAME[1] / FRAME[0]
    x = (p @ right) / depth / half_w
    y = (p @ up) / depth / half_h
    return np.stack([(x + 1.0) * 0.5 * FRAME[0], (y + 1.0) * 0.5 * FRAME[1]], 1)


# ---- closest hits, float64 -------------------------------------------------------------------------------------------
REF_DTYPE = np.dtype([("t", np.float64), ("instance", np.uint32), ("ptype", np.uint32), ("pindex", np.uint32),
                      ("point", np.float64, 3), ("normal", np.float64, 3), ("ambiguous", np.bool_)])


def _in01(x):
    return (x > -FZERO) & (x < 1.0 + FZERO)                  # Range::inRange of [0, 1] with its 1e-6 windows


def closest64(sc, rays, chunk=1024):
    """REF_DTYPE [rays]: the closest hit over the instances whose class is not "singular" (instance abi.MISS and
    t = inf on a miss).  Per instance the ray goes to the local frame with the float64 inverse of m64 (the direction
    is not normalised, so t is the world's); triangles by Moeller-Trumbore as Triangle.cu:4-44 (|det| < 1e-6 is a
    miss, u and v in [0, 1] with 1e-6 windows, u + v <= 1), spheres as Sphere.cu:4-49 (the nearer root if in range,
    else the farther), parallelograms as Parallelogram.cu:4-46 (|n . d| < 1e-6 is a miss) and only where the ray
    crosses the q-centred box the BVH leaf is built from (Parallelogram.cu:48-50); t in [0.001 - 1e-6, inf).  The
    normal is the unit inverse transpose times the local normal (interpolated vertex normals for the mesh), turned to
    face the ray.

    ambiguous: deep_tree_ref.ambiguous over all surfaces (a sphere's far side is one) — two nearest hits within
    1e-4 t, or the nearest within 1e-5 (barycentric) of an edge; for a parallelogram also a hit within 1e-4 of a face
    of its box, or before the ray enters the box (the reference then finds it or not with what it found before)."""
    rays = np.asarray(rays, np.float64)
    keep = [k for k, d in enumerate(sc.instances) if group_of(d["cls"]) != "singular"]
    fwd = np.stack([instance_m64(sc.instances[k]) for k in keep])
    inv = np.linalg.inv(fwd)
    by = {t: [i for i, k in enumerate(keep) if sc.instances[k]["type"] == t]
          for t in (abi.TRIANGLE, abi.SPHERE, abi.PARALLELOGRAM)}
    tri_first = np.array([sc.instances[keep[i]]["index"] for i in by[abi.TRIANGLE]])
    nt = MESH_TRIANGLES
    p = np.stack([sc.triangles["vertex"][f:f + nt] for f in tri_first]).astype(np.float64)     # [I, 64, 3, 3]
    e1, e2 = p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 0]
    q, qu, qv = (np.asarray(x, F32).astype(np.float64) for x in QUAD)
    qn = np.cross(qu, qv)
    qden = qn @ qn
    qh = np.abs(qu + qv) * 0.5
    # surface s of the concatenated [triangles | spheres | parallelograms] -> (index into keep, ptype, pindex)
    ns = len(by[abi.SPHERE])
    s_inst = np.concatenate([np.repeat(by[abi.TRIANGLE], nt), by[abi.SPHERE], by[abi.SPHERE], by[abi.PARALLELOGRAM]])
    s_type = np.concatenate([np.full(nt * len(by[abi.TRIANGLE]), abi.TRIANGLE), np.full(2 * ns, abi.SPHERE),
                             np.full(len(by[abi.PARALLELOGRAM]), abi.PARALLELOGRAM)])
    s_prim = np.concatenate([(tri_first[:, None] + np.arange(nt)).reshape(-1), np.zeros(2 * ns, int),
                             np.zeros(len(by[abi.PARALLELOGRAM]), int)])
    out = np.zeros(len(rays), REF_DTYPE)
    out["t"], out["instance"] = np.inf, abi.MISS
    tlo = TMIN - FZERO
    for a in range(0, len(rays), chunk):
        r = rays[a:a + chunk]
        o = np.einsum("iab,rb->ria", inv[:, :3, :3], r[:, :3]) + inv[None, :, :3, 3]
        d = np.einsum("iab,rb->ria", inv[:, :3, :3], r[:, 3:])
        with np.errstate(divide="ignore", invalid="ignore"):
            # triangles
            ot, dt = o[:, by[abi.TRIANGLE]], d[:, by[abi.TRIANGLE]]
            h = np.cross(dt[:, :, None, :], e2[None])
            det = (e1[None] * h).sum(-1)
            s = ot[:, :, None, :] - p[None, :, :, 0]
            u = (s * h).sum(-1) / det
            qq = np.cross(s, e1[None])
            v = (dt[:, :, None, :] * qq).sum(-1) / det
            t = (e2[None] * qq).sum(-1) / det
            ok = (np.abs(det) >= FZERO) & _in01(u) & _in01(v) & (u + v <= 1.0) & (t > tlo)
            T = [np.where(ok, t, np.inf).reshape(len(r), -1)]
            U, V = [u.reshape(len(r), -1)], [v.reshape(len(r), -1)]
            # spheres (centre 0)
            os_, ds = o[:, by[abi.SPHERE]], d[:, by[abi.SPHERE]]
            qa = (ds * ds).sum(-1)
            qb = 2.0 * (os_ * ds).sum(-1)
            qc = (os_ * os_).sum(-1) - RADIUS * RADIUS
            delta = qb * qb - 4.0 * qa * qc
            sq = np.sqrt(np.where(delta >= 0, delta, np.nan))
            r1, r2 = (-qb - sq) / (2.0 * qa), (-qb + sq) / (2.0 * qa)
            t = np.where(r1 > tlo, r1, np.where(r2 > tlo, r2, np.inf))
            T.append(np.where(np.isfinite(t), t, np.inf))
            T.append(np.where((r1 > tlo) & np.isfinite(r2), r2, np.inf))       # the far side: a surface of its own
            for _ in range(2):
                U.append(np.full(t.shape, 1.0 / 3.0))
                V.append(np.full(t.shape, 1.0 / 3.0))
            # parallelograms
            oq, dq = o[:, by[abi.PARALLELOGRAM]], d[:, by[abi.PARALLELOGRAM]]
            nu = qn / np.sqrt(qden)
            ndd = dq @ nu
            t = (nu @ q - oq @ nu) / ndd
            rel = oq + dq * t[..., None] - q
            al = np.cross(rel, qv) @ qn / qden
            be = np.cross(qu, rel) @ qn / qden
            # its leaf's box [q - h, q + h]: BoundingBox::hit over [0.001, closest so far] (BoundingBox.cu:34-72).  The
            # ray must cross the box; crossing it at or before the hit always passes, crossing it only beyond the hit
            # passes or not with what was found before — kept, and ambiguous
            par = np.abs(dq) < FZERO
            ta, tb_ = (q - qh - oq) / dq, (q + qh - oq) / dq
            inside = (oq >= q - qh) & (oq <= q + qh)
            te = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(ta, tb_)).max(-1)
            tx = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(ta, tb_)).min(-1)
            crossed = np.maximum(te, TMIN) < tx
            ok = (np.abs(ndd) >= FZERO) & _in01(al) & _in01(be) & crossed & (t > tlo)
            T.append(np.where(ok, t, np.inf))
            edge = np.minimum(np.minimum(al, 1.0 - al), np.minimum(be, 1.0 - be))
            face = np.where(te > t, -1.0, (qh - np.abs(rel)).min(-1) * (D.AMBIGUOUS_EDGE / QUAD_BOX_MARGIN))
            face = np.where(np.all(np.abs(rel) <= qh, axis=-1) | (te > t), face, 1.0)      # outside, box crossed before
            m = np.clip(np.minimum(edge, face), -1.0, 1.0 / 3.0)       # so that min(u, v, 1 - u - v) is this margin
            U.append(m)
            V.append(m)
        T, U, V = (np.concatenate(x, axis=1) for x in (T, U, V))
        best = np.argmin(T, axis=1)
        rr = np.arange(len(r))
        tb = T[rr, best]
        hit = np.isfinite(tb)
        rec = out[a:a + chunk]
        with np.errstate(invalid="ignore"):                  # inf - inf where a ray meets one surface or none
            rec["ambiguous"] = D.ambiguous(T, U, V)
        i = s_inst[best]
        ol, dl = o[rr, i], d[rr, i]
        pl = ol + dl * np.where(hit, tb, 0.0)[:, None]
        # local normals by type
        tri_slot = np.minimum(best, nt * len(by[abi.TRIANGLE]) - 1)
        g = s_prim[tri_slot]
        ub, vb = U[rr, tri_slot][:, None], V[rr, tri_slot][:, None]
        nrm = sc.triangles["normal"][g].astype(np.float64)
        n_tri = nrm[:, 0] * (1.0 - ub - vb) + nrm[:, 1] * ub + nrm[:, 2] * vb
        n = np.where((s_type[best] == abi.TRIANGLE)[:, None], n_tri,
                     np.where((s_type[best] == abi.SPHERE)[:, None], pl, qn[None]))
        with np.errstate(invalid="ignore", divide="ignore"):
            n = n / np.linalg.norm(n, axis=1, keepdims=True)
            n = np.where(((dl * n).sum(-1) < 0.0)[:, None], n, -n)
            nw = np.einsum("rba,rb->ra", inv[i][:, :3, :3], n)
            nw = nw / np.linalg.norm(nw, axis=1, keepdims=True)
        pw = np.einsum("rab,rb->ra", fwd[i][:, :3, :3], pl) + fwd[i][:, :3, 3]
        rec["t"] = tb
        rec["instance"] = np.where(hit, np.asarray(keep)[i], abi.MISS)
        rec["ptype"] = np.where(hit, s_type[best], 0)
        rec["pindex"] = np.where(hit, s_prim[best], 0)
        rec["point"] = np.where(hit[:, None], pw, 0.0)
        rec["normal"] = np.where(hit[:, None], nw, 0.0)
    return out
