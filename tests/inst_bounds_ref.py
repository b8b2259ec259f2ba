"""RT_TRI_UPDATE_BOUNDS on the CPU: a numpy restatement of the centroid reduction's shape (csrc/inst_bounds_map.hpp), the
host path's rule it must reproduce (build.cpp bounds_from_prims, update.cpp host_bounds), and the scenes of tests/test_gpu_update_device_bounds.py,
so that tests/test_inst_bounds_ref.py can check without a GPU what those tests rest on.

Scenes.  particles(P, T) is scenes.synth_particles cut to the first T triangles of each particle (the generator makes
multiples of 64), translated by OFFSET in the particles' local space, under one unrotated transform (scale 3, shift
(0, 4, 0)), so a world point is 3 * local + (0, 4, 0) and rays can be aimed at triangles without restating the matrix
code.  The demo's own triangle is translated too.  No quantisation is needed: every centroid coordinate then lies in
[1, 16), where a float is a multiple of 2^-23 below 2^4, so a sum of up to 2^16 of them is a multiple of 2^-23 below
2^20 and fits a double's 53 bits: the host's sequential double sum is exact, and so is any other order.
tests/test_inst_bounds_ref.py checks both facts for every scene against math.fsum.
"""
import numpy as np

from rtamd import abi, scenes

WAVE, WAVES, ROUNDS = 64, 4, 4
BLOCK = WAVE * WAVES
CHUNK = BLOCK * ROUNDS

OFFSET = np.asarray([2.0, 2.0, 2.0], np.float32)
SCALE, SHIFT_Y = 3.0, 4.0
T_CASES = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
P = 4


def tri_centroids(vertex):
    """hm::tri_centroid's float operations: (n, 3, 3) float32 -> (n, 3) float32."""
    v = np.asarray(vertex, np.float32)
    return ((v[:, 0] + v[:, 1]) + v[:, 2]) / np.float32(3.0)


def _wave_sum(v):
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def _block_sum(lane):
    """(..., 256) float64 -> (...)"""
    w = _wave_sum(lane.reshape(lane.shape[:-1] + (WAVES, WAVE)))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _strided_sum(x):
    """(n, A) float64: thread t adds rows t, t + 256, ... to +0.0, then wave and block steps."""
    n, a = x.shape
    rows = -(-n // BLOCK)
    pad = np.zeros((rows * BLOCK, a))
    pad[:n] = x
    acc = np.zeros((BLOCK, a))
    for r in pad.reshape(rows, BLOCK, a):
        acc = acc + r
    return _block_sum(acc.T)


def _chunk_sum(c):
    """(m <= 1024, A) float32: lane l of wave w holds triangle (4 r + w) 64 + l in round r."""
    pad = np.zeros((CHUNK, c.shape[1]))
    pad[:len(c)] = c.astype(np.float64)
    acc = np.zeros((BLOCK, c.shape[1]))
    for r in pad.reshape(ROUNDS, BLOCK, -1):
        acc = acc + r
    return _block_sum(acc.T)


def device_sum(cent):
    """S per axis in the device's shape, a pure function of len(cent)."""
    chunks = [_chunk_sum(cent[k:k + CHUNK]) for k in range(0, len(cent), CHUNK)]
    return chunks[0] if len(chunks) == 1 else _strided_sum(np.stack(chunks))


def sequential_sum(cent):
    """bounds_from_prims: c += pc in triangle order, from +0.0."""
    return np.add.accumulate(np.concatenate([np.zeros((1, cent.shape[1])), cent.astype(np.float64)]), axis=0)[-1]


def centroid(vertex, total=device_sum):
    c = tri_centroids(vertex)
    if len(c) == 1:
        return c[0]                                   # one triangle keeps its own centroid
    return (total(c) / np.float64(len(c))).astype(np.float32)


def group_centroid(member_centroids, total=_strided_sum):
    m = np.asarray(member_centroids, np.float32)
    return (total(m.astype(np.float64)) / np.float64(len(m))).astype(np.float32)


def tri_boxes(vertex):
    """hm::tri_box: min / max of the three vertices, a range shorter than 1e-6 widened by 1e-6 each way
    (Box::ensure_volume, float arithmetic) -> (n, 3, 2) float32."""
    v = np.asarray(vertex, np.float32)
    lo, hi = v.min(axis=1), v.max(axis=1)
    f0 = np.float32(1e-6)
    length = np.where((lo >= hi) | (np.abs(lo - hi) < f0), np.float32(0), hi - lo)
    thin = length < f0
    return np.stack([np.where(thin, lo - f0, lo), np.where(thin, hi + f0, hi)], axis=2).astype(np.float32)


def union_box(vertex):
    b = tri_boxes(vertex)
    return np.stack([b[:, :, 0].min(axis=0), b[:, :, 1].max(axis=0)], axis=1)


def particles(p, t, local_bounds, offset=OFFSET, seed=0x5EED):
    """The demo scene + p particles of t triangles each.  Returns the Scene; its particle triangles are [0, p t), the
    demo's own single-triangle instance follows at p t.  local_bounds: the particle instances carry bounds
    (has_local_bounds = 1, the uncut particle's) or derive them (0)."""
    t64 = -(-t // 64) * 64
    tris, inst = scenes.synth_particles(p, t64, seed)
    tris = tris.reshape(p, t64)[:, :t].reshape(-1).copy()
    tris["vertex"] += np.asarray(offset, np.float32)
    s = scenes.demo_scene()
    s.triangles["vertex"] += np.asarray(offset, np.float32)
    s.triangles = np.concatenate([tris, s.triangles])
    for d in s.instances:
        if d["type"] == abi.TRIANGLE:
            d["index"] += p * t
    for k, d in enumerate(inst):
        d.update(index=k * t, count=t, shift=(0.0, SHIFT_Y, 0.0), rotate=(0.0, 0.0, 0.0), scale=(SCALE,) * 3)
        if local_bounds:
            b = np.asarray(d["bounds"], np.float32).reshape(3, 2) + np.asarray(offset, np.float32)[:, None]
            d["bounds"] = tuple(float(x) for x in b.reshape(-1))
            d["centroid"] = tuple(float(x) for x in np.asarray(d["centroid"], np.float32) + np.asarray(offset, np.float32))
        else:
            del d["bounds"], d["centroid"]
    s.instances = s.instances + inst
    return s


def moved(tris, lo, hi, shift):
    t = tris.copy()
    t["vertex"][lo:hi] += np.asarray(shift, np.float32)
    return t


def rays_at(tris, lo, hi, n, seed=7):
    """n rays aimed at random points of the particle triangles [lo, hi) in world space (3 * local + (0, 4, 0)), from
    origins a few units in front of them (+z), directions unnormalised as rt_trace_rays takes them."""
    rng = np.random.default_rng(seed)
    v = tris["vertex"][lo:hi].astype(np.float64)
    k = rng.integers(0, len(v), n)
    w = 0.1 + 0.7 * rng.dirichlet((1.0, 1.0, 1.0), n)       # away from the edges: no ties between neighbours
    local = (v[k] * w[:, :, None]).sum(axis=1)
    tgt = SCALE * local + np.asarray([0.0, SHIFT_Y, 0.0])
    org = tgt + np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(3, 5, n)], 1)
    return np.concatenate([org, tgt - org], 1).astype(np.float32)


# the shifts the GPU tests move geometry by: every moved scene is checked for the same conditions
SHIFTS = {"near": (0.25, -0.125, 0.0625), "away": (0.5, 0.5, -0.25),
          "frames": [(0.03125 * f, 0.015625 * (f % 3), -0.0234375 * f) for f in range(6)]}
