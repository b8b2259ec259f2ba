"""rt_scene_update_triangles_device (csrc/tri_update.hip, update.cpp): triangle geometry handed over in device memory.

Scenes are scenes.demo_with_particles(8): 8 192 particle triangles whose instances carry their own bounds, then the
demo's own triangle at index 8 192, whose instance derives its bounds from it.  Frames are 256 x 144 at depth 2, as in
tests/test_gpu_lbvh.py.  "Equal" is np.array_equal everywhere: the device path and the host path feed identical bytes
to the same builder, so there is nothing to tolerate.

blas_quads is compared at the slots the builder writes (the quads rooted at every second binary level below a root,
found by walking the GPU's own pairs): the slots between them are never written and hold whatever the allocation held.
"""
import ctypes as C

import numpy as np
import pytest

from rtamd import Renderer, abi, scenes
from test_gpu_lbvh import PAIR_DT, QUAD_DT, REF_INDEX, REF_LEAF, ROOT_DT

pytestmark = pytest.mark.gpu

P = 8
N_P = P * 1024                 # particle triangles; the demo's triangle follows at index N_P
W, H = 256, 144
SHIFT = np.asarray([0.05, 0.0, -0.03], np.float32)


def _rays():
    """The 20 000 rays of tests/test_gpu_lbvh.py::test_trace_rays_hits_match_oracle."""
    rng = np.random.default_rng(5)
    n = 20000
    org = np.stack([rng.uniform(-6, 6, n), rng.uniform(0.5, 8, n), rng.uniform(6, 12, n)], 1)
    tgt = np.stack([rng.uniform(-2, 2, n), rng.uniform(3.5, 5.5, n), rng.uniform(-1, 1, n)], 1)
    return np.concatenate([org, tgt - org], 1).astype(np.float32)


RAYS = _rays()


def build(scene, **options):
    r = Renderer(scene)
    for k, v in options.items():
        r.set_option(k, v)
    return r.build_acceleration_structure(0, mode="lbvh").configure_camera(W, H, ray_trace_depth=2)


def moved(tris, lo, hi, normals, shift=SHIFT):
    """`tris` with the vertices of [lo, hi) shifted and, with `normals`, their normals replaced (vertex 0's and
    vertex 2's swapped: still unit vectors, and different ones) and has_normals = 1."""
    t = tris.copy()
    t["vertex"][lo:hi] += shift
    if normals:
        t["normal"][lo:hi] = t["normal"][lo:hi][:, ::-1]
        t["has_normals"][lo:hi] = 1
    return t


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()


def update_device(r, t, lo, hi, normals, **kw):
    r.update_triangles_device(lo, dev(t["vertex"][lo:hi]), dev(t["normal"][lo:hi]) if normals else None, **kw)


def written_quads(pairs, quads, roots):
    slots = []
    for root in roots:
        todo = [int(root["ref"]) & REF_INDEX] if not int(root["ref"]) & REF_LEAF else []
        while todo:
            q = todo.pop()
            slots.append(q)
            for r in (int(pairs[q]["ref0"]), int(pairs[q]["ref1"])):
                if r & REF_LEAF:
                    continue
                g = pairs[r & REF_INDEX]
                todo += [int(x) & REF_INDEX for x in (g["ref0"], g["ref1"]) if not int(x) & REF_LEAF]
    return quads[np.sort(np.asarray(slots, np.int64))]


def state(r, hits=True):
    """A frame (its update rebuilds the BLASes), the forest it traced, and per-ray hit records."""
    out = {"frame": r.render(0, want_rgb=True)[1]}
    pairs = r.debug_read("blas_pairs").view(PAIR_DT)
    roots = r.debug_read("blas_roots").view(ROOT_DT)
    out["blas_pairs"], out["blas_roots"] = pairs, roots
    out["blas_quads"] = written_quads(pairs, r.debug_read("blas_quads").view(QUAD_DT), roots)
    out["leaf_prims"] = r.debug_read("leaf_prims").view(np.uint32)
    if hits:
        out["hits"] = r.trace_rays(RAYS, exact=True)
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if a[k].dtype.names:
            for f in a[k].dtype.names:
                assert np.array_equal(a[k][f], b[k][f]), what + (k, f)
        else:
            assert np.array_equal(a[k], b[k]), what + (k,)


@pytest.mark.parametrize("normals", [True, False], ids=["normals", "no_normals"])
@pytest.mark.parametrize("cold", [0, 1])
def test_device_path_equals_host_path_and_fresh_scene(gpu_lib, cold, normals):
    s = scenes.demo_with_particles(P)
    t = moved(s.triangles, 0, N_P, normals)
    d = build(s, cold_records=cold)
    before = d.render(0, want_rgb=True)[1]
    update_device(d, t, 0, N_P, normals)
    got = state(d)
    assert not np.array_equal(before, got["frame"])
    assert (got["hits"]["pindex"][got["hits"]["ptype"] == abi.TRIANGLE] < N_P).sum() > 0       # some rays see the particles
    h = build(s, cold_records=cold)
    h.update_triangles(0, t[:N_P])
    assert_same(got, state(h), ("host", cold, normals))
    s2 = scenes.demo_with_particles(P)
    s2.triangles = t
    assert_same(got, state(build(s2, cold_records=cold)), ("fresh", cold, normals))


@pytest.mark.parametrize("first,count", [(1000, 3000), (N_P - 1, 1), (0, 1), (3, 255), (3, 256), (3, 257)])
def test_ranges_equal_host_path(gpu_lib, first, count):
    """Ranges that start and end inside BLASes, the last particle triangle, the first, and counts around the kernel's
    workgroup size at an odd `first` (records 8-byte but not 16-byte aligned): each equals the host path over the same
    range, which also shows that the triangles outside the range stay as they were."""
    s = scenes.demo_with_particles(P)
    t = moved(s.triangles, first, first + count, True, shift=np.asarray([0.3, -0.2, 0.1], np.float32))
    d, h = build(s), build(s)
    before = d.render(0, want_rgb=True)[1]
    update_device(d, t, first, first + count, True)
    h.update_triangles(first, t[first:first + count])
    got = state(d)
    assert_same(got, state(h), (first, count))
    if count > 100:
        assert not np.array_equal(before, got["frame"])


@pytest.mark.parametrize("cold", [0, 1])
def test_flat_triangles(gpu_lib, cold):
    """Particle triangles without stored normals: a device update without normals leaves them flat, their normals
    follow the new vertices (equal to a fresh scene); with normals they become has_normals = 1 (equal to the host
    update that says so)."""
    s = scenes.demo_with_particles(2)
    n = 2048
    s.triangles["has_normals"][:n] = 0
    flat = moved(s.triangles, 0, n, False)
    d = build(s, cold_records=cold)
    update_device(d, flat, 0, n, False)
    s2 = scenes.demo_with_particles(2)
    s2.triangles = flat
    got = state(d)
    assert_same(got, state(build(s2, cold_records=cold)), ("flat", cold))
    smooth = moved(s.triangles, 0, n, True)
    assert smooth["has_normals"][:n].all()
    d2, h2 = build(s, cold_records=cold), build(s, cold_records=cold)
    update_device(d2, smooth, 0, n, True)
    h2.update_triangles(0, smooth[:n])
    got2 = state(d2)
    assert_same(got2, state(h2), ("smooth", cold))
    assert not np.array_equal(got["hits"]["normal"], got2["hits"]["normal"])


@pytest.mark.parametrize("group,L,sets", [(1, 3, 3), (0, 3, 3)])
def test_pipelined_frames_from_one_reused_buffer(gpu_lib, group, L, sets):
    """tests/test_gpu_lbvh.py::test_update_triangles_pipelined_frames with the triangles coming from device memory: a
    producer stream overwrites one device tensor with frame f's vertices, the update takes it on that stream without
    waiting, the frame is launched on one of L lanes without waiting.  Every frame equals the synchronous host-update
    sequence: the scene's stream waited for the producer, and the producer for the kernel before it overwrote the
    tensor with frame f + 1's vertices."""
    import torch
    s = scenes.demo_with_particles(P)
    F = max(9, 2 * L + 3)

    def deform(f):
        t = s.triangles[:N_P].copy()
        t["vertex"] += np.asarray([0.02 * f, 0.01 * (f % 3), -0.015 * f], np.float32)
        return t

    ref_r = build(s, group=group)
    ref = []
    for f in range(F):
        ref_r.update_triangles(0, deform(f))
        ref.append(ref_r.render(f)[0])
    ref_r.cleanup()
    assert not np.array_equal(ref[0], ref[F - 1])
    r = build(s, group=group, blas_sets=sets)
    r.set_option("overlap", L)
    lanes = [torch.cuda.Stream() for _ in range(L)]
    producer = torch.cuda.Stream()
    source = [dev(deform(f)["vertex"]) for f in range(F)]
    verts = torch.zeros(9 * N_P, dtype=torch.float32, device="cuda")
    bufs = [torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda") for _ in range(F)]
    torch.cuda.synchronize()
    for f in range(F):
        with torch.cuda.stream(producer):
            verts.copy_(source[f], non_blocking=True)
        r.update_triangles_device(0, verts, stream=producer, sync=False)
        r.render(f, want_rgba=False, rgba8_device=bufs[f].data_ptr(), stream=lanes[f % L].cuda_stream, sync=False)
    r.synchronize()
    torch.cuda.synchronize()
    for f in range(F):
        assert np.array_equal(bufs[f].cpu().numpy().reshape(H, W, 4), ref[f]), f
    r.cleanup()


def test_traces_need_a_frame_update_after_a_device_update(gpu_lib):
    """As tests/test_gpu_lbvh.py::test_trace_after_triangle_update_needs_a_frame_update."""
    import torch
    s = scenes.demo_with_particles(4)
    r = Renderer(s).build_acceleration_structure(0, mode="lbvh").configure_camera(64, 48, ray_trace_depth=2)
    a = r.render(0)[0]
    assert np.array_equal(r.render(0, skip_update=True)[0], a)
    t = moved(s.triangles, 0, 1024, False, shift=np.asarray([0.01, 0.0, 0.0], np.float32))
    update_device(r, t, 0, 1024, False)
    ray = np.asarray([[0.0, 2.0, 10.0, 0.0, 0.0, -1.0]], np.float32)
    with pytest.raises(abi.RtError, match="RT_ERR_STATE"):
        r.render(0, skip_update=True)
    with pytest.raises(abi.RtError, match="RT_ERR_STATE"):
        r.trace_rays(ray)
    with pytest.raises(abi.RtError, match="RT_ERR_STATE"):
        r.query_rays(torch.from_numpy(ray).cuda())
    b = r.render(0)[0]                                 # the update rebuilds the BLASes
    assert np.array_equal(r.render(0, skip_update=True)[0], b)
    r.trace_rays(ray)
    r.query_rays(torch.from_numpy(ray).cuda())
    r.cleanup()


@pytest.mark.parametrize("order", ["host_then_device", "device_then_host"])
def test_overlapping_host_and_device_updates_last_writer_wins(gpu_lib, order):
    """Host range [0, 4096) and device range [2048, 6144) in either order: the later call's values stand where they
    overlap, and the result equals a fresh scene built with the final values.  device_then_host also updates the demo's
    own triangle through the host path afterwards: its instance derives its bounds from the host mirror, which the
    device update left stale (the library reads the triangles back first)."""
    s = scenes.demo_with_particles(P)
    a = moved(s.triangles, 0, 4096, True, shift=np.asarray([0.04, 0.02, 0.0], np.float32))
    b = moved(s.triangles, 2048, 6144, False, shift=np.asarray([-0.03, 0.0, 0.05], np.float32))
    final = s.triangles.copy()
    r = build(s)
    if order == "host_then_device":
        r.update_triangles(0, a[:4096])
        update_device(r, b, 2048, 6144, False)
        final[:4096] = a[:4096]
        final["vertex"][2048:6144] = b["vertex"][2048:6144]       # the device update keeps a's normals in [2048, 4096)
    else:
        update_device(r, b, 2048, 6144, False)
        r.update_triangles(0, a[:4096])
        final[2048:6144] = b[2048:6144]
        final[:4096] = a[:4096]
        final["vertex"][N_P] += np.asarray([0.2, 0.1, 0.0], np.float32)
        r.update_triangles(N_P, final[N_P:N_P + 1])
    s2 = scenes.demo_with_particles(P)
    s2.triangles = final
    assert_same(state(r), state(build(s2)), (order,))


def test_second_build_sees_device_updated_triangles(gpu_lib):
    """rt_scene_build on a built scene after a device update builds from the updated triangles (read back once)."""
    s = scenes.demo_with_particles(P)
    t = moved(s.triangles, 0, N_P, True)
    r = build(s)
    update_device(r, t, 0, N_P, True)
    r.build_acceleration_structure(0, mode="lbvh")
    s2 = scenes.demo_with_particles(P)
    s2.triangles = t
    assert_same(state(r), state(build(s2)), ("rebuilt",))


def _call(r, **fields):
    u = abi.TriangleUpdate()
    for k, v in fields.items():
        setattr(u, k, v)
    return r.lib.rt_scene_update_triangles_device(r.h, C.byref(u))


def test_errors(gpu_lib):
    import torch
    INVALID, UNSUPPORTED = 1, 5
    s = scenes.demo_with_particles(P)
    n = len(s.triangles)
    assert n == N_P + 1
    v = dev(s.triangles["vertex"][:16])
    device_before = torch.cuda.current_device()
    sah = Renderer(s).build_acceleration_structure(0, mode="sah").configure_camera(32, 32)
    assert _call(sah, first=0, count=16, vertices_device=v.data_ptr()) == UNSUPPORTED
    sah.cleanup()
    r = build(s)
    before = r.render(0, want_rgb=True)[1]
    # [8191, 8193) reaches the demo's triangle, whose instance derives its bounds from it: refused, nothing changes
    with pytest.raises(abi.RtError, match="RT_ERR_UNSUPPORTED.*instance"):
        r.update_triangles_device(N_P - 1, dev(s.triangles["vertex"][N_P - 1:N_P + 1] + 1.0))
    assert np.array_equal(r.render(0, skip_update=True, want_rgb=True)[1], before)       # not even marked stale
    assert np.array_equal(r.render(0, want_rgb=True)[1], before)
    assert _call(r, first=n - 8, count=16, vertices_device=v.data_ptr()) == INVALID
    assert _call(r, first=2**64 - 1, count=2, vertices_device=v.data_ptr()) == INVALID
    host = np.zeros(16 * 9, np.float32)
    assert _call(r, first=0, count=16, vertices_device=host.ctypes.data) == INVALID
    assert _call(r, first=0, count=16, vertices_device=v.data_ptr(), normals_device=host.ctypes.data) == INVALID
    assert _call(r, first=0, count=16, vertices_device=v.data_ptr(), reserved=1) == INVALID
    assert _call(r, first=0, count=16, vertices_device=v.data_ptr(), flags=1 << 5) == INVALID
    assert _call(r, first=0, count=16, vertices_device=None) == INVALID
    assert _call(r, first=0, count=0) == abi.RT_OK
    assert _call(r, first=n, count=0) == abi.RT_OK
    with pytest.raises(ValueError):
        r.update_triangles_device(0, v.double())
    with pytest.raises(ValueError):
        r.update_triangles_device(0, v.cpu())
    with pytest.raises(ValueError):
        r.update_triangles_device(0, v[:10])
    with pytest.raises(ValueError):
        r.update_triangles_device(0, v.view(-1, 2)[:, 0])
    with pytest.raises(ValueError):
        r.update_triangles_device(0, v, v[:9])
    assert np.array_equal(r.render(0, skip_update=True, want_rgb=True)[1], before)       # none of them changed anything
    assert torch.cuda.current_device() == device_before
    r.cleanup()
