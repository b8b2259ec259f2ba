"""RT_TRI_UPDATE_BOUNDS (csrc/inst_bounds.hip, instances.hip, update.cpp): a device triangle update that also derives the
bounds of the instances it overlaps on the device.

Scenes are inst_bounds_ref.particles(P, T): scenes.synth_particles cut to T triangles per particle and translated so that
every centroid coordinate lies in [1, 16), where the host's sequential double sum and the device's fixed-shape sum are
both exact (tests/test_inst_bounds_ref.py checks that for every scene and shift used here, without a GPU).  There the
device path must equal the host path bit for bit: "equal" is np.array_equal everywhere but in the one inexact case.
Scenes are static (no update callback) unless a test passes its own.  Frames are 256 x 144 at depth 2.

The instance records of debug_read("instances") are compared with option "group" 0: while a group is intact its
members are inactive records, kept out of the TLAS, and a device-bounded inactive member's record shows the box of
the root it maps to (the group's), which no ray ever tests.
"""
import ctypes as C

import numpy as np
import pytest

import inst_bounds_ref as ref
from rtamd import Renderer, abi
from test_gpu_lbvh import PAIR_DT, QUAD_DT, ROOT_DT
from test_gpu_update_device import assert_same, written_quads

pytestmark = pytest.mark.gpu

W, H = 256, 144
P, CHUNK = ref.P, ref.CHUNK
FIRST_PARTICLE = 5                      # the demo's five instances come first
MISS = 0xFFFFFFFF


def scene(p, t, local_bounds, **kw):
    s = ref.particles(p, t, local_bounds, **kw)
    s.animated = False
    return s


def build(s, update=False, **options):
    r = Renderer(s, update=update)
    for k, v in options.items():
        r.set_option(k, v)
    return r.build_acceleration_structure(0, mode="lbvh").configure_camera(W, H, ray_trace_depth=2)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()


def update_flagged(r, t, lo, hi, **kw):
    r.update_triangles_device(lo, dev(t["vertex"][lo:hi]), bounds=True, **kw)


def records(r):
    return r.debug_read("instances").view(np.float32).reshape(-1, 45)


def state(r, rays):
    """A frame (its update rebuilds the BLASes and takes the new bounds), the instance records, the TLAS, the BLAS
    forest, and per-ray hit records."""
    out = {"frame": r.render(0, want_rgb=True)[1], "instances": records(r)}
    out["tlas_boxes"], out["tlas_ci"], out["tlas_refs"] = r.export_tlas()
    pairs = r.debug_read("blas_pairs").view(PAIR_DT)
    roots = r.debug_read("blas_roots").view(ROOT_DT)
    out["blas_pairs"], out["blas_roots"] = pairs, roots
    out["blas_quads"] = written_quads(pairs, r.debug_read("blas_quads").view(QUAD_DT), roots)
    out["leaf_prims"] = r.debug_read("leaf_prims").view(np.uint32)
    out["hits"] = r.trace_rays(rays, exact=True)
    return out


def fresh(p, t, local_bounds, tris, **kw):
    s2 = scene(p, t, local_bounds, **kw)
    s2.triangles = tris
    return s2


def oracle_hits(s, rays):
    from oracle.oracle import OracleScene
    o = OracleScene(s, build_seed=0)
    h, _ = o.trace(rays, brute_force=True)
    o.close()
    return h


def assert_hits_equal(got, want, what):
    for f in want.dtype.names:
        assert np.array_equal(got[f], want[f]), what + (f,)


@pytest.mark.parametrize("cold", [0, 1])
@pytest.mark.parametrize("t", ref.T_CASES)
def test_derived_instances_equal_the_host_path(gpu_lib, t, cold):
    """Particles without bounds of their own (has_local_bounds = 0): the parent commit refuses this update."""
    from oracle.oracle import OracleScene
    s = scene(P, t, False)
    n = P * t
    m = ref.moved(s.triangles, 0, n, ref.SHIFTS["near"])
    rays = ref.rays_at(m, 0, n, 3000)
    d = build(s, cold_records=cold, group=0)
    before = records(d).copy()
    update_flagged(d, m, 0, n)
    got = state(d, rays)
    assert not np.array_equal(before[FIRST_PARTICLE:, 36:], got["instances"][FIRST_PARTICLE:, 36:])
    assert (got["hits"]["instance"][got["hits"]["instance"] != MISS] >= FIRST_PARTICLE).sum() > 1000
    h = build(s, cold_records=cold, group=0)
    h.update_triangles(0, m[:n])
    assert_same(got, state(h, rays), ("host", t, cold))
    s2 = fresh(P, t, False, m)
    assert_same(got, state(build(s2, cold_records=cold, group=0), rays), ("fresh", t, cold))
    o = OracleScene(s2, build_seed=0)
    assert np.array_equal(got["instances"], o.instance_state()), (t, cold)
    o.close()


def test_a_mesh_that_leaves_its_bounds(gpu_lib):
    """Particles with bounds of their own, every vertex shifted by several box sizes (a box is ~0.1 wide, the shift
    0.5).  The rays start in front of the new place (+z, at most 1 to the side over 3 to 5 of depth); a particle's
    old box lies 0.75 nearer and 1.5 to the side in world units, so no ray towards a particle crosses that
    particle's old box: without the flag its TLAS item is never entered (option "group" 0: a group's box is the
    union of all old boxes, which other particles' new places do touch)."""
    t = 128
    s = scene(P, t, True)
    n = P * t
    m = ref.moved(s.triangles, 0, n, ref.SHIFTS["away"])
    rays = ref.rays_at(m, 0, n, 3000)
    want = oracle_hits(fresh(P, t, True, m), rays)
    assert (want["instance"][want["instance"] != MISS] >= FIRST_PARTICLE).sum() > 2500
    r0 = build(s, group=0)
    r0.update_triangles_device(0, dev(m["vertex"][:n]))
    r0.render(0)
    h0 = r0.trace_rays(rays, exact=True)
    assert not ((h0["instance"] != MISS) & (h0["instance"] >= FIRST_PARTICLE)).any()      # today: silently culled
    for group in (0, 1):
        r = build(s, group=group)
        update_flagged(r, m, 0, n)
        r.render(0)
        assert_hits_equal(r.trace_rays(rays, exact=True), want, ("flag", group))


@pytest.mark.parametrize("lo,hi", [(65 - 10, 65 + 10), (P * 65, P * 65 + 1), (2 * 65, 3 * 65), (0, P * 65 + 1)],
                         ids=["across_two", "demo_triangle", "one_whole", "all"])
def test_partial_ranges(gpu_lib, lo, hi):
    """A range that begins inside one instance and ends inside the next; the last triangle of the array (the demo's own
    single-triangle instance); one whole instance; everything.  Equal to the host path over the same range, which
    reduces an overlapped instance over its whole range; the other instances keep their records bit for bit."""
    t = 65
    s = scene(P, t, False)
    m = ref.moved(s.triangles, lo, hi, ref.SHIFTS["near"])
    rays = ref.rays_at(m, 0, P * t, 2000)
    d, h = build(s, group=0), build(s, group=0)
    before = records(d).copy()
    update_flagged(d, m, lo, hi)
    h.update_triangles(lo, m[lo:hi])
    got = state(d, rays)
    assert_same(got, state(h, rays), (lo, hi))
    for i, x in enumerate(s.instances):
        if x["type"] != abi.TRIANGLE:
            touched = False
        else:
            touched = x["index"] < hi and x["index"] + max(1, x.get("count", 0)) > lo
        assert np.array_equal(before[i], got["instances"][i]) == (not touched), i


def test_groups(gpu_lib):
    """Default option "group": the particles stay one TLAS item across three flagged updates; a member moved through the
    update callback breaks the group, and the members' records are the derived ones; moved back, the group re-forms.
    Hits equal the oracle's tree-free trace throughout."""
    from oracle.oracle import OracleScene
    p, t = 8, 64
    s = scene(p, t, True)
    n, ni = p * t, len(s.instances)
    k = FIRST_PARTICLE + 3
    mode = {"moved": False}

    def update(xs, count, frame):
        xs[k].shift.x = 0.75 if mode["moved"] else 0.0

    r = build(s, update=update)
    r0 = build(s, group=0)
    m = s.triangles
    for f in range(3):
        m = ref.moved(s.triangles, 0, n, ref.SHIFTS["frames"][f + 1])
        rays = ref.rays_at(m, 0, n, 2000, seed=f)
        want = oracle_hits(fresh(p, t, True, m), rays)
        for x in (r, r0):
            update_flagged(x, m, 0, n)
            x.render(f)
            assert_hits_equal(x.trace_rays(rays, exact=True), want, ("intact", f))
        refs = r.export_tlas()[2]
        assert (refs >= ni).sum() == 1 and not ((refs >= FIRST_PARTICLE) & (refs < ni)).any()
        assert not (r0.export_tlas()[2] >= ni).any()
    # break: the oracle's scene carries the moved member; its instances derive their bounds (has_local_bounds = 0)
    mode["moved"] = True
    sb = fresh(p, t, False, m)
    sb.instances[k]["shift"] = (0.75, ref.SHIFT_Y, 0.0)
    rays = np.concatenate([ref.rays_at(m, 0, n, 1500, seed=9), ref.rays_at(ref.moved(m, 3 * t, 4 * t, (0.25, 0, 0)), 3 * t, 4 * t, 500)])
    r.render(3)
    refs = r.export_tlas()[2]
    assert not (refs >= ni).any() and ((refs >= FIRST_PARTICLE) & (refs < ni)).sum() == p
    assert_hits_equal(r.trace_rays(rays, exact=True), oracle_hits(sb, rays), ("broken",))
    o = OracleScene(sb, build_seed=0)
    assert np.array_equal(records(r)[FIRST_PARTICLE:], o.instance_state()[FIRST_PARTICLE:])
    o.close()
    m = ref.moved(s.triangles, 0, n, ref.SHIFTS["frames"][4])           # a flagged update while the group is broken
    update_flagged(r, m, 0, n)
    r.render(4)
    sb.triangles = m
    rays = ref.rays_at(m, 0, n, 1500, seed=10)
    assert_hits_equal(r.trace_rays(rays, exact=True), oracle_hits(sb, rays), ("broken, updated",))
    mode["moved"] = False                                                # re-form
    r.render(5)
    refs = r.export_tlas()[2]
    assert (refs >= ni).sum() == 1 and not ((refs >= FIRST_PARTICLE) & (refs < ni)).any()
    assert_hits_equal(r.trace_rays(rays, exact=True), oracle_hits(fresh(p, t, True, m), rays), ("re-formed",))


def test_lanes(gpu_lib):
    """Six frames on two lanes, each behind a flagged NO_SYNC update with another shift, no host synchronisation until
    the end: every frame equals the serial twin's ("overlap" 0, synchronous calls) byte for byte."""
    import torch
    t = CHUNK + 1
    s = scene(P, t, False)
    n = P * t
    shifts = ref.SHIFTS["frames"]
    src = [dev(ref.moved(s.triangles, 0, n, sh)["vertex"][:n]) for sh in shifts]
    serial = build(s, cold_records=1)
    want = []
    for f in range(len(shifts)):
        serial.update_triangles_device(0, src[f], bounds=True)
        want.append(serial.render(f)[0])
    serial.cleanup()
    assert not np.array_equal(want[0], want[-1])
    r = build(s, cold_records=1)
    r.set_option("overlap", 2)
    lanes = [torch.cuda.Stream() for _ in range(2)]
    bufs = [torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda") for _ in shifts]
    torch.cuda.synchronize()
    for f in range(len(shifts)):
        r.update_triangles_device(0, src[f], bounds=True, sync=False)
        r.render(f, want_rgba=False, rgba8_device=bufs[f].data_ptr(), stream=lanes[f % 2].cuda_stream, sync=False)
    r.synchronize()
    torch.cuda.synchronize()
    for f in range(len(shifts)):
        assert np.array_equal(bufs[f].cpu().numpy().reshape(H, W, 4), want[f]), f
    r.cleanup()


def test_state_transitions(gpu_lib):
    t = 65
    n = P * t
    s = scene(P, t, False)
    a = ref.moved(s.triangles, 0, n, ref.SHIFTS["near"])
    b = ref.moved(s.triangles, 0, n, ref.SHIFTS["away"])
    rays = ref.rays_at(b, 0, n, 2000)
    # a host update on the same range takes the bounds back: equal to the twin that only ever used the host path
    d, h = build(s, group=0), build(s, group=0)
    update_flagged(d, a, 0, n)
    d.render(0)
    d.update_triangles(0, b[:n])
    h.update_triangles(0, a[:n])
    h.render(0)
    h.update_triangles(0, b[:n])
    assert_same(state(d, rays), state(h, rays), ("host after flag",))
    # ... also with default groups, where the group comes back with its members
    d, h = build(s), build(s)
    update_flagged(d, a, 0, n)
    d.render(0)
    d.update_triangles(0, b[:n])
    h.update_triangles(0, b[:n])
    assert_same(state(d, rays), state(h, rays), ("host after flag, group",))
    # rt_scene_update_instances with bounds: those bounds apply
    sl = scene(P, t, True)
    loose = [dict(i) for i in sl.instances[FIRST_PARTICLE:]]
    for i in loose:
        bb = np.asarray(i["bounds"], np.float32).reshape(3, 2) + np.asarray([[-1.0, 1.0]] * 3, np.float32)
        i["bounds"] = tuple(float(v) for v in bb.reshape(-1))
    d, h = build(sl, group=0), build(sl, group=0)
    update_flagged(d, a, 0, n)
    d.render(0)
    d.update_instances(FIRST_PARTICLE, loose)
    h.update_triangles(0, a[:n])
    h.update_instances(FIRST_PARTICLE, loose)
    ra = ref.rays_at(a, 0, n, 2000)
    x = state(d, ra)
    assert_same(x, state(h, ra), ("instances after flag",))
    assert not np.array_equal(x["instances"][FIRST_PARTICLE:, 36:42], state(build(fresh(P, t, False, a), group=0), ra)["instances"][FIRST_PARTICLE:, 36:42])
    # rt_scene_build: derived instances from the triangles read back, described ones back to their description
    for lb in (False, True):
        d = build(scene(P, t, lb), group=0)
        update_flagged(d, a, 0, n)
        d.render(0)
        d.build_acceleration_structure(0, mode="lbvh")
        assert_same(state(d, ra), state(build(fresh(P, t, lb, a), group=0), ra), ("rebuilt", lb))
    # errors
    u = abi.TriangleUpdate()
    v = dev(a["vertex"][:16])
    u.first, u.count, u.vertices_device = 0, 16, v.data_ptr()
    d = build(s)
    u.flags = 1 << 5
    assert d.lib.rt_scene_update_triangles_device(d.h, C.byref(u)) == 1          # RT_ERR_INVALID_ARGUMENT
    u.flags = abi.RT_TRI_UPDATE_BOUNDS | (1 << 5)
    assert d.lib.rt_scene_update_triangles_device(d.h, C.byref(u)) == 1
    sah = Renderer(s, update=False).build_acceleration_structure(0, mode="sah").configure_camera(32, 32)
    u.flags = abi.RT_TRI_UPDATE_BOUNDS
    assert sah.lib.rt_scene_update_triangles_device(sah.h, C.byref(u)) == 5      # RT_ERR_UNSUPPORTED
    sah.cleanup()
    u.flags = 0                                                                  # without the flag: refused as before
    assert d.lib.rt_scene_update_triangles_device(d.h, C.byref(u)) == 5
    # a second instance over a shorter range from the same first triangle shares the first one's BLAS: its root is
    # not that instance's box, so the flag refuses it
    s3 = scene(P, t, False)
    s3.instances.append(dict(s3.instances[FIRST_PARTICLE], count=t - 1))
    d3 = build(s3)
    u.flags = abi.RT_TRI_UPDATE_BOUNDS
    assert d3.lib.rt_scene_update_triangles_device(d3.h, C.byref(u)) == 5


def test_inexact_sums(gpu_lib):
    """scenes.synth_particles as it comes, coordinates around 0: the host's sequential sum need not be exact, nor equal
    to the device's shape.  Boxes are min / max and stay equal; both sums carry a relative error below 2^-40 (n x
    2^-53) before their one rounding to float, so the centroids differ by at most one float ulp; hits do not depend on
    the centroid but through the TLAS's shape."""
    t = CHUNK + 1
    s = scene(P, t, False, offset=(0.0, 0.0, 0.0))
    n = P * t
    m = ref.moved(s.triangles, 0, n, (0.05, 0.0, -0.03))
    rays = ref.rays_at(m, 0, n, 3000)
    d, h = build(s, group=0), build(s, group=0)
    update_flagged(d, m, 0, n)
    h.update_triangles(0, m[:n])
    d.render(0), h.render(0)
    x, y = records(d), records(h)
    assert np.array_equal(x[:, :42], y[:, :42])
    ulps = np.abs(x[:, 42:].view(np.int32).astype(np.int64) - y[:, 42:].view(np.int32).astype(np.int64))
    print("centroid ulps:", ulps.max())
    assert ulps.max() <= 1
    assert_hits_equal(d.trace_rays(rays, exact=True), oracle_hits(fresh(P, t, False, m, offset=(0.0, 0.0, 0.0)), rays), ("inexact",))


def test_vtk_series_played_with_derived_bounds(gpu_lib):
    """VtkSeriesPlayer.preload(derive_bounds=True) plays an entry with the flag and without rt_scene_update_instances: the
    particles stay one TLAS item (the default playback breaks their group for good), and the frame shows the second
    file's geometry: the same surfaces as a scene created from that file, whose TLAS differs (per-particle bounds from
    the reader against the group's derived box), so the bar is the suite's for one geometry under two trees
    (tests/test_gpu_group.py: >= 99.9 % of pixels within 1 LSB)."""
    import os
    from rtamd.vtk import VtkSeriesPlayer, vtk_scene
    vtk_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vtk")
    series = os.path.join(vtk_dir, "particle_mesh.vtk.series")
    s = vtk_scene(series)
    ni = len(s.instances)
    r = Renderer(s).build_acceleration_structure(0, mode="lbvh").configure_camera(W, H, ray_trace_depth=2)
    first = r.render(0)[0]
    grouped = (r.export_tlas()[2] >= ni).sum()
    player = VtkSeriesPlayer(r, series).preload("cuda", derive_bounds=True)
    player.load(1)
    played = r.render(0)[0]
    assert not np.array_equal(first, played)
    assert (r.export_tlas()[2] >= ni).sum() == grouped
    f1 = os.path.join(vtk_dir, "particle_000000000000100.vtk")
    want = Renderer(vtk_scene(f1)).build_acceleration_structure(0, mode="lbvh").configure_camera(W, H, ray_trace_depth=2).render(0)[0]
    close = (np.abs(played.astype(np.int32) - want.astype(np.int32)).max(axis=-1) <= 1).mean()
    print("within 1 LSB:", close, "group items:", grouped)
    assert close >= 0.999
    if grouped:
        default = Renderer(s).build_acceleration_structure(0, mode="lbvh").configure_camera(W, H, ray_trace_depth=2)
        VtkSeriesPlayer(default, series).preload("cuda").load(1)
        default.render(0)
        assert (default.export_tlas()[2] >= ni).sum() == 0
