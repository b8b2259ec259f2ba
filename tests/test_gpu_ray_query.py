"""rt_query_rays (Renderer.query_rays): device ray streams traced by the persistent query kernel, against the oracle.

The reference for every check is oracle.OracleScene.trace (closest hit, range [0.001, inf)) on the CPU.  The truth of a
ranged query is derived from it: with the oracle's closest t_c, tmax = 2 t_c must return the oracle's hit and tmax =
0.5 t_c must miss (nothing lies nearer than the closest hit).  Both need t_c well away from the 1e-6 tie window around
tmax, so those tests assert t_c >= 0.05 for every hit ray (on this scene and generator the smallest t_c is 0.55).

Tolerances: on the reference's trees (compat build) EXACT and FAST are bit-identical to the oracle; on SAH / LBVH trees
(instance, pindex) equal on >= 99.9 % of rays with |dt| <= 1e-4 t on those, as tests/test_gpu_parity.py states.
"""
import ctypes as C

import numpy as np
import pytest

from rtamd import Renderer, abi, scenes
from rtamd.renderer import hits_to_numpy

pytestmark = pytest.mark.gpu

FIELDS = ("t", "instance", "pindex", "ptype", "mtype", "midx", "point", "normal")
BUILD_SEED = 9
N_RAYS = 20000


def gen_rays(n, seed):
    g = np.random.default_rng(seed)
    o = np.stack([g.uniform(-3, 3, n), g.uniform(0.5, 6, n), g.uniform(4, 12, n)], 1)
    tgt = np.stack([g.uniform(-4, 4, n), g.uniform(-1, 5, n), g.uniform(-4, 4, n)], 1)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], 1).astype(np.float32)


def assert_records_equal(got, want, fields=FIELDS):
    for k in fields:
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


def miss_records(n):
    m = np.zeros(n, dtype=hits_to_numpy(np.zeros((0, 48), np.uint8)).dtype)
    m["t"] = np.inf
    m["instance"] = abi.MISS
    return m


class Ref:
    """The shared scene, its oracle, the 20 000 rays of seed 4 and the oracle's hits for them (computed once)."""

    def __init__(self):
        from oracle.oracle import OracleScene
        self.scene = scenes.demo_with_particles(16)
        self.oracle = OracleScene(self.scene, build_seed=BUILD_SEED)
        self.rays = gen_rays(N_RAYS, 4)
        self.hits = self.oracle.trace(self.rays)[0]
        self.hit = self.hits["instance"] != abi.MISS
        self.hits.setflags(write=False)
        self.rays.setflags(write=False)


@pytest.fixture(scope="module")
def ref(gpu_lib, oracle_lib):
    return Ref()


@pytest.fixture(scope="module")
def compat(ref):
    r = Renderer(ref.scene).build_acceleration_structure(BUILD_SEED)
    yield r
    r.cleanup()


def closest(r, rays, tmax=None, **kw):
    import torch
    t, h = r.query_rays(torch.from_numpy(np.array(rays, np.float32)).cuda(),
                        None if tmax is None else torch.from_numpy(np.ascontiguousarray(tmax, np.float32)).cuda(), **kw)
    return t.cpu().numpy(), (None if h is None else hits_to_numpy(h))


def occluded(r, rays, tmax=None, **kw):
    import torch
    o = r.query_rays(torch.from_numpy(np.array(rays, np.float32)).cuda(),
                     None if tmax is None else torch.from_numpy(np.ascontiguousarray(tmax, np.float32)).cuda(),
                     any_hit=True, **kw)
    assert o.dtype == torch.bool
    return o.cpu().numpy()


# ---- 1. closest, reference trees -----------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
def test_closest_reference_trees(ref, compat, exact):
    t, h = closest(compat, ref.rays, exact=exact)
    assert_records_equal(h, ref.hits)                    # misses included: t = +inf, instance MISS, the rest 0
    miss = ~ref.hit
    assert miss.sum() > 1000 and ref.hit.sum() > 10000
    assert np.all(h["t"][miss] == np.inf) and np.all(h["instance"][miss] == abi.MISS)
    for k in ("ptype", "pindex", "mtype", "midx"):
        assert not h[k][miss].any(), k
    assert not h["point"][miss].any() and not h["normal"][miss].any()
    assert np.array_equal(t, h["t"])
    t_only, none = closest(compat, ref.rays, exact=exact, want_hits=False)
    assert none is None and np.array_equal(t_only, ref.hits["t"])


# ---- 2. sizes ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(ref):
    rays = gen_rays((1 << 20) + 37, 11)
    return rays, ref.oracle.trace(rays)[0]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, (1 << 20) + 37])
def test_sizes(ref, compat, big, n):
    """FAST, t-only plus records, into over-allocated outputs whose elements past N keep their sentinel."""
    import torch
    if n > N_RAYS:
        rays, want = big
    else:
        rays, want = ref.rays[:n], ref.hits[:n]
    pad = 70
    d_rays = torch.from_numpy(np.array(rays, np.float32)).cuda()
    t_buf = torch.full((n + pad,), -7.0, dtype=torch.float32, device="cuda")
    t2_buf = torch.full((n + pad,), -7.0, dtype=torch.float32, device="cuda")
    h_buf = torch.full((n + pad, 48), 0xAB, dtype=torch.uint8, device="cuda")
    for t_ptr, h_ptr in ((t_buf.data_ptr(), h_buf.data_ptr()), (t2_buf.data_ptr(), None)):
        q = abi.RayQuery()
        q.rays_device = d_rays.data_ptr() if n else None
        q.ray_count = n
        q.t_device = t_ptr
        q.hits_device = h_ptr
        abi.check(compat.lib, compat.lib.rt_query_rays(compat.h, C.byref(q)))
    torch.cuda.synchronize()
    t, t2, h = t_buf.cpu().numpy(), t2_buf.cpu().numpy(), h_buf.cpu().numpy()
    assert np.all(t[n:] == -7.0) and np.all(t2[n:] == -7.0) and np.all(h[n:] == 0xAB)
    got = hits_to_numpy(h[:n])
    assert np.array_equal(t[:n], want["t"]) and np.array_equal(t2[:n], want["t"])
    assert_records_equal(got, want, ("t", "instance", "pindex") if n > N_RAYS else FIELDS)
    # the Python wrapper on the same sizes (its outputs are exactly N long)
    if n <= 257:
        tt, hh = closest(compat, rays.reshape(-1, 6))
        assert tt.shape == (n,) and hh.shape == (n,)
        assert_records_equal(hh, want)
        assert occluded(compat, rays.reshape(-1, 6)).shape == (n,)


# ---- 3. tmax -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
def test_tmax(ref, compat, exact):
    tc = ref.hits["t"]
    assert np.all(tc[ref.hit] >= 0.05)                   # precondition of both derivations: no filtering
    n = len(tc)
    # tmax = 2 t_c: the oracle's record / occluded; rays the oracle misses: tmax = 10, still a miss
    far = np.where(ref.hit, 2.0 * tc, 10.0).astype(np.float32)
    t, h = closest(compat, ref.rays, far, exact=exact)
    assert_records_equal(h, ref.hits)
    assert np.array_equal(t, ref.hits["t"])
    assert np.array_equal(occluded(compat, ref.rays, far, exact=exact), ref.hit)
    # tmax = 0.5 t_c: nothing is nearer than the closest hit
    near = np.where(ref.hit, 0.5 * tc, 10.0).astype(np.float32)
    t, h = closest(compat, ref.rays, near, exact=exact)
    assert_records_equal(h, miss_records(n))
    assert np.all(t == np.inf)
    assert not occluded(compat, ref.rays, near, exact=exact).any()
    # an explicit +inf array is tmax = None
    inf = np.full(n, np.inf, np.float32)
    t, h = closest(compat, ref.rays, inf, exact=exact)
    assert_records_equal(h, ref.hits)
    assert np.array_equal(occluded(compat, ref.rays, inf, exact=exact), ref.hit)
    # empty ranges
    for v in (0.0, 0.0005, -1.0, np.nan):
        tm = np.full(n, v, np.float32)
        t, h = closest(compat, ref.rays, tm, exact=exact)
        assert_records_equal(h, miss_records(n))
        assert np.all(t == np.inf), v
        assert not occluded(compat, ref.rays, tm, exact=exact).any(), v


# ---- 4. any-hit, reference trees -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ao(ref):
    """Ambient-occlusion rays: origins at the oracle's hit points, directions uniform on the normal's hemisphere."""
    g = np.random.default_rng(7)
    p = ref.hits["point"][ref.hit]
    nrm = ref.hits["normal"][ref.hit]
    d = g.normal(size=p.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.where((d * nrm).sum(1) < 0, -1.0, 1.0)[:, None]
    rays = np.concatenate([p, d], 1).astype(np.float32)
    return rays, ref.oracle.trace(rays)[0]


@pytest.mark.parametrize("exact", [True, False])
def test_any_hit_reference_trees(ref, compat, ao, exact):
    assert np.array_equal(occluded(compat, ref.rays, exact=exact), ref.hit)
    rays, want = ao
    occ = want["instance"] != abi.MISS
    assert 14000 <= len(rays) <= 16000 and 0.2 < occ.mean() < 0.4
    assert (want["t"][occ] < 0.05).mean() > 0.01         # rays that start on a surface: what the fixed tmin is for
    assert np.array_equal(occluded(compat, rays, exact=exact), occ)
    t, _ = closest(compat, rays, exact=exact, want_hits=False)
    assert np.array_equal(t, want["t"])


# ---- 5. other trees ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("mode", ["sah", "lbvh"])
def test_other_trees(ref, mode, exact):
    r = Renderer(ref.scene).build_acceleration_structure(BUILD_SEED, mode=mode)
    t, h = closest(r, ref.rays, exact=exact)
    same = (h["instance"] == ref.hits["instance"]) & (h["pindex"] == ref.hits["pindex"])
    assert same.mean() >= 0.999, same.mean()
    both = same & ref.hit
    assert np.all(np.abs(h["t"][both] - ref.hits["t"][both]) <= 1e-4 * ref.hits["t"][both])
    assert np.all(h["t"][same & ~ref.hit] == np.inf)
    assert np.array_equal(t, h["t"])
    occ = occluded(r, ref.rays, exact=exact)
    assert (occ == ref.hit).mean() >= 0.999
    r.cleanup()


# ---- 6. frames in flight -------------------------------------------------------------------------------------------
def test_frames_in_flight():
    """A render without a host wait, then a NO_SYNC query on a side stream, per frame: each query must see the frame
    block of the update just before it, whatever the lanes' renders and the next frames' uploads are doing."""
    import torch
    from oracle.oracle import OracleScene
    s = scenes.demo_with_particles(6)
    r = Renderer(s).build_acceleration_structure(BUILD_SEED).configure_camera(160, 96, ray_trace_depth=2)
    r.set_option("overlap", -1)
    r.set_option("stage_depth", 2)
    rays = gen_rays(4096, 5)
    d_rays = torch.from_numpy(rays).cuda()
    side = torch.cuda.Stream()
    frames = (0, 37, 79, 118, 157, 196)
    rgba = [torch.zeros(96 * 160 * 4, dtype=torch.uint8, device="cuda") for _ in frames]
    torch.cuda.synchronize()
    outs = []
    for f, img in zip(frames, rgba):
        r.render(f, sync=False, rgba8_device=img.data_ptr(), want_rgba=False)
        outs.append(r.query_rays(d_rays, exact=True, stream=side, sync=False))
    r.synchronize()
    torch.cuda.synchronize()
    o = OracleScene(s, build_seed=BUILD_SEED)
    for f, (t, h) in zip(frames, outs):
        o.update(f)
        want = o.trace(rays)[0]
        assert_records_equal(hits_to_numpy(h), want)
        assert np.array_equal(t.cpu().numpy(), want["t"]), f
    r.cleanup()


def test_synchronize_covers_queries_behind_overlapped_frames():
    """NO_SYNC queries, each on a stream of its own, with frames on the scene's lanes launched after them (the last one
    on the same frame block), then rt_synchronize alone: the lanes' launches replace the scene's completion events
    without waiting for a query on a caller stream, and the outputs must be complete all the same."""
    import torch
    from oracle.oracle import OracleScene
    s = scenes.demo_with_particles(6)
    r = Renderer(s).build_acceleration_structure(BUILD_SEED).configure_camera(160, 96, ray_trace_depth=2)
    r.set_option("overlap", -1)
    r.set_option("stage_depth", 2)
    rays = gen_rays(65536, 6)
    d_rays = torch.from_numpy(rays).cuda()
    frames = (0, 37, 79, 118)
    streams = [torch.cuda.Stream() for _ in frames]
    img = torch.zeros(96 * 160 * 4, dtype=torch.uint8, device="cuda")
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())      # the rays' upload; the only ordering the test adds
    outs = []
    for f, st in zip(frames, streams):
        r.render(f, sync=False, want_rgba=False)
        outs.append(r.query_rays(d_rays, exact=True, stream=st, sync=False))
    r.render(frames[-1], sync=False, skip_update=True, rgba8_device=img.data_ptr(), want_rgba=False)
    r.synchronize()
    got = [(t.cpu().numpy(), hits_to_numpy(h)) for t, h in outs]
    o = OracleScene(s, build_seed=BUILD_SEED)
    for f, (t, h) in zip(frames, got):
        o.update(f)
        want = o.trace(rays)[0]
        assert_records_equal(h, want)
        assert np.array_equal(t, want["t"]), f
    r.cleanup()


def test_triangle_update_waits_for_queries_behind_a_lane_frame(gpu_lib):
    """GPU-built trees without cold records: a hit's normals, material and caller index are read from the caller's
    triangles (raw_tris), which rt_scene_update_triangles rewrites in place.  A NO_SYNC records query on a stream of its
    own, a lane frame behind it (which replaces the scene's completion events), then the triangle update: the copy
    must wait for the query, whose records are those of the triangles before the update."""
    import torch
    s = scenes.demo_with_particles(8)
    r = Renderer(s).set_option("cold_records", 0).build_acceleration_structure(0, mode="lbvh")
    r.configure_camera(160, 96, ray_trace_depth=2)
    r.set_option("overlap", -1)
    rays = gen_rays(1 << 18, 8)
    d_rays = torch.from_numpy(rays).cuda()
    r.render(0, want_rgba=False)
    _, want = closest(r, rays)                           # synchronous: the reference before the update
    assert (want["ptype"][want["instance"] != abi.MISS] == abi.TRIANGLE).sum() > 10000   # records that read raw_tris
    moved = s.triangles[:8 * 1024].copy()
    moved["vertex"] += np.asarray([0.3, 0.2, 0.0], np.float32)
    moved["material_type"], moved["material_index"] = abi.ROUGH, 2       # was metal 0: a raced record would show it
    moved["normal"] = moved["normal"][..., [1, 2, 0]]                       # and another interpolated normal
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    t, h = r.query_rays(d_rays, stream=st, sync=False)
    r.render(0, sync=False, want_rgba=False)
    r.update_triangles(0, moved)
    r.synchronize()
    assert_records_equal(hits_to_numpy(h), want)
    assert np.array_equal(t.cpu().numpy(), want["t"])
    r.render(0, want_rgba=False)                         # the update is in effect after the next frame's rebuild
    _, after = closest(r, rays)
    assert (after["t"] != want["t"]).any() and (after["mtype"] != want["mtype"]).any()
    r.cleanup()


# ---- 7. stream order without host syncs ----------------------------------------------------------------------------
def test_stream_order_without_host_syncs(ref, compat):
    import torch
    want, _ = closest(compat, ref.rays)
    base = torch.from_numpy(np.array(ref.rays)).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rays = base + 0
        t, _ = compat.query_rays(rays, want_hits=False, sync=False)
        out = t.clone()
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


# ---- 8. errors -----------------------------------------------------------------------------------------------------
def test_errors(ref, compat):
    import torch
    d_rays = torch.from_numpy(np.array(ref.rays[:64])).cuda()
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    h = torch.zeros((64, 48), dtype=torch.uint8, device="cuda")
    occ = torch.zeros(64, dtype=torch.uint8, device="cuda")
    lib = compat.lib

    def query(handle, **kw):
        q = abi.RayQuery()
        q.rays_device, q.ray_count, q.t_device = d_rays.data_ptr(), 64, t.data_ptr()
        for k, v in kw.items():
            setattr(q, k, v)
        return lib.rt_query_rays(handle, C.byref(q))

    INVALID, STATE = 1, 4
    unbuilt = Renderer(ref.scene)
    assert query(unbuilt.h) == STATE
    assert b"rt_scene_build" in lib.rt_last_error()
    unbuilt.cleanup()
    assert query(compat.h) == 0
    assert query(compat.h, flags=abi.RT_QUERY_ANY_HIT, t_device=None, occluded_device=occ.data_ptr(),
                 hits_device=h.data_ptr()) == INVALID
    assert query(compat.h, flags=abi.RT_QUERY_ANY_HIT, occluded_device=occ.data_ptr()) == INVALID   # t_device set
    assert query(compat.h, t_device=None) == INVALID                 # closest with no output
    assert query(compat.h, occluded_device=occ.data_ptr()) == INVALID
    assert query(compat.h, reserved=1) == INVALID
    assert query(compat.h, flags=1 << 3) == INVALID
    assert query(compat.h, rays_device=None) == INVALID
    assert query(compat.h, ray_count=1 << 32) == INVALID
    assert query(compat.h, ray_count=0, rays_device=None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), ref.hits["t"][:64])      # the refused calls launched nothing

    with pytest.raises(ValueError):
        compat.query_rays(d_rays.double())
    with pytest.raises(ValueError):
        compat.query_rays(torch.from_numpy(np.array(ref.rays[:64])))       # a CPU tensor
    with pytest.raises(ValueError):
        compat.query_rays(torch.zeros((6, 64), dtype=torch.float32, device="cuda").t())
    with pytest.raises(ValueError):
        compat.query_rays(d_rays, torch.zeros(63, dtype=torch.float32, device="cuda"))


def test_triangle_update_needs_a_frame(gpu_lib):
    s = scenes.demo_with_particles(4)
    r = Renderer(s).build_acceleration_structure(0, mode="lbvh").configure_camera(64, 48, ray_trace_depth=2)
    rays = gen_rays(257, 3)
    before, _ = closest(r, rays)
    moved = s.triangles[:1024].copy()
    moved["vertex"] += np.asarray([0.01, 0.0, 0.0], np.float32)
    r.update_triangles(0, moved)
    with pytest.raises(abi.RtError, match="RT_ERR_STATE"):
        closest(r, rays)
    r.render(0)
    after, h = closest(r, rays, exact=True)
    want = r.trace_rays(rays, exact=True)                # the one-thread-per-ray kernel: the same rebuilt trees, the
    assert_records_equal(h, want)                        # same binary pairs and arithmetic
    assert np.array_equal(after, want["t"]) and after.shape == before.shape
    r.cleanup()


# ---- 9. current device preserved -----------------------------------------------------------------------------------
def test_current_device_preserved(ref, compat):
    import torch
    n = torch.cuda.device_count()
    cur = n - 1                                   # another device than the scene's where there is one
    torch.cuda.set_device(cur)
    try:
        t, _ = compat.query_rays(ref.rays[:257].copy(), want_hits=False)
        assert torch.cuda.current_device() == cur
        assert np.array_equal(t.cpu().numpy(), ref.hits["t"][:257])
    finally:
        torch.cuda.set_device(0)
