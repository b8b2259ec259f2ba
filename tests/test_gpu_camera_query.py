"""rt_query_camera (Renderer.query_camera): the camera's own rays, generated and traced on the device.

References: tests/camera_rays_ref.py for the rays (numpy float32, pinned against the oracle's frames by
tests/test_camera_rays_ref.py), oracle.OracleScene.trace for the records, rt_query_rays for "nothing changed behind the
new ray source", and rt_render's own frame for the first-sample rays (depth 1, 1 spp, rough materials only: the pixel is
the albedo of what its first ray hits, see tests/test_camera_rays_ref.py).  Every comparison is bit for bit.

The frame is 100 x 60: the pitch (112) is not the width, a row is no whole number of 64-pixel chunks, and the 13 x 8
blocks of 8 x 8 pixels have partial right and top edges.
"""
import ctypes as C

import numpy as np
import pytest

import camera_rays_ref as ref
from rtamd import Renderer, abi, scenes
from rtamd.renderer import hits_to_numpy

pytestmark = pytest.mark.gpu

W, H = ref.W, ref.H
WHOLE = (0, 0, W, H)
BUILD_SEED = 9
SEEDS = (0, 0xC0FFEE12345)         # 0 means 0x5EED
GUARD = 64                          # elements kept around every output buffer
FILL = {"rays": -7.0, "t": -7.0, "hits": 0xAB, "albedo": -7.0}
WIDTH = {"rays": 6, "t": 1, "hits": 48, "albedo": 3}
INVALID, STATE = 1, 4
EXACT, NO_SYNC, FIRST = abi.RT_CAMERA_QUERY_EXACT, abi.RT_CAMERA_QUERY_NO_SYNC, abi.RT_CAMERA_QUERY_FIRST_SAMPLE


class Ref:
    """Scenes, the oracle and the reference rays, computed once and left unchanged."""

    def __init__(self):
        from oracle.oracle import OracleScene
        self.rough = ref.rough_only_scene()
        self.metal = scenes.demo_with_particles(6)                        # metal particles, and the radius-2 sphere
        self.metal.spheres[1] = (abi.METAL, 0) + tuple(self.metal.spheres[1][2:])
        self.oracle = OracleScene(self.rough, build_seed=BUILD_SEED)
        self.cam = {}
        for name, over in ref.CAMERAS.items():
            self.oracle.camera(W, H, ray_trace_depth=1, **over)
            self.cam[name] = self.oracle.camera_export()
        self._rays = {}

    def rays(self, name, seed=None):
        """Whole-frame reference rays [H W, 6]: centre rays (seed None) or the first-sample rays of `seed`."""
        key = ("centre", None) if seed is None else (name, seed)
        if key not in self._rays:
            r = ref.centre_rays(self.cam[name], WHOLE) if seed is None else \
                ref.first_sample_rays(self.cam[name], W, WHOLE, seed, ref.CAMERAS[name]["focus_disk_radius"])
            r.setflags(write=False)
            self._rays[key] = r
        return self._rays[key]


@pytest.fixture(scope="module")
def data(gpu_lib, oracle_lib):
    return Ref()


def make(scene, camera="pinhole", mode="compat", depth=1, **options):
    r = Renderer(scene)
    for k, v in options.items():
        r.set_option(k, v)
    r.build_acceleration_structure(BUILD_SEED, mode=mode)
    return r.configure_camera(W, H, ray_trace_depth=depth, **ref.CAMERAS[camera])


def raw_query(r, rect, flags=0, seed=0, want=("rays", "t", "hits", "albedo"), stream=None, handle=None, **fields):
    """One rt_query_camera call into buffers with guard bands.  Returns (status, {name: array [w h, width]}) after
    checking that the bands kept their fill."""
    import torch
    x0, y0, w, h = rect
    n = w * h if max(w, h) < 1 << 16 else 0
    q = abi.CameraQuery()
    q.x0, q.y0, q.width, q.height, q.frame_seed, q.flags = x0, y0, w, h, seed, flags
    q.stream = stream
    bufs = {}
    for k in want:
        dt = torch.uint8 if k == "hits" else torch.float32
        b = torch.full(((n + 2 * GUARD) * WIDTH[k],), FILL[k], dtype=dt, device="cuda")
        setattr(q, k + "_device", b.data_ptr() + GUARD * WIDTH[k] * b.element_size())
        bufs[k] = b
    for k, v in fields.items():
        setattr(q, k, v)
    torch.cuda.synchronize()
    rc = r.lib.rt_query_camera(r.h if handle is None else handle, C.byref(q))
    r.synchronize() if handle is None else None
    torch.cuda.synchronize()
    out = {}
    for k, b in bufs.items():
        a = b.cpu().numpy().reshape(n + 2 * GUARD, WIDTH[k])
        assert (a[:GUARD] == a.dtype.type(FILL[k])).all() and (a[n + GUARD:] == a.dtype.type(FILL[k])).all(), k
        out[k] = a[GUARD:n + GUARD]
    return rc, out


def untouched(out):
    return all((a == a.dtype.type(FILL[k])).all() for k, a in out.items())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def cut(whole, width, rect):
    x0, y0, w, h = rect
    return whole.reshape(H, W, width)[y0:y0 + h, x0:x0 + w].reshape(w * h, width)


# ---- 1. the rays ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["exact", "fast", "fast_math"])
@pytest.mark.parametrize("camera", list(ref.CAMERAS))
def test_rays(data, camera, flavour):
    r = make(data.rough, camera, **({"fast_math": 1} if flavour == "fast_math" else {}))
    ex = EXACT if flavour == "exact" else 0
    rc, out = raw_query(r, WHOLE, ex, want=("rays",))                     # rays as the only output
    assert rc == 0 and same_bits(out["rays"], data.rays(camera))
    for seed in SEEDS:
        rc, out = raw_query(r, WHOLE, ex | FIRST, seed, want=("rays", "t"))
        assert rc == 0 and same_bits(out["rays"], data.rays(camera, seed or ref.DEFAULT_SEED)), seed
        rc, only = raw_query(r, WHOLE, ex | FIRST, seed, want=("rays",))
        assert rc == 0 and same_bits(only["rays"], out["rays"])
    # the seed is no input of the centre rays
    rc, out = raw_query(r, WHOLE, ex, seed=12345, want=("rays",))
    assert rc == 0 and same_bits(out["rays"], data.rays(camera))
    r.cleanup()


# ---- 2. rectangles -------------------------------------------------------------------------------------------------
RECTS = [WHOLE, (99, 59, 1, 1), (0, 7, 64, 1), (35, 59, 65, 1), (8, 8, 8, 8), (3, 5, 9, 9), (3, 5, 70, 9)]


@pytest.fixture(scope="module")
def disk_compat(data):
    r = make(data.metal, "disk")
    yield r
    r.cleanup()


@pytest.fixture(scope="module")
def whole_frame(disk_compat):
    out = {}
    for flags in (0, FIRST):
        rc, o = raw_query(disk_compat, WHOLE, flags, SEEDS[1])
        assert rc == 0
        out[flags] = o
    return out


@pytest.mark.parametrize("flags", [0, FIRST])
@pytest.mark.parametrize("rect", RECTS, ids=lambda r: "%dx%d@%d,%d" % (r[2], r[3], r[0], r[1]))
def test_rectangles(disk_compat, whole_frame, rect, flags):
    rc, out = raw_query(disk_compat, rect, flags, SEEDS[1])               # (the guard bands are checked in there)
    assert rc == 0
    for k, a in out.items():
        assert same_bits(a, cut(whole_frame[flags][k], WIDTH[k], rect)), k
    hit = np.isfinite(whole_frame[flags]["t"])
    assert 0.2 < hit.mean() < 0.98                                        # hits and misses both in view


def test_python_wrapper(disk_compat, whole_frame):
    import torch
    o = disk_compat.query_camera((3, 5, 70, 9), first_sample=True, frame_seed=SEEDS[1], want_rays=True, want_hits=True,
                                 want_albedo=True)
    assert {k: (tuple(v.shape), v.dtype) for k, v in o.items()} == {
        "rays": ((9, 70, 6), torch.float32), "t": ((9, 70), torch.float32), "hits": ((9, 70, 48), torch.uint8),
        "albedo": ((9, 70, 3), torch.float32)}
    for k, v in o.items():
        assert v.is_cuda and same_bits(v.cpu().numpy().reshape(630, -1), cut(whole_frame[FIRST][k], WIDTH[k], (3, 5, 70, 9))), k
    o = disk_compat.query_camera()                                        # the whole frame, t only, centre rays
    assert list(o) == ["t"] and same_bits(o["t"].cpu().numpy().reshape(-1, 1), whole_frame[0]["t"])
    o = disk_compat.query_camera((5, 5, 0, 3), want_rays=True)
    assert tuple(o["t"].shape) == (3, 0) and tuple(o["rays"].shape) == (3, 0, 6)


# ---- 3. against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [None, SEEDS[1]])
def test_records_equal_the_oracles(data, seed):
    r = make(data.rough, "disk")
    rc, out = raw_query(r, WHOLE, EXACT | (0 if seed is None else FIRST), seed or 0, want=("rays", "t", "hits"))
    assert rc == 0
    want, _ = data.oracle.trace(data.rays("disk", seed))
    got = hits_to_numpy(out["hits"])
    for k in ("t", "instance", "pindex", "ptype", "mtype", "midx", "point", "normal"):
        assert same_bits(got[k], want[k]), k
    assert same_bits(out["t"].reshape(-1), got["t"])
    r.cleanup()


# ---- 4. against the buffer query -----------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["compat", "sah", "lbvh-cold0", "lbvh-cold1"])
def test_equals_the_ray_query_on_its_own_rays(data, build):
    """hits and t of the camera query, byte for byte what rt_query_rays writes for the camera query's rays: quad and
    binary trees, EXACT and FAST."""
    import torch
    mode, _, cold = build.partition("-cold")
    r = make(data.metal, "disk", mode=mode, depth=2, **({"cold_records": int(cold)} if cold else {}))
    r.render(0, want_rgba=False)
    for wide in (1, 0):
        r.set_option("wide", wide)
        for exact in (True, False):
            rc, out = raw_query(r, WHOLE, FIRST | (EXACT if exact else 0), 77, want=("rays", "t", "hits"))
            assert rc == 0
            t, h = r.query_rays(torch.from_numpy(out["rays"].copy()).cuda(), exact=exact)
            assert same_bits(h.cpu().numpy(), out["hits"]), (wide, exact)
            assert same_bits(t.cpu().numpy(), out["t"].reshape(-1)), (wide, exact)
            assert 0.2 < np.isfinite(out["t"]).mean() < 0.98
    r.cleanup()


# ---- 5. against the frame ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("camera", ["pinhole", "disk"])
def test_albedo_is_the_depth_one_frame(data, camera, exact):
    import torch
    r = make(data.rough, camera)
    for seed in SEEDS:
        frame = torch.full((H * W * 3,), -7.0, dtype=torch.float32, device="cuda")
        r.render(0, frame_seed=seed or ref.DEFAULT_SEED, exact=exact, rgb32_device=frame.data_ptr(), want_rgba=False)
        rc, out = raw_query(r, WHOLE, FIRST | (EXACT if exact else 0), seed, want=("albedo",))
        assert rc == 0
        torch.cuda.synchronize()
        f = frame.cpu().numpy().reshape(H * W, 3)
        assert same_bits(out["albedo"], f), int((out["albedo"] != f).any(axis=1).sum())
        assert len(np.unique(f, axis=0)) >= 5                             # the four roughs and the background
    r.cleanup()


@pytest.mark.parametrize("exact", [True, False])
def test_albedo_is_the_hit_materials(data, disk_compat, exact):
    rc, out = raw_query(disk_compat, WHOLE, EXACT if exact else 0, want=("hits", "albedo"))
    assert rc == 0
    h = hits_to_numpy(out["hits"])
    assert ((h["instance"] != abi.MISS) & (h["mtype"] == abi.METAL)).sum() > 50
    assert (h["instance"] == abi.MISS).sum() > 50
    assert same_bits(out["albedo"], ref.albedo_of(data.metal, h, data.metal.camera["background"]))


# ---- 6. the contract -----------------------------------------------------------------------------------------------
def test_errors(data, disk_compat):
    import torch
    r = disk_compat
    host = np.zeros(W * H, np.float32)

    def refused(status, rect=(3, 5, 9, 9), handle=None, **kw):
        rc, out = raw_query(r, rect, handle=handle, **kw)
        assert rc == status and untouched(out), (rc, kw)

    refused(INVALID, reserved=1)
    refused(INVALID, flags=1 << 1)                                        # rt_query_rays' any-hit bit: unknown here
    refused(INVALID, flags=1 << 4)
    refused(INVALID, want=())                                             # no output buffer
    refused(INVALID, t_device=host.ctypes.data)                           # not accessible from the device
    for rect in ((92, 5, 9, 9), (3, 52, 9, 9), (100, 0, 1, 1), (0, 60, 1, 1), (0xFFFFFFFF, 0, 2, 1),
                 (2, 0, 0xFFFFFFFF, 1), (0, 0xFFFFFFFF, 1, 2), (0, 2, 1, 0xFFFFFFFF), (0, 0, 101, 60), (101, 0, 0, 1)):
        refused(INVALID, rect=rect)
    assert b"rectangle" in r.lib.rt_last_error()
    for rect in ((3, 5, 0, 9), (3, 5, 9, 0), (100, 60, 0, 0)):             # nothing to do: RT_OK, nothing launched
        refused(0, rect=rect)
    unbuilt = Renderer(data.metal)
    refused(STATE, handle=unbuilt.h)
    assert b"rt_scene_build" in r.lib.rt_last_error()
    unbuilt.build_acceleration_structure(BUILD_SEED)
    refused(STATE, handle=unbuilt.h)
    assert b"rt_camera_set" in r.lib.rt_last_error()
    unbuilt.cleanup()
    with pytest.raises(abi.RtError, match="RT_ERR_INVALID_ARGUMENT"):
        r.query_camera((0, 0, 101, 60))
    rc, out = raw_query(r, (3, 5, 9, 9))                                  # and the scene still answers
    assert rc == 0 and not untouched(out)
    assert torch.cuda.current_device() == 0


def test_triangle_update_needs_a_frame(gpu_lib):
    import torch
    s = scenes.demo_with_particles(4)
    r = Renderer(s).build_acceleration_structure(0, mode="lbvh").configure_camera(W, H, ray_trace_depth=2)
    r.render(0, want_rgba=False)
    rc, before = raw_query(r, WHOLE, want=("t",))
    assert rc == 0
    moved = s.triangles["vertex"][:4 * 1024] + np.float32(0.01)           # inside the bounds the meshes were built with
    r.update_triangles_device(0, torch.from_numpy(np.ascontiguousarray(moved).reshape(-1)).cuda())
    rc, out = raw_query(r, WHOLE, want=("t", "rays"))
    assert rc == STATE and untouched(out)
    r.render(0, want_rgba=False)
    rc, after = raw_query(r, WHOLE, want=("t",))
    assert rc == 0 and (after["t"] != before["t"]).any()
    r.cleanup()


def test_no_sync_on_a_torch_stream(disk_compat, whole_frame):
    import torch
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        o = disk_compat.query_camera(first_sample=True, frame_seed=SEEDS[1], want_hits=True, want_albedo=True, sync=False)
        t, a = o["t"].clone(), o["albedo"] * 1.0                          # torch ops on that stream
    side.synchronize()
    assert same_bits(t.cpu().numpy().reshape(-1, 1), whole_frame[FIRST]["t"])
    assert same_bits(a.cpu().numpy().reshape(-1, 3), whole_frame[FIRST]["albedo"])
    assert same_bits(o["hits"].cpu().numpy().reshape(-1, 48), whole_frame[FIRST]["hits"])


def test_back_to_back_with_ray_queries_between_overlapped_frames(data):
    """NO_SYNC frames on "overlap" lanes, each followed by a camera query and a ray query without a host wait: the
    results of the serialised sequence."""
    import torch
    frames = (0, 37, 79, 118)
    d_rays = torch.from_numpy(np.array(data.rays("pinhole"))).cuda()

    def run(r, sync):
        outs = []
        img = [torch.zeros(H * W * 4, dtype=torch.uint8, device="cuda") for _ in frames]
        torch.cuda.synchronize()
        for f, im in zip(frames, img):
            r.render(f, sync=sync, rgba8_device=im.data_ptr(), want_rgba=False)
            c = r.query_camera(want_hits=True, sync=sync)
            t, h = r.query_rays(d_rays, sync=sync)
            outs.append((c["t"], c["hits"], t, h))
        r.synchronize()
        torch.cuda.synchronize()
        return [[x.cpu().numpy() for x in o] for o in outs]

    r = make(data.metal, "pinhole", depth=2)
    want = run(r, True)
    r.set_option("overlap", -1)
    r.set_option("stage_depth", 2)
    got = run(r, False)
    for f, g, w in zip(frames, got, want):
        for a, b in zip(g, w):
            assert same_bits(a, b), f
        assert same_bits(g[0].reshape(-1), g[2]) and same_bits(g[1].reshape(-1, 48), g[3])    # centre rays: the two agree
    assert any(not same_bits(want[0][0], w[0]) for w in want[1:])        # the frames moved the scene
    r.cleanup()


def test_accepted_with_a_communicator_attached(data, whole_frame):
    r = make(data.metal, "disk")
    r.attach_comm(Renderer.comm_unique_id(), 0, 1)
    rc, out = raw_query(r, WHOLE, FIRST, SEEDS[1])
    assert rc == 0
    for k, a in out.items():
        assert same_bits(a, whole_frame[FIRST][k]), k
    r.detach_comm()
    r.cleanup()
