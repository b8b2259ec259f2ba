"""rt_accumulate_motion on the GPU against tests/motion_ref.py, bit for bit.

The harness is tests/test_gpu_accumulate.py's (its helpers are copied, that file is not changed): synthetic guides
uploaded as tensors, guard bands around every buffer the call writes, and here also around the motion records, which
hold exactly instance_count records: a kernel that read a record for the instance id past them would find the guard's
fill, an unknown flag, and reset pixels the reference keeps.  tests/test_motion_ref.py shows on the CPU that the
restatement tells the motion classes apart and that no fault of the kernel could hide."""
import ctypes as C

import numpy as np
import pytest

import accumulate_ref as A
import guided_ref as G
import motion_ref as M
from rtamd import Renderer, abi, scenes
from rtamd.renderer import hits_to_numpy

pytestmark = pytest.mark.gpu

GUARD = 256                                    # bytes kept around every guarded buffer (a multiple of 16)
FILL = 0xA5
SIZES_VIEWS = [(w, h, v) for (w, h) in A.SIZES for v in M.VIEWS]


def upload(g):
    import torch
    H, W = g["color"].shape[:2]
    rec = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(H, W, 48).copy()).cuda()
    f32 = lambda a: torch.from_numpy(np.array(a, np.float32)).cuda()
    t = {"color": f32(g["color"]), "hits": rec(g["hits"]), "prev_hits": rec(g["prev_hits"]),
         "prev_history": f32(g["prev_history"])}
    for k in ("albedo", "prev_moments"):
        if k in g:
            t[k] = f32(g[k])
    return t


def rows_struct(view):
    if view is None:
        return None
    r = abi.Reprojection()
    for k in ("centre", "rx", "ry", "rw"):
        for a in range(3):
            getattr(r, k)[a] = float(view[k][a])
    return r


def guarded(nbytes):
    import torch
    return torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")


def inner(buf, dtype, shape):
    return buf[GUARD:buf.numel() - GUARD].view(dtype).reshape(shape)


def guarded_records(records):
    """The records in a buffer of exactly their size between two guard bands."""
    import torch
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1)
    buf = guarded(raw.size)
    if raw.size:
        buf[GUARD:GUARD + raw.size] = torch.from_numpy(raw.copy()).cuda()
    return buf


def call(lib, t, view, records, *, moments=False, entry="motion", stream=None, flags=0, device=0, **over):
    """One call of rt_accumulate_motion (entry "motion"; records None: a NULL buffer and a count of 0), or of the
    parent's rt_accumulate / rt_accumulate_moments (entry "parent") on the same buffers.  Returns (history [H, W, 4],
    rgb [H, W, 3], moments [H, W, 2] | None) as numpy arrays after checking that every guard band kept its fill."""
    import torch
    H, W = t["color"].shape[:2]
    n = W * H
    kw = dict(M.KW)
    kw.update(over)
    d = abi.AccumulateDesc()
    d.width, d.height, d.flags = W, H, flags
    d.max_history, d.normal_cos, d.plane_tolerance = kw["max_history"], kw["normal_cos"], kw["plane_tolerance"]
    rows = rows_struct(view)
    if rows is not None:
        d.prev_view = C.pointer(rows)
    bufs = {"history": guarded(16 * n), "rgb": guarded(12 * n)}
    d.history_device, d.rgb32_device = bufs["history"].data_ptr() + GUARD, bufs["rgb"].data_ptr() + GUARD
    assert d.history_device % 16 == 0
    d.color_device, d.hits_device = t["color"].data_ptr(), t["hits"].data_ptr()
    d.prev_hits_device, d.prev_history_device = t["prev_hits"].data_ptr(), t["prev_history"].data_ptr()
    d.stream = stream.cuda_stream if stream is not None else None
    m = None
    if moments:
        m = abi.MomentsDesc()
        bufs["moments"] = guarded(8 * n)
        m.albedo_device, m.prev_moments_device = t["albedo"].data_ptr(), t["prev_moments"].data_ptr()
        m.moments_device = bufs["moments"].data_ptr() + GUARD
    mo = abi.MotionDesc()
    if records is not None:
        bufs["records"] = guarded_records(records)
        mo.motion_device, mo.instance_count = bufs["records"].data_ptr() + GUARD, len(records)
        assert mo.motion_device % 16 == 0
    torch.cuda.synchronize()
    if entry == "motion":
        rc = lib.rt_accumulate_motion(device, C.byref(d), C.byref(m) if moments else None, C.byref(mo))
    elif moments:
        rc = lib.rt_accumulate_moments(device, C.byref(d), C.byref(m))
    else:
        rc = lib.rt_accumulate(device, C.byref(d))
    assert rc == abi.RT_OK, lib.rt_last_error()
    if stream is not None:
        stream.synchronize()
    elif flags & abi.RT_ACCUMULATE_NO_SYNC:
        torch.cuda.synchronize()
    for k, b in bufs.items():
        raw = b.cpu().numpy()
        assert (raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all(), f"{k}: bytes beyond the buffer were written"
    if records is not None:                                    # an input: the call leaves it as it was
        assert np.array_equal(inner(bufs["records"], torch.uint8, (-1,)).cpu().numpy(),
                              np.ascontiguousarray(records).view(np.uint8).reshape(-1))
    history = inner(bufs["history"], torch.float32, (H, W, 4)).cpu().numpy()
    rgb = inner(bufs["rgb"], torch.float32, (H, W, 3)).cpu().numpy()
    mom = inner(bufs["moments"], torch.float32, (H, W, 2)).cpu().numpy() if moments else None
    return history, rgb, mom


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def assert_is_reference(name, got, want):
    wrong = (bits(got) != bits(want)).any(axis=-1)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{name}: {int(wrong.sum())} of {wrong.size} pixels differ from the float32 reference, max |gpu - ref| = {err:.3g}")
    assert not wrong.any(), (name, int(wrong.sum()), err)


# ---- synthetic cases -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ("r", "b"))
@pytest.mark.parametrize("case", SIZES_VIEWS, ids=lambda c: "%dx%d_%s" % c)
def test_matches_reference_bit_for_bit(gpu_lib, monkeypatch, case, form):
    """Every size of accumulate_ref.SIZES under every view that has a prev_view, in both pixel mappings, without and
    with the moments: history, rgb and moments equal tests/motion_ref.py's."""
    g = M.case(*case)
    t = upload(g)
    monkeypatch.setenv("RTAMD_ACCUMULATE_FORM", form)
    name = "%dx%d %s form=%s" % (case + (form,))
    history, rgb, _ = call(gpu_lib, t, g["view"], g["records"])
    assert_is_reference(name, history, g["history32"])
    assert same_bits(rgb, history[..., :3])
    history, rgb, mom = call(gpu_lib, t, g["view"], g["records"], moments=True)
    assert_is_reference(name + " moments: history", history, g["moments32"][0])
    assert_is_reference(name + " moments", mom, g["moments32"][1])
    assert same_bits(rgb, history[..., :3])
    assert same_bits(history, g["history32"])                 # the moments change no colour


@pytest.mark.parametrize("case", ((1, 1, "same"), (9, 9, "moved"), (65, 2, "pan"), (37, 23, "moved"), (96, 64, "moved"),
                                  (96, 64, "behind")), ids=lambda c: "%dx%d_%s" % c)
def test_static_records_and_no_records_equal_the_parent(gpu_lib, case):
    """On the parent's own cases: all-static records, and no records at all, give rt_accumulate's and
    rt_accumulate_moments' bytes."""
    g = G.moments_case(*case)
    t = upload(g)
    static = np.zeros(4, M.motion_dtype())
    static["point"], static["normal"] = np.eye(3, 4, dtype=np.float32), np.eye(3, dtype=np.float32)
    for moments in (False, True):
        want = call(gpu_lib, t, g["view"], None, moments=moments, entry="parent")
        assert same_bits(want[0], g["with_albedo32"][0] if moments else g["ref32"])
        for records in (static, static[:1], None):             # the sphere's id inside the records, past them, none
            got = call(gpu_lib, t, g["view"], records, moments=moments)
            for a, b in zip(got, want):
                assert (a is None and b is None) or a.tobytes() == b.tobytes()


def test_no_records_with_a_still_camera_equals_the_parent(gpu_lib):
    """instance_count == 0 needs no prev_view: the single-tap path of the parent."""
    g = G.moments_case(37, 23, "null")
    t = upload(g)
    for moments in (False, True):
        want = call(gpu_lib, t, None, None, moments=moments, entry="parent")
        got = call(gpu_lib, t, None, None, moments=moments)
        for a, b in zip(got, want):
            assert (a is None and b is None) or a.tobytes() == b.tobytes()


def test_inaccessible_and_overlapping_records_are_rejected(gpu_lib):
    import torch
    g = M.case(8, 8, "same")
    t = upload(g)
    n = 64
    d = abi.AccumulateDesc()
    d.width, d.height = 8, 8
    d.max_history, d.normal_cos, d.plane_tolerance = A.MAX_HISTORY, A.NORMAL_COS, A.PLANE_TOLERANCE
    rows = rows_struct(g["view"])
    d.prev_view = C.pointer(rows)
    history = torch.zeros((8, 8, 4), device="cuda")
    d.color_device, d.hits_device = t["color"].data_ptr(), t["hits"].data_ptr()
    d.prev_hits_device, d.prev_history_device = t["prev_hits"].data_ptr(), t["prev_history"].data_ptr()
    d.history_device = history.data_ptr()
    records = torch.from_numpy(np.ascontiguousarray(g["records"]).view(np.uint8).copy()).cuda()
    mo = abi.MotionDesc()
    mo.motion_device, mo.instance_count = records.data_ptr(), len(g["records"])
    assert gpu_lib.rt_accumulate_motion(0, C.byref(d), None, C.byref(mo)) == abi.RT_OK, gpu_lib.rt_last_error()
    host = np.zeros(96 * 8 + 16, np.uint8)
    mo.motion_device = host.ctypes.data // 16 * 16 + 16       # pageable host memory
    assert gpu_lib.rt_accumulate_motion(0, C.byref(d), None, C.byref(mo)) == 1
    assert b"accessible" in gpu_lib.rt_last_error()
    mo.motion_device = history.data_ptr() + 16 * n - 16       # the last texel of the output
    assert gpu_lib.rt_accumulate_motion(0, C.byref(d), None, C.byref(mo)) == 1
    assert b"overlap" in gpu_lib.rt_last_error()
    mo.motion_device = records.data_ptr()
    assert gpu_lib.rt_accumulate_motion(gpu_lib.rt_device_count(), C.byref(d), None, C.byref(mo)) == 1
    current = torch.cuda.current_device()
    assert gpu_lib.rt_accumulate_motion(0, C.byref(d), None, C.byref(mo)) == abi.RT_OK
    assert torch.cuda.current_device() == current


# ---- a real scene ----------------------------------------------------------------------------------------------------

W, H = 64, 48
MESH = 0                                        # the instance that moves
CAMERA = dict(scenes.DEMO_CAMERA, center=(0.0, 1.6, 6.0), target=(0.0, 0.7, 0.0), fov=40.0, ray_trace_depth=2, sample_count=1)
CAMERA_BEFORE = dict(center=(0.25, 1.7, 5.9), target=(0.05, 0.7, 0.0))     # where the moved camera stood in the first frame
XFORMS = (dict(shift=(-0.3, 1.0, 0.0), rotate=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)),
          dict(shift=(0.3, 1.1, 0.2), rotate=(0.0, 25.0, 10.0), scale=(1.0, 1.0, 1.0)))
KW = dict(max_history=A.MAX_HISTORY, normal_cos=A.NORMAL_COS, plane_tolerance=A.PLANE_TOLERANCE)


def small_scene():
    """A 256-triangle unit sphere mesh with vertex normals (the instance that moves), the ground as a large sphere, a
    small sphere and a parallelogram."""
    verts, faces = scenes.uv_sphere_template(256)
    vn = scenes._vertex_normals(verts, faces)
    tris = np.zeros(len(faces), scenes.TRIANGLE_DTYPE)
    tris["vertex"], tris["normal"], tris["has_normals"] = verts[faces], vn[faces], 1
    tris["material_type"], tris["material_index"] = abi.ROUGH, 0
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    mesh = dict(type=abi.TRIANGLE, index=0, count=len(faces), centroid=(0.0, 0.0, 0.0),
                bounds=tuple(float(x) for x in (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])), **XFORMS[0])
    return scenes.Scene(spheres=[(abi.ROUGH, 1, (0.0, 0.0, 0.0), 1.0)],
                        parallelograms=[(abi.ROUGH, 2, (-0.5, 0.0, -0.5), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))], triangles=tris,
                        roughs=[(.65, .05, .05), (.73, .73, .73), (.12, .45, .15)], metals=[],
                        instances=[mesh, dict(type=abi.SPHERE, index=0, shift=(0.0, -500.0, 0.0), scale=(500.0, 500.0, 500.0)),
                                   dict(type=abi.SPHERE, index=0, shift=(2.0, 0.4, -1.0), scale=(0.4, 0.4, 0.4)),
                                   dict(type=abi.PARALLELOGRAM, index=0, shift=(-2.2, 0.0, -1.0), rotate=(0.0, 30.0, 0.0))],
                        animated=False, camera=dict(CAMERA))


def xform_rows(scene, mesh):
    rows = []
    for k, d in enumerate(scene.instances):
        d = dict(d, **mesh) if k == MESH else d
        rows.append(tuple(d.get("shift", (0, 0, 0))) + tuple(d.get("rotate", (0, 0, 0))) + tuple(d.get("scale", (1, 1, 1))))
    return np.asarray(rows, np.float32)


def two_frames(r, scene, moved_camera, stream=None, sync=True, records=None, guided=False, render=False):
    """The first frame with the mesh at XFORMS[0], the second with it at XFORMS[1], through update_instances; per frame
    query_camera's hits and a constant colour (render: the frame rendered with one sample) go to accumulate, the second
    time with `records` and the previous camera's rows.  -> (frames: [{"hits", "color", "out"}], the rows, the filtered
    second frame or None)."""
    import contextlib
    import torch
    import rtamd
    frames, prev, view, den = [], None, None, None
    for f in (0, 1):
        if f == 1:
            r.update_instances(MESH, [dict(scene.instances[MESH], **XFORMS[1])])
        r.configure_camera(W, H, **(CAMERA_BEFORE if moved_camera and f == 0 else {}))
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            color = torch.full((H, W, 3), 0.5 + 0.25 * f, dtype=torch.float32, device="cuda")
        if render:
            r.render(f, frame_seed=0x5EED + f, want_rgba=False, rgb32_device=color.data_ptr(),
                     stream=stream.cuda_stream if stream is not None else None, sync=sync)
        else:
            r.update(f)
        q = r.query_camera(want_t=False, want_hits=True, want_albedo=True, stream=stream, sync=sync)
        kw = dict(KW, stream=stream, sync=sync, moments=guided, albedo=q["albedo"] if guided else None)
        if f == 0:
            prev = r.accumulate(color, q["hits"], None, **kw)
        else:
            prev = r.accumulate(color, q["hits"], prev, prev_view=view, motion=records, **kw)
            if guided:
                den = r.denoise_guided(prev, q["albedo"], stream=stream, sync=sync)
        frames.append({"hits": q["hits"], "color": color, "out": prev})
        view = rtamd.reprojection(r.camera, W, H)              # this frame's camera: the next frame's prev_view
    return frames, view, den


def rows_dict(r):
    return {k: np.array(list(getattr(r, k)), np.float32) for k in ("centre", "rx", "ry", "rw")}


@pytest.mark.parametrize("moved_camera", (False, True), ids=("still_camera", "moved_camera"))
def test_a_moving_mesh_keeps_its_history(gpu_lib, moved_camera):
    """64 x 48, four instances, the mesh translating and turning between two frames.  The GPU's second frame equals the
    restatement on the downloaded records bit for bit, with the records of rtamd.instance_motion and without any; by
    the restatement's own count the mesh's pixels of length 2 are some with the records and none without."""
    import rtamd
    scene = small_scene()
    records = rtamd.instance_motion(xform_rows(scene, XFORMS[0]), xform_rows(scene, XFORMS[1]))
    assert list(records["flags"]) == [M.MOVED, M.STATIC, M.STATIC, M.STATIC]
    results = {}
    for name, recs in (("records", records), ("none", None)):
        r = Renderer(scene, update=False).build_acceleration_structure(7)
        frames, _, _ = two_frames(r, scene, moved_camera, records=recs)
        view = rows_dict(rtamd.reprojection(scene.camera_input(**(CAMERA_BEFORE if moved_camera else {})), W, H))
        r.cleanup()
        hits = [hits_to_numpy(f["hits"]).reshape(H, W) for f in frames]
        first = frames[0]["out"]["history"].cpu().numpy()
        ref, _, valid = M.accumulate_motion(frames[1]["color"].cpu().numpy(), hits[1], hits[0], first, view,
                                            records if recs is not None else records[:0], **KW)
        results[name] = (frames[1]["out"]["history"].cpu().numpy(), ref, valid, hits)
    got, ref, valid, hits = results["records"]
    mesh = hits[1]["instance"] == MESH
    assert mesh.sum() > 100 and (hits[0]["instance"] == MESH).sum() > 100
    # the move is larger than the plane test's tolerance at every pixel of the mesh, so the test can catch it
    carried = M.carry(hits[1], records)
    moved_by = np.linalg.norm(carried["point"].astype(np.float64) - hits[1]["point"], axis=-1)
    assert (moved_by[mesh] > A.PLANE_TOLERANCE * hits[1]["t"][mesh]).all()
    # ... and on the reference, before the GPU is looked at: at most half of the mesh's pixels find no tap on it
    without_tap = mesh & ~valid.any(axis=-1)
    print(f"mesh pixels {int(mesh.sum())}, without a tap on the mesh in the previous frame {int(without_tap.sum())}")
    assert 2 * without_tap.sum() <= mesh.sum()
    kept = {k: int((mesh & (results[k][1][..., 3] == 2.0)).sum()) for k in results}
    print("mesh pixels of length 2 after the second frame:", kept)
    assert kept["records"] > 0 and kept["none"] == 0
    for k in results:
        assert_is_reference(f"mesh {'moved' if moved_camera else 'still'} camera, {k}", results[k][0], results[k][1])
    # pixels off the mesh do not depend on the records
    assert same_bits(results["records"][0][~mesh], results["none"][0][~mesh])


def test_one_stream_without_host_sync_equals_the_synchronous_run(gpu_lib):
    """render -> query_camera -> accumulate(motion=..., moments) -> denoise_guided, sync=False on one torch stream: the
    bytes of the synchronous run, and the caller's current device stays."""
    import torch
    import rtamd
    scene = small_scene()
    records = rtamd.instance_motion(xform_rows(scene, XFORMS[0]), xform_rows(scene, XFORMS[1]))
    current = torch.cuda.current_device()
    out = []
    for stream in (None, torch.cuda.Stream()):
        r = Renderer(scene, update=False).build_acceleration_structure(7)
        frames, _, den = two_frames(r, scene, True, stream=stream, sync=stream is None, records=records, guided=True,
                                    render=True)
        if stream is not None:
            stream.synchronize()
        r.synchronize()
        out.append([frames[1]["out"][k].cpu().numpy() for k in ("history", "rgb", "moments")] + [den["rgb"].cpu().numpy()])
        r.cleanup()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
    assert (out[0][0][..., 3] == 2.0).any()
    assert torch.cuda.current_device() == current
    # a device tensor of the records is taken as it is
    r = Renderer(scene, update=False).build_acceleration_structure(7)
    dev = torch.from_numpy(records.view(np.uint8).reshape(-1, 96).copy()).cuda()
    frames, _, _ = two_frames(r, scene, True, records=dev, guided=True, render=True)
    assert frames[1]["out"]["history"].cpu().numpy().tobytes() == out[0][0].tobytes()
    with pytest.raises(ValueError):
        r.accumulate(frames[1]["color"], frames[1]["hits"], frames[0]["out"], motion=records, **KW)      # no prev_view
    r.cleanup()
