"""Python mirror of the reference's host `Renderer` (include/Global/Renderer.cuh:109-146) over
the C ABI of librtamd.so.  Method names follow the reference lifecycle:

    commitGeometryData + commitMaterialData + configureInstances -> Renderer(scene)
    buildAccelerationStructure                                   -> build_acceleration_structure()
    configureCamera                                              -> configure_camera()
    one iteration of startRender                                 -> render(frame)
    cleanup                                                      -> cleanup()

There is no CPU fallback: constructing a Renderer without librtamd.so or without a GPU raises.
"""
from __future__ import annotations

import ctypes as C
import sys
from contextlib import nullcontext as _null_context

import numpy as np

from . import abi

HIT_DTYPE = np.dtype([("t", np.float32), ("instance", np.uint32), ("ptype", np.uint32),
                      ("pindex", np.uint32), ("point", np.float32, 3), ("normal", np.float32, 3),
                      ("mtype", np.uint32), ("midx", np.uint32)])     # rt_hit, as Renderer.trace_rays returns it


# Renderer.denoise's default (sigma_color, sigma_normal, sigma_plane): the best point of the grid in
# profiles/denoise/README.md (the C2 scene at 1080p, 1 sample per pixel, against 1 024 samples)
DENOISE_SIGMAS = (3.0, 0.1, 0.1)


# Renderer.denoise_guided's default (sigma_luminance, sigma_normal, sigma_plane): the best point, an interior one, of
# the grid in profiles/guided/README.md (the C2 scene at 1080p, 64 accumulated one-sample frames from a still and a
# strafing camera, against 1 024 samples).  sigma_luminance is dimensionless, in standard deviations of the accumulated
# colour's luminance, and the same for every frame: the score stays within 1.4 % of the best from 2 to 16.
# sigma_plane was not varied: rt_denoise's grid found it flat on this scene, and its 0.1 world units are kept.
GUIDED_SIGMAS = (4.0, 0.1, 0.1)


# Renderer.accumulate's default (max_history, normal_cos, plane_tolerance): the best interior point of the grid in
# profiles/accumulate/README.md (the C2 scene at 1080p with a strafing camera, 96 frames of 1 sample per pixel, against
# 1 024 samples).  The error still falls with a longer history, ever more slowly, and does not depend on the plane
# tolerance while nothing in the scene moves.
ACCUMULATE_DEFAULTS = (32.0, 0.999, 0.02)


def reprojection(camera_input: abi.CameraInput, width: int, height: int) -> abi.Reprojection:
    """rt_camera_reprojection: the rows that map a world point to the frame of `camera_input` at this size (host only,
    no scene, no GPU): what Renderer.accumulate takes as prev_view when the camera has moved since the last frame."""
    lib = abi.load_library()
    out = abi.Reprojection()
    abi.check(lib, lib.rt_camera_reprojection(C.byref(camera_input), int(width), int(height), C.byref(out)))
    return out


MOTION_DTYPE = np.dtype([("point", np.float32, (3, 4)), ("normal", np.float32, (3, 3)), ("flags", np.uint32),
                         ("reserved", np.uint32, 2)])                # rt_instance_motion, 96 bytes
XFORM_DTYPE = np.dtype([("shift", np.float32, 3), ("rotate_deg", np.float32, 3), ("scale", np.float32, 3)])   # rt_xform


def _xforms(x, name):
    """An rt_xform array as numpy: a ctypes array of abi.Xform, a structured array of XFORM_DTYPE, or floats [n, 9]
    (shift, rotate in degrees, scale)."""
    if isinstance(x, C.Array) and issubclass(x._type_, abi.Xform):
        return np.frombuffer(x, dtype=XFORM_DTYPE).copy()
    a = np.asarray(x)
    if a.dtype == XFORM_DTYPE:
        return np.ascontiguousarray(a).reshape(-1)
    if a.dtype.fields is not None or a.ndim != 2 or a.shape[1] != 9:
        raise ValueError(f"{name}: a ctypes array of abi.Xform, a numpy array of XFORM_DTYPE or floats [n, 9]")
    return np.ascontiguousarray(a, np.float32).view(XFORM_DTYPE).reshape(-1)


def instance_motion(prev_xforms, cur_xforms) -> np.ndarray:
    """rt_instance_motion_records: one record per instance that carries a world point and normal of this frame back to
    where the instance stood in the last one (host only, no scene, no GPU), from last frame's and this frame's
    transforms (see _xforms for the forms taken).  Returns a numpy array of MOTION_DTYPE: what Renderer.accumulate
    takes as motion."""
    lib = abi.load_library()
    prev, cur = _xforms(prev_xforms, "prev_xforms"), _xforms(cur_xforms, "cur_xforms")
    if len(prev) != len(cur):
        raise ValueError(f"prev_xforms holds {len(prev)} transforms, cur_xforms {len(cur)}")
    out = np.zeros(len(cur), MOTION_DTYPE)
    as_ptr = lambda a, t: C.cast(a.ctypes.data, C.POINTER(t))
    abi.check(lib, lib.rt_instance_motion_records(as_ptr(prev, abi.Xform), as_ptr(cur, abi.Xform), len(cur),
                                                  as_ptr(out, abi.InstanceMotion)))
    return out


def hits_to_numpy(hits) -> np.ndarray:
    """The rt_hit records of Renderer.query_rays (torch uint8 [N, 48], any device) as the structured array
    Renderer.trace_rays returns."""
    raw = hits.detach().cpu().numpy() if hasattr(hits, "detach") else np.asarray(hits, np.uint8)
    return np.ascontiguousarray(raw).reshape(-1, HIT_DTYPE.itemsize).view(HIT_DTYPE).reshape(-1).copy()


def _raw_stream(stream):
    """The hipStream_t of a descriptor's stream field: of a torch stream, or the raw handle given; None for the null
    stream."""
    return (stream.cuda_stream if hasattr(stream, "cuda_stream") else stream) or None


def checked(x, tail, dtype, name, dev):
    """x as a filter call takes it: a contiguous torch tensor [h, w, tail] of dtype on the torch device dev."""
    import torch                                  # here: `import rtamd` needs no torch

    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name}: a torch tensor")
    if x.dtype != dtype:
        raise ValueError(f"{name}: {dtype}, not {x.dtype}")
    if x.device != dev:
        raise ValueError(f"{name}: on {x.device}, the scene is on {dev}")
    if x.dim() != 3 or x.shape[2] != tail:
        raise ValueError(f"{name}: shape [h, w, {tail}], not {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError(f"{name}: not contiguous")
    return x


class Renderer:
    def __init__(self, scene, device: int = 0, update=None):
        """update: None -> the scene's own animation (Main.cu updateInstance via the native
        rt_demo_update when scene.animated), False -> static, or a Python callable
        f(xforms: ctypes array of Xform, n, frame) (slow path, crosses into Python per frame)."""
        self.lib = abi.load_library()
        self.scene = scene
        self._cb = None
        if update is None:
            fn = C.cast(self.lib.rt_demo_update, C.c_void_p) if scene.animated else None
        elif update is False:
            fn = None
        else:
            self._cb = abi.UPDATE_FN(lambda user, xs, n, frame: update(xs, n, frame))
            fn = C.cast(self._cb, C.c_void_p)
        self._desc = scene.desc(fn)
        h = C.c_void_p()
        abi.check(self.lib, self.lib.rt_scene_create(C.byref(self._desc), device, C.byref(h)))
        self.h = h
        self.device = device
        self.width = self.height = 0

    def _torch_call(self, stream):
        """What a call on torch tensors starts with: (torch, the scene's torch device, the stream — torch's current one
        if none was given —, the context that makes it torch's current stream while the call allocates, or a null
        context for a raw hipStream_t, and the raw handle for the descriptor)."""
        import torch                              # here: `import rtamd` needs no torch

        dev = torch.device("cuda", self.device)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        ctx = torch.cuda.stream(stream) if isinstance(stream, torch.cuda.Stream) else _null_context()
        return torch, dev, stream, ctx, _raw_stream(stream)

    # ---- lifecycle ---------------------------------------------------------------------
    def build_acceleration_structure(self, seed: int = 0, mode: str = "compat"):
        """mode "compat": the reference's random-axis median split (pinned seed); "sah": SAH trees;
        "lbvh": BLASes and the per-frame TLAS built on the GPU (linear BVH)."""
        m = {"compat": abi.RT_BUILD_COMPAT_MEDIAN, "sah": abi.RT_BUILD_SAH, "lbvh": abi.RT_BUILD_LBVH}[mode]
        abi.check(self.lib, self.lib.rt_scene_build(self.h, m, seed))
        return self

    def configure_camera(self, width: int, height: int, **camera):
        ci = self.scene.camera_input(**camera)
        abi.check(self.lib, self.lib.rt_camera_set(self.h, C.byref(ci), width, height))
        self.width, self.height = width, height
        self.camera = ci
        return self

    def set_camera(self, camera_input: abi.CameraInput):
        """Renderer::configureCamera with an explicit CameraInput (the interactive loop's moved camera,
        Renderer.cu:247-251 -> RenderPin.cu:73-95), same framebuffer size."""
        abi.check(self.lib, self.lib.rt_camera_set(self.h, C.byref(camera_input), self.width, self.height))
        self.camera = camera_input
        return self

    def set_comm_timeout(self, timeout_ms: int):
        """rt_comm_set_timeout: bounded waits on multi-GPU frames (0 = unbounded, async errors still polled)."""
        abi.check(self.lib, self.lib.rt_comm_set_timeout(self.h, int(timeout_ms)))
        return self

    def set_option(self, key: str, value: int):
        abi.check(self.lib, self.lib.rt_scene_set_option(self.h, key.encode(), int(value)))
        return self

    def update_triangles(self, first: int, triangles):
        """Replace triangles [first, first + len) (scenes.TRIANGLE_DTYPE array); "lbvh" scenes only."""
        t = np.ascontiguousarray(triangles)
        abi.check(self.lib, self.lib.rt_scene_update_triangles(self.h, first, t.shape[0], t.ctypes.data))
        return self

    def update_triangles_device(self, first: int, vertices, normals=None, stream=None, sync: bool = True,
                                bounds: bool = False):
        """rt_scene_update_triangles_device: the geometry of triangles [first, first + n) from device memory; "lbvh"
        scenes only.  vertices (and optionally normals): 9 floats per triangle, either an object with data_ptr() — a
        torch tensor: float32, contiguous, numel() == 9 n, on the scene's device — or a (device pointer, n) tuple.
        Materials stay; without normals each triangle keeps its normals (a flat one follows its new vertices).
        stream: the stream the buffers were produced on, a raw hipStream_t or an object with .cuda_stream (None =
        torch's current stream when torch is loaded, else the null stream).  With sync=False the call returns after
        the enqueue; the buffers may be overwritten in stream order either way.  bounds=True (RT_TRI_UPDATE_BOUNDS):
        the device derives the local bounds of every triangle instance the range overlaps, so instances without
        bounds of their own are accepted and a mesh may leave the bounds it was built with."""
        def stream_of(x, name):
            if isinstance(x, tuple):
                ptr, n = x
                return int(ptr or 0), int(n)
            if not hasattr(x, "data_ptr"):
                raise ValueError(f"{name}: a tensor with data_ptr() or a (pointer, triangle count) tuple")
            if str(x.dtype) != "torch.float32":
                raise ValueError(f"{name}: float32, not {x.dtype}")
            if not x.is_contiguous():
                raise ValueError(f"{name}: not contiguous")
            dev = x.device
            if dev.type != "cuda" or (dev.index if dev.index is not None else 0) != self.device:
                raise ValueError(f"{name}: on {dev}, the scene is on cuda:{self.device}")
            if x.numel() % 9:
                raise ValueError(f"{name}: 9 floats per triangle, not {x.numel()} in all")
            return (x.data_ptr() if x.numel() else 0), x.numel() // 9

        vptr, n = stream_of(vertices, "vertices")
        nptr = 0
        if normals is not None:
            nptr, nn = stream_of(normals, "normals")
            if nn != n:
                raise ValueError(f"normals: {nn} triangles, vertices hold {n}")
        if stream is None:
            torch = sys.modules.get("torch")       # never imported here: `import rtamd` needs no torch
            if torch is not None and torch.cuda.is_available():
                stream = torch.cuda.current_stream(self.device)
        u = abi.TriangleUpdate()
        u.first, u.count = first, n
        u.vertices_device = vptr or None
        u.normals_device = nptr or None
        u.flags = (0 if sync else abi.RT_TRI_UPDATE_NO_SYNC) | (abi.RT_TRI_UPDATE_BOUNDS if bounds else 0)
        u.stream = _raw_stream(stream)
        abi.check(self.lib, self.lib.rt_scene_update_triangles_device(self.h, C.byref(u)))
        return self

    def update_instances(self, first: int, instances):
        """Replace instance descriptions [first, first + len) (dicts as in scenes.Scene.instances)."""
        from .scenes import instance_desc_array
        arr = instance_desc_array(instances)
        abi.check(self.lib, self.lib.rt_scene_update_instances(self.h, first, len(instances), arr))
        return self

    def update(self, frame: int):
        abi.check(self.lib, self.lib.rt_scene_update(self.h, frame))

    def render(self, frame: int = 0, frame_seed: int = 0x5EED, exact: bool = False, count_work: bool = False,
               want_rgb: bool = False, want_rgba: bool = True, skip_update: bool = False,
               tiles=None, rgba8_device=None, rgb32_device=None, stream=None, sync: bool = True,
               keep_counters: bool = False):
        """One frame.  Returns (rgba[H,W,4] uint8 | None, rgb[H,W,3] float32 | None, stats dict).
        tiles = (tile_w, tile_h, rank, count) renders a tile shard into tile-compact outputs."""
        o = abi.RenderOpts()
        o.frame_seed = frame_seed
        o.flags = (abi.RT_RENDER_EXACT if exact else 0) | (abi.RT_RENDER_COUNT_WORK if count_work else 0) | \
                  (abi.RT_RENDER_SKIP_UPDATE if skip_update else 0) | (0 if sync else abi.RT_RENDER_NO_SYNC) | \
                  (abi.RT_RENDER_KEEP_COUNTERS if keep_counters else 0)
        comm = getattr(self, "comm", None)
        if comm is not None and comm[0] != 0:
            want_rgba = False                     # only rank 0 receives the assembled frame
        if tiles is not None:
            o.tile_w, o.tile_h, o.tile_rank, o.tile_count = tiles
            npix = self.tiles_for_rank(*tiles) * tiles[0] * tiles[1]
            shape = (npix,)
        else:
            shape = (self.height, self.width)
        o.rgba8_device = rgba8_device
        o.rgb32_device = rgb32_device
        o.stream = stream
        rgba = np.zeros(shape + (4,), np.uint8) if (want_rgba and sync) else None
        rgb = np.zeros(shape + (3,), np.float32) if (want_rgb and sync) else None
        st = abi.Stats()
        abi.check(self.lib, self.lib.rt_render(self.h, frame, C.byref(o),
                                               rgba.ctypes.data if rgba is not None else None,
                                               rgb.ctypes.data if rgb is not None else None, C.byref(st)))
        stats = {k: getattr(st, k) for k, _ in abi.Stats._fields_}
        return rgba, rgb, stats

    def collect(self, capacity: int = 256):
        """After pipelined renders: (accumulated stats dict, list of per-frame kernel ms)."""
        st = abi.Stats()
        ms = (C.c_float * capacity)()
        n = C.c_uint32()
        abi.check(self.lib, self.lib.rt_scene_collect(self.h, C.byref(st), ms, capacity, C.byref(n)))
        return {k: getattr(st, k) for k, _ in abi.Stats._fields_}, [ms[i] for i in range(n.value)]

    def debug_read(self, name: str) -> np.ndarray:
        """Debug buffer of the last launch that recorded it ("timeline", "costmap"), as raw bytes."""
        n = C.c_size_t()
        abi.check(self.lib, self.lib.rt_scene_debug_read(self.h, name.encode(), None, 0, C.byref(n)))
        buf = np.zeros(n.value, np.uint8)
        abi.check(self.lib, self.lib.rt_scene_debug_read(self.h, name.encode(), buf.ctypes.data, n.value, C.byref(n)))
        return buf

    def timeline(self):
        """Per-wave timeline of the last persistent launch (set_option("timeline", 1) first).
        Structured array: start/end in s_memrealtime ticks (100 MHz), xcc, hw_id, pixels."""
        w = self.debug_read("timeline").view(np.uint64).reshape(-1, 24)
        out = np.zeros(len(w), dtype=[("start", np.uint64), ("end", np.uint64), ("xcc", np.uint32),
                                      ("hw_id", np.uint32), ("pixels", np.uint32), ("exhaust", np.uint64),
                                      ("rounds", np.uint32), ("shades", np.uint32), ("grabs", np.uint32),
                                      ("cyc_refill", np.uint64), ("cyc_interior", np.uint64), ("cyc_leaf", np.uint64),
                                      ("cyc_shade", np.uint64), ("iters", np.uint64), ("refill_iters", np.uint64),
                                      ("cyc_lanes", np.uint64), ("cyc_scatter", np.uint64),
                                      ("lanes_interior", np.uint64), ("lanes_leaf_tlas", np.uint64),
                                      ("lanes_leaf_blas", np.uint64), ("lanes_shade", np.uint64),
                                      ("lanes_postpone", np.uint64), ("iters_idle", np.uint64),
                                      ("hits", np.uint64), ("hits_last_rough", np.uint64)])
        out["start"], out["end"], out["exhaust"] = w[:, 0], w[:, 1], w[:, 4]
        out["xcc"], out["hw_id"], out["pixels"] = w[:, 2] & 0xFFFFFFFF, w[:, 2] >> 32, w[:, 3]
        out["rounds"], out["shades"], out["grabs"] = w[:, 5], w[:, 6], w[:, 7]
        out["cyc_refill"], out["cyc_interior"], out["cyc_leaf"], out["cyc_shade"] = w[:, 8], w[:, 9], w[:, 10], w[:, 11]
        out["iters"], out["refill_iters"] = w[:, 12], w[:, 13]
        out["cyc_lanes"], out["cyc_scatter"] = w[:, 14], w[:, 15]       # diagnostic builds only: lane refill work, scatter sampling
        # diagnostic builds only: lane sums per interior iteration / leaf phase (TLAS, BLAS leaves) / shade step
        out["lanes_interior"], out["lanes_leaf_tlas"], out["lanes_leaf_blas"], out["lanes_shade"] = w[:, 16], w[:, 17], w[:, 18], w[:, 19]
        # ... lanes postponing a leaf in the interior loop, interior iterations without a node step, shaded hits and
        # those on a path's last segment with a rough material
        out["lanes_postpone"], out["iters_idle"], out["hits"], out["hits_last_rough"] = w[:, 20], w[:, 21], w[:, 22], w[:, 23]
        return out

    def costmap(self):
        """Traversal rounds per output pixel of the last COUNT_WORK render with option "costmap"."""
        return self.debug_read("costmap").view(np.uint32)

    def tiles_for_rank(self, tile_w, tile_h, rank, count):
        return int(self.lib.rt_tiles_for_rank(self.h, tile_w, tile_h, rank, count))

    def assemble_tiles(self, gathered_device, slab_tiles, tile_w, tile_h, tile_count, frame_device, stream=None):
        abi.check(self.lib, self.lib.rt_assemble_tiles(self.h, gathered_device, slab_tiles, tile_w, tile_h,
                                                       tile_count, frame_device, stream))

    # ---- multi-GPU frames (rt_scene_attach_comm) ---------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        """Rank 0: a fresh RCCL unique id (128 bytes) to hand to every rank out of band."""
        lib = abi.load_library()
        cid = abi.CommId()
        abi.check(lib, lib.rt_comm_unique_id(C.byref(cid)))
        return bytes(bytearray(cid))

    def attach_comm(self, comm_id: bytes, rank: int, world: int, tile_w: int = 64, tile_h: int = 64):
        """Make this scene rank `rank` of a `world`-GPU frame: render() traces this rank's tiles, gathers
        them to rank 0 over RCCL and assembles the frame there (collective over the ranks)."""
        cid = abi.CommId.from_buffer_copy(bytes(comm_id))
        abi.check(self.lib, self.lib.rt_scene_attach_comm(self.h, C.byref(cid), rank, world, tile_w, tile_h))
        self.comm = (rank, world, tile_w, tile_h)
        return self

    def detach_comm(self):
        abi.check(self.lib, self.lib.rt_scene_detach_comm(self.h))
        self.comm = None
        return self

    def trace_rays(self, rays, exact: bool = False):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        hits = (abi.Hit * max(1, n))()
        abi.check(self.lib, self.lib.rt_trace_rays(self.h, rays.ctypes.data, n,
                                                   abi.RT_RENDER_EXACT if exact else 0, hits))
        out = np.zeros(n, dtype=[("t", np.float32), ("instance", np.uint32), ("ptype", np.uint32),
                                 ("pindex", np.uint32), ("point", np.float32, 3), ("normal", np.float32, 3),
                                 ("mtype", np.uint32), ("midx", np.uint32)])
        out[:] = np.frombuffer(hits, dtype=out.dtype, count=n)
        return out

    def query_rays(self, rays, tmax=None, *, any_hit: bool = False, exact: bool = False, want_hits: bool = True,
                   stream=None, sync: bool = True):
        """rt_query_rays on device tensors: rays [N, 6] (origin, direction) and optional tmax [N] (range
        [0.001, tmax], None = +inf) as torch CUDA float32 tensors on the scene's device (numpy arrays are uploaded
        through torch).  stream: a torch.cuda.Stream or a raw hipStream_t (None = torch's current stream).
        Closest mode returns (t float32 [N] with +inf on a miss, hits uint8 [N, 48] rt_hit records — see
        hits_to_numpy — or None without want_hits); any_hit returns occluded bool [N].  With sync=False the call
        returns after the enqueue and the tensors are valid in stream order."""
        # uploads and outputs are made on the query's stream (ctx), so they are ordered with the launch and torch's
        # allocator orders their reuse with it.  A raw hipStream_t gives torch nothing to order with: a numpy input's
        # upload is then waited for, and the call waits for the query before the temporary is released.
        torch, dev, stream, ctx, raw = self._torch_call(stream)
        uploaded = []

        def device_f32(x, shape, name):
            if isinstance(x, np.ndarray):
                x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
                uploaded.append(x)
            if not isinstance(x, torch.Tensor):
                raise ValueError(f"{name}: a torch tensor or a numpy array")
            if x.dtype != torch.float32:
                raise ValueError(f"{name}: float32, not {x.dtype}")
            if x.device != dev:
                raise ValueError(f"{name}: on {x.device}, the scene is on {dev}")
            if tuple(x.shape[1:]) != shape or x.dim() != 1 + len(shape):
                raise ValueError(f"{name}: shape [N{''.join(', %d' % k for k in shape)}], not {tuple(x.shape)}")
            if not x.is_contiguous():
                raise ValueError(f"{name}: not contiguous")
            return x

        with ctx:
            rays = device_f32(rays, (6,), "rays")
            n = rays.shape[0]
            if tmax is not None:
                tmax = device_f32(tmax, (), "tmax")
                if tmax.shape[0] != n:
                    raise ValueError("tmax: one value per ray")
        if uploaded and not isinstance(stream, torch.cuda.Stream):
            torch.cuda.current_stream(dev).synchronize()
            sync = True
        q = abi.RayQuery()
        q.rays_device = rays.data_ptr() if n else None
        q.tmax_device = tmax.data_ptr() if (tmax is not None and n) else None
        q.ray_count = n
        q.flags = (abi.RT_QUERY_EXACT if exact else 0) | (abi.RT_QUERY_ANY_HIT if any_hit else 0) | \
                  (0 if sync else abi.RT_QUERY_NO_SYNC)
        q.stream = raw
        with ctx:
            if any_hit:
                occ = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
                q.occluded_device = occ.data_ptr()
            else:
                t = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
                hits = torch.empty((max(n, 1), C.sizeof(abi.Hit)), dtype=torch.uint8, device=dev) if want_hits else None
                q.t_device = t.data_ptr()
                q.hits_device = hits.data_ptr() if want_hits else None
        abi.check(self.lib, self.lib.rt_query_rays(self.h, C.byref(q)))
        if any_hit:
            return occ[:n].view(torch.bool)
        return t[:n], (hits[:n] if want_hits else None)

    def query_camera(self, rect=None, *, first_sample: bool = False, frame_seed: int = 0x5EED, exact: bool = False,
                     want_rays: bool = False, want_t: bool = True, want_hits: bool = False, want_albedo: bool = False,
                     stream=None, sync: bool = True):
        """rt_query_camera: the camera's own rays over rect = (x0, y0, width, height) of the current frame (None: the
        whole frame; row 0 is the bottom row), traced on the device.  The rays go through the pixel centres, or with
        first_sample are the rays render() starts each pixel's first path with for frame_seed.  Returns a dict of
        torch CUDA tensors with the keys asked for: "t" float32 [h, w] (+inf on a miss), "rays" float32 [h, w, 6],
        "hits" uint8 [h, w, 48] (rt_hit records, see hits_to_numpy) and "albedo" float32 [h, w, 3] (the hit
        material's albedo, the background on a miss).  stream: a torch.cuda.Stream or a raw hipStream_t (None =
        torch's current stream); with sync=False the call returns after the enqueue and the tensors are valid in
        stream order."""
        torch, dev, stream, ctx, raw = self._torch_call(stream)
        x0, y0, w, h = (0, 0, self.width, self.height) if rect is None else (int(v) for v in rect)
        q = abi.CameraQuery()
        q.x0, q.y0, q.width, q.height = x0, y0, w, h
        q.frame_seed = frame_seed
        q.flags = (abi.RT_CAMERA_QUERY_EXACT if exact else 0) | (0 if sync else abi.RT_CAMERA_QUERY_NO_SYNC) | \
                  (abi.RT_CAMERA_QUERY_FIRST_SAMPLE if first_sample else 0)
        q.stream = raw
        out = {}
        with ctx:                                 # outputs made on the query's stream, as query_rays
            for want, key, field, tail, dtype in ((want_rays, "rays", "rays_device", (6,), torch.float32),
                                                  (want_t, "t", "t_device", (), torch.float32),
                                                  (want_hits, "hits", "hits_device", (C.sizeof(abi.Hit),), torch.uint8),
                                                  (want_albedo, "albedo", "albedo_device", (3,), torch.float32)):
                if want:
                    buf = torch.empty((max(h, 0) * max(w, 0) + 1,) + tail, dtype=dtype, device=dev)
                    setattr(q, field, buf.data_ptr())
                    out[key] = buf
        abi.check(self.lib, self.lib.rt_query_camera(self.h, C.byref(q)))
        return {k: v[:h * w].reshape((h, w) + tuple(v.shape[1:])) for k, v in out.items()}

    def denoise(self, rgb, hits, albedo=None, *, iterations: int = 5, sigma_color: float = DENOISE_SIGMAS[0],
                sigma_normal: float = DENOISE_SIGMAS[1], sigma_plane: float = DENOISE_SIGMAS[2],
                want_rgba: bool = False, out=None, stream=None, sync: bool = True):
        """rt_denoise: the edge-avoiding a-trous filter (include/rt.h, "Denoising") on torch CUDA tensors of the
        shapes render and query_camera produce: rgb float32 [h, w, 3] (a frame rendered into rgb32_device), hits uint8
        [h, w, 48] (query_camera(want_hits=True)) and optionally albedo float32 [h, w, 3] (want_albedo=True), all
        contiguous and on the scene's device.  The sigma defaults are the best point of the grid in
        profiles/denoise/README.md; float("inf") switches a term off.  out: the float32 [h, w, 3] tensor to write,
        which may be rgb itself (None: a new one).  Returns {"rgb": out} and, with want_rgba, "rgba" uint8 [h, w, 4].
        stream: a torch.cuda.Stream or a raw hipStream_t (None = torch's current stream); the scratch and the outputs
        are allocated on it, and with sync=False the call returns after the enqueue."""
        torch, dev, stream, ctx, raw = self._torch_call(stream)

        rgb = checked(rgb, 3, torch.float32, "rgb", dev)
        h, w = int(rgb.shape[0]), int(rgb.shape[1])
        for x, tail, dtype, name in ((hits, C.sizeof(abi.Hit), torch.uint8, "hits"), (albedo, 3, torch.float32, "albedo"),
                                     (out, 3, torch.float32, "out")):
            if x is not None or name == "hits":
                if tuple(checked(x, tail, dtype, name, dev).shape[:2]) != (h, w):
                    raise ValueError(f"{name}: {tuple(x.shape[:2])}, rgb is {(h, w)}")
        if not isinstance(stream, torch.cuda.Stream):
            sync = True      # a raw hipStream_t gives torch nothing to order the scratch's release with (as query_rays)
        d = abi.DenoiseDesc()
        d.width, d.height, d.iterations = w, h, int(iterations)
        d.flags = 0 if sync else abi.RT_DENOISE_NO_SYNC
        d.sigma_color, d.sigma_normal, d.sigma_plane = float(sigma_color), float(sigma_normal), float(sigma_plane)
        d.scratch_bytes = self.lib.rt_denoise_scratch_bytes(w, h)
        d.stream = raw
        with ctx:                                 # made on the call's stream, as query_camera's outputs
            if out is None:
                out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
            rgba = torch.empty((h, w, 4), dtype=torch.uint8, device=dev) if want_rgba else None
            scratch = torch.empty(max(int(d.scratch_bytes), 16), dtype=torch.uint8, device=dev)
        res = {"rgb": out}
        if want_rgba:
            res["rgba"] = rgba
        if h * w == 0:
            return res
        d.color_device, d.hits_device = rgb.data_ptr(), hits.data_ptr()
        d.albedo_device = albedo.data_ptr() if albedo is not None else None
        d.rgb32_device = out.data_ptr()
        d.rgba8_device = rgba.data_ptr() if want_rgba else None
        d.scratch_device = scratch.data_ptr()
        abi.check(self.lib, self.lib.rt_denoise(self.device, C.byref(d)))
        return res

    def accumulate(self, rgb, hits, prev=None, *, prev_view=None, max_history: float = ACCUMULATE_DEFAULTS[0],
                   normal_cos: float = ACCUMULATE_DEFAULTS[1], plane_tolerance: float = ACCUMULATE_DEFAULTS[2],
                   out_rgb=None, stream=None, sync: bool = True, albedo=None, moments: bool = False, motion=None):
        """rt_accumulate: temporal accumulation (include/rt.h, "Temporal accumulation") on torch CUDA tensors of the
        shapes render and query_camera produce: rgb float32 [h, w, 3] (this frame, rendered into rgb32_device) and hits
        uint8 [h, w, 48] (query_camera(want_hits=True) of this frame), contiguous and on the scene's device.  prev: the
        dict the last call returned (None: the first frame, every pixel restarts).  prev_view: rtamd.reprojection of the
        last frame's camera (None: the camera has not moved).  The threshold defaults are the best point of the grid in
        profiles/accumulate/README.md; normal_cos=-inf and plane_tolerance=inf switch a test off.  out_rgb: the float32
        [h, w, 3] tensor to write, which may be rgb itself (None: a new one).  Returns {"history": float32 [h, w, 4]
        (r, g, b, length), "rgb": out_rgb, "hits": hits}: pass it back as prev for the next frame, and leave its
        tensors unchanged until that call has run.  stream: a torch.cuda.Stream or a raw hipStream_t (None = torch's
        current stream); the outputs are allocated on it, and with sync=False the call returns after the enqueue.
        moments=True is rt_accumulate_moments (include/rt.h, "Variance-guided denoising"): the same history and rgb, and
        the dict also holds "moments", float32 [h, w, 2], the first two moments of the luminance of rgb / albedo (albedo:
        float32 [h, w, 3], optional, the one denoise_guided will be given); prev must then be a dict of such a call.
        motion: rt_accumulate_motion (include/rt.h, "Moving instances"), with or without the moments: the records of
        rtamd.instance_motion as the numpy array it returns (uploaded on the call's stream) or as a contiguous uint8 or
        float32 CUDA tensor of [n, 96] bytes, indexed by the hits' instance; with prev given it needs prev_view (a still
        camera passes rtamd.reprojection of its own camera)."""
        torch, dev, stream, ctx, raw = self._torch_call(stream)

        rgb = checked(rgb, 3, torch.float32, "rgb", dev)
        h, w = int(rgb.shape[0]), int(rgb.shape[1])
        nhit = C.sizeof(abi.Hit)
        named = [(hits, nhit, torch.uint8, "hits")]
        if out_rgb is not None:
            named.append((out_rgb, 3, torch.float32, "out_rgb"))
        if prev is not None:
            named += [(prev["hits"], nhit, torch.uint8, "prev hits"), (prev["history"], 4, torch.float32, "prev history")]
        if albedo is not None and not moments:
            raise ValueError("albedo: only the moments read it (moments=True)")
        if moments:
            if prev is not None and "moments" not in prev:
                raise ValueError("prev: it holds no moments (the last call had moments=False)")
            if prev is not None:
                named.append((prev["moments"], 2, torch.float32, "prev moments"))
            if albedo is not None:
                named.append((albedo, 3, torch.float32, "albedo"))
        for x, tail, dtype, name in named:
            if tuple(checked(x, tail, dtype, name, dev).shape[:2]) != (h, w):
                raise ValueError(f"{name}: {tuple(x.shape[:2])}, rgb is {(h, w)}")
        if prev_view is not None and not isinstance(prev_view, abi.Reprojection):
            raise ValueError("prev_view: an abi.Reprojection (rtamd.reprojection)")
        if not isinstance(stream, torch.cuda.Stream):
            sync = True      # a raw hipStream_t gives torch nothing to order the outputs' allocation with (as denoise)
        nrec = C.sizeof(abi.InstanceMotion)
        if motion is not None:
            if prev is not None and prev_view is None:
                raise ValueError("motion: prev_view is needed (a still camera passes rtamd.reprojection of its own camera)")
            if isinstance(motion, np.ndarray):
                if motion.dtype != MOTION_DTYPE:
                    raise ValueError("motion: a numpy array of MOTION_DTYPE (rtamd.instance_motion)")
                host = torch.from_numpy(np.ascontiguousarray(motion).reshape(-1).view(np.uint8).reshape(-1, nrec))
                with ctx:                         # uploaded on the call's stream
                    motion = host.to(dev, non_blocking=False)
            elif not (isinstance(motion, torch.Tensor) and motion.device == dev and motion.is_contiguous() and motion.dim() == 2
                      and motion.dtype in (torch.uint8, torch.float32)
                      and motion.shape[1] * motion.element_size() == nrec):
                raise ValueError(f"motion: rtamd.instance_motion's array, or a contiguous uint8 / float32 tensor of [n, {nrec}] "
                                 f"bytes on {dev}")
        d = abi.AccumulateDesc()
        d.width, d.height = w, h
        d.flags = 0 if sync else abi.RT_ACCUMULATE_NO_SYNC
        d.max_history, d.normal_cos, d.plane_tolerance = float(max_history), float(normal_cos), float(plane_tolerance)
        d.stream = raw
        with ctx:                                 # made on the call's stream, as query_camera's outputs
            history = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
            if out_rgb is None:
                out_rgb = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
            mom = torch.empty((h, w, 2), dtype=torch.float32, device=dev) if moments else None
        res = {"history": history, "rgb": out_rgb, "hits": hits}
        if moments:
            res["moments"] = mom
        if h * w == 0:
            return res
        if prev_view is not None:
            d.prev_view = C.pointer(prev_view)
        d.color_device, d.hits_device = rgb.data_ptr(), hits.data_ptr()
        if prev is not None:
            d.prev_hits_device, d.prev_history_device = prev["hits"].data_ptr(), prev["history"].data_ptr()
        d.history_device, d.rgb32_device = history.data_ptr(), out_rgb.data_ptr()
        m = None
        if moments:
            m = abi.MomentsDesc()
            m.albedo_device = albedo.data_ptr() if albedo is not None else None
            m.prev_moments_device = prev["moments"].data_ptr() if prev is not None else None
            m.moments_device = mom.data_ptr()
        if motion is not None:
            mo = abi.MotionDesc()
            mo.instance_count = int(motion.shape[0])
            mo.motion_device = motion.data_ptr() if mo.instance_count else None
            abi.check(self.lib, self.lib.rt_accumulate_motion(self.device, C.byref(d), C.byref(m) if moments else None,
                                                              C.byref(mo)))
        elif moments:
            abi.check(self.lib, self.lib.rt_accumulate_moments(self.device, C.byref(d), C.byref(m)))
        else:
            abi.check(self.lib, self.lib.rt_accumulate(self.device, C.byref(d)))
        return res

    def denoise_guided(self, acc, albedo=None, *, iterations: int = 5, sigma_luminance: float = GUIDED_SIGMAS[0],
                       sigma_normal: float = GUIDED_SIGMAS[1], sigma_plane: float = GUIDED_SIGMAS[2],
                       want_rgba: bool = False, want_variance: bool = False, out=None, stream=None, sync: bool = True,
                       feedback: bool = False):
        """rt_denoise_guided: the variance-steered a-trous filter (include/rt.h, "Variance-guided denoising") on the
        dict accumulate(..., moments=True) returned: its history, moments and hits, and optionally the albedo that call
        was given.  sigma_luminance is dimensionless and needs no scaling per frame; float("inf") switches a term off.
        out: the float32 [h, w, 3] tensor to write (None: a new one).  Returns {"rgb": out} and, with want_rgba, "rgba"
        uint8 [h, w, 4]; with want_variance, "variance" float32 [h, w], the variance of the accumulated luminance the
        first pass starts from.  stream and sync as denoise.
        feedback=True is rt_denoise_guided_feedback (include/rt.h, "History feedback"): the same outputs, and the dict
        also holds "history", a new float32 [h, w, 4] tensor with the first pass's colour and acc's lengths, and "prev",
        {**acc, "history": that tensor}, which the next frame's accumulate takes as prev; acc itself is left as it was.
        Off by default, for what profiles/feedback/README.md measured on C2's scene at 1080p over 64 frames: on the
        frozen scene the flicker falls by 3 to 6 %, with the animation running it does not change, and the error against
        1 024 spp rises by 2 to 4 % in all three runs (the variance still describes the unfiltered mean, so the filter
        blurs more); a call costs 1.1 to 1.4 % more."""
        torch, dev, stream, ctx, raw = self._torch_call(stream)

        if not isinstance(acc, dict) or "moments" not in acc:
            raise ValueError("acc: the dict accumulate(..., moments=True) returned")
        history = checked(acc["history"], 4, torch.float32, "history", dev)
        h, w = int(history.shape[0]), int(history.shape[1])
        for x, tail, dtype, name in ((acc["moments"], 2, torch.float32, "moments"),
                                     (acc["hits"], C.sizeof(abi.Hit), torch.uint8, "hits"),
                                     (albedo, 3, torch.float32, "albedo"), (out, 3, torch.float32, "out")):
            if x is not None or name in ("moments", "hits"):
                if tuple(checked(x, tail, dtype, name, dev).shape[:2]) != (h, w):
                    raise ValueError(f"{name}: {tuple(x.shape[:2])}, the history is {(h, w)}")
        if not isinstance(stream, torch.cuda.Stream):
            sync = True      # a raw hipStream_t gives torch nothing to order the scratch's release with (as denoise)
        d = abi.DenoiseGuidedDesc()
        d.width, d.height, d.iterations = w, h, int(iterations)
        d.flags = 0 if sync else abi.RT_DENOISE_NO_SYNC
        d.sigma_luminance, d.sigma_normal, d.sigma_plane = float(sigma_luminance), float(sigma_normal), float(sigma_plane)
        d.scratch_bytes = self.lib.rt_denoise_guided_scratch_bytes(w, h)
        d.stream = raw
        with ctx:                                 # made on the call's stream, as query_camera's outputs
            if out is None:
                out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
            rgba = torch.empty((h, w, 4), dtype=torch.uint8, device=dev) if want_rgba else None
            variance = torch.empty((h, w), dtype=torch.float32, device=dev) if want_variance else None
            scratch = torch.empty(max(int(d.scratch_bytes), 16), dtype=torch.uint8, device=dev)
            fed = torch.empty((h, w, 4), dtype=torch.float32, device=dev) if feedback else None
        res = {"rgb": out}
        if want_rgba:
            res["rgba"] = rgba
        if want_variance:
            res["variance"] = variance
        if feedback:
            res["history"] = fed
            res["prev"] = {**acc, "history": fed}
        if h * w == 0:
            return res
        d.history_device, d.moments_device, d.hits_device = history.data_ptr(), acc["moments"].data_ptr(), acc["hits"].data_ptr()
        d.albedo_device = albedo.data_ptr() if albedo is not None else None
        d.rgb32_device = out.data_ptr()
        d.rgba8_device = rgba.data_ptr() if want_rgba else None
        d.variance_device = variance.data_ptr() if want_variance else None
        d.scratch_device = scratch.data_ptr()
        if feedback:
            f = abi.FeedbackDesc()
            f.feedback_device = fed.data_ptr()
            abi.check(self.lib, self.lib.rt_denoise_guided_feedback(self.device, C.byref(d), C.byref(f)))
        else:
            abi.check(self.lib, self.lib.rt_denoise_guided(self.device, C.byref(d)))
        return res

    def synchronize(self):
        abi.check(self.lib, self.lib.rt_synchronize(self.h))

    def info(self):
        i = abi.SceneInfo()
        abi.check(self.lib, self.lib.rt_scene_get_info(self.h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in abi.SceneInfo._fields_}

    def export_blas(self, b: int):
        nn, npr = C.c_uint32(), C.c_uint32()
        abi.check(self.lib, self.lib.rt_scene_export_blas(self.h, b, None, None, None, C.byref(nn), C.byref(npr)))
        boxes = np.zeros((nn.value, 6), np.float32)
        ci = np.zeros((nn.value, 2), np.uint32)
        refs = np.zeros(npr.value, np.uint32)
        abi.check(self.lib, self.lib.rt_scene_export_blas(self.h, b, boxes.ctypes.data, ci.ctypes.data,
                                                          refs.ctypes.data, C.byref(nn), C.byref(npr)))
        return boxes, ci, refs

    def export_tlas(self):
        nn, npr = C.c_uint32(), C.c_uint32()
        abi.check(self.lib, self.lib.rt_scene_export_tlas(self.h, None, None, None, C.byref(nn), C.byref(npr)))
        boxes = np.zeros((nn.value, 6), np.float32)
        ci = np.zeros((nn.value, 2), np.uint32)
        refs = np.zeros(npr.value, np.uint32)
        abi.check(self.lib, self.lib.rt_scene_export_tlas(self.h, boxes.ctypes.data, ci.ctypes.data,
                                                          refs.ctypes.data, C.byref(nn), C.byref(npr)))
        return boxes, ci, refs

    def cleanup(self):
        if getattr(self, "h", None):
            self.lib.rt_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.cleanup()


BOX_MODES = {"reference": 0, "cull": 1, "decide": 2, "quad_pair": 3, "quad_greedy": 4}   # rt_box_mode (include/rt.h)


def box_test(boxes, rays, tmax=None, mode: str = "reference", device: int = 0):
    """rt_box_test: which boxes the trace kernel named by `mode` keeps for each (box, ray) in range [0.001, tmax]
    (tmax None = +inf); returns (hit bool array, entry t array, +inf on a miss)."""
    lib = abi.load_library()
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = boxes.shape[0]
    if rays.shape[0] != n:
        raise ValueError("one ray per box")
    tm = np.full(n, np.inf, np.float32) if tmax is None else np.ascontiguousarray(
        np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
    hit = np.zeros(max(1, n), np.uint8)
    te = np.zeros(max(1, n), np.float32)
    abi.check(lib, lib.rt_box_test(device, boxes.ctypes.data, rays.ctypes.data, tm.ctypes.data, n, BOX_MODES[mode],
                                   hit.ctypes.data, te.ctypes.data))
    return hit[:n].astype(bool), te[:n]
