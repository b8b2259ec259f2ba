/*
 * rt.h — C ABI of the MI355X-native trace path (drop-in for the reference's
 * Scene / Camera / render(framebuffer) lifecycle).
 *
 * The reference has no FFI; its boundary is the static C++ class `Renderer`
 * (include/Global/Renderer.cuh:109-146) plus the kernel contract
 * `render(const TraverseData*, cudaSurfaceObject_t)` with a `__constant__ Camera`
 * (include/Global/RendererImpl.cuh:196-199).  Every entry point below names the
 * reference call it replaces.  All types are plain C: no torch, no HIP types.
 *
 * Conventions
 *  - Every call returns rt_status; on failure rt_last_error() returns a
 *    thread-local message.  The library never exit()s (the reference exits with
 *    -200 on any CUDA error, src/Global/Global.cu:34-41).
 *  - A scene is not thread-safe; use one scene per host thread (the reference
 *    drives everything from one thread, src/Global/Renderer.cu:180-366).
 *  - Framebuffer layout matches the reference surface: row-major W x H RGBA8,
 *    row 0 = bottom of the image (viewport origin bottom-left,
 *    src/Global/RenderPin.cu:91-92).
 */
#ifndef RT_H
#define RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: rt_stats gained update_wait_ms; rt_comm_* / rt_slab_tiles / rt_tile_pixels / rt_scene_detach_comm;
 *    rt_camera_move / rt_frame_pacer_* / rt_comm_set_timeout (round 3)
 * 3: rt_scene_info gained overlap_lanes / stage_depth; "overlap" -1 = library-picked lanes on library streams
 * 4: rt_query_rays
 * 5: rt_scene_update_triangles_device
 *    (RT_TRI_UPDATE_BOUNDS arrived within 5: a flag value that was rejected before is accepted now;
 *     rt_query_camera / rt_camera_query arrived within 5: a new entry point, no existing struct changed;
 *     rt_denoise / rt_denoise_scratch_bytes / rt_denoise_desc arrived within 5 the same way;
 *     rt_accumulate / rt_accumulate_desc / rt_camera_reprojection / rt_reprojection arrived within 5 the same way;
 *     rt_accumulate_moments / rt_moments_desc / rt_denoise_guided / rt_denoise_guided_scratch_bytes /
 *     rt_denoise_guided_desc arrived within 5 the same way;
 *     rt_instance_motion_records / rt_instance_motion / rt_accumulate_motion / rt_motion_desc arrived within 5 the same
 *     way;
 *     rt_denoise_guided_feedback / rt_feedback_desc arrived within 5 the same way) */
#define RT_ABI_VERSION 5u

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARGUMENT = 1,
    RT_ERR_DEVICE = 2,          /* HIP runtime error, or no GPU present        */
    RT_ERR_OUT_OF_MEMORY = 3,
    RT_ERR_STATE = 4,           /* call out of lifecycle order                 */
    RT_ERR_UNSUPPORTED = 5
} rt_status;

/* include/Basic/BasicTypes.cuh:9-11 */
typedef enum rt_primitive_type {
    RT_PRIM_SPHERE = 0,
    RT_PRIM_PARALLELOGRAM = 1,
    RT_PRIM_TRIANGLE = 2
} rt_primitive_type;

/* include/Basic/BasicTypes.cuh:14-16 */
typedef enum rt_material_type {
    RT_MAT_ROUGH = 0,
    RT_MAT_METAL = 1
} rt_material_type;

typedef struct rt_vec3 { float x, y, z; } rt_vec3;

/* Sphere(MaterialType, size_t, Point3 center, float radius) — include/Geometry/Sphere.cuh:27 */
typedef struct rt_sphere {
    rt_vec3 center;
    float radius;
    uint32_t material_type;
    uint32_t material_index;
} rt_sphere;

/* Parallelogram(MaterialType, size_t, q, u, v) — include/Geometry/Parallelogram.cuh:26-39 */
typedef struct rt_parallelogram {
    rt_vec3 q, u, v;
    uint32_t material_type;
    uint32_t material_index;
} rt_parallelogram;

/* Triangle(MaterialType, size_t, vertexes[, vertexNormals]) — include/Geometry/Triangle.cuh:26-46.
 * has_normals = 0 selects the 3-vertex constructor (all three normals = unit(e1 x e2)). */
typedef struct rt_triangle {
    rt_vec3 vertex[3];
    rt_vec3 normal[3];
    uint32_t material_type;
    uint32_t material_index;
    uint32_t has_normals;
    uint32_t reserved;
} rt_triangle;

/* Rough{albedo} — include/Material/Rough.cuh:11-12; Metal{albedo, fuzz} — include/Material/Metal.cuh:11-13 */
typedef struct rt_rough { rt_vec3 albedo; } rt_rough;
typedef struct rt_metal { rt_vec3 albedo; float fuzz; } rt_metal;

/* Instance::updateTransformArguments(shift, rotate(degrees, x->y->z), scale)
 * — src/AS/Instance.cu:4-17, src/Util/Matrix.cu:183-249. */
typedef struct rt_xform {
    rt_vec3 shift;
    rt_vec3 rotate_deg;
    rt_vec3 scale;
} rt_xform;

/* One entry of the reference instance map {PrimitiveType, primitiveIndex}
 * (src/Global/Main.cu:93-99) plus the fields VTK instances carry
 * (src/Global/VTKReader.cu:204-214).
 *  primitive_count == 0 -> single-primitive instance; local bounds / centroid come
 *    from the primitive (src/Global/RenderPin.cu:124-139).
 *  primitive_count  > 0 -> a group of primitive_count primitives of one type starting at
 *    primitive_index; has_local_bounds = 1 supplies the pre-transform bounds/centroid the
 *    VTK reader would (bounds = [xmin,xmax,ymin,ymax,zmin,zmax]); has_local_bounds = 0
 *    uses the union of the primitive boxes and the mean of primitive centroids (extension).
 */
typedef struct rt_instance_desc {
    uint32_t primitive_type;
    uint32_t primitive_index;
    uint32_t primitive_count;
    uint32_t has_local_bounds;
    float local_bounds[6];
    rt_vec3 local_centroid;
    rt_xform xform;           /* initial transform (used when no update callback is set) */
} rt_instance_desc;

/* Per-frame instance update, replaces
 * void (*updateInstances)(Instance*, size_t instanceCount, size_t frameCount)
 * (include/Global/Renderer.cuh:94).  The callback rewrites the (shift, rotate, scale)
 * triple of each instance; the library then recomputes matrices and bounds exactly like
 * Instance::updateTransformArguments and rebuilds the TLAS (src/Global/Renderer.cu:269-276). */
typedef void (*rt_update_fn)(void *user, rt_xform *xforms, size_t instance_count, uint64_t frame);

/* GeometryData + MaterialData + instance map (include/Global/Renderer.cuh:33-43,
 * src/Global/Renderer.cu:9-121).  The caller keeps ownership; the library copies. */
typedef struct rt_scene_desc {
    const rt_sphere *spheres;               size_t sphere_count;
    const rt_parallelogram *parallelograms; size_t parallelogram_count;
    const rt_triangle *triangles;           size_t triangle_count;
    const rt_rough *roughs;                 size_t rough_count;
    const rt_metal *metals;                 size_t metal_count;
    const rt_instance_desc *instances;      size_t instance_count;
    rt_update_fn update;
    void *update_user;
} rt_scene_desc;

/* CameraInput — include/Global/Renderer.cuh:54-64 (field for field). */
typedef struct rt_camera_input {
    rt_vec3 background;
    rt_vec3 center;
    rt_vec3 target;
    float fov;                 /* horizontal field of view, degrees */
    rt_vec3 up;
    float focus_disk_radius;
    float sample_range;        /* carried, unused (as in the reference) */
    uint32_t sample_count;     /* traced samples = floor(sqrt(n))^2 (RenderPin.cu:93) */
    uint32_t ray_trace_depth;
} rt_camera_input;

/* BVH build policy.  COMPAT_MEDIAN restates BLAS::constructBLAS / TLAS::constructTLAS
 * (src/AS/BLAS.cu:4-117, src/AS/TLAS.cu:4-129): top-down median split on a pseudo-random
 * axis, leaf <= 4 primitives (BLAS) / <= 2 instances (TLAS).  The reference draws the axis
 * from std::mt19937(random_device); here the axis stream is a pinned function of `seed`
 * so builds are reproducible, and centroid ties are broken by primitive index. */
typedef enum rt_build_mode {
    RT_BUILD_COMPAT_MEDIAN = 0,
    /* Surface-area-heuristic BLAS and per-frame TLAS (leaf <= 4 items).  Different trees than the
     * reference: hits agree except where two surfaces tie within the 1e-6 window. */
    RT_BUILD_SAH = 1,
    /* GPU builder: every BLAS and the per-frame TLAS are linear BVHs
     * (30-bit Morton order per tree, Karras radix-tree hierarchy, subtrees of <= 4 primitives /
     * <= 2 instances collapsed into leaves) built by HIP kernels on the scene's stream.  The host
     * still runs the update callback and the instance matrices (Instance.cu:4-17); the TLAS build
     * never blocks the host.  With rt_scene_set_option("rebuild", 1) every BLAS is rebuilt on the
     * GPU each frame (config C5's per-frame rebuild); rt_scene_update_triangles and
     * rt_scene_update_triangles_device mark them stale. */
    RT_BUILD_LBVH = 2
} rt_build_mode;

typedef enum rt_render_flags {
    RT_RENDER_EXACT = 1u << 0,        /* bit-faithful arithmetic (IEEE division, no FMA) */
    RT_RENDER_COUNT_WORK = 1u << 1,   /* fill rt_stats work counters (slower)              */
    RT_RENDER_NO_SYNC = 1u << 2,      /* return after enqueue (device outputs only)        */
    RT_RENDER_SKIP_UPDATE = 1u << 3,  /* do not run the instance update / TLAS rebuild (with
                                         "overlap": the frame waits for the whole launch that
                                         uploaded its frame block, i.e. it serialises with it);
                                         RT_ERR_STATE after rt_scene_update_triangles until a
                                         frame has run its update (which rebuilds the BLASes) */
    RT_RENDER_KEEP_COUNTERS = 1u << 4 /* accumulate device counters (see rt_scene_collect); a
                                         synchronous frame with "overlap" then waits for every lane
                                         and reports the totals over all lanes                 */
} rt_render_flags;

/* Per-call options for rt_render.  Zero-initialise, then set what you need. */
typedef struct rt_render_opts {
    uint64_t frame_seed;       /* replaces clock64() in curand_init (Kernel.cu:114); 0 -> 0x5EED */
    uint32_t flags;            /* rt_render_flags */
    /* Screen-tile sharding (multi-GPU): the frame is cut into tile_w x tile_h tiles in
     * row-major tile order; this call renders tiles t with t % tile_count == tile_rank.
     * tile_count == 0 renders the whole frame into the frame-layout outputs.
     * With tile_count > 0, device outputs are written tile-compact: local tile k occupies
     * pixels [k*tile_w*tile_h, (k+1)*tile_w*tile_h), row-major inside the tile. */
    uint32_t tile_w, tile_h;
    uint32_t tile_rank, tile_count;
    /* Optional device outputs (hipMalloc'd / torch device memory on this scene's GPU). */
    void *rgba8_device;        /* uchar4 per pixel */
    void *rgb32_device;        /* 3 floats per pixel, linear average before gamma */
    void *stream;              /* hipStream_t to enqueue on; NULL -> the scene's stream, and when a device
                                * output is given the frame is ordered after the caller's null-stream work
                                * enqueued before the call, and that null stream's later work after the frame */
} rt_render_opts;

typedef struct rt_stats {
    uint64_t rays;             /* closest-hit traversals (one per TLAS::hit call, Kernel.cu:68) */
    uint64_t pixels;
    uint64_t aabb_tests;       /* filled with RT_RENDER_COUNT_WORK */
    uint64_t triangle_tests;
    uint64_t sphere_quad_tests;  /* sphere + parallelogram tests                                */
    uint64_t quad_tests;         /* parallelogram tests                                         */
    uint64_t instance_visits;
    uint64_t hits;               /* closest hits found (rays - misses)                          */
    double kernel_ms;          /* device time of the trace kernel (HIP events)             */
    double frame_ms;           /* host wall time of the call                               */
    double update_ms;          /* host time of instance update + TLAS rebuild + upload     */
    double update_wait_ms;     /* part of update_ms blocked on the GPU (a staging buffer still
                                  read by an earlier frame's copy); the rest is host compute */
} rt_stats;
/* sizeof(rt_stats) == 96 on LP64 (RT_ABI_VERSION 3) */

/* Closest-hit record for rt_trace_rays (per-ray parity tests). */
typedef struct rt_hit {
    float t;
    uint32_t instance;         /* 0xFFFFFFFF = miss */
    uint32_t primitive_type;
    uint32_t primitive_index;  /* index into the caller's primitive array */
    rt_vec3 point;             /* world-space hit point   (Instance.cu:41) */
    rt_vec3 normal;            /* world-space unit normal (Instance.cu:44) */
    uint32_t material_type;
    uint32_t material_index;
} rt_hit;

typedef struct rt_scene rt_scene;

/* --- lifecycle ---------------------------------------------------------------- */

uint32_t rt_abi_version(void);
const char *rt_last_error(void);
/* Number of visible GPUs (0 when no HIP device is present). */
int rt_device_count(void);

/* Renderer::commitGeometryData + commitMaterialData + configureInstances
 * (src/Global/Renderer.cu:9-121).  Copies the description; no device work yet. */
rt_status rt_scene_create(const rt_scene_desc *desc, int device, rt_scene **out_scene);

/* Renderer::buildAccelerationStructure (src/Global/Renderer.cu:123-155): builds every BLAS
 * (deduplicated per (type, primitiveIndex), RenderPin.cu:99-201), uploads geometry, BVHs
 * and materials to HBM, and builds the frame-0 TLAS. */
rt_status rt_scene_build(rt_scene *scene, rt_build_mode mode, uint64_t seed);

/* Renderer::configureCamera (src/Global/Renderer.cu:157-178) ->
 * RendererImpl::calculateCameraProperties (src/Global/RenderPin.cu:73-95). */
rt_status rt_camera_set(rt_scene *scene, const rt_camera_input *camera,
                        uint32_t width, uint32_t height);

/* Host half of one iteration of startRender (src/Global/Renderer.cu:264-303): run the
 * instance update for `frame`, rebuild the TLAS and upload it (double-buffered). */
rt_status rt_scene_update(rt_scene *scene, uint64_t frame);

/* Device half of one iteration of startRender (src/Global/Renderer.cu:305-317) = the
 * `render` kernel (src/Global/Kernel.cu:105-147).  Unless RT_RENDER_SKIP_UPDATE is set,
 * first calls rt_scene_update(scene, frame).  Host outputs (may be NULL) receive the
 * frame after completion; device outputs are described in rt_render_opts.
 *
 * Traversal depth: a ray's traversal stack holds 64 entries, the reference's (BLAS.cu:129, TLAS.cu:138): 16 in
 * LDS, the rest paged to scratch in half-windows of 8.  A traversal that needs more loses 8 of its entries (the
 * half-window paged out last is overwritten) and goes on, so the pixel may miss geometry.  This is reported
 * only with RT_RENDER_COUNT_WORK and without RT_RENDER_NO_SYNC: the call then returns RT_ERR_UNSUPPORTED
 * ("traversal stack overflow") after the frame and its outputs are complete.  Without COUNT_WORK, and for
 * frames collected later (rt_scene_collect), an overflow is silent.  A binary tree holds one entry per level of
 * the current path and a TLAS leaf's remainder; a quad tree ("wide") at most 3 per two binary levels and 2 more
 * at a leaf: with tlas_height + blas_height_max <= 40 (rt_scene_info) no kernel reaches the 64 entries.  Deep
 * chains that page without overflowing are pinned by tests/test_gpu_deep_stack.py. */
rt_status rt_render(rt_scene *scene, uint64_t frame, const rt_render_opts *opts,
                    uint8_t *rgba8_host, float *rgb32_host, rt_stats *stats);

/* Assemble tile-compact buffers gathered from `tile_count` ranks into a frame-layout RGBA8
 * device buffer (the multi-GPU gather's scatter step).  `gathered` holds tile_count slabs of
 * slab_tiles tiles each (rank r's slab = its tiles in render order, padded). */
rt_status rt_assemble_tiles(rt_scene *scene, const void *gathered_device, uint32_t slab_tiles,
                            uint32_t tile_w, uint32_t tile_h, uint32_t tile_count,
                            void *frame_rgba8_device, void *stream);

/* Number of tiles rank `tile_rank` owns for the current camera size. */
uint32_t rt_tiles_for_rank(const rt_scene *scene, uint32_t tile_w, uint32_t tile_h,
                           uint32_t tile_rank, uint32_t tile_count);

/* --- multi-GPU frames: screen tiles + RCCL gather inside the library --------------
 * One process (or thread) per GPU, each holding its own scene built from the same inputs (the
 * reference is single-GPU: Renderer.cu:305-317 launches one kernel over the whole surface).  After
 * rt_scene_attach_comm, every rt_render of the scene traces only this rank's screen tiles (tile t of
 * the row-major tile grid belongs to rank t mod world), gathers the tiles to rank 0 over RCCL (grouped
 * ncclSend / ncclRecv, xGMI) and assembles the frame there (csrc/assemble.hip), all enqueued on the
 * call's stream.  Rank 0's rgba8 outputs receive the whole frame; other ranks' output arguments are
 * ignored.  Every rank must make the same sequence of rt_render calls (with "overlap", the same lane
 * sequence).  rgb32 outputs and rt_render_opts tile fields are rejected while attached; rt_stats count
 * this rank's work.  The assembled frame is byte-identical for any world size: the RNG is keyed by the
 * global padded pixel index. */
typedef struct rt_comm_id { char internal[128]; } rt_comm_id;      /* an ncclUniqueId */

/* Rank 0 creates the id (ncclGetUniqueId) and passes it to every rank out of band. */
rt_status rt_comm_unique_id(rt_comm_id *id);
/* Collective over the `world` ranks (same id, world, tile size); world == 1 is allowed.  librccl.so.1 is
 * resolved at this call (the one already in the process, else ROCm's): single-GPU callers never need it. */
rt_status rt_scene_attach_comm(rt_scene *scene, const rt_comm_id *id, int rank, int world,
                               uint32_t tile_w, uint32_t tile_h);
rt_status rt_scene_detach_comm(rt_scene *scene);

/* Tile bookkeeping shared by the kernels and the host (no GPU needed): the largest number of tiles a
 * rank owns (slabs are padded to it), and the frame pixel of slab pixels [first, first + n) of `rank`
 * (xy[2i], xy[2i+1]; -1, -1 for pixels outside the frame). */
uint32_t rt_slab_tiles(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t tile_count);
rt_status rt_tile_pixels(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t tile_rank,
                         uint32_t tile_count, uint64_t first, uint64_t n, int32_t *xy);

/* Trace arbitrary world rays (origin xyz, direction xyz per ray) against the current TLAS
 * with t in [0.001, inf) and return the closest hit (TLAS::hit, src/AS/TLAS.cu:131-201).
 * RT_ERR_STATE after rt_scene_update_triangles until a frame has run its update.
 * A traversal deeper than the 64 stack entries (see rt_render) is not reported here: the kernel counts the
 * overflow per lane and discards the count, and the ray's record is whatever the remaining entries give. */
rt_status rt_trace_rays(rt_scene *scene, const float *rays_host, size_t ray_count,
                        uint32_t flags, rt_hit *hits_host);

/* Ray queries: closest hit or occlusion for rays the caller holds in device memory, traced on the caller's
 * stream by the render kernel's traversal (persistent waves, quad trees, the scene region in LDS; csrc/ray_query.hpp).
 * The query reads the scene as of the last frame update (rt_scene_update, or rt_render without
 * RT_RENDER_SKIP_UPDATE), on every build mode and option rt_trace_rays works on.
 *
 * Rays     : 6 floats per ray, origin xyz then direction xyz, used as given (not normalised), like rt_trace_rays.
 * Range    : [0.001, tmax[i]] with the reference's range test (Range.cuh:33-43) — the traversal starts with
 *            currentRange.max = tmax[i] instead of +inf.  tmax_device NULL means +inf for every ray.  A ray with
 *            !(tmax > 0.001), NaN included, is a miss and is not traversed.  As in the reference the two ends of the
 *            test differ between primitives and boxes: a primitive's t is accepted when |t - tmax| < 1e-6 or
 *            0.001 < t < tmax, but a box is left out once its entry t >= tmax (BoundingBox.cu:34-72).  So tmax = t of
 *            a known hit, or one ulp above it, finds that hit again except where the surface touches a face of a box
 *            around it and the box's entry t rounds to t or above (the ground sphere's top under its box's top, the
 *            parallelogram in its q-centred box: 29 of 15 003 hits on the ray-query test scene); which boxes lie
 *            around a surface depends on the build mode.  Pass a bound with slack (the occlusion radius, 2 t) where
 *            the hit must be kept.  There is no per-ray tmin: the lower bound
 *            is the render kernel's constant, and a per-ray value would have to pass through every shared box and
 *            primitive test of that kernel, whose register budget is tight.  Start occlusion rays on a surface as the
 *            renderer starts its bounces: from the hit point, hits nearer than 0.001 are ignored.
 * Closest  : (RT_QUERY_ANY_HIT clear) at least one of hits_device / t_device; occluded_device must be NULL.
 *            hits_device[i] is exactly the record rt_trace_rays writes — a miss is t = +inf, instance 0xFFFFFFFF and
 *            every other field 0; t_device[i] = the hit's t, +inf on a miss.  With t_device alone the hit point,
 *            normal and material are never computed.
 * Any-hit  : (RT_QUERY_ANY_HIT) occluded_device[i] = 1 when anything lies in the ray's range, else 0; hits_device and
 *            t_device must be NULL.  The traversal stops at the first accepted hit; it is a prefix of the closest
 *            traversal, so a ray is occluded exactly when the closest query with the same flags finds a hit.
 * Flags    : RT_QUERY_EXACT selects the EXACT build's arithmetic and visit order (as RT_RENDER_EXACT); otherwise the FAST
 *            kernel of the scene's kind runs (option "fast_math" included).
 * Ordering : the launch is enqueued on `stream` (NULL: the scene's stream, ordered with the caller's null-stream work
 *            before and after the call as rt_render orders device outputs).  It waits for what it reads — the upload
 *            or GPU build of the last update's frame block and a BLAS build still running — for the scene's most
 *            recent launch and the last launch that read that frame block, and for the scene's previous query; with
 *            "overlap" it does not wait for the other lanes' frames.  Every later upload
 *            into a frame block and every later BLAS rebuild waits for the queries still in flight, so frames and
 *            queries may be enqueued back to back without host synchronisation.  Without RT_QUERY_NO_SYNC the call
 *            returns once the outputs are complete; with it, it returns after the enqueue: the outputs are ordered
 *            on `stream`, and rt_synchronize and rt_scene_destroy wait for every query.  Queries of one scene run
 *            in the order of their calls, whatever streams they are given and whatever frames lie between them.
 * Errors   : RT_ERR_INVALID_ARGUMENT for reserved != 0, unknown flags, ray_count > 0xFFFFFFFF, an output combination
 *            the mode does not allow, or a buffer that hipPointerGetAttributes does not report as accessible from the
 *            scene's device — all before anything is enqueued; RT_ERR_STATE before rt_scene_build and after
 *            rt_scene_update_triangles until a frame has run its update.  ray_count == 0 returns RT_OK and launches
 *            nothing.  The caller's current device is preserved.  Allowed while a communicator is attached: the query
 *            is local to this rank and launches no RCCL work.  A traversal deeper than the 64 stack entries (see
 *            rt_render) is not an error here either: the query kernel has no counter output, the overflow count
 *            stays in the lane, and the ray's answer comes from the entries that were kept. */
typedef enum rt_query_flags {
    RT_QUERY_EXACT   = 1u << 0,  /* the EXACT build's arithmetic and visit order (as RT_RENDER_EXACT) */
    RT_QUERY_ANY_HIT = 1u << 1,  /* occlusion: stop at the first accepted hit */
    RT_QUERY_NO_SYNC = 1u << 2   /* return after enqueue */
} rt_query_flags;

typedef struct rt_ray_query {
    const float *rays_device;    /* 6 floats per ray: origin xyz, direction xyz (used as given, like rt_trace_rays) */
    const float *tmax_device;    /* optional, 1 float per ray: range [0.001, tmax]; NULL = +inf */
    uint64_t ray_count;          /* <= 0xFFFFFFFF */
    uint32_t flags;
    uint32_t reserved;           /* 0 */
    rt_hit  *hits_device;        /* closest: optional; exactly the records rt_trace_rays writes (misses included) */
    float   *t_device;           /* closest: optional; t per ray, +inf on a miss */
    uint8_t *occluded_device;    /* any-hit: 1 / 0 per ray */
    void    *stream;             /* hipStream_t; NULL = the scene's stream, ordered with the null stream as rt_render documents */
} rt_ray_query;

rt_status rt_query_rays(rt_scene *scene, const rt_ray_query *query);

/* Camera ray queries: per pixel of a rectangle of the current camera frame, the camera's own ray, its closest hit and
 * the hit material's albedo, all on the device.  The ray is built in registers by the query kernel from the camera the
 * scene holds (csrc/ray_query.hpp): no ray buffer is written unless rays_device asks for one.
 *
 * Outputs  : each optional, at least one; row-major over the rectangle — pixel (x0 + i, y0 + j) is element
 *            j * width + i; row 0 is the bottom row, as in the framebuffer.
 * Rays     : evaluated without FMA contraction and with correctly rounded 1 / sqrt in all three flavours (option
 *            "fast_math" included, whose render kernels may start a path one rounding away from it).
 *            Default (pixel centre): origin = the camera's centre, direction = unit((pixel_origin + dx * (float)px +
 *            dy * (float)py) - centre) in the render kernels' operation order with the sample offset 0: no RNG and no
 *            focus disk, whatever the camera's sample_count and focus_disk_radius.  The picking and depth ray; it
 *            depends on no seed.
 *            RT_CAMERA_QUERY_FIRST_SAMPLE: the ray rt_render starts the pixel's first path with for frame_seed (0 ->
 *            0x5EED, as rt_render_opts.frame_seed): the pixel's RNG stream (keyed by the padded pitch), the jitter
 *            inside sample cell (0, 0) of the sqrt(sample_count) grid, and the focus disk when its radius is > 0.
 *            Only sample 0 is offered: a later sample's ray depends on the RNG values the pixel's earlier paths
 *            consumed, which only rendering them yields.
 * Trace    : closest hit over [0.001, +inf), the renderer's range, on the scene as of the last frame update and the
 *            camera as of this call (rt_camera_set).  hits_device[k] and t_device[k] are byte for byte what
 *            rt_query_rays writes for rays_device[k] with tmax_device NULL and the same EXACT flag.  albedo_device: the
 *            albedo of the hit's material slot, rough or metal; on a miss the camera's background (what multiplies
 *            the path there, and the usual convention for a denoiser's albedo guide).  With rays_device as the only
 *            output nothing is traversed.
 * Flags    : RT_CAMERA_QUERY_EXACT / RT_CAMERA_QUERY_NO_SYNC as RT_QUERY_EXACT / RT_QUERY_NO_SYNC.
 * Ordering : rt_query_rays' rules: `stream`, the null-stream behaviour, what the launch waits for, what waits for it,
 *            rt_synchronize and rt_scene_destroy.  Camera queries and ray queries of one scene share one sequence and
 *            run in the order of their calls.
 * Errors   : all before anything is enqueued.  RT_ERR_INVALID_ARGUMENT for a NULL scene or query, reserved != 0,
 *            unknown flags, no output buffer, a rectangle not inside the camera's frame (x0 + width and y0 + height
 *            checked without overflow), or a buffer that hipPointerGetAttributes does not report as accessible from
 *            the scene's device; RT_ERR_STATE before rt_scene_build, before the first rt_camera_set, and after a
 *            triangle update until a frame has run its update.  width * height == 0 returns RT_OK and launches
 *            nothing.  The caller's current device is preserved.  Allowed while a communicator is attached. */
typedef enum rt_camera_query_flags {
    RT_CAMERA_QUERY_EXACT        = 1u << 0,  /* as RT_QUERY_EXACT */
    RT_CAMERA_QUERY_NO_SYNC      = 1u << 2,  /* as RT_QUERY_NO_SYNC (same bit) */
    RT_CAMERA_QUERY_FIRST_SAMPLE = 1u << 3   /* the frame's own first camera ray */
} rt_camera_query_flags;

typedef struct rt_camera_query {
    uint32_t x0, y0, width, height; /* pixel rectangle of the current camera frame; row 0 = bottom, as the framebuffer */
    uint64_t frame_seed;            /* FIRST_SAMPLE only: as rt_render_opts.frame_seed (0 -> 0x5EED) */
    uint32_t flags;
    uint32_t reserved;              /* 0 */
    float  *rays_device;            /* optional, 6 floats per pixel: origin xyz, direction xyz */
    float  *t_device;               /* optional, 1 float per pixel: +inf on a miss */
    rt_hit *hits_device;            /* optional: exactly the record rt_query_rays writes for that ray */
    float  *albedo_device;          /* optional, 3 floats per pixel: the hit material's albedo; the camera's background on a miss */
    void   *stream;                 /* as rt_ray_query.stream */
} rt_camera_query;                  /* 72 bytes on LP64 */

rt_status rt_query_camera(rt_scene *scene, const rt_camera_query *query);

/* Denoising: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a frame in device memory, guided by
 * the rt_hit records and, optionally, the albedo that rt_query_camera writes for the same pixels (csrc/denoise.hip).
 * The call takes a device, like rt_box_test, and no scene: it reads nothing of one, and its only ordering is the
 * stream's.  It allocates nothing.
 *
 * Inputs   : contiguous row-major width x height buffers.  color_device: 3 floats per pixel, what rt_render writes to
 *            rgb32_device.  hits_device: what rt_query_camera writes to hits_device for the same rectangle; only
 *            instance (0xFFFFFFFF = miss), point and normal are read.  albedo_device (optional): 3 floats per pixel.
 * Filter   : per pixel p, miss(p) = (hits[p].instance == 0xFFFFFFFF); n(p), x(p) = the record's normal and point as
 *            stored (0 in a miss record); a(p) = max(albedo(p), 1e-3) per channel, 1 without albedo; c_0 = color / a.
 *            Pass i = 0 .. iterations - 1 has step s = 2^i and sigma_c,i = sigma_color * 2^-i:
 *              c_{i+1}(p) = sum_q h(q) w(p, q) c_i(q) / sum_q h(q) w(p, q),  q = p + s * (dx, dy), dx, dy in -2 .. 2,
 *              taps outside the image left out; h = k[dx] * k[dy], k = (1/16, 1/4, 3/8, 1/4, 1/16) (B3 spline);
 *              w(p, q) = 0 when miss(p) != miss(q), else
 *              exp(-(|c_i(p) - c_i(q)|^2 / sigma_c,i^2 + |n(p) - n(q)|^2 / sigma_normal^2
 *                    + (n(p) . (x(q) - x(p)))^2 / sigma_plane^2)).
 *            A sigma of +inf contributes 0 (its term is switched off).  The centre tap has w = 1, so the denominator
 *            is at least 9/64.  Hits blend only with hits, sky only with sky.  The result is c_iterations * a.
 *            In float32, without FMA contraction, taps summed row by row (dy, then dx, ascending); each term is
 *            multiplied by 1 / sigma^2, computed once per pass and capped at FLT_MAX.
 * Outputs  : at least one.  rgb32_device: 3 floats per pixel, the result; it may be color_device itself (the first
 *            pass copies what it needs into the scratch, so the call works in place at any iteration count).
 *            rgba8_device: uchar4 per pixel, Color3::castToUchar4 of the result as rt_render's rgba8 has it
 *            (correctly rounded sqrt, clamp to [0, 0.999], x 256; alpha 255).  No other buffers may overlap.
 * Scratch  : scratch_device holds at least rt_denoise_scratch_bytes(width, height) bytes (64 per pixel), 16-byte
 *            aligned, and is the call's only working memory; its contents afterwards are unspecified.  Calls that
 *            may run concurrently need a scratch each.
 * Ordering : everything is enqueued on `stream` (NULL: the device's null stream).  With RT_DENOISE_NO_SYNC the call
 *            returns after the enqueue, else once the outputs are complete.  Render, camera query and denoiser on one
 *            stream with their NO_SYNC flags need no host synchronisation between them.
 * Errors   : all before anything is enqueued, the argument checks first (they answer without a GPU):
 *            RT_ERR_INVALID_ARGUMENT for a NULL desc, reserved != 0, unknown flags, iterations outside 1..5, a sigma
 *            that is not > 0 (NaN included), width or height above 16384, no output buffer, a NULL color_device,
 *            hits_device or scratch_device, scratch_bytes too small, a scratch not 16-byte aligned or another buffer
 *            not 4-byte aligned; then for no such device, or a buffer that hipPointerGetAttributes does not report as
 *            accessible from it.  width * height == 0 with otherwise valid arguments returns RT_OK and touches no
 *            device.  The caller's current device is preserved.  Non-finite input colours are not detected: a NaN or
 *            infinity spreads to the pixels whose taps reach it. */
typedef enum rt_denoise_flags { RT_DENOISE_NO_SYNC = 1u << 2 } rt_denoise_flags;   /* the queries' NO_SYNC bit */

typedef struct rt_denoise_desc {
    uint32_t width, height;        /* each <= 16384; buffers are contiguous row-major W x H */
    uint32_t iterations;           /* 1..5: steps 1, 2, 4, 8, 16 */
    uint32_t flags;
    float sigma_color;             /* > 0; +inf switches the term off; halved every pass */
    float sigma_normal;            /* > 0; +inf off */
    float sigma_plane;             /* > 0, world units; +inf off */
    uint32_t reserved;             /* 0 */
    const float  *color_device;    /* 3 floats per pixel: what rt_render writes to rgb32_device */
    const rt_hit *hits_device;     /* what rt_query_camera writes to hits_device for the same rectangle */
    const float  *albedo_device;   /* optional, 3 floats per pixel: demodulate before, remodulate after */
    float  *rgb32_device;          /* optional output, 3 floats per pixel; may be color_device itself */
    void   *rgba8_device;          /* optional output, uchar4 per pixel: Color3::castToUchar4 of the result */
    void   *scratch_device;        /* >= rt_denoise_scratch_bytes(width, height) bytes, 16-byte aligned */
    uint64_t scratch_bytes;
    void   *stream;                /* hipStream_t; NULL = the device's null stream */
} rt_denoise_desc;                 /* 96 bytes on LP64 */

uint64_t  rt_denoise_scratch_bytes(uint32_t width, uint32_t height);
rt_status rt_denoise(int device, const rt_denoise_desc *desc);

/* Temporal accumulation: last frame's accumulated colour carried to this frame's pixels by reprojecting each pixel's
 * hit point into the previous camera, and blended with this frame's colour (csrc/accumulate.hip).  Like rt_denoise the
 * call takes a device and buffers, no scene; its only ordering is the stream's, and it allocates nothing.
 *
 * Reprojection: rt_camera_reprojection derives, on the host and without a scene or a GPU, the rows that map a world
 *            point x to a camera's frame: v = x - centre, fx = (rx . v) / (rw . v), fy = (ry . v) / (rw . v); pixel
 *            (i, j)'s centre lands on (fx, fy) = (i, j), and rw . v > 0 in front of the camera.  The camera is derived
 *            as rt_camera_set derives it (one shared function); from its float pixel_origin, dx, dy and center, in
 *            double: p0 = pixel_origin - center, det = dx . (dy x p0), rx = (dy x p0) / det, ry = (p0 x dx) / det,
 *            rw = (dx x dy) / det, each rounded to float.  RT_ERR_INVALID_ARGUMENT for a NULL argument, a width or
 *            height of 0 or above 32768, or a non-finite result (center == target is one such camera).  The focus
 *            disk is ignored: the rows describe the pinhole through `center`.
 * Inputs   : contiguous row-major width x height buffers.  color_device: this frame, 3 floats per pixel (rt_render's
 *            rgb32_device).  hits_device: this frame's rt_query_camera records; prev_hits_device: last frame's.
 *            prev_history_device: the history_device of the last call, float4 {r, g, b, length} per pixel.
 *            prev_view: a HOST pointer to the previous frame's rows, read during the call; NULL = the camera has not
 *            moved, every pixel looks at itself.
 * Filter   : for pixel p = (i, j), k = j W + i, c = color[k], rec = hits[k], n and x its normal and point as stored,
 *            H(q) = prev_history[q].
 *              reset(p): history[k] = (c, 1), rgb32[k] = c.  It applies when prev_history_device is NULL (the first
 *              frame), when rec.instance == 0xFFFFFFFF (sky is the noise-free part of a frame and is not reused), and
 *              whenever a test below fails.
 *              Position: with prev_view NULL a single tap q = p with weight b = 1.  Otherwise v = x - centre per
 *              component, r0 = (rx.x v.x + rx.y v.y) + rx.z v.z, r1 and r2 the same from ry and rw; reset unless
 *              r2 > 0; fx = r0 / r2, fy = r1 / r2; reset unless fx >= -1 && fx < (float)W && fy >= -1 &&
 *              fy < (float)H (a NaN fails every comparison); ix = floorf(fx), wx = fx - ix, likewise iy, wy; the taps
 *              are (ix + tx, iy + ty) for (tx, ty) = (0,0), (1,0), (0,1), (1,1) in that order, with
 *              b = (tx ? wx : 1 - wx) * (ty ? wy : 1 - wy).
 *              A tap q is valid when it lies inside the image and, with m = prev_hits[q] and e = m.point - x:
 *              m.instance == rec.instance; (n.x m.n.x + n.y m.n.y) + n.z m.n.z >= normal_cos;
 *              fabsf((n.x e.x + n.y e.y) + n.z e.z) <= plane_tolerance * rec.t.
 *              Blend: S = sum b H(q) over the four channels and D = sum b over the valid taps, both from 0 in tap
 *              order, each product rounded before it is added; reset unless D > 0; Hm = S / D per channel;
 *              N = fminf(Hm.w + 1, max_history), a = 1 / N; out.rgb = Hm.rgb + a (c - Hm.rgb), out.w = N;
 *              history[k] = out, rgb32[k] = out.rgb.
 *            In float32 without FMA contraction, IEEE division, no transcendental function: the float32 restatement
 *            in tests/accumulate_ref.py gives the kernel's bits.
 * Not done : no 3 x 3 fallback search around a failed reprojection; sky is not reused.  rt_accumulate itself does not
 *            compensate instance motion (a moved instance is caught by the plane test, so its pixels restart):
 *            rt_accumulate_motion below does.  Shadows and reflections of a moving instance on static pixels are not
 *            compensated by either: the surface has not moved, so its history is kept while its shading changes.
 *            (Luminance moments and the variance-guided filter: rt_accumulate_moments and rt_denoise_guided below;
 *            the filtered colour as next frame's history: rt_denoise_guided_feedback, "History feedback" below.)
 * Outputs  : history_device (required): float4 per pixel, next frame's prev_history_device.  rgb32_device (optional):
 *            3 floats per pixel, out.rgb; it may be color_device itself (a thread reads only its own pixel's colour).
 *            Otherwise no output may overlap an input or the other output: the byte ranges are compared on the host.
 *            So the caller ping-pongs two history buffers and two hits buffers.  (The one other exact alias the
 *            filters allow: rt_denoise_guided_feedback's feedback_device may be its history_device, "History feedback"
 *            below, for the same reason.)
 * Ordering : as rt_denoise, with RT_ACCUMULATE_NO_SYNC for RT_DENOISE_NO_SYNC.
 * Errors   : all before anything is enqueued, the argument checks first (they answer without a GPU):
 *            RT_ERR_INVALID_ARGUMENT for a NULL desc, reserved or reserved1 != 0, unknown flags, width or height above
 *            16384, max_history not >= 1, normal_cos not <= 1, plane_tolerance not > 0 (NaN fails each), a NULL
 *            color_device, hits_device or history_device, only one of prev_hits_device and prev_history_device, a
 *            history buffer not 16-byte aligned or another buffer not 4-byte aligned, overlapping buffers as above;
 *            then for no such device, or a buffer that hipPointerGetAttributes does not report as accessible from
 *            it.  width * height == 0 with otherwise valid arguments returns RT_OK and touches no device.  The
 *            caller's current device is preserved.  A non-finite colour or history texel is not detected: it reaches
 *            every pixel that has it among its valid taps, a tap of weight 0 included (0 * inf is a NaN in S), and it
 *            stays in the history until that pixel resets.  The window on fx and fy decides no result by itself (at
 *            fx = -1 the one inside tap has weight 0 and at fx = W no tap is inside, so D = 0 either way); it keeps
 *            values that no int holds, 1e30 or a NaN, from the conversion. */
typedef struct rt_reprojection { float centre[3], rx[3], ry[3], rw[3]; } rt_reprojection;   /* 48 bytes */

rt_status rt_camera_reprojection(const rt_camera_input *camera, uint32_t width, uint32_t height, rt_reprojection *out);

typedef enum rt_accumulate_flags { RT_ACCUMULATE_NO_SYNC = 1u << 2 } rt_accumulate_flags;  /* the queries' NO_SYNC bit */

typedef struct rt_accumulate_desc {
    uint32_t width, height, flags, reserved;          /* reserved 0; width, height <= 16384 */
    float max_history;                                /* >= 1, +inf allowed: blend weight never below 1 / max_history */
    float normal_cos;                                 /* <= 1, not NaN; -inf switches the test off */
    float plane_tolerance;                            /* > 0, a fraction of the pixel's hit distance t; +inf off */
    uint32_t reserved1;                               /* 0 */
    const rt_reprojection *prev_view;                 /* HOST pointer, read during the call; NULL = same pixel (static camera) */
    const float  *color_device;                       /* 3 floats per pixel: this frame (rt_render's rgb32_device) */
    const rt_hit *hits_device;                        /* this frame's rt_query_camera records */
    const rt_hit *prev_hits_device;                   /* last frame's records; NULL with prev_history_device NULL = first frame */
    const float  *prev_history_device;                /* last call's history_device: float4 {r, g, b, length} per pixel, 16-byte aligned */
    float  *history_device;                           /* required output, float4 per pixel, 16-byte aligned */
    float  *rgb32_device;                             /* optional output, 3 floats per pixel; may be color_device itself */
    void   *stream;                                   /* hipStream_t; NULL = the device's null stream */
} rt_accumulate_desc;                                 /* 96 bytes on LP64 */

rt_status rt_accumulate(int device, const rt_accumulate_desc *desc);

/* Variance-guided denoising, in the manner of SVGF (Schied et al. 2017): the accumulation also carries the first two
 * moments of each pixel's luminance (rt_accumulate_moments), and rt_denoise_guided turns them into a per-pixel
 * variance of the accumulated colour that steers the a-trous passes and is filtered along with the colour
 * (csrc/accumulate.hip, csrc/guided.hip).  The caller states one dimensionless sigma_luminance, the same for every
 * frame and every pixel, where rt_denoise's sigma_color has to follow the noise level by hand.
 *
 * rt_accumulate_moments does all of rt_accumulate(device, desc): the same argument checks, ordering, NO_SYNC flag and
 * outputs; history_device and rgb32_device receive, bit for bit, what rt_accumulate writes (one kernel, instantiated
 * with and without the moments).  The same kernel accumulates the moments with the same taps, the same validity and
 * the same weights b.  Per pixel, in float32 without FMA contraction:
 *              a = max(albedo, 1e-3) per channel, 1 without albedo (rt_denoise's a(p));  L = lum(c / a) with
 *              lum(r, g, b) = (0.2126f r + 0.7152f g) + 0.0722f b.
 *              Wherever rt_accumulate resets the pixel: moments[k] = (L, L L).
 *              Otherwise S1 = sum b M(q).x and S2 = sum b M(q).y over the valid taps (M = prev_moments), from 0 in tap
 *              order, each product rounded before it is added; M1 = S1 / D, M2 = S2 / D;
 *              moments[k] = (M1 + a_N (L - M1), M2 + a_N (L L - M2)) with the call's own a_N = 1 / N.
 *            The float32 restatement in tests/guided_ref.py gives the kernel's bits.
 * Errors   : rt_accumulate's, and before anything is enqueued (the first six answer without a GPU):
 *            RT_ERR_INVALID_ARGUMENT for a NULL moments, reserved != 0, a NULL moments_device, prev_moments_device
 *            present without prev_history_device or the reverse, a moments buffer not 8-byte aligned or an albedo not
 *            4-byte aligned, a moments_device that overlaps any input or either other output; then for a buffer that
 *            is not accessible from the device.  width * height == 0 returns RT_OK and touches no device.
 *
 * rt_denoise_guided filters what rt_accumulate_moments wrote.  miss, n, x, a, h (the B3 kernel), the taps and their
 * order are rt_denoise's.  Per pixel p: N = history.w (at least 1, as rt_accumulate writes it), (m1, m2) = moments,
 * c_0 = history.rgb / a.
 * Variance : v_t = max(0, m2 - m1 m1), the temporal estimate.  Where N < 4 it is not trusted and a spatial one
 *            replaces it, over the 7 x 7 window q = p + (dx, dy), dx, dy in -3 .. 3, taps outside the image left out,
 *            summed over dy, then dx, ascending: g(p, q) = 0 when miss(p) != miss(q), else
 *            exp(-(|n(p) - n(q)|^2 / sigma_normal^2 + (n(p) . (x(q) - x(p)))^2 / sigma_plane^2)), 1 at the centre;
 *            v_s = max(0, sum g m2(q) / sum g - (sum g m1(q) / sum g)^2).
 *            v_0 = (N >= 4 ? v_t : v_s) / N: the moments estimate the variance of one sample, and the accumulated
 *            colour is a mean of about N of them.  At the history cap the blend is exponential and the true factor
 *            is 1 / (2 max_history - 1), so dividing by N there overstates the variance by up to 2: the conservative
 *            side (the filter trusts the colour less, never more, than it should).
 * Filter   : pass i = 0 .. iterations - 1 has step s = 2^i.
 *              vbar_i(p) = the 3 x 3 Gaussian, kernel (1/4, 1/2, 1/4) per axis, of v_i over the neighbours at distance
 *              1 (at every step, not s), taps outside the image left out, summed over dy, then dx, ascending, and
 *              divided by the sum of the kernel weights that are in.
 *              k(p) = 1 / (sigma_luminance sqrtf(vbar_i(p)) + 1e-6f), 0 when sigma_luminance is +inf;  l_i = lum(c_i).
 *              w(p, q) = 0 when miss(p) != miss(q), else
 *              exp(-((|l_i(p) - l_i(q)| k(p) + |n(p) - n(q)|^2 / sigma_normal^2)
 *                    + (n(p) . (x(q) - x(p)))^2 / sigma_plane^2));  the centre tap has w = 1.
 *              c_{i+1}(p) = sum h w c_i(q) / sum h w;   v_{i+1}(p) = sum h^2 w^2 v_i(q) / (sum h w)^2.
 *            sigma_luminance is not halved per pass: the variance shrinks by being filtered.  The result is
 *            c_iterations a.  In float32 without FMA contraction; the terms of sigma_normal and sigma_plane are
 *            multiplied by 1 / sigma^2, computed once and capped at FLT_MAX, as rt_denoise's.
 * Outputs  : at least one of rgb32_device and rgba8_device, written as rt_denoise writes them.  variance_device
 *            (optional): v_0, 1 float per pixel.  No output may overlap an input, another output or the scratch.
 * Scratch  : as rt_denoise: rt_denoise_guided_scratch_bytes(width, height) bytes (64 per pixel), 16-byte aligned.
 * Ordering : as rt_denoise; everything goes on `stream`, and the call allocates nothing.
 * Errors   : all before anything is enqueued, the argument checks first (they answer without a GPU):
 *            RT_ERR_INVALID_ARGUMENT for a NULL desc, reserved != 0, unknown flags, iterations outside 1..5, a sigma
 *            that is not > 0 (NaN included), width or height above 16384, no output buffer, a NULL history_device,
 *            moments_device, hits_device or scratch_device, scratch_bytes too small, a scratch or history not 16-byte
 *            aligned, moments not 8-byte aligned, another buffer not 4-byte aligned, overlapping buffers as above;
 *            then for no such device, or a buffer that is not accessible from it.  width * height == 0 with otherwise
 *            valid arguments returns RT_OK and touches no device.  The caller's current device is preserved.
 *            Non-finite history colours are not detected: a NaN or infinity spreads to the pixels whose taps reach it,
 *            the box |dx|, |dy| <= 2 (2^iterations - 1) around it, across the hit / sky boundary too (0 * NaN), and
 *            to no other pixel; v_0 reads no colour and is unaffected.  Non-finite moments are not detected either
 *            and their effect is unspecified (an infinite variance gives k(p) = 0 and a finite result).
 * Not done : moving instances are compensated by rt_accumulate_motion ("Moving instances" below), not by
 *            rt_accumulate_moments, and the shadows and reflections a moving instance casts on static pixels by
 *            neither; the colour accumulates modulated while the moments are demodulated, so where the albedo changes
 *            under a kept pixel the two disagree for up to max_history frames.  (The filtered colour as history:
 *            rt_denoise_guided_feedback, "History feedback" below.) */
typedef struct rt_moments_desc {
    const float *albedo_device;        /* optional, 3 floats per pixel: the albedo the guided filter will be given */
    const float *prev_moments_device;  /* last call's moments_device; NULL exactly when desc->prev_history_device is NULL */
    float       *moments_device;       /* required output: float2 {m1, m2} per pixel, 8-byte aligned */
    uint64_t     reserved;             /* 0 */
} rt_moments_desc;                     /* 32 bytes on LP64 */

rt_status rt_accumulate_moments(int device, const rt_accumulate_desc *desc, const rt_moments_desc *moments);

typedef struct rt_denoise_guided_desc {
    uint32_t width, height;          /* each <= 16384 */
    uint32_t iterations;             /* 1..5 */
    uint32_t flags;                  /* RT_DENOISE_NO_SYNC */
    float sigma_luminance;           /* > 0, dimensionless (in standard deviations); +inf switches the term off */
    float sigma_normal, sigma_plane; /* as rt_denoise */
    uint32_t reserved;               /* 0 */
    const float  *history_device;    /* float4 {r, g, b, length}: rt_accumulate_moments' history_device, 16-byte aligned */
    const float  *moments_device;    /* float2 {m1, m2}: its moments_device, 8-byte aligned */
    const rt_hit *hits_device;       /* this frame's records */
    const float  *albedo_device;     /* optional; the one given to rt_accumulate_moments */
    float  *rgb32_device;            /* optional output, 3 floats per pixel */
    void   *rgba8_device;            /* optional output, as rt_denoise's */
    float  *variance_device;         /* optional output, 1 float per pixel: v_0 */
    void   *scratch_device;          /* >= rt_denoise_guided_scratch_bytes(width, height) bytes, 16-byte aligned */
    uint64_t scratch_bytes;
    void   *stream;                  /* hipStream_t; NULL = the device's null stream */
} rt_denoise_guided_desc;            /* 112 bytes on LP64 */

uint64_t  rt_denoise_guided_scratch_bytes(uint32_t width, uint32_t height);
rt_status rt_denoise_guided(int device, const rt_denoise_guided_desc *desc);

/* History feedback, as SVGF has it: the colour the guided filter's first pass leaves becomes the next frame's temporal
 * history in place of the accumulated one-sample colour, so what is accumulated from then on has been filtered once
 * per frame it went through.  The pass is fixed at the first one: on the float32 restatement (tests/feedback_ref.py)
 * a later pass removes no more flicker and costs far more error.
 *
 * rt_denoise_guided_feedback does all of rt_denoise_guided(device, desc): the same argument checks, ordering,
 * RT_DENOISE_NO_SYNC and scratch; rgb32_device, rgba8_device and variance_device receive the same bits.  Its first
 * pass (one kernel, instantiated with and without the feedback) also writes, for every pixel k, sky included:
 *              feedback[k] = (c_1(p) a(p), history[k].w)
 *            c_1 a: per channel the product the same call with iterations = 1 writes to rgb32_device (c_1 without
 *            albedo); with iterations = 1 the outputs and the feedback are the same three products.  .w: the history
 *            texel's length, copied as bits.
 *            The caller passes feedback_device as the next frame's prev_history_device; rt_accumulate*, the moments and
 *            rt_denoise_guided_desc do not change.  tests/feedback_ref.py restates the chain.
 * Variance : the moments still accumulate the unfiltered samples, so v_0 = v_t / N describes the unfiltered mean of N
 *            samples and overstates the variance of a fed-back history.  The filter therefore errs towards more blur:
 *            where the signal varies faster than the filter's reach the error rises frame by frame while the flicker
 *            falls (profiles/feedback/README.md has both cases).  A trade-off that depends on the scene, not a default.
 * Outputs  : feedback_device (required): float4 per pixel, 16-byte aligned.  It may be exactly desc->history_device:
 *            the pack kernel has copied the history's colour into the scratch before the first pass writes, all on one
 *            stream, and a texel's length is read by the thread that then writes that texel (the rule that lets
 *            rt_accumulate's rgb32_device be color_device).  Any other overlap with an input, another output or the
 *            scratch, a partial overlap with the history included, is an error.
 * Errors   : rt_denoise_guided's, and, before anything is enqueued and without a GPU, RT_ERR_INVALID_ARGUMENT for a
 *            NULL feedback, reserved != 0, a NULL feedback_device, a feedback_device that is not 16-byte aligned, the
 *            overlaps above; then for a feedback_device the device cannot access.  width * height == 0 returns RT_OK
 *            and touches no device. */
typedef struct rt_feedback_desc {
    float   *feedback_device;  /* required output: float4 {r, g, b, length} per pixel, 16-byte aligned */
    uint64_t reserved;         /* 0 */
} rt_feedback_desc;            /* 16 bytes */

rt_status rt_denoise_guided_feedback(int device, const rt_denoise_guided_desc *desc,
                                     const rt_feedback_desc *feedback);

/* Moving instances: rt_accumulate and rt_accumulate_moments reproject a pixel's hit point as if the surface had stood
 * still, so on an instance that moved the point lands on a previous record of where the surface was, the plane test
 * rejects it and the pixel restarts, every frame.  rt_accumulate_motion first carries the point and the normal back to
 * where their instance was in the previous frame, and runs the reprojection and the instance, normal and plane tests
 * there.  The accumulation stays scene-less: rt_instance_motion_records derives one record per instance, on the host
 * and without a scene or a GPU (as rt_camera_reprojection), from the two rt_xform arrays the caller holds anyway, the
 * caller uploads the records, and the kernel reads the one rt_hit.instance names.
 *
 * rt_instance_motion_records: for each instance i of `count`:
 *            prev[i] and cur[i] bytewise equal: flags = RT_MOTION_STATIC, point = the identity rows, normal = the
 *            identity.
 *            Otherwise Fp and Fc are the float forward matrices of prev[i] and cur[i] exactly as rt_scene_update
 *            derives them (one shared function: (shift * ((Rx * Ry) * Rz)) * scale from the host's cos and sin of the
 *            degrees); Lp, tp, Lc, tc their 3 x 3 linear parts and translations, widened to double.  In double, with
 *            every product and sum rounded on its own:
 *              C(L)[i][j] = L[i+1][j+1] L[i+2][j+2] - L[i+1][j+2] L[i+2][j+1] (indices modulo 3: the cofactors);
 *              det(L) = (L[0][0] C[0][0] + L[0][1] C[0][1]) + L[0][2] C[0][2];   L^-1[i][j] = C[j][i] / det;
 *              A = Lp Lc^-1 and M = Lc Lp^-1, each element (X[i][0] Y[0][j] + X[i][1] Y[1][j]) + X[i][2] Y[2][j];
 *              b[i] = tp[i] - ((A[i][0] tc[0] + A[i][1] tc[1]) + A[i][2] tc[2]);   Nn = M^T.
 *            point = the rows (A | b) and normal = Nn, each value rounded to float; flags = RT_MOTION_MOVED.
 *            flags = RT_MOTION_NO_HISTORY with point and normal all zero when either determinant is 0 or not finite,
 *            when any resulting float is not finite, or when either forward matrix is one the library does not invert
 *            (a pivot of the reference's elimination below 1e-6, Matrix.cu:5-68: such an instance is traced with its
 *            forward matrix in the inverse's place, and its hit points say nothing about the surface).  A scale of 0
 *            is legal input.
 *            RT_ERR_INVALID_ARGUMENT for a NULL pointer with count > 0; count == 0 is RT_OK.
 * rt_accumulate_motion does all of rt_accumulate(device, desc) when `moments` is NULL and all of
 * rt_accumulate_moments(device, desc, moments) otherwise: their argument checks, ordering, NO_SYNC flag and outputs.
 * One kernel, instantiated with and without the motion: per pixel, with inst = rec.instance, x and n as stored, still in
 * float32 without FMA contraction:
 *              inst >= instance_count: handled as static; nothing is read from the records.
 *              f = motion[inst].flags.
 *              f == RT_MOTION_STATIC: xp = x, np = n, no arithmetic: the pixel gets rt_accumulate's bits.
 *              f == RT_MOTION_MOVED: with P = point (3 rows of 4) and Nn = normal (3 rows of 3), per component c:
 *                xp.c = ((P[c][0] x.x + P[c][1] x.y) + P[c][2] x.z) + P[c][3];
 *                u.c = (Nn[c][0] n.x + Nn[c][1] n.y) + Nn[c][2] n.z;   l2 = (u.x u.x + u.y u.y) + u.z u.z;
 *                reset unless l2 > 0 (a NaN fails);  s = sqrtf(l2), correctly rounded;  np.c = u.c / s.
 *              any other f (RT_MOTION_NO_HISTORY included): reset.
 *              Everything after that is rt_accumulate's text with xp for x and np for n: v = xp - centre, the taps,
 *              (np . m.normal) >= normal_cos, e = m.point - xp, fabsf(np . e) <= plane_tolerance * rec.t.  The
 *              tolerance keeps the current frame's t, m.instance == inst stays, the blend and the moments are unchanged.
 *            tests/motion_ref.py restates it in float32 and gives the kernel's bits.
 *            The records are not validated on the device.  Non-finite matrix elements behave like non-finite points:
 *            the window test on fx, fy or l2 > 0 resets the pixel.
 * Errors   : rt_accumulate's (and rt_accumulate_moments' when `moments` is given), and, before anything is enqueued
 *            and without a GPU, RT_ERR_INVALID_ARGUMENT for a NULL motion, reserved != 0, instance_count above
 *            0xFFFFFFFE, exactly one of motion_device and instance_count being zero, a motion_device that is not
 *            16-byte aligned or whose instance_count records overlap any output, and instance_count > 0 together with a
 *            prev_history_device and a NULL prev_view (a moved point needs a camera to land in: a caller whose camera
 *            stands still passes the current camera's rows); then for a motion_device the device cannot access.
 *            width * height == 0 returns RT_OK and touches no device.
 * Not done : motion of the geometry inside an instance (rt_scene_update_triangles*) has no per-instance map; shadows
 *            and reflections of a moving instance on static pixels are not compensated. */
typedef struct rt_instance_motion {
    float point[12];     /* rows of the 3 x 4 map: previous-frame world point = A x + b, x a current-frame world point */
    float normal[9];     /* rows of the 3 x 3 map of normals, (A^-1)^T; its result is normalised by the kernel */
    uint32_t flags;      /* rt_instance_motion_flags */
    uint32_t reserved[2];/* 0 */
} rt_instance_motion;    /* 96 bytes */

typedef enum rt_instance_motion_flags {
    RT_MOTION_STATIC = 0,      /* the instance did not move: the pixel is handled exactly as rt_accumulate handles it */
    RT_MOTION_MOVED = 1,       /* apply point[] and normal[] */
    RT_MOTION_NO_HISTORY = 2   /* every pixel of the instance resets (new, teleported, singular transform) */
} rt_instance_motion_flags;

rt_status rt_instance_motion_records(const rt_xform *prev, const rt_xform *cur, size_t count, rt_instance_motion *out);

typedef struct rt_motion_desc {
    const rt_instance_motion *motion_device;  /* instance_count records, 16-byte aligned, indexed by rt_hit.instance */
    uint64_t instance_count;                  /* <= 0xFFFFFFFE; 0 with motion_device NULL = no instance moves */
    uint64_t reserved;                        /* 0 */
} rt_motion_desc;                             /* 24 bytes on LP64 */

rt_status rt_accumulate_motion(int device, const rt_accumulate_desc *desc,
                               const rt_moments_desc *moments /* NULL: as rt_accumulate */,
                               const rt_motion_desc *motion);

/* The box decisions of the trace kernels on caller data, for parity tests (no scene needed): box i =
 * {xmin, xmax, ymin, ymax, zmin, zmax} (6 floats), ray i = origin xyz, direction xyz, range [0.001, tmax[i]].
 * hit[i] = 1 when the kernel the mode names keeps the box; te[i] = the entry t it orders children by (+inf on a
 * miss).  RT_BOX_REFERENCE is BoundingBox::hit (src/AS/BoundingBox.cu:34-72) as the EXACT kernel computes it; the
 * FAST modes are the reciprocal-plane slabs the persistent kernel culls with, conservative (a box the reference keeps
 * is never culled), and — in the exact-decision modes — with every decision inside their error margin re-taken with
 * the reference's slab, so they keep exactly the boxes the reference keeps. */
typedef enum rt_box_mode {
    RT_BOX_REFERENCE = 0,      /* EXACT kernel: the reference's division slab */
    RT_BOX_CULL = 1,           /* FAST single-box cull (SAH / GPU-built scenes' instance and root boxes) */
    RT_BOX_DECIDE = 2,         /* FAST single box, exact decisions (binary pairs; the reference's trees; "exact_decisions") */
    RT_BOX_QUAD_PAIR = 3,      /* FAST quad slot, pair order, exact decisions (the reference's trees; "exact_decisions") */
    RT_BOX_QUAD_GREEDY = 4     /* FAST quad slot, conservative cull (host SAH trees; GPU-built trees by default) */
} rt_box_mode;
rt_status rt_box_test(int device, const float *boxes_host, const float *rays_host, const float *tmax_host, size_t count,
                      uint32_t mode, uint8_t *hit_host, float *te_host);

/* Scene options (19 keys; every default is the measured best, so a drop-in caller sets none of them but
 * "overlap").  Unknown keys return RT_ERR_INVALID_ARGUMENT.
 * Frames and lanes:
 *   "overlap"   : L = consecutive rt_render calls cycle through L (2..8) internal lanes (work-queue heads, unit costs,
 *                 schedule); a launch waits only for the previous launch of its own lane and for its frame block, so
 *                 frame k+1's launch runs in the CUs frame k's tail leaves idle.  Frames with opts.stream NULL run on
 *                 lane streams the scene creates; a caller that passes streams cycles its own.  -1 = auto: the scene
 *                 also picks L and the staging depth per frame kind (2 lanes with a per-frame rebuild, else 8 lanes /
 *                 64 buffers for a rank's tile share, else 4).  With lanes the caller orders its own output buffers:
 *                 device outputs of NO_SYNC frames without a stream are complete once rt_synchronize returns
 *                 (default 0 = 1 lane: every launch of the scene is serialised)
 *   "stage_depth": pinned host staging buffers the per-frame upload cycles through (2..64, default 16, allocated on
 *                 first use): the host stages frame k once frame k - depth's trace is done (drains the scene)
 *   "lane_priority": the lane streams the scene creates for "overlap" frames without a caller stream: 1 (default) =
 *                 the device's highest stream priority (hardware queues of their own: full overlap at the default
 *                 GPU_MAX_HW_QUEUES of 4), 0 = normal priority
 *   "grid_pct"  : persistent grid as a percentage of the resident workgroup capacity (1..100; default 0 = auto:
 *                 100 when no other lane's launch is in flight, else 50 with up to 3 lanes and 100 / lanes + 12
 *                 with more, so several lanes' launches run side by side; a launch of >= 16 M camera paths: 100)
 * GPU-built scenes (RT_BUILD_LBVH; the builder's options are set before rt_scene_build):
 *   "rebuild"   : 1 = rebuild every BLAS on the GPU every frame (default 0)
 *   "cold_records": 1 = the GPU builder writes TriCold records (normals, material, caller index) beside TriHot;
 *                 0 = a hit reads the caller's triangle instead; -1 (default) = 1 unless "rebuild" is 1 at
 *                 rt_scene_build (same pixels either way)
 *   "blas_double": per-frame rebuilds: 1 = write a spare BLAS set and swap it in, so a frame's rebuild overlaps the
 *                 previous frames' traces (default 1; 0 = one set, a rebuild waits for every lane's trace)
 *   "blas_sets" : with "blas_double": BLAS sets cycled (2..8, default 3): frame k+1's rebuild waits only for the trace
 *                 of frame k + 1 - sets
 *   "tlas_small": 1 (default) = a GPU TLAS of at most 512 records is built by one workgroup in one launch; 0 = the
 *                 multi-kernel builder (results identical up to the tree's shape)
 *   "exact_decisions": 1 = the FAST kernel re-takes every box decision and pair-order comparison inside its slabs'
 *                 error margin with the reference's slab, as it always does on the reference's own trees, so its
 *                 frames equal the EXACT kernel's on the same trees bit for bit (C5: ~34 % slower per frame: sibling
 *                 boxes' entry t's often tie); 0 (default) = conservative culls (frames within SURVEY's bars)
 * Host-built scenes:
 *   "group"     : triangle instances with bit-identical transforms (each with a BLAS of its own) share one BLAS over
 *                 all their triangles, entered as one TLAS item while every member keeps that transform (default 1;
 *                 set before rt_scene_build; hits report the member instance; 0 = one TLAS item per instance)
 *   "gpu_tlas"  : RT_BUILD_SAH: 1 = keep the host-built SAH BLASes but compute the instance records and build the
 *                 TLAS on the GPU every frame, as RT_BUILD_LBVH does.  Set before rt_scene_build (default 0)
 *   "tlas_sah"  : RT_BUILD_SAH: 1 (default) = build the per-frame host TLAS with SAH; 0 = the reference's median
 *                 split (TLAS.cu:4-129)
 * Kernel:
 *   "kernel"    : 0 = one-thread-per-pixel grid kernel, 1 = persistent-wave megakernel (default)
 *   "wide"      : FAST persistent kernel: 1 (default) = quad trees (the reference's trees and GPU-built ones: two
 *                 binary levels per quad visited in the binary tree's order; RT_BUILD_SAH: the greedy collapse
 *                 visited by entry t), 0 = binary node pairs
 *   "fast_math" : FAST frames only: 1 = hardware reciprocal / rsq and FMA contraction in the primitive tests, transforms
 *                 and shading (about 8 % faster; 0.01-0.09 % of pixels then differ from the reference's arithmetic);
 *                 0 (default) = the reference's correctly rounded arithmetic wherever a value reaches a hit or a pixel
 *   "reorder"   : 1 (default) = each launch claims its band's 8x8 units heaviest-first, ordered by the traversal work
 *                 the lane's last recording launch measured per unit (schedule.hip); 0 = screen order.  Images are
 *                 identical either way (the RNG is keyed by pixel)
 * Debug:
 *   "timeline"  : 1 = record a per-wave timeline of each persistent launch
 *   "costmap"   : 1 = with RT_RENDER_COUNT_WORK, record per-pixel traversal steps
 * (Removed in round 6, measured defaults kept: threshold, leaf_early, queue_parts, grab, supertile, merge, split,
 * reorder_period, reserve, lds_scene, lds_blas, inst_by_slot, blas_leaf, tlas_leaf, tlas_median_leaf; removed with
 * their code as measured negative or neutral: variant, nt_store, cost_max, tlas_classes, wide_merge, scene_priority.
 * DESIGN.md §4 keeps the measurements.) */
rt_status rt_scene_set_option(rt_scene *scene, const char *key, int64_t value);

/* Debug buffers of the last launch that recorded them (synchronises the scene's stream):
 *   "timeline": 24 u64 per wave of the persistent kernel: start and end s_memrealtime (100 MHz),
 *               (HW_ID << 32) | XCC_ID, pixels finished by the wave, time the queue ran dry,
 *               traversal rounds, shade phases, queue grabs, and (diagnostic builds only) shader
 *               cycles spent refilling, descending, testing leaves and shading, descent-loop
 *               iterations, refill-loop iterations, cycles claiming lanes and sampling scatter, lane
 *               sums per descent iteration / TLAS leaf phase / BLAS leaf phase / shade step, lanes
 *               postponing a leaf in the descent loop, descent iterations without a node step,
 *               shaded hits and those on a path's last rough segment;
 *   "costmap" : 1 u32 per output pixel: traversal steps (interior steps + leaf phases) of its path;
 *   "unit_cost", "unit_order": option "reorder" — per 8x8 unit, the work the lane's last launch recorded
 *               (after the next launch's schedule: the costs that schedule read), and the claim order the
 *               last launch used (band b's items start at 4 x its first unit: unit << 4 | piece << 2 | log2 pieces);
 *   "instances": RT_BUILD_LBVH or "gpu_tlas": 45 floats per instance, the records the GPU computed for the current frame
 *               (instances.hip): inverse, forward and inverse-transpose rows 1-3 (12 each), transformed box
 *               {xmin,xmax,ymin,ymax,zmin,zmax} (may be all +inf for a record kept out of the TLAS: a member of
 *               an intact instance group, option "group"), transformed centroid;
 *   "blas_pairs", "blas_quads", "blas_roots": RT_BUILD_LBVH: the GPU-built forest as NodePair / NodeQuad /
 *               TreeRoot records (csrc/layout.hpp; quad q is the 4-wide node rooted at pair q);
 *   "leaf_prims": 1 u32 per leaf-ordered triangle slot: the caller's triangle index stored there (each
 *               BLAS owns the contiguous slots of its primitives, in leaf order);
 *   "rebuild_stages": RT_BUILD_LBVH with option "timeline" set before the frame: float64 values — the last BLAS
 *               build's items, interior nodes, node pairs written, items in trees of > 2048 items, such trees, then
 *               the ms of each builder stage (prep, bounds, morton, sort, hierarchy_small, hierarchy_large, scan,
 *               emit_roots, collapse); RT_ERR_STATE when the last build ran untimed.
 * Copies min(capacity, size) bytes to dst and stores the buffer's full size in *bytes. */
rt_status rt_scene_debug_read(rt_scene *scene, const char *name, void *dst, size_t capacity, size_t *bytes);

/* Pipelined frames (RT_RENDER_NO_SYNC): wait for the last enqueued frame, return the device
 * counters accumulated since the last frame rendered without RT_RENDER_KEEP_COUNTERS (rays, pixels
 * and, with RT_RENDER_COUNT_WORK, the work counters) and the kernel duration of every frame
 * rendered since the previous collect (HIP events on the kernel's stream; up to 256 kept). */
rt_status rt_scene_collect(rt_scene *scene, rt_stats *accumulated, float *kernel_ms, uint32_t capacity,
                           uint32_t *count);

/* Replace triangles [first, first + count) of the scene's triangle array (deforming geometry,
 * e.g. the next frame of a VTK series, Renderer.cu:394-443).  RT_BUILD_LBVH scenes only: the
 * BLASes are rebuilt on the GPU by the next frame update, before that frame traces; until then a
 * trace that skips the update (RT_RENDER_SKIP_UPDATE, rt_trace_rays) returns RT_ERR_STATE, since it
 * would traverse the old trees while its hits read the new triangles.  Instances keep the local
 * bounds their description supplied (has_local_bounds), as the reference keeps the VTK reader's. */
rt_status rt_scene_update_triangles(rt_scene *scene, size_t first, size_t count, const rt_triangle *triangles);

/* Triangle updates from device memory: the geometry of triangles [first, first + count) from flat float streams the
 * caller holds in device memory (a simulation's or a skinning pass's output, a torch tensor), written into the scene
 * by one kernel (csrc/tri_update.hip) without crossing the host.  RT_BUILD_LBVH scenes only.
 *
 * Changes  : only geometry.  Each triangle keeps its material type and index, so nothing read from device memory needs
 *            validating on the host.  With normals_device the three normals are replaced and has_normals becomes 1.
 *            Without it normal[] and has_normals stay as they are: a flat triangle (has_normals == 0) gets its normal
 *            from the new vertices when its leaf record is built, a triangle with stored normals keeps them.
 * Effect   : that of rt_scene_update_triangles with records that differ from the current ones in exactly those fields.
 *            The BLASes are rebuilt by the next frame update; until then RT_RENDER_SKIP_UPDATE, rt_trace_rays and
 *            rt_query_rays return RT_ERR_STATE, as after rt_scene_update_triangles.
 * Bounds   : without RT_TRI_UPDATE_BOUNDS instance bounds stay the caller's.  A triangle instance with
 *            has_local_bounds == 1 keeps its bounds, as in the host path; rt_scene_update_instances replaces them.  The
 *            host path recomputes the bounds of a triangle instance with has_local_bounds == 0 (a single-primitive
 *            instance included) from its triangles; the host cannot see the new vertices, so a range that overlaps
 *            such an instance returns RT_ERR_UNSUPPORTED, naming the first such instance, and nothing is enqueued or
 *            changed.
 *            With RT_TRI_UPDATE_BOUNDS the device derives them, and that refusal does not apply.  Every triangle
 *            instance whose primitive range overlaps [first, first + count) becomes device-bounded, whatever its
 *            has_local_bounds, single-primitive instances included (spheres and parallelograms never).  From the next
 *            frame update on — the one that rebuilds the BLASes from the new triangles — its local box is the union of
 *            its triangles' boxes and its local centroid the mean of their centroids over its whole primitive range,
 *            the rules of the host path (one triangle keeps its own centroid).  The box is a min / max and so exact
 *            (where two extremes are -0 and +0 only their value is promised); the centroid is (float)(S / count) with
 *            S a double-precision sum in a fixed shape that depends on count alone (csrc/inst_bounds_map.hpp): two
 *            runs give the same bits, and they are the host path's whenever the host's sequential sum is exact, else
 *            within one float ulp of them.  The centroid only feeds the TLAS build, so hits depend on it through the
 *            tree's shape alone.
 *            A device-bounded instance goes back to host bounds by rt_scene_update_instances on it (the description's
 *            bounds with has_local_bounds == 1, else derived from the triangles, read back once; a group it belongs
 *            to breaks, as always), by rt_scene_build (has_local_bounds == 1 instances return to their description's
 *            bounds, the others get bounds derived from the triangles read back), and by a host
 *            rt_scene_update_triangles whose range touches it or a group that holds a device-bounded member: that call
 *            reads the triangles back once and derives those instances' bounds on the host.
 *            A later device update without the flag leaves a device-bounded instance device-bounded: its box follows
 *            the rebuilt BLAS, its centroid stays that of the last flagged update.
 *            Option "group": a group with a device-bounded member is device-bounded itself: while it is intact its box
 *            is the union over all its members' triangles, its centroid the mean of its members' centroids.  The flag
 *            never breaks a group; a broken group's members are ordinary instances with BLASes of their own.
 * Ordering : the library records an event on `stream`, makes the scene's stream wait for it and writes the triangles
 *            with one kernel on the scene's stream: behind every BLAS build already enqueued there, exactly where the
 *            host path's copy sits.  Where traces and query records read the caller's triangles (option
 *            "cold_records" 0), the kernel also waits for the last frame of every lane and for the queries in flight.
 *            The library then makes `stream` wait for the kernel's completion event, so the caller may overwrite or
 *            free its buffers in stream order straight after the call returns, with or without
 *            RT_TRI_UPDATE_NO_SYNC.  stream NULL: the caller's null stream, ordered with the scene's stream before and
 *            after the kernel as rt_render and rt_query_rays order device buffers.  Without RT_TRI_UPDATE_NO_SYNC the
 *            call returns once the write is complete; rt_synchronize and rt_scene_destroy wait for it in any case.
 *            Host and device updates of one scene take effect in call order.  Nothing on this path waits for the device
 *            to drain.  RT_TRI_UPDATE_BOUNDS adds kernels behind that one on the scene's stream; they wait for the
 *            instance-record updates of frames already enqueued (microseconds), never for a trace.
 * Errors   : all before anything is enqueued.  RT_ERR_INVALID_ARGUMENT for a NULL scene or update, a NULL
 *            vertices_device with count > 0, reserved != 0, unknown flags, a range outside the scene's triangle array,
 *            or a buffer that hipPointerGetAttributes does not report as accessible from the scene's device;
 *            RT_ERR_STATE before rt_scene_build; RT_ERR_UNSUPPORTED for a build mode other than RT_BUILD_LBVH and,
 *            without RT_TRI_UPDATE_BOUNDS, for the bounds rule above; with it, for an instance in the range that shares
 *            its BLAS (same first primitive) with an instance of another primitive count.  count == 0 returns RT_OK and
 *            enqueues nothing.  The caller's current device is preserved.  Non-finite vertices are not detected: they behave as they do through the host path.
 * Rebuilds : rt_scene_build may be called again on a built scene; it then builds from the device-updated triangles
 *            (the library reads them back once; so does a later rt_scene_update_triangles that has to recompute an
 *            instance's bounds).
 * Out of scope: device-derived bounds for spheres and parallelograms; indexed meshes (gather verts[faces] on `stream`
 *            first); material changes from device memory; refitting instead of rebuilding. */
typedef enum rt_triangle_update_flags {
    RT_TRI_UPDATE_NO_SYNC = 1u << 0,  /* return after enqueue */
    RT_TRI_UPDATE_BOUNDS = 1u << 1    /* derive the bounds of the instances the range overlaps on the device */
} rt_triangle_update_flags;

typedef struct rt_triangle_update {
    uint64_t first, count;         /* triangles [first, first + count) of the scene's triangle array */
    const float *vertices_device;  /* 9 floats per triangle: vertex 0, 1, 2, xyz each */
    const float *normals_device;   /* optional, 9 floats per triangle: normal 0, 1, 2 */
    uint32_t flags;                /* rt_triangle_update_flags */
    uint32_t reserved;             /* 0 */
    void *stream;                  /* hipStream_t the caller produced the buffers on; NULL as rt_query_rays documents */
} rt_triangle_update;
/* sizeof(rt_triangle_update) == 48 on LP64 */

rt_status rt_scene_update_triangles_device(rt_scene *scene, const rt_triangle_update *update);

/* Replace instance descriptions [first, first + count) — local bounds / centroid and the transform
 * used when no update callback is set (the next VTK frame's particles, VTKReader.cu:203-215).  The
 * primitives an instance refers to (type, index, count) may not change.  Takes effect with the next
 * TLAS build (rt_scene_update / rt_render); any build mode. */
rt_status rt_scene_update_instances(rt_scene *scene, size_t first, size_t count, const rt_instance_desc *instances);

/* Blocks until all work the scene enqueued has finished. */
rt_status rt_synchronize(rt_scene *scene);

/* Renderer::cleanup (src/Global/Renderer.cu:368-391). */
void rt_scene_destroy(rt_scene *scene);

/* --- interactive loop without a window -------------------------------------------
 * The reference's frame loop (src/Global/Renderer.cu:232-338) reads SDL key / mouse events, moves the
 * camera (SDL_OpenGLWindow::calculateNewPosition, src/Global/SDL_OpenGLWindow.cu:182-256), recomputes the
 * camera (RenderPin.cu:73-95), steps the move speed on the mouse wheel and caps the frame rate at 120 fps.
 * These calls restate that host logic on caller-supplied input, so a scripted or remote input stream drives
 * the same camera path; the window, the GL surface and SDL itself stay out (presentation).  Host-only. */

/* OperateArgs (include/Global/SDL_OpenGLWindow.cuh:34-45, filled by getOperateArgs :63-74) plus the loop's
 * relative-mouse-mode state (Renderer.cu:230, toggled by a click :239-241). */
typedef struct rt_camera_control {
    float mouse_sensitivity;       /* radians per mouse count */
    float pitch_limit;             /* as getOperateArgs stores it: PI / degreeToRadian(pitch_limit_degree) */
    float move_speed;              /* world units per frame; the wheel steps it */
    float move_speed_change_step;
    float fps_limit;               /* INFINITY: no cap */
    uint32_t restrict_frame_count; /* fps_limit != INFINITY */
    int64_t target_frame_us;       /* microseconds((int64)(1e6f / fps_limit)) */
    int64_t sleep_margin_us;       /* 2000 */
    uint32_t relative_mouse;       /* mouse motion counts only in relative mode (on at loop start) */
    uint32_t reserved;
} rt_camera_control;

/* KeyMouseInputArgs (include/Global/SDL_OpenGLWindow.cuh:47-60) for one frame: held keys, the mouse motion
 * and wheel accumulated since the previous frame (getKeyMouseInput resets them per frame,
 * SDL_OpenGLWindow.cu:135-141), a click, quit. */
typedef struct rt_input_state {
    uint32_t key_w, key_a, key_s, key_d, key_space, key_lshift;
    int32_t dx, dy;
    int32_t d_speed;
    uint32_t mouse_click;
    uint32_t key_quit;
} rt_input_state;

/* getOperateArgs(fpsLimit, mouseSensitivity, pitchLimitDegree, moveSpeedNTimesStep, moveSpeedChangeStep); the
 * reference's loop uses (120, 0.001, 80, 2, 0.05) (Renderer.cu:224-225). */
rt_status rt_camera_control_init(rt_camera_control *ctl, float fps_limit, float mouse_sensitivity,
                                 float pitch_limit_degree, uint32_t move_speed_n_steps, float move_speed_change_step);

/* The camera half of one loop iteration (Renderer.cu:236-262): mouse motion (counted in relative mode) turns
 * the view (yaw about V, then pitch about U, pitch clamp), held keys translate center and target in the
 * horizontal plane / along up; a click toggles relative mode; the wheel steps ctl->move_speed (after the
 * move, as the reference does).  `camera` is updated in place (center, target); *moved = 1 when the camera
 * moved, i.e. when the reference recomputes the camera (the caller then passes it to rt_camera_set with the
 * framebuffer size; the U / V / W the move used are those rt_camera_set derives from `camera`). */
rt_status rt_camera_move(rt_camera_input *camera, rt_camera_control *ctl, const rt_input_state *input,
                         uint32_t *moved);

/* Monotonic clock (steady_clock) in nanoseconds. */
int64_t rt_clock_ns(void);

/* The frame limiter (Renderer.cu:327-337): when less than ctl->target_frame_us has passed since
 * frame_start_ns, sleep until sleep_margin_us before the target, then spin until it.  Returns the
 * nanoseconds spent waiting (0 when the frame took longer). */
int64_t rt_frame_pace(const rt_camera_control *ctl, int64_t frame_start_ns);

/* Abort a stuck multi-GPU frame instead of blocking: with a timeout set, every wait the library does on a
 * frame that gathers over RCCL polls ncclCommGetAsyncError; on an asynchronous RCCL error or when the
 * frame has not completed after `timeout_ms`, the communicators are aborted (ncclCommAbort), the scene is
 * detached and the call returns RT_ERR_DEVICE.  0 (default) = wait without limit, polling only for
 * asynchronous errors. */
rt_status rt_comm_set_timeout(rt_scene *scene, uint32_t timeout_ms);

/* --- introspection (tests / tooling) -------------------------------------------- */

typedef struct rt_scene_info {
    uint64_t blas_count;
    uint64_t blas_node_pairs;      /* interior nodes over all BLAS (= node-pair records) */
    uint64_t blas_leaves;
    uint64_t tlas_node_pairs;
    uint64_t device_bytes;         /* HBM held by the scene */
    uint32_t width, height;
    uint32_t sqrt_sample_count;
    uint32_t ray_trace_depth;
    uint32_t tlas_height;          /* interior levels on the longest TLAS root-to-leaf path */
    uint32_t blas_height_max;      /* the same, deepest BLAS */
    uint32_t overlap_lanes;        /* lanes consecutive frames cycle through (option "overlap"; -1 = auto, resolved
                                    * by the last rt_render) */
    uint32_t stage_depth;          /* pinned staging buffers of the per-frame upload */
} rt_scene_info;

rt_status rt_scene_get_info(const rt_scene *scene, rt_scene_info *info);

/* Export a BLAS in the reference's node form (BLASNode array + BLASIndex array,
 * include/AS/BLAS.cuh:20-34) for tree-identity tests.  Pass NULL buffers to query sizes.
 * nodes: 8 floats per node {xmin,xmax,ymin,ymax,zmin,zmax, count, index} (count/index as
 * exact float-encoded integers < 2^24 are NOT assumed: use the uint32 arrays). */
rt_status rt_scene_export_blas(const rt_scene *scene, uint32_t blas_index,
                               float *node_boxes /* 6 per node */, uint32_t *node_count_index /* 2 per node */,
                               uint32_t *prim_refs /* primitive index per slot */,
                               uint32_t *n_nodes, uint32_t *n_prims);

/* Export the current TLAS (include/AS/TLAS.cuh:24-39) in the same form; prim_refs receive
 * instance indices (option "group": a ref >= instance_count is group ref - instance_count, standing for
 * its member instances in this frame). */
rt_status rt_scene_export_tlas(const rt_scene *scene,
                               float *node_boxes, uint32_t *node_count_index,
                               uint32_t *instance_refs, uint32_t *n_nodes, uint32_t *n_refs);

/* Built-in copy of the demo animation (src/Global/Main.cu:6-42 updateInstance) so that
 * benchmarks do not cross into Python per frame.  Matches rt_update_fn; `user` unused. */
void rt_demo_update(void *user, rt_xform *xforms, size_t instance_count, uint64_t frame);

/* --- scene ingestion: legacy VTK particle files ------------------------------
 * VTKReader::readVTKFile (src/Global/VTKReader.cu:16-164): DATASET POLYDATA, ASCII or BINARY,
 * POINTS + TRIANGLE_STRIPS (one strip = one particle; other cell types are rejected), cell arrays
 * "id" and "vel".  Vertex normals restate vtkPolyDataNormals (VTKReader.cu:60-70) from its
 * documented behaviour — parity unpinned at that third-party boundary.
 * Host-only: no GPU is needed. */
typedef struct rt_vtk_file rt_vtk_file;

typedef struct rt_vtk_info {
    uint64_t point_count;
    uint64_t particle_count;       /* strip cells */
    uint64_t strip_vertex_count;   /* sum of strip lengths (VTKParticle::vertices, concatenated) */
    uint64_t triangle_count;       /* sum of (strip length - 2) */
} rt_vtk_info;

/* VTKParticle (include/Global/VTKReader.cuh:12-30) without its vertex arrays. */
typedef struct rt_vtk_particle {
    uint64_t id;
    rt_vec3 velocity;
    float bounds[6];               /* [xmin,xmax,ymin,ymax,zmin,zmax] of the cell's points */
    rt_vec3 centroid;              /* mean of the cell's points (double sum, cast to float) */
    uint32_t first_vertex;         /* into the concatenated strip vertex stream */
    uint32_t vertex_count;
} rt_vtk_particle;

rt_status rt_vtk_read(const char *path, rt_vtk_file **out);
void rt_vtk_free(rt_vtk_file *file);
rt_status rt_vtk_get_info(const rt_vtk_file *file, rt_vtk_info *info);
/* particles[particle_count] */
rt_status rt_vtk_particles(const rt_vtk_file *file, rt_vtk_particle *particles);
/* strip vertex stream: positions / normals [strip_vertex_count] (either may be NULL) */
rt_status rt_vtk_vertices(const rt_vtk_file *file, rt_vec3 *positions, rt_vec3 *normals);
/* VTKReader::convertToRendererData (VTKReader.cu:166-220): triangles[triangle_count] (METAL 0,
 * odd strip triangles swap vertices 2/3), instances[particle_count] (local bounds / centroid of the
 * particle, transform shift (0,4,0) rotate (90,0,0) scale 3).  triangle_index_base = index of the
 * first particle triangle in the scene's triangle array (0 when prepended, Renderer.cu:13-18). */
rt_status rt_vtk_convert(const rt_vtk_file *file, uint32_t triangle_index_base, rt_triangle *triangles,
                         rt_instance_desc *instances);

/* Renderer::configureVTKFiles (src/Global/Renderer.cu:394-443): the .vtk.series JSON index;
 * entry paths are resolved against the series file's directory. */
typedef struct rt_vtk_series rt_vtk_series;
rt_status rt_vtk_series_read(const char *path, rt_vtk_series **out);
size_t rt_vtk_series_count(const rt_vtk_series *series);
rt_status rt_vtk_series_entry(const rt_vtk_series *series, size_t index, const char **path, float *time);
void rt_vtk_series_free(rt_vtk_series *series);

#ifdef __cplusplus
}
#endif

#endif /* RT_H */
