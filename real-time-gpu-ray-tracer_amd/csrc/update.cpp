// update.cpp — the geometry updates between frames: rt_scene_update_triangles (host memory), _triangles_device
// (device memory, RT_BUILD_LBVH) and _instances, with the state that says who holds a record's local bounds — the
// host, or the device after RT_TRI_UPDATE_BOUNDS (rt_scene::dev_bounded, inst_bounds.hip) — and the host mirror of
// the triangles a device update wrote.
#include "launch.hpp"
#include "scene.hpp"

namespace rtamd {

// The host mirror `tris` after rt_scene_update_triangles_device: read raw_tris back once (a cold path: the device is
// drained).  Called before the mirror's geometry is read: prim_box / prim_centroid, the host builders, the upload
// of raw_tris by a second rt_scene_build.
rt_status refresh_tris_mirror(rt_scene *s) {
    if (!s->tris_host_stale) return RT_OK;
    RT_TRY(drain(s));
    HIP_TRY(hipMemcpy(s->tris.data(), s->raw_tris.p, s->tris.size() * sizeof(rt_triangle), hipMemcpyDeviceToHost));
    s->tris_host_stale = false;
    return RT_OK;
}

// RT_TRI_UPDATE_BOUNDS (inst_bounds.hip), at rt_scene_build: the static tables — an instance's primitives never
// change — the partial sums, and every record's local centroid as the host holds it.  No record is device-bounded.
rt_status setup_inst_bounds(rt_scene *s) {
    const size_t n = s->inst.size() + s->groups.size();
    s->dev_bounded.assign(n, 0);
    s->ib_entry_of.assign(s->inst.size(), rt_scene::NONE);
    std::vector<InstBoundsEntry> table;
    std::vector<uint32_t> chunk_inst, multi, members;
    std::vector<uint2> groups;
    for (size_t i = 0; i < s->inst.size(); i++) {
        const InstState &in = s->inst[i];
        if (in.ptype != RT_PRIM_TRIANGLE) continue;
        s->ib_entry_of[i] = (uint32_t)table.size();
        const uint32_t nc = ib_chunks(in.pcount);
        if (nc > 1) multi.push_back((uint32_t)table.size());
        table.push_back(InstBoundsEntry{in.pindex, in.pcount, (uint32_t)chunk_inst.size(), (uint32_t)i});
        chunk_inst.insert(chunk_inst.end(), nc, (uint32_t)table.size() - 1);
    }
    for (const InstGroup &G : s->groups) {
        groups.push_back(make_uint2((uint32_t)members.size(), (uint32_t)G.members.size()));
        for (uint32_t m : G.members) members.push_back(s->ib_entry_of[m]);       // groups hold triangle instances only
    }
    RT_TRY(upload(s->ib_table, table));
    RT_TRY(upload(s->ib_chunk_inst, chunk_inst));
    RT_TRY(upload(s->ib_multi, multi));
    RT_TRY(upload(s->ib_groups, groups));
    RT_TRY(upload(s->ib_members, members));
    RT_TRY(alloc_buf(s->ib_partials, 3 * chunk_inst.size()));
    std::vector<float4> cent(n);
    for (size_t i = 0; i < n; i++) {
        const hm::V3 c = record_state(s, i).centroid;
        cent[i] = make_float4(c.x, c.y, c.z, 0.0f);
    }
    RT_TRY(upload(s->ib_cent, cent));
    if (s->ib_cent_stage) HIP_TRY(hipHostFree(s->ib_cent_stage));
    s->ib_cent_stage = nullptr;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&s->ib_cent_stage), (n ? n : 1) * sizeof(float4), hipHostMallocDefault));
    return RT_OK;
}

}  // namespace rtamd

namespace {

// setup_inst_bounds' tables as the kernels of inst_bounds.hip take them
InstBoundsGPU inst_bounds_gpu(const rt_scene *s) {
    return InstBoundsGPU{s->ib_table.p, s->ib_chunk_inst.p, s->ib_multi.p, s->ib_groups.p, s->ib_members.p,
                         (uint32_t)s->ib_chunk_inst.n, (uint32_t)s->ib_multi.n, (uint32_t)s->ib_groups.n,
                         (uint32_t)s->inst.size(), s->ib_partials.p, s->ib_cent.p};
}

bool tri_range_overlaps(const InstState &in, uint64_t first, uint64_t count) {
    return in.ptype == RT_PRIM_TRIANGLE && (uint64_t)in.pindex + in.pcount > first && in.pindex < first + count;
}

// RT_TRI_UPDATE_BOUNDS: the host changed the local centroids of `records` (sorted): their entries of the device array,
// which a group's mean reads, on the scene stream — through the pinned stage, after the record chains of the frames
// already enqueued (a chain may still read the device-written value of a record the host just took back)
rt_status refresh_dev_centroids(rt_scene *s, const std::vector<uint32_t> &records) {
    if (records.empty() || !s->ib_cent.p) return RT_OK;
    RT_TRY(wait_record_chains(s, s->stream));
    for (size_t k = 0; k < records.size();) {
        size_t e = k;
        while (e + 1 < records.size() && records[e + 1] == records[e] + 1) e++;
        for (size_t j = k; j <= e; j++) {
            const hm::V3 c = record_state(s, records[j]).centroid;
            s->ib_cent_stage[records[j]] = make_float4(c.x, c.y, c.z, 0.0f);
        }
        HIP_TRY(hipMemcpyAsync(s->ib_cent.p + records[k], s->ib_cent_stage + records[k], (e - k + 1) * sizeof(float4),
                               hipMemcpyHostToDevice, s->stream));
        k = e + 1;
    }
    return RT_OK;
}

// an instance's bounds as rt_scene_update_triangles derives them from the (current) host mirror
void host_bounds(rt_scene *s, InstState &in) {
    bounds_from_prims(s, in);
    if (in.pcount == 1) in.centroid = prim_centroid(s, in.ptype, in.pindex);   // not the mean of one: keeps a -0
}

// What rt_scene_update_triangles and rt_scene_update_triangles_device check alike: the scene's state, its build mode
// and the range, overflow-safe.
rt_status tri_update_check(const rt_scene *s, uint64_t first, uint64_t count) {
    if (!s->built) return fail(RT_ERR_STATE, "rt_scene_build has not been called");
    if (s->build_mode != RT_BUILD_LBVH) return fail(RT_ERR_UNSUPPORTED, "triangle updates need RT_BUILD_LBVH");
    if (first > s->tris.size() || count > s->tris.size() - first) return fail(RT_ERR_INVALID_ARGUMENT, "triangle range out of bounds");
    return RT_OK;
}

// ... and what both order their write into raw_tris behind.  No drain: the write goes on the scene stream, behind its
// pending BLAS builds (the next build, which the frame update enqueues after it, reads the new triangles); with
// raw_shading() traces read raw_tris at their hits too, so it also waits for every lane's last trace (and the last
// synchronous one)
rt_status tri_update_waits(rt_scene *s) {
    if (!s->raw_shading()) return RT_OK;
    if (s->r_done) HIP_TRY(hipStreamWaitEvent(s->stream, s->r_done, 0));
    for (const Lane &l : s->ln)
        if (l.r_done) HIP_TRY(hipStreamWaitEvent(s->stream, l.r_done, 0));
    return wait_queries(s, s->stream);               // a query's records read raw_tris too (finalize, RAW 1)
}

}  // namespace

extern "C" {

rt_status rt_scene_update_triangles(rt_scene *s, size_t first, size_t count, const rt_triangle *tris) {
    if (!s || (count && !tris)) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    RT_TRY(tri_update_check(s, first, count));
    if (count == 0) return RT_OK;
    RT_TRY(check_materials(s, tris, count, "triangle"));
    HIP_TRY(hipSetDevice(s->device));
    if (s->ev_raw_staged) RT_TRY(wait_event(s, s->ev_raw_staged));      // the previous staged copy is done
    else HIP_TRY(hipEventCreateWithFlags(&s->ev_raw_staged, hipEventDisableTiming));
    if (count > s->raw_stage_cap) {
        if (s->raw_stage) HIP_TRY(hipHostFree(s->raw_stage));
        s->raw_stage = nullptr;
        s->raw_stage_cap = 0;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&s->raw_stage), count * sizeof(rt_triangle), hipHostMallocDefault));
        s->raw_stage_cap = count;
    }
    std::memcpy(s->raw_stage, tris, count * sizeof(rt_triangle));
    std::memcpy(s->tris.data() + first, tris, count * sizeof(rt_triangle));
    RT_TRY(tri_update_waits(s));
    HIP_TRY(hipMemcpyAsync(s->raw_tris.p + first, s->raw_stage, count * sizeof(rt_triangle), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(extract_tri_verts(s->raw_tris.p, s->raw_verts.p, first, count, s->stream));
    HIP_TRY(hipEventRecord(s->ev_raw_staged, s->stream));
    // instance boxes derived from the triangles (RenderPin.cu:124-139); VTK-style bounds stay as given.  A
    // device-bounded instance in the range, or in a group with a member in the range, comes back to the host: its
    // bounds from the mirror, read back first (RT_TRI_UPDATE_BOUNDS)
    const size_t ni = s->inst.size();
    std::vector<uint8_t> back(ni, 0);
    for (size_t g = 0; g < s->groups.size(); g++) {
        const InstGroup &G = s->groups[g];
        if (!dev_bounded_rec(s, ni + g)) continue;
        bool touched = false;
        for (uint32_t m : G.members) touched = touched || tri_range_overlaps(s->inst[m], first, count);
        if (!touched) continue;
        for (uint32_t m : G.members) back[m] = s->dev_bounded[m];
        s->dev_bounded[ni + g] = 0;
    }
    std::vector<uint32_t> changed;                     // group members whose centroid the host changed
    for (size_t i = 0; i < s->inst.size(); i++) {
        InstState &in = s->inst[i];
        const rt_instance_desc &id = s->inst_desc[i];
        const bool in_range = tri_range_overlaps(in, first, count);
        const bool take_back = back[i] || (dev_bounded_rec(s, i) && in_range);
        if (!take_back && (!in_range || id.has_local_bounds)) continue;
        RT_TRY(refresh_tris_mirror(s));     // after a device update: raw_tris, this call's copy included, read back once
        host_bounds(s, in);
        instance_update(in, in.x);
        if (take_back) s->dev_bounded[i] = 0;
        if (s->gpu_tlas()) s->inst_dirty[i] = rt_scene::ALL_BLOCKS;     // the GPU copies of its local box
        if (s->group_of[i]) changed.push_back((uint32_t)i);
    }
    for (size_t g = 0; g < s->groups.size(); g++) {   // option "group" (LBVH): the union of the members' boxes
        if (dev_bounded_rec(s, ni + g)) continue;                       // the device's, untouched by this range
        group_bounds(s, s->groups[g]);
        if (s->gpu_tlas()) s->inst_dirty[s->inst.size() + g] = rt_scene::ALL_BLOCKS;
    }
    RT_TRY(refresh_dev_centroids(s, changed));
    s->blas_dirty = true;
    return RT_OK;
}

rt_status rt_scene_update_triangles_device(rt_scene *s, const rt_triangle_update *u) {
    if (!s || !u) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (u->reserved != 0 || (u->flags & ~(uint32_t)(RT_TRI_UPDATE_NO_SYNC | RT_TRI_UPDATE_BOUNDS)))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_update_triangles_device: reserved bits set");
    if (u->count && !u->vertices_device) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    RT_TRY(tri_update_check(s, u->first, u->count));
    if (u->count == 0) return RT_OK;
    DeviceRestore restore;
    HIP_TRY(hipSetDevice(s->device));
    if (!device_accessible(u->vertices_device, s->device) || (u->normals_device && !device_accessible(u->normals_device, s->device)))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_update_triangles_device: a buffer is not accessible from the scene's device");
    const bool bounds = (u->flags & RT_TRI_UPDATE_BOUNDS) != 0;
    // instance bounds derived from the triangles (rt_scene_update_triangles recomputes them on the host) cannot
    // follow vertices the host never sees, unless the device derives them (RT_TRI_UPDATE_BOUNDS)
    for (size_t i = 0; i < s->inst.size() && !bounds; i++) {
        const InstState &in = s->inst[i];
        if (in.ptype != RT_PRIM_TRIANGLE || s->inst_desc[i].has_local_bounds) continue;
        if ((uint64_t)in.pindex + in.pcount <= u->first || in.pindex >= u->first + u->count) continue;
        return fail(RT_ERR_UNSUPPORTED, "rt_scene_update_triangles_device: instance " + std::to_string(i) +
                                            " derives its bounds from triangles in the range (has_local_bounds == 0)");
    }
    // a device-bounded instance's box is its BLAS's root: the BLAS must hold exactly the instance's triangles (instances
    // with one first primitive share a BLAS whatever their counts)
    for (size_t i = 0; i < s->inst.size() && bounds; i++) {
        const InstState &in = s->inst[i];
        if (!tri_range_overlaps(in, u->first, u->count) || s->lbvh_segs[in.blas].count == in.pcount) continue;
        return fail(RT_ERR_UNSUPPORTED, "rt_scene_update_triangles_device: instance " + std::to_string(i) +
                                            " shares the BLAS of an instance with another primitive count");
    }
    if (!s->ev_tri_update) HIP_TRY(hipEventCreateWithFlags(&s->ev_tri_update, hipEventDisableTiming));
    // scene stream after the caller's (the buffers' producer), the kernel where the host path's copy sits, the
    // caller's stream after the kernel (the buffers are free again in its order)
    hipStream_t from = static_cast<hipStream_t>(u->stream);
    if (from || hipStreamQuery(nullptr) == hipErrorNotReady) RT_TRY(order_after_stream(s, from, s->stream));
    RT_TRY(tri_update_waits(s));
    HIP_TRY(launch_tri_update(s->raw_tris.p, s->raw_verts.p, u->vertices_device, u->normals_device, u->first, u->count, s->stream));
    HIP_TRY(hipEventRecord(s->ev_tri_update, s->stream));
    HIP_TRY(hipStreamWaitEvent(from, s->ev_tri_update, 0));
    if (bounds) {
        // every triangle instance the range overlaps, and its group, is device-bounded from the next frame update on:
        // that update rebuilds the BLASes (their roots are the boxes) behind these kernels on the scene stream, and
        // every record chain waits for that build.  The centroid array is shared by all frame blocks, so the kernels
        // wait for the chains already enqueued; nothing here waits for a trace or for the device to drain
        const size_t ni = s->inst.size();
        for (size_t i = 0; i < ni; i++) {
            if (!tri_range_overlaps(s->inst[i], u->first, u->count)) continue;
            if (!s->dev_bounded[i]) { s->dev_bounded[i] = 1; s->inst_dirty[i] = rt_scene::ALL_BLOCKS; }
            if (!s->group_of[i]) continue;
            const size_t gr = ni + s->group_of[i] - 1;             // its group's record
            if (!s->dev_bounded[gr]) { s->dev_bounded[gr] = 1; s->inst_dirty[gr] = rt_scene::ALL_BLOCKS; }
        }
        RT_TRY(wait_record_chains(s, s->stream));
        HIP_TRY(launch_inst_bounds(inst_bounds_gpu(s), s->raw_verts.p, u->first, u->count, s->stream));
    }
    s->tris_host_stale = true;
    s->blas_dirty = true;
    if (u->flags & RT_TRI_UPDATE_NO_SYNC) return RT_OK;
    return wait_event(s, s->ev_tri_update);
}

rt_status rt_scene_update_instances(rt_scene *s, size_t first, size_t count, const rt_instance_desc *d) {
    if (!s || (count && !d)) return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!s->built) return fail(RT_ERR_STATE, "rt_scene_build has not been called");
    if (first > s->inst.size() || count > s->inst.size() - first) return fail(RT_ERR_INVALID_ARGUMENT, "instance range out of bounds");
    for (size_t k = 0; k < count; k++) {
        const rt_instance_desc &o = s->inst_desc[first + k], &n = d[k];
        if (o.primitive_type != n.primitive_type || o.primitive_index != n.primitive_index ||
            o.primitive_count != n.primitive_count)
            return fail(RT_ERR_INVALID_ARGUMENT, "an instance update may not change its primitives (type / index / count)");
    }
    for (size_t k = 0; k < count; k++) {
        const size_t i = first + k;
        s->inst_desc[i] = d[k];
        InstState &in = s->inst[i];
        if (d[k].has_local_bounds) {                                          // VTKReader.cu:204-209
            bounds_from_desc(d[k], in);
        } else if (dev_bounded_rec(s, i)) {                                   // back from the device: the mirror, read back
            RT_TRY(refresh_tris_mirror(s));
            host_bounds(s, in);
        }
        if (!s->dev_bounded.empty()) s->dev_bounded[i] = 0;                   // RT_TRI_UPDATE_BOUNDS ends here
        instance_update(in, d[k].xform);
        if (s->gpu_tlas()) s->inst_dirty[i] = rt_scene::ALL_BLOCKS;
        // option "group": the group's box and transform were taken at the build; its members go back to
        // their own TLAS items for good
        if (s->group_of[i]) s->groups[s->group_of[i] - 1].valid = false;
    }
    return RT_OK;
}

}  // extern "C"
