// tri_update.hip — rt_scene_update_triangles_device's kernel: the caller's flat vertex (and normal) streams into the
// scene's raw triangles, in one launch what the host path does with a staged copy and extract_tri_verts.
//
// Access widths (tri_update_map.hpp holds the mapping; the host replay tests/cpp/tri_update_map_check.cpp checks it):
//   reads   the caller's streams are contiguous floats whose base the caller chooses (a torch view may start at any
//           4-byte boundary) and a triangle is 9 floats, an odd count: only dword loads are aligned for every caller
//           and every triangle.  Consecutive lanes read consecutive dwords (the raw_verts copy) or dwords two apart
//           within the ~130 floats a wave's 7-8 triangles span (the record pairs), so every load instruction of a
//           wave falls into two or three 128 B lines that the copy just fetched.
//   stores  raw_verts: the same flat stream, shifted by 9 first floats (odd for odd first): dword stores, 256
//           contiguous bytes per wave instruction.  raw_tris: records are 88 B apart, 8-byte but not 16-byte aligned,
//           so 8-byte stores (float2) are the widest aligned for every record; 9 of them cover the 72 B of vertex and
//           normal fields and leave material_type / material_index / reserved untouched.  A 16-byte store would be
//           aligned for every other record only and would need a second code path per parity of first + t.
// Memory-bound: per triangle 72 B read (36 without normals) and 112 B written (76); a grid capped at 2048 workgroups
// strides over the 9 count work items with 64-bit indices (9 x 2^26 triangles do not fit 32 bits as bytes).
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "tri_update_map.hpp"

namespace rtamd {

namespace {

constexpr uint32_t TRI_UPDATE_BLOCK = 256;
constexpr uint64_t TRI_UPDATE_MAX_GRID = 2048;   // 256 CUs x 8 workgroups; the rest by the grid stride

template <bool NORMALS>
__global__ __launch_bounds__(TRI_UPDATE_BLOCK) void tri_update_kernel(float *__restrict__ recs, float *__restrict__ verts_out,
                                                                      const float *__restrict__ vertices,
                                                                      const float *__restrict__ normals, uint64_t first,
                                                                      uint64_t count) {
    const uint64_t total = count * TRI_ITEMS, stride = (uint64_t)gridDim.x * TRI_UPDATE_BLOCK;
    for (uint64_t w = (uint64_t)blockIdx.x * TRI_UPDATE_BLOCK + threadIdx.x; w < total; w += stride) {
        const TriUpdateItem it = tri_update_map(w, first, NORMALS);
        verts_out[it.verts_dst] = vertices[w];
        if (it.rec_floats == 2) {
            float2 pair;
            pair.x = tri_update_source(vertices, normals, it.src, it.field);
            pair.y = tri_update_source(vertices, normals, it.src, it.field + 1);
            *reinterpret_cast<float2 *>(recs + it.rec_dst) = pair;       // 8-byte aligned: 88 (first + t) + 8 p
        } else if (it.rec_floats == 1) {
            recs[it.rec_dst] = tri_update_source(vertices, normals, it.src, it.field);
        }
        if (it.set_flag) reinterpret_cast<uint32_t *>(recs)[it.flag_dst] = 1u;
    }
}

}  // namespace

hipError_t launch_tri_update(rt_triangle *raw_tris, float *raw_verts, const float *vertices, const float *normals,
                             uint64_t first, uint64_t count, hipStream_t stream) {
    static_assert(sizeof(rt_triangle) == TRI_RECORD_FLOATS * sizeof(float), "tri_update_map.hpp: record size");
    static_assert(offsetof(rt_triangle, normal) == 9 * sizeof(float) &&
                  offsetof(rt_triangle, material_type) == TRI_FIELD_FLOATS * sizeof(float) &&
                  offsetof(rt_triangle, has_normals) == TRI_HAS_NORMALS_WORD * sizeof(float), "tri_update_map.hpp: record layout");
    if (count == 0) return hipSuccess;
    const uint64_t blocks = (count * TRI_ITEMS + TRI_UPDATE_BLOCK - 1) / TRI_UPDATE_BLOCK;
    const dim3 grid((uint32_t)(blocks < TRI_UPDATE_MAX_GRID ? blocks : TRI_UPDATE_MAX_GRID));
    float *recs = reinterpret_cast<float *>(raw_tris);
    if (normals)
        hipLaunchKernelGGL(tri_update_kernel<true>, grid, dim3(TRI_UPDATE_BLOCK), 0, stream, recs, raw_verts, vertices, normals,
                           first, count);
    else
        hipLaunchKernelGGL(tri_update_kernel<false>, grid, dim3(TRI_UPDATE_BLOCK), 0, stream, recs, raw_verts, vertices,
                           (const float *)nullptr, first, count);
    return hipGetLastError();
}

}  // namespace rtamd
