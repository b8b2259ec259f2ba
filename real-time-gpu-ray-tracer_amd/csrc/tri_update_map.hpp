// tri_update_map.hpp — rt_scene_update_triangles_device: which floats one work item of the update kernel moves.
// Shared by the kernel (tri_update.hip) and the host replay that checks it (tests/cpp/tri_update_map_check.cpp), so
// the header is plain C++ without HIP types.
//
// A caller's triangle t is 9 vertex floats (and optionally 9 normal floats) in flat streams; the scene keeps it twice:
// as the first 18 floats of its 22-float (88 B) rt_triangle record in raw_tris, and as 9 floats of raw_verts.  The
// update of `count` triangles is cut into 9 * count work items, 9 per triangle: item w = 9 t + p
//   - copies vertex-stream element w to raw_verts[9 first + w]: both sides are the same flat stream, so a wave reads
//     and writes 64 consecutive dwords;
//   - writes float pair p (floats 2p, 2p + 1) of record first + t.  A record starts at a multiple of 88 B, which is
//     8-byte but only every other time 16-byte aligned, so the pair — one 8-byte store — is the widest store that is
//     aligned for every record and every `first`; 9 pairs cover the 72 bytes of the vertex and normal fields exactly.
//     Pair 4 straddles the fields (vertex float 8, normal float 0): without normals it shrinks to one float and pairs
//     5..8 write nothing to the record;
//   - with normals, item p = 8 also sets the record's has_normals word.
// material_type, material_index and reserved are never written.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TRI_UPDATE_HD __host__ __device__
#else
#define TRI_UPDATE_HD
#endif

namespace rtamd {

constexpr uint32_t TRI_RECORD_FLOATS = 22;        // sizeof(rt_triangle) / 4
constexpr uint32_t TRI_FIELD_FLOATS = 18;         // vertex[3] + normal[3]
constexpr uint32_t TRI_HAS_NORMALS_WORD = 20;     // offsetof(rt_triangle, has_normals) / 4
constexpr uint32_t TRI_ITEMS = 9;                 // work items per triangle

struct TriUpdateItem {
    uint64_t verts_dst;    // raw_verts float index that receives vertex-stream element w
    uint64_t rec_dst;      // float index into raw_tris (as floats) of the first float this item stores
    uint64_t src;          // 9 * t: the triangle's first element in the vertex and in the normal stream
    uint32_t field;        // first record float stored (2p): < 9 comes from vertices[src + field], else normals[src + field - 9]
    uint32_t rec_floats;   // floats stored into the record: 2 (one 8-byte store), 1 or 0
    uint64_t flag_dst;     // word index into raw_tris of has_normals, valid when set_flag
    bool set_flag;
};

// work item w of an update of triangles [first, first + count), w < 9 * count
TRI_UPDATE_HD inline TriUpdateItem tri_update_map(uint64_t w, uint64_t first, bool normals) {
    const uint64_t t = w / TRI_ITEMS;
    const uint32_t p = (uint32_t)(w - t * TRI_ITEMS);
    const uint64_t rec = (first + t) * TRI_RECORD_FLOATS;
    TriUpdateItem it;
    it.verts_dst = first * 9 + w;
    it.src = t * 9;
    it.field = 2 * p;
    it.rec_dst = rec + it.field;
    it.rec_floats = normals ? 2u : (p < 4 ? 2u : (p == 4 ? 1u : 0u));
    it.flag_dst = rec + TRI_HAS_NORMALS_WORD;
    it.set_flag = normals && p == TRI_ITEMS - 1;
    return it;
}

// record float `field` (0..17) of the triangle whose streams start at element `src`
TRI_UPDATE_HD inline float tri_update_source(const float *vertices, const float *normals, uint64_t src, uint32_t field) {
    return field < 9 ? vertices[src + field] : normals[src + field - 9];
}

}  // namespace rtamd
