// Host replay of rt_scene_update_triangles_device's kernel (csrc/tri_update.hip): every work item of an update of
// triangles [first, first + count) of an n-triangle scene is mapped with the kernel's own tri_update_map
// (csrc/tri_update_map.hpp) and applied to host arrays.  Usage: tri_update_map_check n first count normals(0|1)
// Prints one JSON line:
//   written_once   every target float of raw_tris and raw_verts was written exactly once (0: some twice or never)
//   wrong_source   target floats that do not hold their source element
//   outside_bytes  bytes outside the target fields and range that changed (material_type, material_index, reserved,
//                  normal[] and has_normals without normals, neighbouring records, raw_verts outside the range)
//   flag_writes    has_normals words written;  flag_bad  of them outside the range, not 1, or written without normals
//   misaligned     8-byte record stores whose address is not 8-byte aligned (the records' array is 16-byte aligned)
//   verts_equal    raw_verts of the range equals the caller's vertex stream
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/rt.h"
#include "../../real-time-gpu-ray-tracer_amd/csrc/tri_update_map.hpp"

using namespace rtamd;

static_assert(sizeof(rt_triangle) == TRI_RECORD_FLOATS * sizeof(float), "record size");
static_assert(offsetof(rt_triangle, normal) == 9 * sizeof(float), "normal");
static_assert(offsetof(rt_triangle, material_type) == TRI_FIELD_FLOATS * sizeof(float), "material_type");
static_assert(offsetof(rt_triangle, has_normals) == TRI_HAS_NORMALS_WORD * sizeof(float), "has_normals");

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const uint64_t n = std::strtoull(argv[1], nullptr, 10), first = std::strtoull(argv[2], nullptr, 10);
    const uint64_t count = std::strtoull(argv[3], nullptr, 10);
    const bool normals = std::atoi(argv[4]) != 0;
    if (first > n || count > n - first) return 2;

    // the scene's arrays, filled with a pattern no source value repeats; the records 16-byte aligned as hipMalloc's
    std::vector<uint32_t> store(n * TRI_RECORD_FLOATS + 4), verts(n * 9);
    uint32_t *recs = store.data();
    while ((uintptr_t)recs & 15u) recs++;
    for (uint64_t i = 0; i < n * TRI_RECORD_FLOATS; i++) recs[i] = 0xA0000000u + (uint32_t)i;
    for (uint64_t i = 0; i < n * 9; i++) verts[i] = 0xB0000000u + (uint32_t)i;
    const std::vector<uint32_t> recs0(recs, recs + n * TRI_RECORD_FLOATS), verts0 = verts;
    // the caller's streams, exactly 9 * count floats each: one element past them is out of bounds for the sanitizer
    std::vector<float> vsrc(count * 9), nsrc(normals ? count * 9 : 0);
    for (uint64_t i = 0; i < vsrc.size(); i++) vsrc[i] = (float)(1 + i);
    for (uint64_t i = 0; i < nsrc.size(); i++) nsrc[i] = -(float)(1 + i);
    std::vector<uint8_t> rec_writes(n * TRI_RECORD_FLOATS, 0), vert_writes(n * 9, 0);
    uint64_t flag_writes = 0, flag_bad = 0, misaligned = 0, out_of_array = 0;

    float *recf = reinterpret_cast<float *>(recs), *vertf = reinterpret_cast<float *>(verts.data());
    const float *np = normals ? nsrc.data() : nullptr;
    for (uint64_t w = 0; w < count * TRI_ITEMS; w++) {           // the kernel's loop body, one work item at a time
        const TriUpdateItem it = tri_update_map(w, first, normals);
        if (it.verts_dst >= n * 9 || it.rec_dst + it.rec_floats > n * TRI_RECORD_FLOATS) { out_of_array++; continue; }
        vertf[it.verts_dst] = vsrc[w];
        vert_writes[it.verts_dst]++;
        if (it.rec_floats == 2 && ((uintptr_t)(recf + it.rec_dst) & 7u)) misaligned++;
        for (uint32_t k = 0; k < it.rec_floats; k++) {
            recf[it.rec_dst + k] = tri_update_source(vsrc.data(), np, it.src, it.field + k);
            rec_writes[it.rec_dst + k]++;
        }
        if (it.set_flag) {
            flag_writes++;
            const uint64_t t = it.flag_dst / TRI_RECORD_FLOATS;
            if (!normals || it.flag_dst % TRI_RECORD_FLOATS != TRI_HAS_NORMALS_WORD || t < first || t >= first + count) flag_bad++;
            if (it.flag_dst < n * TRI_RECORD_FLOATS) { recs[it.flag_dst] = 1u; rec_writes[it.flag_dst]++; }
            else out_of_array++;
        }
    }

    uint64_t not_once = 0, wrong = 0, outside = 0;
    const uint32_t fields = normals ? 18u : 9u;
    for (uint64_t t = 0; t < n; t++)
        for (uint32_t f = 0; f < TRI_RECORD_FLOATS; f++) {
            const uint64_t i = t * TRI_RECORD_FLOATS + f;
            const bool in_range = t >= first && t < first + count;
            const bool target = in_range && (f < fields || (normals && f == TRI_HAS_NORMALS_WORD));
            if (target) {
                if (rec_writes[i] != 1) not_once++;
                float want;
                uint32_t want_bits;
                if (f == TRI_HAS_NORMALS_WORD) want_bits = 1u;
                else {
                    want = f < 9 ? vsrc[(t - first) * 9 + f] : nsrc[(t - first) * 9 + f - 9];
                    std::memcpy(&want_bits, &want, 4);
                }
                if (recs[i] != want_bits) wrong++;
            } else {
                if (rec_writes[i] != 0) not_once++;
                if (recs[i] != recs0[i]) outside += 4;
            }
        }
    bool verts_equal = true;
    for (uint64_t i = 0; i < n * 9; i++) {
        const bool target = i >= first * 9 && i < (first + count) * 9;
        if (vert_writes[i] != (target ? 1 : 0)) not_once++;
        if (target) verts_equal = verts_equal && std::memcmp(&verts[i], &vsrc[i - first * 9], 4) == 0;
        else if (verts[i] != verts0[i]) outside += 4;
    }
    std::printf("{\"written_once\": %d, \"wrong_source\": %llu, \"outside_bytes\": %llu, \"flag_writes\": %llu, "
                "\"flag_bad\": %llu, \"misaligned\": %llu, \"out_of_array\": %llu, \"verts_equal\": %d}\n",
                not_once == 0 ? 1 : 0, (unsigned long long)wrong, (unsigned long long)outside,
                (unsigned long long)flag_writes, (unsigned long long)flag_bad, (unsigned long long)misaligned,
                (unsigned long long)out_of_array, verts_equal ? 1 : 0);
    return 0;
}
