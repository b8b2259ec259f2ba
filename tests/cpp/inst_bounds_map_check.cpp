// Host replay of RT_TRI_UPDATE_BOUNDS's centroid kernels (csrc/inst_bounds.hip) with the kernels' own map
// (csrc/inst_bounds_map.hpp).  Usage: inst_bounds_map_check verts.f32 first_tri count [count ...]
// verts.f32 holds 9 floats per triangle; the instances lie back to back from triangle first_tri on (an odd first_tri
// makes every wave's loads start at an odd float), with the given triangle counts.  The static table is built as
// rt_scene_build builds it, then every (instance, chunk) work item runs as the chunk kernel runs it: per wave and round
// the 9 masked loads of 64 consecutive floats — from a copy of the instance's floats that is exactly 9 * count long, so
// one float past it is out of bounds for the address sanitizer — the register pick, the cross-lane read, the lanes' double
// sums, wave and block steps, then the fold over the chunks' partials.  Prints one JSON line:
//   covered_once    every triangle of every instance was accumulated exactly once, none outside
//   transpose_bad   (lane, component) pairs that did not receive float 9 t + j of the wave's triangles
//   asker_bad       (source lane, component) pairs asked by no lane or by more than one
//   items_bad       work items whose table entry or chunk is wrong, partial slots written twice or never
//   shape_bad       axis sums of the replay that differ from ib_instance_sum (the header's statement of the shape)
//   sums            per instance the three double sums as hex bit patterns;  centroids  the float results likewise
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../real-time-gpu-ray-tracer_amd/csrc/inst_bounds_map.hpp"

using namespace rtamd;

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    std::vector<float> all;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        float buf[4096];
        size_t n;
        while ((n = std::fread(buf, sizeof(float), 4096, f)) > 0) all.insert(all.end(), buf, buf + n);
        std::fclose(f);
    }
    const uint64_t first_tri = std::strtoull(argv[2], nullptr, 10);
    std::vector<InstBoundsEntry> table;
    std::vector<uint32_t> chunk_inst;
    uint64_t at = first_tri;
    for (int k = 3; k < argc; k++) {                                   // as setup_inst_bounds (update.cpp)
        const uint32_t count = (uint32_t)std::strtoul(argv[k], nullptr, 10);
        if (count == 0 || (at + count) * 9 > all.size()) return 2;
        table.push_back(InstBoundsEntry{(uint32_t)at, count, (uint32_t)chunk_inst.size(), (uint32_t)table.size()});
        chunk_inst.insert(chunk_inst.end(), ib_chunks(count), (uint32_t)table.size() - 1);
        at += count;
    }

    uint64_t transpose_bad = 0, asker_bad = 0, items_bad = 0, shape_bad = 0, cover_bad = 0;
    for (uint32_t j = 0; j < 9; j++) {
        uint32_t asked[IB_WAVE] = {};
        for (uint32_t t = 0; t < IB_WAVE; t++) {
            const uint32_t s = ib_src_lane(t, j);
            asked[s]++;
            if (ib_asker(s, j) != t || ib_src_reg(t, j) >= IB_LOADS) asker_bad++;
        }
        for (uint32_t s = 0; s < IB_WAVE; s++) asker_bad += asked[s] != 1;
    }

    std::vector<double> partials(3 * chunk_inst.size(), 0.0);
    std::vector<uint8_t> partial_writes(chunk_inst.size(), 0);
    std::vector<std::vector<uint32_t>> seen(table.size());
    std::vector<std::vector<float>> verts(table.size());
    for (size_t i = 0; i < table.size(); i++) {
        seen[i].assign(table[i].count, 0);
        verts[i].assign(all.begin() + (size_t)table[i].pindex * 9, all.begin() + ((size_t)table[i].pindex + table[i].count) * 9);
    }
    std::vector<double> sums(3 * table.size(), 0.0);
    std::vector<float> cents(3 * table.size(), 0.0f);
    auto mean = [](double S, uint32_t n) { return (float)(S / n); };

    for (uint32_t item = 0; item < chunk_inst.size(); item++) {       // the chunk kernel, one workgroup per item
        const uint32_t ti = chunk_inst[item];
        const InstBoundsEntry e = table[ti];
        if (item < e.first_chunk || item - e.first_chunk >= ib_chunks(e.count)) { items_bad++; continue; }
        const uint32_t c = item - e.first_chunk;
        const float *base = verts[ti].data();                          // = raw_verts + 9 pindex
        double lane_acc[3][IB_BLOCK];
        float own[3] = {0, 0, 0};
        for (uint32_t wave = 0; wave < IB_WAVES; wave++) {
            double acc[IB_WAVE][3];
            for (uint32_t l = 0; l < IB_WAVE; l++) acc[l][0] = acc[l][1] = acc[l][2] = 0.0;
            for (uint32_t r = 0; r < IB_ROUNDS; r++) {
                const uint64_t t0 = ib_tri(c, r, wave, 0);
                if (t0 >= e.count) break;
                const uint64_t left = e.count - t0;
                const uint32_t live = 9u * (uint32_t)(left < IB_WAVE ? left : IB_WAVE);
                const float *src = base + t0 * 9u;
                float reg[IB_WAVE][IB_LOADS];
                for (uint32_t l = 0; l < IB_WAVE; l++)
                    for (uint32_t k = 0; k < IB_LOADS; k++) reg[l][k] = IB_WAVE * k + l < live ? src[IB_WAVE * k + l] : 0.0f;
                for (uint32_t l = 0; l < IB_WAVE; l++) {
                    float v[9];
                    for (uint32_t j = 0; j < 9; j++) {
                        const uint32_t s = ib_src_lane(l, j);                         // the lane read across
                        const uint32_t want = ib_src_reg(ib_asker(s, j), j);          // what that lane picked
                        v[j] = reg[s][want];
                        if (9u * l < live && std::memcmp(&v[j], &src[9u * l + j], 4) != 0) transpose_bad++;
                    }
                    if (9u * l >= live) continue;
                    const uint64_t k = ib_tri(c, r, wave, l);
                    if (k < e.count) seen[ti][k]++; else cover_bad++;
                    for (int a = 0; a < 3; a++) {
                        const float ca = ib_tri_centroid(v, a);
                        if (r == 0 && wave == 0 && l == 0) own[a] = ca;
                        acc[l][a] += (double)ca;
                    }
                }
            }
            for (uint32_t l = 0; l < IB_WAVE; l++)
                for (int a = 0; a < 3; a++) lane_acc[a][wave * IB_WAVE + l] = acc[l][a];
        }
        double S[3];
        for (int a = 0; a < 3; a++) S[a] = ib_block_sum(lane_acc[a]);
        if (ib_chunks(e.count) > 1) {
            for (int a = 0; a < 3; a++) partials[3 * (size_t)item + a] = S[a];
            partial_writes[item]++;
        } else {
            for (int a = 0; a < 3; a++) {
                sums[3 * ti + a] = S[a];
                cents[3 * ti + a] = e.count == 1 ? own[a] : mean(S[a], e.count);
            }
        }
    }
    for (size_t ti = 0; ti < table.size(); ti++) {                    // the fold kernel
        const InstBoundsEntry e = table[ti];
        const uint32_t nc = ib_chunks(e.count);
        if (nc > 1)
            for (int a = 0; a < 3; a++) {
                sums[3 * ti + a] = ib_strided_sum(nc, [&](uint64_t j) { return partials[3 * ((size_t)e.first_chunk + j) + a]; });
                cents[3 * ti + a] = mean(sums[3 * ti + a], e.count);
            }
        for (uint32_t j = 0; j < nc; j++) items_bad += partial_writes[e.first_chunk + j] != (nc > 1 ? 1 : 0);
        for (uint32_t k = 0; k < e.count; k++) cover_bad += seen[ti][k] != 1;
        for (int a = 0; a < 3; a++) {
            const double want = ib_instance_sum(e.count, [&](uint64_t k) { return ib_tri_centroid(verts[ti].data() + 9 * k, a); });
            shape_bad += std::memcmp(&want, &sums[3 * ti + a], 8) != 0;
        }
    }

    std::printf("{\"covered_once\": %d, \"transpose_bad\": %" PRIu64 ", \"asker_bad\": %" PRIu64 ", \"items_bad\": %" PRIu64
                ", \"shape_bad\": %" PRIu64 ", \"sums\": [", cover_bad == 0 ? 1 : 0, transpose_bad, asker_bad, items_bad, shape_bad);
    for (size_t k = 0; k < sums.size(); k++) {
        uint64_t b;
        std::memcpy(&b, &sums[k], 8);
        std::printf("%s\"%016" PRIx64 "\"", k ? ", " : "", b);
    }
    std::printf("], \"centroids\": [");
    for (size_t k = 0; k < cents.size(); k++) {
        uint32_t b;
        std::memcpy(&b, &cents[k], 4);
        std::printf("%s\"%08x\"", k ? ", " : "", b);
    }
    std::printf("]}\n");
    return 0;
}
