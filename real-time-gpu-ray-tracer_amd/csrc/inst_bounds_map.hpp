// inst_bounds_map.hpp — RT_TRI_UPDATE_BOUNDS: the shape of the centroid reduction (inst_bounds.hip), shared with the
// host replay that checks it (tests/cpp/inst_bounds_map_check.cpp; tests/inst_bounds_ref.py restates it in numpy), so
// the header is plain C++ without HIP types.
//
// An instance's local centroid is (float)(S / count), S the double-precision sum of its `count` triangle centroids
// (build.cpp bounds_from_prims, update.cpp host_bounds).  The device forms S in a fixed shape that depends on `count` alone:
//   chunk   the instance's triangles are cut into chunks of IB_CHUNK; chunk c holds triangles [c IB_CHUNK, ...).  One
//           workgroup of IB_WAVES waves of IB_WAVE lanes sums a chunk in IB_ROUNDS rounds: in round r, lane l of wave w
//           holds triangle ib_tri(c, r, w, l) (a triangle past `count` counts as +0.0).
//   lane    each lane adds its rounds' centroids, widened to double, to +0.0 in round order.
//   wave    ib_wave_sum: for off = 32, 16, 8, 4, 2, 1 lane l < off becomes v[l] + v[l + off]; lane 0 holds the sum.
//   block   ((w0 + w1) + w2) + w3 over the waves' sums.
//   fold    an instance of more than one chunk: thread t of one workgroup adds the chunk sums t, t + IB_BLOCK, ... to
//           +0.0 in that order, then wave and block as above (ib_strided_sum).  A group's centroid is the same
//           strided sum over its members' centroids, in member order.
// Every step adds to an accumulator that starts at +0.0, as the host's does, so S is never -0.0.  count == 1 keeps
// the triangle's own float centroid (a -0.0 included), as rt_scene_update_triangles does.
//
// Reading a wave's 64 triangles (576 consecutive floats of raw_verts) takes 9 loads of 64 consecutive dwords: load k,
// lane l holds float 64 k + l.  Component j (0..8) of lane t's triangle is float 9 t + j: register (9 t + j) >> 6 of
// lane (9 t + j) & 63.  9 is a unit modulo 64 (9 x 57 = 513), so for a fixed j every source lane is asked by exactly
// one lane, ib_asker(s, j), and can pick the register that lane needs before one cross-lane read moves it.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IB_HD __host__ __device__
#else
#define IB_HD
#endif

namespace rtamd {

constexpr uint32_t IB_WAVE = 64;                            // gfx950 wave width
constexpr uint32_t IB_WAVES = 4;
constexpr uint32_t IB_BLOCK = IB_WAVE * IB_WAVES;           // 256 threads
constexpr uint32_t IB_ROUNDS = 4;
constexpr uint32_t IB_CHUNK = IB_BLOCK * IB_ROUNDS;         // 1 024 triangles per (instance, chunk) work item
constexpr uint32_t IB_LOADS = 9;                            // dword loads per wave and round: 9 x 64 floats

// one triangle instance of the static table (rt_scene_build): its triangles, its first chunk among all work items,
// its record (instance index)
struct InstBoundsEntry { uint32_t pindex, count, first_chunk, record; };

IB_HD inline uint32_t ib_chunks(uint32_t count) { return (count + IB_CHUNK - 1) / IB_CHUNK; }

// triangle (relative to the instance's first) of lane l, wave w, round r of chunk c
IB_HD inline uint64_t ib_tri(uint32_t c, uint32_t r, uint32_t w, uint32_t l) {
    return (uint64_t)c * IB_CHUNK + (uint64_t)(r * IB_WAVES + w) * IB_WAVE + l;
}

// the wave's 9 x 64 loaded floats -> per-lane triangles: where lane t finds component j ...
IB_HD inline uint32_t ib_src_lane(uint32_t t, uint32_t j) { return (9u * t + j) & 63u; }
IB_HD inline uint32_t ib_src_reg(uint32_t t, uint32_t j) { return (9u * t + j) >> 6; }
// ... and the one lane that asks source lane s for component j
IB_HD inline uint32_t ib_asker(uint32_t s, uint32_t j) { return ((s - j) * 57u) & 63u; }

// tri_centroid's float operations (host_math.hpp) on the 9 floats of a triangle, component a
IB_HD inline float ib_tri_centroid(const float *v, int a) {
    float r = v[a] + v[3 + a] + v[6 + a];
    r /= 3.0f;
    return r;
}

// the wave step on host arrays of IB_WAVE doubles (the device uses cross-lane reads of the same shape)
inline double ib_wave_sum(double *v) {
    for (uint32_t off = IB_WAVE / 2; off; off >>= 1)
        for (uint32_t l = 0; l < off; l++) v[l] = v[l] + v[l + off];
    return v[0];
}

inline double ib_block_sum(const double *lane /* IB_BLOCK */) {
    double w[IB_WAVES];
    for (uint32_t k = 0; k < IB_WAVES; k++) {
        double v[IB_WAVE];
        for (uint32_t l = 0; l < IB_WAVE; l++) v[l] = lane[k * IB_WAVE + l];
        w[k] = ib_wave_sum(v);
    }
    return ((w[0] + w[1]) + w[2]) + w[3];
}

// fold / group step: n values, thread t takes t, t + IB_BLOCK, ...
template <typename Get>
inline double ib_strided_sum(uint64_t n, Get get) {
    double lane[IB_BLOCK];
    for (uint32_t t = 0; t < IB_BLOCK; t++) {
        double acc = 0.0;
        for (uint64_t j = t; j < n; j += IB_BLOCK) acc += get(j);
        lane[t] = acc;
    }
    return ib_block_sum(lane);
}

// S of one axis for an instance of `count` triangles whose centroids' axis component is cent(k), in the device's shape
template <typename Cent>
inline double ib_instance_sum(uint32_t count, Cent cent) {
    const uint32_t nc = ib_chunks(count);
    auto chunk_sum = [&](uint32_t c) {
        double lane[IB_BLOCK];
        for (uint32_t w = 0; w < IB_WAVES; w++)
            for (uint32_t l = 0; l < IB_WAVE; l++) {
                double acc = 0.0;
                for (uint32_t r = 0; r < IB_ROUNDS; r++) {
                    const uint64_t k = ib_tri(c, r, w, l);
                    acc += k < count ? (double)cent(k) : 0.0;
                }
                lane[w * IB_WAVE + l] = acc;
            }
        return ib_block_sum(lane);
    };
    if (nc == 1) return chunk_sum(0);
    return ib_strided_sum(nc, [&](uint64_t c) { return chunk_sum((uint32_t)c); });
}

}  // namespace rtamd
