// lbvh_items.hpp — what the GPU BVH builder knows about one item (device side; lbvh.hip maps the headers): the
// reference's primitive boxes and centroids, and the leaf-ordered hot / cold records of a BLAS gather.  Vectors and
// their algebra are host_math.hpp's (the same functions the host builders evaluate); under -ffp-contract=off a
// GPU-built leaf holds the bytes a host build would.  Also the constants every lbvh_*.hpp shares.
#pragma once
#include "host_math.hpp"
#include "lbvh.hpp"

namespace rtamd::lbvh {

constexpr int BLOCK = 256;
constexpr uint32_t LEAF_BIT = 1u << 31;
constexpr uint32_t NONE = 0xFFFFFFFFu;
using hm::FZERO;                                    // Global.cuh:147

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + BLOCK - 1) / BLOCK); }

// ---- reference box / primitive arithmetic: host_math.hpp's vectors (Vec3.cuh:113-137), the boxes as six floats ----
using hm::V3, hm::v3, hm::of, hm::dot, hm::cross, hm::unit;

struct Box { float b[6]; };                                // {xmin,xmax,ymin,ymax,zmin,zmax}
__device__ __forceinline__ float rlength(float mn, float mx) {   // Range.cuh: length()
    return (mn >= mx || fabsf(mn - mx) < FZERO) ? 0.0f : mx - mn;
}
// (hm::Box::from_points(...).store() here changes .text, .rodata and the kernel descriptors: the two stay apart)
__device__ __forceinline__ Box from_points(const V3 p1, const V3 p2) {     // BoundingBox.cuh:24-28, 41-47
    Box r;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float a = p1[i], c = p2[i];
        float mn = a < c ? a : c, mx = a < c ? c : a;
        if (rlength(mn, mx) < FZERO) { mn -= FZERO; mx += FZERO; }
        r.b[2 * i] = mn; r.b[2 * i + 1] = mx;
    }
    return r;
}
__device__ __forceinline__ void merge_into(float *m, const float *a) {   // BoundingBox.cuh:50-55
#pragma unroll
    for (int i = 0; i < 3; i++) {
        m[2 * i] = a[2 * i] < m[2 * i] ? a[2 * i] : m[2 * i];
        m[2 * i + 1] = a[2 * i + 1] > m[2 * i + 1] ? a[2 * i + 1] : m[2 * i + 1];
    }
}

__device__ __forceinline__ void tri_box_centroid(const float *t, Box &bx, V3 &c) {   // Triangle.cu:46-62, .cuh:53-61
    V3 mn, mx;
    float lo[3], hi[3], cc[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float a = t[i], b = t[3 + i], d = t[6 + i];              // vertices 0, 1, 2 (9 floats)
        float l = a, h = a;
        if (b < l) l = b;
        if (d < l) l = d;
        if (h < b) h = b;
        if (h < d) h = d;
        lo[i] = l; hi[i] = h;
        float s = a + b + d;
        s /= 3.0f;
        cc[i] = s;
    }
    mn = v3(lo[0], lo[1], lo[2]); mx = v3(hi[0], hi[1], hi[2]);
    bx = from_points(mn, mx);
    c = v3(cc[0], cc[1], cc[2]);
}
__device__ __forceinline__ void sphere_box_centroid(const rt_sphere &s, Box &bx, V3 &c) {   // Sphere.cu:51-55
    const V3 ce = of(s.center), e = v3(s.radius, s.radius, s.radius);
    bx = from_points(ce - e, ce + e);
    c = ce;
}
__device__ __forceinline__ void quad_box_centroid(const rt_parallelogram &p, Box &bx, V3 &c) {   // Parallelogram.cu:48-50 (q-centred), .cuh:45-47
    const V3 h = (of(p.u) + of(p.v)) * 0.5f;
    bx = from_points(of(p.q) + h, of(p.q) - h);
    c = of(p.q) + of(p.u) * 0.5f + of(p.v) * 0.5f;
}

// a triangle's hot record as gather_item writes it without cold records (caller index and member in the pads);
// gather_item fills the same record itself (built through this function its code changes)
__device__ __forceinline__ TriHot tri_hot_record(const float *tv, uint32_t prim, uint32_t member) {
    const V3 v0 = v3(tv[0], tv[1], tv[2]);
    const V3 e1 = v3(tv[3], tv[4], tv[5]) - v0, e2 = v3(tv[6], tv[7], tv[8]) - v0;
    TriHot H;
    H.v0[0] = v0.x; H.v0[1] = v0.y; H.v0[2] = v0.z; H.pad0 = __uint_as_float(prim);
    H.e1[0] = e1.x; H.e1[1] = e1.y; H.e1[2] = e1.z; H.pad1 = __uint_as_float(member);
    H.e2[0] = e2.x; H.e2[1] = e2.y; H.e2[2] = e2.z; H.pad2 = 0.0f;
    return H;
}

// Leaf-ordered BLAS records (rt_api.cpp builds the same records on the host: Triangle.cuh:26-46,
// Parallelogram.cuh:26-39).
__device__ __forceinline__ uint32_t material_slot(uint32_t type, uint32_t index, uint32_t rough_count) {
    return type == RT_MAT_ROUGH ? index : ((rough_count + index) | MAT_METAL_BIT);
}

__device__ __forceinline__ void gather_item(const LbvhSeg &S, uint32_t p, const uint32_t *vals, const RawPrimsGPU &raw,
                                            const PrimOutGPU &out, const uint32_t *item_member, const TriHot *stage) {
    const uint32_t slot = S.slot_base + (p - S.item_base);
    if (stage && S.ptype == RT_PRIM_TRIANGLE && !out.tri_cold) {     // prep staged the record in item order
        out.tri_hot[slot] = stage[vals[p]];
        return;
    }
    const uint32_t prim = S.prim_base + (vals[p] - S.item_base);
    if (S.ptype == RT_PRIM_TRIANGLE) {
        const float *tv = raw.tri_verts + 9 * (size_t)prim;
        const V3 v0 = v3(tv[0], tv[1], tv[2]);
        const V3 e1 = v3(tv[3], tv[4], tv[5]) - v0, e2 = v3(tv[6], tv[7], tv[8]) - v0;
        const uint32_t member = S.member_count ? item_member[vals[p]] : 0u;   // a group's BLAS: member instance + 1
        TriHot H;                                     // tri_hot_record's, with the pads clear for the cold path
        H.v0[0] = v0.x; H.v0[1] = v0.y; H.v0[2] = v0.z; H.pad0 = 0.0f;
        H.e1[0] = e1.x; H.e1[1] = e1.y; H.e1[2] = e1.z; H.pad1 = 0.0f;
        H.e2[0] = e2.x; H.e2[1] = e2.y; H.e2[2] = e2.z; H.pad2 = 0.0f;
        if (!out.tri_cold) {                          // no cold records: the index and member ride in the pads
            H.pad0 = __uint_as_float(prim);
            H.pad1 = __uint_as_float(member);
            out.tri_hot[slot] = H;
            return;
        }
        const rt_triangle &t = raw.tris[prim];
        V3 nn[3];
        if (t.has_normals) { nn[0] = of(t.normal[0]); nn[1] = of(t.normal[1]); nn[2] = of(t.normal[2]); }
        else { const V3 u = unit(cross(e1, e2)); nn[0] = u; nn[1] = u; nn[2] = u; }
        TriCold C;
        C.n0[0] = nn[0].x; C.n0[1] = nn[0].y; C.n0[2] = nn[0].z;
        C.n1[0] = nn[1].x; C.n1[1] = nn[1].y; C.n1[2] = nn[1].z;
        C.n2[0] = nn[2].x; C.n2[1] = nn[2].y; C.n2[2] = nn[2].z;
        C.material = material_slot(t.material_type, t.material_index, raw.rough_count);
        C.orig_index = prim;
        C.pad = member;
        out.tri_hot[slot] = H;
        out.tri_cold[slot] = C;
    } else if (S.ptype == RT_PRIM_SPHERE) {
        const rt_sphere sp = raw.spheres[prim];
        SphereHot H;
        H.center[0] = sp.center.x; H.center[1] = sp.center.y; H.center[2] = sp.center.z; H.radius = sp.radius;
        PrimCold C;
        C.material = material_slot(sp.material_type, sp.material_index, raw.rough_count);
        C.orig_index = prim; C.pad0 = 0; C.pad1 = 0;
        out.sph_hot[slot] = H;
        out.sph_cold[slot] = C;
    } else {
        const rt_parallelogram q = raw.quads[prim];
        const V3 nx = cross(of(q.u), of(q.v));
        const V3 nn = unit(nx);
        float d = 0.0f;
        d += nn.x * q.q.x; d += nn.y * q.q.y; d += nn.z * q.q.z;
        QuadHot H;
        H.n[0] = nn.x; H.n[1] = nn.y; H.n[2] = nn.z; H.d = d;
        H.q[0] = q.q.x; H.q[1] = q.q.y; H.q[2] = q.q.z; H.den = dot(nx, nx);
        H.u[0] = q.u.x; H.u[1] = q.u.y; H.u[2] = q.u.z; H.pad0 = 0.0f;
        H.v[0] = q.v.x; H.v[1] = q.v.y; H.v[2] = q.v.z; H.pad1 = 0.0f;
        H.nx[0] = nx.x; H.nx[1] = nx.y; H.nx[2] = nx.z; H.pad2 = 0.0f;
        PrimCold C;
        C.material = material_slot(q.material_type, q.material_index, raw.rough_count);
        C.orig_index = prim; C.pad0 = 0; C.pad1 = 0;
        out.quad_hot[slot] = H;
        out.quad_cold[slot] = C;
    }
}

}  // namespace rtamd::lbvh
