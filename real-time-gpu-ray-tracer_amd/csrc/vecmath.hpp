// vecmath.hpp — the trace kernels' vector math, division / 1/sqrt flavours, pinned RNG and instance transforms.
// Includable only from trace_kernel.hip, once, inside namespace rtamd::RT_SUFFIX(dev) (it uses the flavour macros and
// FZERO defined there).

struct f3 { float x, y, z; };
__device__ __forceinline__ f3 mk(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ f3 ld3(const float *p) { return mk(p[0], p[1], p[2]); }
__device__ __forceinline__ f3 add(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 sub(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 scl(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ f3 neg(f3 a) { return mk(-a.x, -a.y, -a.z); }
__device__ __forceinline__ f3 mul(f3 a, f3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ float dot(f3 a, f3 b) {          // Vec3.cuh:113-119
    float s = 0.0f; s += a.x * b.x; s += a.y * b.y; s += a.z * b.z; return s;
}
__device__ __forceinline__ f3 cross(f3 a, f3 b) {           // Vec3.cuh:120-126
    return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
// "fast_math" (RT_FAST_IEEE 0) replaces IEEE division / 1/sqrt by the hardware v_rcp_f32 / v_rsq_f32 (1 ulp);
// EXACT and the default FAST build keep the reference's correctly rounded operations (the box tests' reciprocals
// are the FAST kernels' own: prep / slab4, a cull only).
#define RT_IEEE_PRIM (RT_EXACT || RT_FAST_IEEE)
__device__ __forceinline__ float rcp(float x) {              // slab reciprocals (FAST)
#if RT_EXACT
    return 1.0f / x;
#else
    return __builtin_amdgcn_rcpf(x);
#endif
}
__device__ __forceinline__ float fdiv(float a, float b) {
#if RT_IEEE_PRIM
    return a / b;
#else
    return a * __builtin_amdgcn_rcpf(b);
#endif
}
__device__ __forceinline__ f3 unit(f3 a) {                   // Vec3.cuh:129-137
#if RT_IEEE_PRIM
    const float f = 1.0f / sqrtf(dot(a, a));
#else
    const float f = __builtin_amdgcn_rsqf(dot(a, a));
#endif
    return mk(a.x * f, a.y * f, a.z * f);
}
__device__ __forceinline__ float comp(f3 a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }
// unit(e1 x e2) with the arithmetic the BLAS builders store a triangle's normals with (lbvh_items.hpp gather_item,
// host_math.hpp; Triangle.cuh:26-46): correctly rounded 1 / sqrt, no contraction, in every FAST variant
__device__ __forceinline__ f3 tri_face_normal(f3 a, f3 b) {
#pragma clang fp contract(off)
    const f3 c = mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
    float d = 0.0f;
    d += c.x * c.x; d += c.y * c.y; d += c.z * c.z;
    const float f = 1.0f / sqrtf(d);
    return mk(c.x * f, c.y * f, c.z * f);
}

__device__ __forceinline__ bool f_eq(float a, float b) { return fabsf(a - b) < FZERO; }
__device__ __forceinline__ bool in_range(float v, float mn, float mx) {      // Range.cuh:33-43
    return f_eq(v, mn) || f_eq(v, mx) || (v > mn && v < mx);
}

// ---- pinned RNG contract (replaces curand XORWOW, Kernel.cu:114) ----------
constexpr uint64_t GOLDEN64 = 0x9E3779B97F4A7C15ull;
constexpr uint64_t SUBMUL64 = 0xD1B54A32D192ED03ull;
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
struct Rng {
    uint64_t s;
    __device__ __forceinline__ void init(uint64_t seed, uint64_t sub) { s = mix64((seed * GOLDEN64) ^ ((sub + 1ull) * SUBMUL64)); }
    __device__ __forceinline__ float uniform() {                             // (0, 1]
        s += GOLDEN64;
        const uint64_t x = mix64(s);
        return (float)((uint32_t)(x >> 40) + 1u) * 0x1p-24f;
    }
    __device__ __forceinline__ float range(float mn, float mx) { return mn + (mx - mn) * uniform(); }   // Global.cuh:209-211
};
__device__ __forceinline__ f3 random_space_vector(Rng &r) {   // Vec3.cu:54-65 (length 1)
    f3 v; float l2;
    do {
        v.x = r.range(-1.0f, 1.0f);
        v.y = r.range(-1.0f, 1.0f);
        v.z = r.range(-1.0f, 1.0f);
        l2 = dot(v, v);
    } while (l2 < FZERO * FZERO);
    return scl(unit(v), 1.0f);
}
__device__ __forceinline__ f3 random_plane_vector(Rng &r, float maxlen) {   // Vec3.cu:29-36
    float x, y;
    do {
        x = r.range(-1.0f, 1.0f);
        y = r.range(-1.0f, 1.0f);
    } while (x * x + y * y > maxlen * maxlen);
    return mk(x, y, 0.0f);
}

// (M * toMatrix(Point3)).toPoint() / (M * toMatrix(Vec3)).toVector() over rows 1..3 of a 4x4
// (Matrix.cu:71-86); m = 12 floats (3 rows x 4 cols).
__device__ __forceinline__ f3 xf_point(const float *m, f3 p) {
    f3 r;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        float s = 0.0f;
        s += m[4 * i] * p.x; s += m[4 * i + 1] * p.y; s += m[4 * i + 2] * p.z; s += m[4 * i + 3] * 1.0f;
        if (i == 0) r.x = s; else if (i == 1) r.y = s; else r.z = s;
    }
    return r;
}
__device__ __forceinline__ f3 xf_vector(const float *m, f3 v) {
    f3 r;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        float s = 0.0f;
        s += m[4 * i] * v.x; s += m[4 * i + 1] * v.y; s += m[4 * i + 2] * v.z;
#if RT_EXACT
        s += m[4 * i + 3] * 0.0f;     // keeps the sign-of-zero behaviour of the 4x4 product
#endif
        if (i == 0) r.x = s; else if (i == 1) r.y = s; else r.z = s;
    }
    return r;
}
