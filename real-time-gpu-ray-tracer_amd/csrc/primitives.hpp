// primitives.hpp — the three primitive tests (instance-local space), restating Triangle / Sphere / Parallelogram::hit.
// Includable only from trace_kernel.hip, once, inside namespace rtamd::RT_SUFFIX(dev), after vecmath.hpp and box.hpp
// (RayP).

__device__ __forceinline__ bool tri_test(const TriHot &T, const RayP &r, float tmin, float tmax,
                                         float &t, float &u, float &v) {      // Triangle.cu:4-44
    const f3 e1 = ld3(T.e1), e2 = ld3(T.e2), v0 = ld3(T.v0);
    const f3 h = cross(r.d, e2);
    const float det = dot(e1, h);
    if (fabsf(det) < FZERO) return false;
    const f3 s = sub(r.o, v0);
#if RT_IEEE_PRIM
    u = dot(s, h) / det;
    if (!in_range(u, 0.0f, 1.0f)) return false;
    const f3 q = cross(s, e1);
    v = dot(r.d, q) / det;
    if (!in_range(v, 0.0f, 1.0f) || u + v > 1.0f) return false;
    t = dot(e2, q) / det;
    return in_range(t, tmin, tmax);
#else
    const float inv = __builtin_amdgcn_rcpf(det);
    const f3 q = cross(s, e1);
    u = dot(s, h) * inv;
    v = dot(r.d, q) * inv;
    t = dot(e2, q) * inv;
    return in_range(u, 0.0f, 1.0f) && in_range(v, 0.0f, 1.0f) && !(u + v > 1.0f) && in_range(t, tmin, tmax);
#endif
}

__device__ __forceinline__ bool sphere_test(const SphereHot &S, const RayP &r, float tmin, float tmax, float &t) {
    const f3 c = ld3(S.center);                                               // Sphere.cu:4-28
    const f3 cq = sub(c, r.o);
    const float a = dot(r.d, r.d);
    const float b = -2.0f * dot(cq, r.d);
    const float cc = dot(cq, cq) - S.radius * S.radius;
    float delta = b * b - 4.0f * a * cc;
    if (delta < 0.0f) return false;
    delta = sqrtf(delta);
    // the far root only when the near one is out of range (the same values; one correctly rounded division less
    // for every ray that hits a sphere from outside, e.g. the ground)
    const float root1 = fdiv(-b - delta, a * 2.0f);
    if (in_range(root1, tmin, tmax)) { t = root1; return true; }
    const float root2 = fdiv(-b + delta, a * 2.0f);
    if (in_range(root2, tmin, tmax)) { t = root2; return true; }
    return false;
}

__device__ __forceinline__ bool quad_test(const QuadHot &Q, const RayP &r, float tmin, float tmax,
                                          float &t, float &al, float &be) {   // Parallelogram.cu:4-36
    const f3 n = ld3(Q.n);
    const float ndd = dot(n, r.d);
    if (fabsf(ndd) < FZERO) return false;
    float ndp = 0.0f;
    ndp += n.x * r.o.x; ndp += n.y * r.o.y; ndp += n.z * r.o.z;
    const float tt = fdiv(Q.d - ndp, ndd);
    if (!in_range(tt, tmin, tmax)) return false;
    const f3 inter = add(r.o, scl(r.d, tt));
    const f3 p = sub(inter, ld3(Q.q));
    const f3 nx = ld3(Q.nx);
    if (fabsf(Q.den) < FZERO) return false;
    al = fdiv(dot(cross(p, ld3(Q.v)), nx), Q.den);
    if (!in_range(al, 0.0f, 1.0f)) return false;                              // (the reference tests both after)
    be = fdiv(dot(cross(ld3(Q.u), p), nx), Q.den);
    if (!in_range(be, 0.0f, 1.0f)) return false;
    t = tt;
    return true;
}
