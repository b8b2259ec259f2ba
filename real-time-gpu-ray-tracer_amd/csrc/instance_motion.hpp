// instance_motion.hpp — rt_instance_motion_records (include/rt.h, "Moving instances"): the record that carries a
// current-frame world point and normal of an instance back to the previous frame, from the instance's two rt_xform.
// Host only and plain C++ (host_math.hpp without HIP), so a stand-alone program can include it
// (tests/cpp/instance_motion_check.cpp); tests/motion_ref.py restates motion_record in float64 numpy.  Compile with
// -ffp-contract=off, as everything that includes host_math.hpp: the forward matrices are the library's bits.
//   Fp, Fc   hm::instance_forward(prev), (cur): the float matrices rt_scene_update gives the instance (frame.cpp).
//   in double, every product and sum rounded on its own, L the 3 x 3 linear part and t the translation of F:
//     C(L)[i][j] = L[i+1][j+1] L[i+2][j+2] - L[i+1][j+2] L[i+2][j+1]      (indices modulo 3)
//     det(L)     = (L[0][0] C[0][0] + L[0][1] C[0][1]) + L[0][2] C[0][2];   L^-1[i][j] = C[j][i] / det
//     A = Lp Lc^-1, M = Lc Lp^-1: (X[i][0] Y[0][j] + X[i][1] Y[1][j]) + X[i][2] Y[2][j]
//     b[i] = tp[i] - ((A[i][0] tc[0] + A[i][1] tc[1]) + A[i][2] tc[2]);   Nn = M^T
//   each value rounded to float once.
#pragma once

#include "host_math.hpp"

namespace rtamd {

struct Lin3 { double m[3][3]; };

inline Lin3 linear_part(const hm::Mat &f) {
    Lin3 l;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) l.m[i][j] = (double)f.d[i + 1][j + 1];
    return l;
}

// L^-1 by cofactors; false when det is 0 or not finite (inv is then not written)
inline bool cofactor_inverse(const Lin3 &l, Lin3 &inv) {
    double c[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            c[i][j] = l.m[i1][j1] * l.m[i2][j2] - l.m[i1][j2] * l.m[i2][j1];
        }
    const double det = (l.m[0][0] * c[0][0] + l.m[0][1] * c[0][1]) + l.m[0][2] * c[0][2];
    if (det == 0.0 || !std::isfinite(det)) return false;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) inv.m[i][j] = c[j][i] / det;
    return true;
}

inline Lin3 product(const Lin3 &x, const Lin3 &y) {
    Lin3 r;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r.m[i][j] = (x.m[i][0] * y.m[0][j] + x.m[i][1] * y.m[1][j]) + x.m[i][2] * y.m[2][j];
    return r;
}

// Whether hm::inverse inverts f or leaves by one of its singular exits and returns f itself: the pivot decisions of
// its forward elimination, restated on the 4 x 4 alone (the back substitution tests the same pivots again).
inline bool library_inverts(const hm::Mat &f) {
    float m[5][5];
    for (int i = 1; i < 5; i++)
        for (int j = 1; j < 5; j++) m[i][j] = f.d[i][j];
    for (int i = 1; i < 5; i++) {
        float best = std::fabs(m[i][i]);
        int prow = i;
        for (int p = i + 1; p < 5; p++)
            if (std::fabs(m[p][i]) > best) { best = std::fabs(m[p][i]); prow = p; }
        if (std::fabs(best) < hm::FZERO) return false;
        if (prow != i)
            for (int j = 1; j < 5; j++) { const float t = m[prow][j]; m[prow][j] = m[i][j]; m[i][j] = t; }
        for (int j = i + 1; j < 5; j++) {
            const float g = m[j][i] / m[i][i];
            for (int k = i; k < 5; k++) m[j][k] -= g * m[i][k];
        }
    }
    return true;
}

inline rt_instance_motion motion_record(const rt_xform &prev, const rt_xform &cur) {
    rt_instance_motion r;
    std::memset(&r, 0, sizeof r);
    if (std::memcmp(&prev, &cur, sizeof(rt_xform)) == 0) {
        r.flags = RT_MOTION_STATIC;
        for (int i = 0; i < 3; i++) r.point[4 * i + i] = r.normal[3 * i + i] = 1.0f;
        return r;
    }
    r.flags = RT_MOTION_NO_HISTORY;
    const hm::Mat fp = hm::instance_forward(prev), fc = hm::instance_forward(cur);
    if (!library_inverts(fp) || !library_inverts(fc)) return r;
    const Lin3 lp = linear_part(fp), lc = linear_part(fc);
    Lin3 lpi, lci;
    if (!cofactor_inverse(lp, lpi) || !cofactor_inverse(lc, lci)) return r;
    const Lin3 a = product(lp, lci), m = product(lc, lpi);
    rt_instance_motion out = r;
    bool finite = true;
    for (int i = 0; i < 3; i++) {
        const double tc0 = (double)fc.d[1][4], tc1 = (double)fc.d[2][4], tc2 = (double)fc.d[3][4];
        const double b = (double)fp.d[i + 1][4] - ((a.m[i][0] * tc0 + a.m[i][1] * tc1) + a.m[i][2] * tc2);
        for (int j = 0; j < 3; j++) {
            out.point[4 * i + j] = (float)a.m[i][j];
            out.normal[3 * i + j] = (float)m.m[j][i];
            finite = finite && std::isfinite(out.point[4 * i + j]) && std::isfinite(out.normal[3 * i + j]);
        }
        out.point[4 * i + 3] = (float)b;
        finite = finite && std::isfinite(out.point[4 * i + 3]);
    }
    if (!finite) return r;
    out.flags = RT_MOTION_MOVED;
    return out;
}

}  // namespace rtamd
