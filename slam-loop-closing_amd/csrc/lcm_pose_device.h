// lcm_pose_device.h — the arithmetic of the relative-pose recovery (lcm_pose.hip), stated once for the kernel, the host and
// the tests (tests/poseref.py restates it in numpy; include/lcm.h and DESIGN §9i describe the model):
//   pose_decompose   E -> the two rotations Ra, Rb and the unit translation t of E = [t]x R, in closed form: +, -, x, / and
//                    two square roots, no SVD
//   pose_in_front    the depth test of one record under one (R, t): the least-squares depths of the two rays, compared
//                    without a division
//   pose_candidate   hypothesis k of 0 .. 3: R = (k & 1) ? Rb : Ra, t = (k & 2) ? -t : t
// In double, every product and sum rounded on its own (fp contract off), sums left to right.  Everything is
// __host__ __device__: the host compiles the same text (a stand-alone program runs it under a sanitizer).
// Included by lcm_pose.hip and lcm_pose.cpp only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcm_epi_device.h"      // epi_norm: the normalisation is the RANSAC's

namespace lcm {

constexpr double POSE_FINITE_MAX = 1.7976931348623157e308;      // DBL_MAX: `x <= this` is false for Inf and NaN

// The device's result record = lcm_pose_result (include/lcm.h; lcm_pose.cpp asserts the layout)
struct PoseResult { double R[9]; double t[3]; int32_t counts[4]; int32_t n_used, n_good, choice, status; };

// a x b
__host__ __device__ __forceinline__ void pose_cross(double a0, double a1, double a2, double b0, double b1, double b2,
                                                    double& x, double& y, double& z) {
#pragma clang fp contract(off)
    x = a1 * b2 - a2 * b1;
    y = a2 * b0 - a0 * b2;
    z = a0 * b1 - a1 * b0;
}

// E (row-major, any scale, either sign) -> Ra, Rb (row-major), t (unit).  With e = E x sqrt(2 / |E|^2_F):
//   t  = the cross product of two columns of e with the largest squared norm (c0 = col1 x col2, c1 = col2 x col0,
//        c2 = col0 x col1; first of equals) over its norm: the columns of [t]x R are all orthogonal to t
//   C  = the cofactor matrix of e (row 0 = row1 x row2, row 1 = row2 x row0, row 2 = row0 x row1) = t t^T R
//   M  = [t]x e (column j = t x column j)                                                          = (t t^T - I) R
//   Ra = C - M, Rb = C + M: one is R, the other R turned by 180 degrees about the baseline
// false (everything zeroed): no model.  |E|^2_F is zero, NaN or beyond the range in which the scale is finite, or e has no
// two independent columns.
__host__ __device__ __forceinline__ bool pose_decompose(const double (&E)[9], double (&ra)[9], double (&rb)[9], double (&t)[3]) {
#pragma clang fp contract(off)
    double n2 = E[0] * E[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) n2 = n2 + E[k] * E[k];
    const double s = sqrt(2.0 / n2);
    double e[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = E[k] * s;
    double c0[3], c1[3], c2[3];
    pose_cross(e[1], e[4], e[7], e[2], e[5], e[8], c0[0], c0[1], c0[2]);
    pose_cross(e[2], e[5], e[8], e[0], e[3], e[6], c1[0], c1[1], c1[2]);
    pose_cross(e[0], e[3], e[6], e[1], e[4], e[7], c2[0], c2[1], c2[2]);
    const double m0 = c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2];
    const double m1 = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2];
    const double m2 = c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2];
    const bool take1 = m1 > m0;
    const double m01 = take1 ? m1 : m0;
    const bool take2 = m2 > m01;
    const double m = take2 ? m2 : m01;
    const double len = sqrt(m);
    const bool ok = n2 > 0.0 && s <= POSE_FINITE_MAX && m > 0.0 && m <= POSE_FINITE_MAX;
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = (take2 ? c2[i] : (take1 ? c1[i] : c0[i])) / len;
    double cof[9];
    pose_cross(e[3], e[4], e[5], e[6], e[7], e[8], cof[0], cof[1], cof[2]);
    pose_cross(e[6], e[7], e[8], e[0], e[1], e[2], cof[3], cof[4], cof[5]);
    pose_cross(e[0], e[1], e[2], e[3], e[4], e[5], cof[6], cof[7], cof[8]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double x, y, z;
        pose_cross(t[0], t[1], t[2], e[j], e[3 + j], e[6 + j], x, y, z);
        ra[j] = cof[j] - x;         rb[j] = cof[j] + x;
        ra[3 + j] = cof[3 + j] - y; rb[3 + j] = cof[3 + j] + y;
        ra[6 + j] = cof[6 + j] - z; rb[6 + j] = cof[6 + j] + z;
    }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 9; ++k) { ra[k] = 0.0; rb[k] = 0.0; }
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = 0.0;
    }
    return ok;
}

// Hypothesis k of the four
__host__ __device__ __forceinline__ void pose_candidate(int k, const double (&ra)[9], const double (&rb)[9], const double (&t)[3],
                                                        double (&r)[9], double (&tk)[3]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) r[i] = (k & 1) ? rb[i] : ra[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tk[i] = (k & 2) ? -t[i] : t[i];
}

// The depth test (include/lcm.h): query x1 = (a, b, 1), train x2 = (c, d, 1), X2 = R X1 + t.  u = R x1, v = x2; n1 / D and
// n2 / D are the least-squares depths of the two rays l2 v = l1 u + t.  In front of both cameras and nearer than max_depth
// baselines; identical rays (D == 0) are not.
__host__ __device__ __forceinline__ bool pose_in_front(const double (&r)[9], double t0, double t1, double t2, double a, double b,
                                                       double c, double d, double max_depth) {
#pragma clang fp contract(off)
    const double u0 = r[0] * a + r[1] * b + r[2];
    const double u1 = r[3] * a + r[4] * b + r[5];
    const double u2 = r[6] * a + r[7] * b + r[8];
    const double uu = u0 * u0 + u1 * u1 + u2 * u2;
    const double vv = c * c + d * d + 1.0;
    const double uv = u0 * c + u1 * d + u2;
    const double ut = u0 * t0 + u1 * t1 + u2 * t2;
    const double vt = c * t0 + d * t1 + t2;
    const double D = uu * vv - uv * uv;
    const double n1 = uv * vt - vv * ut;
    const double n2 = uu * vt - uv * ut;
    const double far = max_depth * D;
    return D > 0.0 && n1 > 0.0 && n2 > 0.0 && n1 < far && n2 < far;
}

// Selection: the largest of the four counts, among equals the lowest k
__host__ __device__ __forceinline__ int pose_choose(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    int k = 0;
    uint32_t best = c0;
    if (c1 > best) { best = c1; k = 1; }
    if (c2 > best) { best = c2; k = 2; }
    if (c3 > best) { k = 3; }
    return k;
}

}  // namespace lcm
