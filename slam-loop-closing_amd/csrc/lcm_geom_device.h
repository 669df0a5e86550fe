// lcm_geom_device.h — the records and the arithmetic that the geometry stages share (the pose-graph correction, the bundle
// adjustment, the map building, the local optimisation's eigenvector), stated once:
//   Pose / Point3 / Observation / Camera   lcm_pgo_pose, lcm_ba_point, lcm_ba_obs and the four intrinsics as the device sees them
//   tri_index / sym_index<N>   a packed lower triangle's (r, c), c <= r; a packed upper triangle's (i, j), either order
//   mat3_mul / mat3_mul_tn / mat3_mul_nt / mat3_apply   the 3 x 3 products, every entry a0 b0 + a1 b1 + a2 b2 from the left
//   so3_exp            rotation vector -> rotation matrix (Rodrigues' formula)
//   so3_log            rotation matrix -> rotation vector, first order below s = 1e-5; false at half a turn
//   rigid_apply        Xc = (R X) + t, each row of the product summed left to right (src/main.cpp:155)
//   pinhole_project    u = ((fx x) / z) + cx, v = ((fy y) / z) + cy; no test on z (:157-162)
//   chol<N> / lower_solve<N> / upper_solve<N>   the N x N Cholesky factor (lower triangle, packed) and its two solves
//   solve_damped<N>    H + damping I, its Cholesky and dp = H^-1 (-g); false: a pivot is not > 0
//   jacobi_angle       the gate and the angle of one Jacobi rotation
// In double, every product and sum rounded on its own, sums left to right.  The fp contract pragma is lexical, an inlined callee
// does not take it from its caller: every function states its own.  Everything is __host__ __device__: the host compiles the same
// text (tests/cpp/geom_host_check.cpp runs it under a sanitizer).  Included by lcm_pgo_device.h, lcm_ba_device.h,
// lcm_map_device.h and lcm_lo_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace lcm {

constexpr double SO3_EPSILON = 2.220446049250313e-16;     // DBL_EPSILON: below it a rotation vector is the identity
constexpr double SO3_LOG_SMALL = 1e-5;                    // below this sine the logarithm is its first-order term

// The device's records = lcm_pgo_pose (world-to-camera where a camera's), lcm_ba_point, lcm_ba_obs (include/lcm.h; lcm_pgo.cpp
// and lcm_ba.cpp assert the layouts)
struct Pose { double R[9]; double t[3]; };
struct Point3 { double x, y, z; };
struct Observation { int32_t cam, point; double u, v; };
struct Camera { double fx, fy, cx, cy; };

// index of (r, c), c <= r, in a packed lower triangle
__host__ __device__ constexpr int tri_index(int r, int c) { return r * (r + 1) / 2 + c; }

// position of element (i, j) of the symmetric N x N matrix in the packed upper triangle, row-major
template <int N>
__host__ __device__ constexpr int sym_index(int i, int j) {
    return (i < j ? i : j) * N - (i < j ? i : j) * ((i < j ? i : j) - 1) / 2 + ((i < j ? j : i) - (i < j ? i : j));
}

// C = A B
__host__ __device__ __forceinline__ void mat3_mul(const double (&a)[9], const double (&b)[9], double (&c)[9]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// C = A^T B
__host__ __device__ __forceinline__ void mat3_mul_tn(const double (&a)[9], const double (&b)[9], double (&c)[9]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[i] * b[j] + a[3 + i] * b[3 + j] + a[6 + i] * b[6 + j];
}

// C = A B^T
__host__ __device__ __forceinline__ void mat3_mul_nt(const double (&a)[9], const double (&b)[9], double (&c)[9]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1] + a[3 * i + 2] * b[3 * j + 2];
}

// y = A x
__host__ __device__ __forceinline__ void mat3_apply(const double (&a)[9], const double (&x)[3], double (&y)[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = a[3 * i] * x[0] + a[3 * i + 1] * x[1] + a[3 * i + 2] * x[2];
}

// exp: theta = sqrt(r . r); below DBL_EPSILON the identity; else k = r / theta and
// R = cos(theta) I + (1 - cos(theta)) k k^T + sin(theta) [k]x, entry by entry in this order
__host__ __device__ __forceinline__ void so3_exp(const double (&r)[3], double (&R)[9]) {
#pragma clang fp contract(off)
    const double theta = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (theta < SO3_EPSILON) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    const double c = cos(theta), s = sin(theta), c1 = 1.0 - c;
    const double kx = r[0] / theta, ky = r[1] / theta, kz = r[2] / theta;
    R[0] = c + (c1 * kx) * kx;
    R[1] = (c1 * kx) * ky - s * kz;
    R[2] = (c1 * kx) * kz + s * ky;
    R[3] = (c1 * ky) * kx + s * kz;
    R[4] = c + (c1 * ky) * ky;
    R[5] = (c1 * ky) * kz - s * kx;
    R[6] = (c1 * kz) * kx - s * ky;
    R[7] = (c1 * kz) * ky + s * kx;
    R[8] = c + (c1 * kz) * kz;
}

// log: v = (R21 - R12, R02 - R20, R10 - R01) / 2, s = |v|, c = (trace - 1) / 2 clamped to [-1, 1].
//   s >= 1e-5: v atan2(s, c) / s;   s < 1e-5 and c > 0: v itself;   s < 1e-5 and c <= 0: false (half a turn), r = v.
// R is taken as a rotation and is not projected.
__host__ __device__ __forceinline__ bool so3_log(const double (&R)[9], double (&r)[3]) {
#pragma clang fp contract(off)
    const double vx = 0.5 * (R[7] - R[5]), vy = 0.5 * (R[2] - R[6]), vz = 0.5 * (R[3] - R[1]);
    const double s = sqrt(vx * vx + vy * vy + vz * vz);
    double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    if (s >= SO3_LOG_SMALL) {
        const double f = atan2(s, c) / s;
        r[0] = vx * f; r[1] = vy * f; r[2] = vz * f;
        return true;
    }
    r[0] = vx; r[1] = vy; r[2] = vz;
    return c > 0.0;
}

// Xc = (R X) + t, each row of the product summed left to right
__host__ __device__ __forceinline__ void rigid_apply(const double (&R)[9], const double (&t)[3], const double (&X)[3], double (&Xc)[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i) Xc[i] = (R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2]) + t[i];
}

// The pixel of a point in camera coordinates; z is not looked at
__host__ __device__ __forceinline__ void pinhole_project(const Camera& K, const double (&Xc)[3], double& u, double& v) {
#pragma clang fp contract(off)
    u = ((K.fx * Xc[0]) / Xc[2]) + K.cx;
    v = ((K.fy * Xc[1]) / Xc[2]) + K.cy;
}

// In-place Cholesky of a symmetric N x N matrix given as its packed lower triangle: a = L L^T, row by row, every entry
// a[r][c] - sum_{k < c} l[r][k] l[c][k] from the left.  false: a pivot is not > 0 (NaN included); the factor is then unusable.
template <int N>
__host__ __device__ __forceinline__ bool chol(double (&a)[N * (N + 1) / 2]) {
#pragma clang fp contract(off)
    bool ok = true;
#pragma unroll
    for (int r = 0; r < N; ++r) {
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            double s = a[tri_index(r, c)];
#pragma unroll
            for (int k = 0; k < c; ++k) s = s - a[tri_index(r, k)] * a[tri_index(c, k)];
            if (c == r) {
                ok = ok && (s > 0.0);
                a[tri_index(r, r)] = sqrt(s);
            } else {
                a[tri_index(r, c)] = s / a[tri_index(c, c)];
            }
        }
    }
    return ok;
}

// x <- L^-1 x
template <int N>
__host__ __device__ __forceinline__ void lower_solve(const double (&l)[N * (N + 1) / 2], double (&x)[N]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < N; ++r) {
        double s = x[r];
#pragma unroll
        for (int k = 0; k < r; ++k) s = s - l[tri_index(r, k)] * x[k];
        x[r] = s / l[tri_index(r, r)];
    }
}

// x <- L^-T x
template <int N>
__host__ __device__ __forceinline__ void upper_solve(const double (&l)[N * (N + 1) / 2], double (&x)[N]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = N - 1; r >= 0; --r) {
        double s = x[r];
#pragma unroll
        for (int k = N - 1; k > r; --k) s = s - l[tri_index(k, r)] * x[k];
        x[r] = s / l[tri_index(r, r)];
    }
}

// (H + damping I) dp = -g, H the packed lower triangle before damping; false: a pivot is not > 0 and dp is not to be used
template <int N>
__host__ __device__ __forceinline__ bool solve_damped(const double (&H)[N * (N + 1) / 2], const double (&g)[N], double damping, double (&dp)[N]) {
#pragma clang fp contract(off)
    double L[N * (N + 1) / 2];
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) L[tri_index(r, c)] = (r == c) ? H[tri_index(r, c)] + damping : H[tri_index(r, c)];
    const bool ok = chol<N>(L);
#pragma unroll
    for (int k = 0; k < N; ++k) dp[k] = -g[k];
    lower_solve<N>(L, dp);
    upper_solve<N>(L, dp);
    return ok;
}

// One Jacobi rotation of a symmetric matrix on the pair (p, q), from its entries (p, p), (q, q) and (p, q).  false: the rotation
// is skipped, the off-diagonal entry being zero or below 1e-18 of the geometric mean of the two diagonal entries; t, cs and sn
// are then zero.  Else t = tan, cs = cos and sn = sin of the angle that annihilates (p, q).
// lcm_epi_device.h's rotation stays its own: it is compiled with contraction and its gate has no fabs, so sharing would change its bits.
__host__ __device__ __forceinline__ bool jacobi_angle(double app, double aqq, double apq, double& t, double& cs, double& sn) {
#pragma clang fp contract(off)
    t = cs = sn = 0.0;
    if (!(apq != 0.0 && apq * apq > 1e-36 * fabs(app * aqq))) return false;
    const double zeta = (aqq - app) / (2.0 * apq);
    t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    cs = 1.0 / sqrt(1.0 + t * t);
    sn = cs * t;
    return true;
}

}  // namespace lcm
