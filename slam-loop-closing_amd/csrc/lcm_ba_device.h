// lcm_ba_device.h — the arithmetic of the alternating bundle adjustment (lcm_ba.hip), stated once for the kernels, the host-only
// helpers of lcm_ba_host.h and the tests (tests/baref.py restates it in numpy; include/lcm.h and DESIGN §9q describe the model):
//   ba_camera_point    Xc = (R Xw) + t, each row of the product summed left to right (src/main.cpp:155)
//   ba_residual        (((fx x) / z) + cx) - u, (((fy y) / z) + cy) - v; no test on z (:157-162, :673-674)
//   ba_error           sqrt(dx dx + dy dy) of a residual (:886-888)
//   ba_column          (r_plus - r_minus) (0.5 / eps), one central-difference column of one observation (:712, :828)
//   ba_chol3 / ba_lower_solve3 / ba_upper_solve3   the 3 x 3 Cholesky factor (lower triangle, packed) and its two solves
//   ba_solve6 / ba_solve3   H + damping I, its Cholesky and dp = H^-1 (-g); false: a pivot is not > 0
// The rotation's exp and log, the 3 x 3 products and the 6 x 6 Cholesky are the pose graph's (lcm_pgo_device.h), used and not
// restated.  In double, every product and sum rounded on its own (fp contract off), sums left to right.  Everything is
// __host__ __device__: the host compiles the same text (a stand-alone program runs it under a sanitizer).
// Included by lcm_ba.hip and by lcm_ba_host.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lcm_pgo_device.h"

namespace lcm {

// The device's records = lcm_ba_point, lcm_ba_obs, lcm_ba_elem_info (include/lcm.h; lcm_ba.cpp asserts the layouts); a pose is
// the pose graph's (96 bytes, world-to-camera)
using BaPose = PgoPose;
struct BaPoint { double x, y, z; };
struct BaObs { int32_t cam, point; double u, v; };
struct BaElemInfo { double last_update, cost; int32_t iterations, status; };
struct BaCamera { double fx, fy, cx, cy; };

constexpr int BA_CONVERGED = 0, BA_MAX_ITERS = 1, BA_SOLVE_FAILED = 2, BA_HALF_TURN = 3, BA_SKIPPED = 4;   // lcm_ba_status
constexpr int BA_CAMERA_THREADS = 256;       // k_ba_cameras: one workgroup per camera
constexpr int BA_CAMERA_SUMS = 28;           // the packed lower triangle of H (21), g (6), r . r (1)
constexpr int BA_CAMERA_CHUNK = 32;          // lanes per first-level sum
constexpr int BA_ERROR_THREADS = 256;        // k_ba_error: observations per workgroup = per partial sum

__host__ __device__ __forceinline__ void ba_rotate(const double (&R)[9], const double (&X)[3], double (&Y)[3]) { pgo_apply(R, X, Y); }

__host__ __device__ __forceinline__ void ba_camera_point(const double (&R)[9], const double (&t)[3], const double (&X)[3], double (&Xc)[3]) {
#pragma clang fp contract(off)
    double Y[3];
    ba_rotate(R, X, Y);
#pragma unroll
    for (int k = 0; k < 3; ++k) Xc[k] = Y[k] + t[k];
}

__host__ __device__ __forceinline__ void ba_residual(const BaCamera& K, const double (&Xc)[3], double u, double v, double (&r)[2]) {
#pragma clang fp contract(off)
    r[0] = (((K.fx * Xc[0]) / Xc[2]) + K.cx) - u;
    r[1] = (((K.fy * Xc[1]) / Xc[2]) + K.cy) - v;
}

__host__ __device__ __forceinline__ double ba_error(const double (&r)[2]) {
#pragma clang fp contract(off)
    return sqrt(r[0] * r[0] + r[1] * r[1]);
}

__host__ __device__ __forceinline__ void ba_column(const double (&rp)[2], const double (&rm)[2], double half_inv_eps, double (&col)[2]) {
#pragma clang fp contract(off)
    col[0] = (rp[0] - rm[0]) * half_inv_eps;
    col[1] = (rp[1] - rm[1]) * half_inv_eps;
}

// In-place Cholesky of a symmetric 3 x 3 matrix given as its packed lower triangle, as pgo_chol6
__host__ __device__ __forceinline__ bool ba_chol3(double (&a)[6]) {
#pragma clang fp contract(off)
    bool ok = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            double s = a[pgo_tri(r, c)];
#pragma unroll
            for (int k = 0; k < c; ++k) s = s - a[pgo_tri(r, k)] * a[pgo_tri(c, k)];
            if (c == r) {
                ok = ok && (s > 0.0);
                a[pgo_tri(r, r)] = sqrt(s);
            } else {
                a[pgo_tri(r, c)] = s / a[pgo_tri(c, c)];
            }
        }
    }
    return ok;
}

// x <- L^-1 x
__host__ __device__ __forceinline__ void ba_lower_solve3(const double (&l)[6], double (&x)[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double s = x[r];
#pragma unroll
        for (int k = 0; k < r; ++k) s = s - l[pgo_tri(r, k)] * x[k];
        x[r] = s / l[pgo_tri(r, r)];
    }
}

// x <- L^-T x
__host__ __device__ __forceinline__ void ba_upper_solve3(const double (&l)[6], double (&x)[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 2; r >= 0; --r) {
        double s = x[r];
#pragma unroll
        for (int k = 2; k > r; --k) s = s - l[pgo_tri(k, r)] * x[k];
        x[r] = s / l[pgo_tri(r, r)];
    }
}

// (H + damping I) dp = -g, H the packed lower triangle before damping; false: a pivot is not > 0 and dp is not to be used
__host__ __device__ __forceinline__ bool ba_solve6(const double (&H)[21], const double (&g)[6], double damping, double (&dp)[6]) {
#pragma clang fp contract(off)
    double L[21];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) L[pgo_tri(r, c)] = (r == c) ? H[pgo_tri(r, c)] + damping : H[pgo_tri(r, c)];
    const bool ok = pgo_chol6(L);
#pragma unroll
    for (int k = 0; k < 6; ++k) dp[k] = -g[k];
    pgo_lower_solve6(L, dp);
    pgo_upper_solve6(L, dp);
    return ok;
}

__host__ __device__ __forceinline__ bool ba_solve3(const double (&H)[6], const double (&g)[3], double damping, double (&dp)[3]) {
#pragma clang fp contract(off)
    double L[6];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) L[pgo_tri(r, c)] = (r == c) ? H[pgo_tri(r, c)] + damping : H[pgo_tri(r, c)];
    const bool ok = ba_chol3(L);
#pragma unroll
    for (int k = 0; k < 3; ++k) dp[k] = -g[k];
    ba_lower_solve3(L, dp);
    ba_upper_solve3(L, dp);
    return ok;
}

// One observation's two rows added to the running sums of an element with N parameters: the packed lower triangle of H (entry
// (a, b), b <= a: + Ju[a] Ju[b], then + Jv[a] Jv[b]), g (+ Ju[a] ru, then + Jv[a] rv) and r . r (+ ru ru, then + rv rv)
template <int N>
__host__ __device__ __forceinline__ void ba_accumulate(const double (&Ju)[N], const double (&Jv)[N], const double (&r)[2],
                                                       double (&H)[N * (N + 1) / 2], double (&g)[N], double& cost) {
#pragma clang fp contract(off)
#pragma unroll
    for (int a = 0; a < N; ++a) {
#pragma unroll
        for (int b = 0; b <= a; ++b) {
            H[pgo_tri(a, b)] = H[pgo_tri(a, b)] + Ju[a] * Ju[b];
            H[pgo_tri(a, b)] = H[pgo_tri(a, b)] + Jv[a] * Jv[b];
        }
        g[a] = g[a] + Ju[a] * r[0];
        g[a] = g[a] + Jv[a] * r[1];
    }
    cost = cost + r[0] * r[0];
    cost = cost + r[1] * r[1];
}

// ---- what lcm_ba.cpp hands to lcm_ba.hip -------------------------------------------------------------------------------------
// The tables are lcm_ba_host.h's plan (BaPlan): cam_off / cam_obs and pt_off / pt_obs, the observations of every camera and of
// every point in ascending index of the caller's list.  Poses and points are updated in place: a camera's workgroup reads and
// writes its own pose only, a point's lane its own point only.  The seam pointers are NULL outside lcm_ba_step_*.
struct BaArgs {
    BaPose* poses; BaPoint* points; const uint8_t* valid; const BaObs* obs;
    const uint32_t* cam_off; const uint32_t* cam_obs; const uint32_t* pt_off; const uint32_t* pt_obs;
    BaElemInfo* cam_info; BaElemInfo* pt_info;
    double* seam_r; double* seam_J; double* seam_H; double* seam_g; double* seam_dp;
    double* obs_err; double* partial; double* mean_out;            // k_ba_error / k_ba_mean; obs_err may be NULL
    uint8_t* flags; double* max_err;                               // k_ba_outliers
    uint32_t n_cams, n_points, n_obs, n_partials;
    BaCamera K;
    double eps, damping, min_update, outlier_px, centroid[3], max_dist;
    int32_t inner_iters, min_cam_obs, min_point_obs;
};

hipError_t launch_ba_cameras(const BaArgs& a, hipStream_t st);     // k_ba_cameras
hipError_t launch_ba_points(const BaArgs& a, hipStream_t st);      // k_ba_points
hipError_t launch_ba_error(const BaArgs& a, hipStream_t st);       // k_ba_error, k_ba_mean
hipError_t launch_ba_outliers(const BaArgs& a, hipStream_t st);    // k_ba_outliers

}  // namespace lcm
