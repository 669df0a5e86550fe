// lcm_ba_device.h — the arithmetic of the alternating bundle adjustment (lcm_ba.hip), stated once for the kernels, the host-only
// helpers of lcm_ba_host.h and the tests (tests/baref.py restates it in numpy; include/lcm.h and DESIGN §9q describe the model):
//   ba_residual        the projection minus the pixel: (((fx x) / z) + cx) - u, (((fy y) / z) + cy) - v; no test on z (:157-162, :673-674)
//   ba_error           sqrt(dx dx + dy dy) of a residual (:886-888)
//   ba_column          (r_plus - r_minus) (0.5 / eps), one central-difference column of one observation (:712, :828)
//   ba_accumulate      one observation's two rows added to an element's running sums
// The records, the rotation's exp and log, the camera point, the projection and the damped Cholesky solves are
// lcm_geom_device.h's: called, not restated.  In double, every product and sum rounded on its own (fp contract off), sums left
// to right.  Everything is __host__ __device__: the host compiles the same text (a stand-alone program runs it under a sanitizer).
// Included by lcm_ba.hip and by lcm_ba_host.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lcm_geom_device.h"

namespace lcm {

// The device's record = lcm_ba_elem_info (include/lcm.h; lcm_ba.cpp asserts the layout); the pose, the point, the observation and
// the camera are lcm_geom_device.h's
struct BaElemInfo { double last_update, cost; int32_t iterations, status; };

constexpr int BA_CONVERGED = 0, BA_MAX_ITERS = 1, BA_SOLVE_FAILED = 2, BA_HALF_TURN = 3, BA_SKIPPED = 4;   // lcm_ba_status
constexpr int BA_CAMERA_THREADS = 256;       // k_ba_cameras: one workgroup per camera
constexpr int BA_CAMERA_SUMS = 28;           // the packed lower triangle of H (21), g (6), r . r (1)
constexpr int BA_CAMERA_CHUNK = 32;          // lanes per first-level sum
constexpr int BA_ERROR_THREADS = 256;        // k_ba_error: observations per workgroup = per partial sum

__host__ __device__ __forceinline__ void ba_residual(const Camera& K, const double (&Xc)[3], double u, double v, double (&r)[2]) {
#pragma clang fp contract(off)
    double pu, pv;
    pinhole_project(K, Xc, pu, pv);
    r[0] = pu - u;
    r[1] = pv - v;
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
            H[tri_index(a, b)] = H[tri_index(a, b)] + Ju[a] * Ju[b];
            H[tri_index(a, b)] = H[tri_index(a, b)] + Jv[a] * Jv[b];
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
    Pose* poses; Point3* points; const uint8_t* valid; const Observation* obs;
    const uint32_t* cam_off; const uint32_t* cam_obs; const uint32_t* pt_off; const uint32_t* pt_obs;
    BaElemInfo* cam_info; BaElemInfo* pt_info;
    double* seam_r; double* seam_J; double* seam_H; double* seam_g; double* seam_dp;
    double* obs_err; double* partial; double* mean_out;            // k_ba_error / k_ba_mean; obs_err may be NULL
    uint8_t* flags; double* max_err;                               // k_ba_outliers
    uint32_t n_cams, n_points, n_obs, n_partials;
    Camera K;
    double eps, damping, min_update, outlier_px, centroid[3], max_dist;
    int32_t inner_iters, min_cam_obs, min_point_obs;
};

hipError_t launch_ba_cameras(const BaArgs& a, hipStream_t st);     // k_ba_cameras
hipError_t launch_ba_points(const BaArgs& a, hipStream_t st);      // k_ba_points
hipError_t launch_ba_error(const BaArgs& a, hipStream_t st);       // k_ba_error, k_ba_mean
hipError_t launch_ba_outliers(const BaArgs& a, hipStream_t st);    // k_ba_outliers

}  // namespace lcm
