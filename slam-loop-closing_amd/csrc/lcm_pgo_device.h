// lcm_pgo_device.h — the arithmetic of the pose-graph correction (lcm_pgo.hip), stated once for the kernels, the two host-only
// helpers of lcm_pgo_host.h and the tests (tests/pgoref.py restates it in numpy; include/lcm.h and DESIGN §9p describe the model):
//   pgo_exp            rotation vector -> rotation matrix (Rodrigues' formula)
//   pgo_log            rotation matrix -> rotation vector, first order below s = 1e-5; false at half a turn
//   pgo_mul / pgo_mul_tn / pgo_mul_nt / pgo_apply   the 3 x 3 products, every entry a0 b0 + a1 b1 + a2 b2 from the left
//   pgo_edge_residual  the six residuals of one edge (src/main.cpp:358-381)
//   pgo_chol6 / pgo_lower_solve6 / pgo_upper_solve6   the 6 x 6 Cholesky factor (lower triangle, packed) and its two solves
// In double, every product and sum rounded on its own (fp contract off), sums left to right.  Everything is
// __host__ __device__: the host compiles the same text (a stand-alone program runs it under a sanitizer).
// Included by lcm_pgo.hip and, for pgo_exp / pgo_log and the products, by lcm_pgo_host.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace lcm {

constexpr double PGO_EPSILON = 2.220446049250313e-16;     // DBL_EPSILON: below it a rotation vector is the identity
constexpr double PGO_LOG_SMALL = 1e-5;                    // below this sine the logarithm is its first-order term

// The device's records = lcm_pgo_pose, lcm_pgo_edge (include/lcm.h; lcm_pgo.cpp asserts the layouts)
struct PgoPose { double R[9]; double t[3]; };
struct PgoEdge { double R[9]; double t[3]; double weight; int32_t from, to; };

// index of (r, c), c <= r, in a packed lower triangle
__host__ __device__ constexpr int pgo_tri(int r, int c) { return r * (r + 1) / 2 + c; }

// C = A B
__host__ __device__ __forceinline__ void pgo_mul(const double (&a)[9], const double (&b)[9], double (&c)[9]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// C = A^T B
__host__ __device__ __forceinline__ void pgo_mul_tn(const double (&a)[9], const double (&b)[9], double (&c)[9]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[i] * b[j] + a[3 + i] * b[3 + j] + a[6 + i] * b[6 + j];
}

// C = A B^T
__host__ __device__ __forceinline__ void pgo_mul_nt(const double (&a)[9], const double (&b)[9], double (&c)[9]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1] + a[3 * i + 2] * b[3 * j + 2];
}

// y = A x
__host__ __device__ __forceinline__ void pgo_apply(const double (&a)[9], const double (&x)[3], double (&y)[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = a[3 * i] * x[0] + a[3 * i + 1] * x[1] + a[3 * i + 2] * x[2];
}

// exp: theta = sqrt(r . r); below DBL_EPSILON the identity; else k = r / theta and
// R = cos(theta) I + (1 - cos(theta)) k k^T + sin(theta) [k]x, entry by entry in this order
__host__ __device__ __forceinline__ void pgo_exp(const double (&r)[3], double (&R)[9]) {
#pragma clang fp contract(off)
    const double theta = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (theta < PGO_EPSILON) {
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
__host__ __device__ __forceinline__ bool pgo_log(const double (&R)[9], double (&r)[3]) {
#pragma clang fp contract(off)
    const double vx = 0.5 * (R[7] - R[5]), vy = 0.5 * (R[2] - R[6]), vz = 0.5 * (R[3] - R[1]);
    const double s = sqrt(vx * vx + vy * vy + vz * vz);
    double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    if (s >= PGO_LOG_SMALL) {
        const double f = atan2(s, c) / s;
        r[0] = vx * f; r[1] = vy * f; r[2] = vz * f;
        return true;
    }
    r[0] = vx; r[1] = vy; r[2] = vz;
    return c > 0.0;
}

// The residual of one edge between (Rf, tf) and (Rt, tt): w log((R_rel Rf)^T Rt), w (tt - (R_rel tf + t_rel)), w = sqrt(weight).
// false: the rotational error is half a turn (r[0..3) is then w v).
__host__ __device__ __forceinline__ bool pgo_edge_residual(const double (&Rrel)[9], const double (&trel)[3], double w,
                                                           const double (&Rf)[9], const double (&tf)[3], const double (&Rt)[9],
                                                           const double (&tt)[3], double (&r)[6]) {
#pragma clang fp contract(off)
    double Rexp[9], Rerr[9], rv[3], te[3];
    pgo_mul(Rrel, Rf, Rexp);
    pgo_mul_tn(Rexp, Rt, Rerr);
    const bool ok = pgo_log(Rerr, rv);
    pgo_apply(Rrel, tf, te);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r[k] = w * rv[k];
        r[3 + k] = w * (tt[k] - (te[k] + trel[k]));
    }
    return ok;
}

// In-place Cholesky of a symmetric 6 x 6 matrix given as its packed lower triangle: a = L L^T, row by row, every entry
// a[r][c] - sum_{k < c} l[r][k] l[c][k] from the left.  false: a pivot is not > 0 (NaN included); the factor is then unusable.
__host__ __device__ __forceinline__ bool pgo_chol6(double (&a)[21]) {
#pragma clang fp contract(off)
    bool ok = true;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
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
__host__ __device__ __forceinline__ void pgo_lower_solve6(const double (&l)[21], double (&x)[6]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double s = x[r];
#pragma unroll
        for (int k = 0; k < r; ++k) s = s - l[pgo_tri(r, k)] * x[k];
        x[r] = s / l[pgo_tri(r, r)];
    }
}

// x <- L^-T x
__host__ __device__ __forceinline__ void pgo_upper_solve6(const double (&l)[21], double (&x)[6]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 5; r >= 0; --r) {
        double s = x[r];
#pragma unroll
        for (int k = 5; k > r; --k) s = s - l[pgo_tri(k, r)] * x[k];
        x[r] = s / l[pgo_tri(r, r)];
    }
}

// ---- what lcm_pgo.cpp hands to lcm_pgo.hip ----------------------------------------------------------------------------------
// The run's state on the device: the first 48 bytes are lcm_pgo_info.  `done` ends the run: every kernel of a later iteration
// that finds it set does nothing.  `half_turn` is raised by any log that has no rotation vector.
struct PgoState {
    double cost_first, cost_last, max_update, lambda;
    int32_t iterations, status, n_params, n_border;
    int32_t done, half_turn;
};

// The unknowns' order, the tables and the buffers are lcm_pgo_host.h's plan (PgoPlan): interior slots [0, n_int), border slots
// behind them.  D, C, L, M: 36 doubles per interior slot (C[i] couples slot i to slot i + 1; L packed, pgo_tri); B: n_int x 6 x
// 6 n_border; W: n_int x 6 x ncols, the last column the right-hand side; S: the border's square; T: 6 n_border x ncols, the
// Schur system and its right-hand side; g, dpu: 6 per slot; tr: the trace of a slot's diagonal block.
struct PgoArgs {
    const PgoPose* poses; const uint8_t* valid; const PgoEdge* edges; const int32_t* tab;
    double* params; double* res; double* jac;
    double* D; double* C; double* L; double* M; double* B; double* W; double* S; double* T; double* g; double* dpu; double* tr;
    double* dp_out; PgoPose* poses_out; PgoState* st;
    uint32_t n_poses, n_edges, n_int, n_border;
    uint32_t tab_off, tab_edge, tab_int, tab_border;
    double eps, damping, min_update;
    int32_t max_iters;
};

constexpr int PGO_KERNELS_PER_ITERATION = 5;
hipError_t launch_pgo_params(const PgoArgs& a, hipStream_t st);         // k_pgo_params
hipError_t launch_pgo_iteration(const PgoArgs& a, hipStream_t st);      // k_pgo_linearise, _assemble, _sweep, _schur, _finish
hipError_t launch_pgo_writeback(const PgoArgs& a, hipStream_t st);      // k_pgo_writeback

}  // namespace lcm
