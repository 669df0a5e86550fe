// lcm_lo_device.h — the arithmetic of the RANSAC's local optimisation (lcm_lo.hip), stated once for the kernels, the host and
// the tests (tests/loref.py restates it in numpy; include/lcm.h and DESIGN §9j describe the model):
//   lo_threshold2            the inlier threshold of a round: (t * mult)^2
//   lo_hartley_scale         Hartley's isotropic scale from a side's summed squared distances to its mean
//   lo_add_moments           one record's constraint row r (epi_put_row's layout) added to the 45 sums of r r^T
//   lo_eig9                  the eigenvector of the smallest eigenvalue of the 9 x 9 moment matrix: cyclic Jacobi, fixed sweeps,
//                            the packed index and the rotation's angle lcm_geom_device.h's
//   lo_denormalise           F = T2^T mat(f) T1
//   lo_accepts / lo_lane_key the acceptance rule of a seed and the key that picks the winning seed of a pair
// The inlier rule, the camera normalisation, the constraint row and the projection are lcm_epi_device.h's: called, not restated.
// Everything is __host__ __device__: the host compiles the same text (a stand-alone program runs it under a sanitizer).
// Included by lcm_lo.hip and lcm_lo.cpp only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcm_epi_device.h"
#include "lcm_geom_device.h"

namespace lcm {

constexpr int LO_SEEDS = 64;                  // hypotheses refined per pair: one wave, lane = seed
constexpr int LO_MAX_ROUNDS = 8;
constexpr int LO_MOMENTS = 45;                // upper triangle of the 9 x 9 moment matrix, row-major
constexpr int LO_WORK = LO_MOMENTS + 81;      // lo_eig9's workspace in doubles: the packed matrix and the rotations' product
// A side's mean squared distance to its mean below this is the rounding of the mean, not a spread: normalised camera
// coordinates are O(1), their rounding leaves v near 1e-32, and a hundredth of a pixel of spread at f = 700 gives 2e-10.
constexpr double LO_VAR_MIN = 1e-20;
// tests/loref.py's jacobi_eigvec stops changing after 7 sweeps on every moment matrix of the test scenes: one more.
constexpr int LO_JACOBI_SWEEPS = 8;

// lcm_lo_status (include/lcm.h)
constexpr int32_t LO_OK = 0, LO_TOO_FEW = 1, LO_DEGENERATE = 2, LO_NO_MODEL = 3;

// The device's info record = lcm_lo_info (include/lcm.h; lcm_lo.cpp asserts the layout)
struct LoInfo { int32_t seed_iter, round, n_inliers_ransac, status; };

// tm = t * mult, t2m = tm * tm: mult == 1 gives the model's own t2 (epi_t2) bit for bit
__host__ __device__ __forceinline__ double lo_threshold2(double t, double mult) {
#pragma clang fp contract(off)
    const double tm = t * mult;
    return tm * tm;
}

// v = sum / n of (x - mx)^2 + (y - my)^2 over the selected records; s = sqrt(2 / v).  false (s = 0): no spread, or not finite.
__host__ __device__ __forceinline__ bool lo_hartley_scale(double sum, double n, double* s) {
#pragma clang fp contract(off)
    const double v = sum / n;
    const bool ok = v >= LO_VAR_MIN && v < 1e300;              // also false for NaN
    *s = ok ? sqrt(2.0 / v) : 0.0;
    return ok;
}

// (x - mx)^2 + (y - my)^2
__host__ __device__ __forceinline__ double lo_sqdist(double x, double y, double mx, double my) {
#pragma clang fp contract(off)
    const double dx = x - mx, dy = y - my;
    return dx * dx + dy * dy;
}

// (x - m) * s
__host__ __device__ __forceinline__ double lo_centre(double x, double m, double s) {
#pragma clang fp contract(off)
    const double c = x - m;
    return c * s;
}

// m[k] += r_i r_j over i <= j, k row-major over the upper triangle; r = the constraint row of the normalised record
__host__ __device__ __forceinline__ void lo_add_moments(double (&m)[LO_MOMENTS], double a, double b, double c, double d) {
#pragma clang fp contract(off)
    double r[9];
    epi_put_row<1>(r, 0, a, b, c, d);
    int k = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = i; j < 9; ++j) {
            const double prod = r[i] * r[j];
            m[k] = m[k] + prod;
            ++k;
        }
}

// Eigenvector of the smallest eigenvalue of the symmetric matrix packed in W[k * STRIDE], k < 45 (destroyed): cyclic Jacobi,
// LO_JACOBI_SWEEPS sweeps over the 36 pairs (p, q); the product of the rotations accumulates in W[(45 + 9 i + j) * STRIDE].
// STRIDE = 64 on the device: a lane-private column of LDS, so the runtime indices cost nothing and no lane meets another's
// bank; 1 on the host.  The smallest diagonal entry, first of equals, names the column.  Every loop has fixed bounds.
template <int STRIDE>
__host__ __device__ __forceinline__ void lo_eig9(double* W, double (&f)[9]) {
#pragma clang fp contract(off)
    double* V = W + (size_t)LO_MOMENTS * STRIDE;
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) V[(9 * i + j) * STRIDE] = i == j ? 1.0 : 0.0;
    // one rotation's text, run 36 times a sweep: unrolled over (p, q) it would not fit the instruction cache
#pragma clang loop unroll(disable)
    for (int sweep = 0; sweep < LO_JACOBI_SWEEPS; ++sweep)
#pragma clang loop unroll(disable)
        for (int p = 0; p < 8; ++p)
#pragma clang loop unroll(disable)
            for (int q = p + 1; q < 9; ++q) {
                const int pp = sym_index<9>(p, p), qq = sym_index<9>(q, q), pq = sym_index<9>(p, q);
                const double app = W[pp * STRIDE], aqq = W[qq * STRIDE], apq = W[pq * STRIDE];
                // both rows and both columns are read before the angle is known: their LDS latency hides behind its
                // division and square roots, and no store stands between two loads
                double ap[9], aq[9], vp[9], vq[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    ap[k] = W[sym_index<9>(k, p) * STRIDE]; aq[k] = W[sym_index<9>(k, q) * STRIDE];
                    vp[k] = V[(9 * k + p) * STRIDE]; vq[k] = V[(9 * k + q) * STRIDE];
                }
                double t, cs, sn;
                if (!jacobi_angle(app, aqq, apq, t, cs, sn)) continue;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    if (k != p && k != q) {
                        W[sym_index<9>(k, p) * STRIDE] = cs * ap[k] - sn * aq[k];
                        W[sym_index<9>(k, q) * STRIDE] = sn * ap[k] + cs * aq[k];
                    }
                    V[(9 * k + p) * STRIDE] = cs * vp[k] - sn * vq[k];
                    V[(9 * k + q) * STRIDE] = sn * vp[k] + cs * vq[k];
                }
                W[pp * STRIDE] = app - t * apq;
                W[qq * STRIDE] = aqq + t * apq;
                W[pq * STRIDE] = 0.0;
            }
    int col = 0;
    double least = W[sym_index<9>(0, 0) * STRIDE];
    for (int k = 1; k < 9; ++k) {
        const double dk = W[sym_index<9>(k, k) * STRIDE];
        if (dk < least) { least = dk; col = k; }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = V[(9 * k + col) * STRIDE];
}

// F = T2^T mat(f) T1 in place, T = [[s, 0, -s mx], [0, s, -s my], [0, 0, 1]]: side 1 the query's, side 2 the train's
__host__ __device__ __forceinline__ void lo_denormalise(double (&f)[9], double m1x, double m1y, double s1, double m2x, double m2y, double s2) {
#pragma clang fp contract(off)
    const double u1 = -(s1 * m1x), v1 = -(s1 * m1y), u2 = -(s2 * m2x), v2 = -(s2 * m2y);
    double g[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        g[3 * i + 0] = f[3 * i + 0] * s1;
        g[3 * i + 1] = f[3 * i + 1] * s1;
        g[3 * i + 2] = f[3 * i + 0] * u1 + f[3 * i + 1] * v1 + f[3 * i + 2];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        f[0 + j] = s2 * g[0 + j];
        f[3 + j] = s2 * g[3 + j];
        f[6 + j] = u2 * g[0 + j] + v2 * g[3 + j] + g[6 + j];
    }
}

// A seed adopts a refit only when it holds strictly more inliers than anything the seed has held (the seed itself included):
// the first round of the largest count.  Equal counts keep the earlier matrix, so an unimproved pair keeps the RANSAC's bytes.
__host__ __device__ __forceinline__ bool lo_accepts(uint32_t count, uint32_t best) { return count > best; }

// Across a pair's seeds: the largest count, among equals the lowest lane.  count <= 65 535.
__host__ __device__ __forceinline__ uint32_t lo_lane_key(uint32_t count, uint32_t lane) { return count << 6 | (63u - lane); }

}  // namespace lcm
