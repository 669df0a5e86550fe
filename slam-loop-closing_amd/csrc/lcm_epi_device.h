// lcm_epi_device.h — the arithmetic of the essential-matrix RANSAC (lcm_epi.hip), stated once for the kernels, the host and
// the tests (tests/epiref.py restates it in numpy; include/lcm.h and DESIGN §9h describe the model):
//   epi_hash / epi_sample8   the counter-based sampler: 8 distinct indices of [0, n) by Floyd's algorithm, integers only
//   epi_norm / epi_inlier    normalisation and the inlier rule, in double, every product and sum rounded on its own
//   epi_solve8               one hypothesis: null vector of the 8 x 9 constraint matrix by elimination with full pivoting,
//                            projected onto the essential manifold by a one-sided 3 x 3 Jacobi SVD with a fixed sweep count
// Everything is __host__ __device__: the host compiles the same text (a stand-alone program runs it under a sanitizer).
// Included by lcm_epi.hip and lcm_epi.cpp only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcm {

constexpr int EPI_SAMPLE = 8;                 // correspondences of a minimal sample (the linear eight-point method)
constexpr double EPI_PIVOT_MIN = 1e-12;       // a pivot below this (normalised coordinates: the entries are O(1)) = rank-deficient sample
constexpr double EPI_RANK2_MIN = 1e-12;       // second singular value below this x the first: no essential matrix in the sample
constexpr int EPI_JACOBI_SWEEPS = 8;          // fixed: a 3 x 3 one-sided Jacobi is at rounding level after 5
constexpr uint32_t EPI_MAX_POINTS = 65535;    // per pair: the packed key holds the count in 16 bits
constexpr uint32_t EPI_MAX_ITERS = 65536;     // ... and 0xFFFF - hypothesis in the other 16

// The device's result record = lcm_epi_result (include/lcm.h; lcm_epi.cpp asserts the layout)
struct EpiResult { double E[9]; int32_t n_points, n_inliers, best_iter, status; };

// MurmurHash3's 32-bit finaliser (Appleby, public domain)
__host__ __device__ __forceinline__ uint32_t epi_fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// draw k of hypothesis `iter` of pair `pair`: the finaliser chained over the four counters, all arithmetic mod 2^32
__host__ __device__ __forceinline__ uint32_t epi_hash(uint32_t seed, uint32_t pair, uint32_t iter, uint32_t k) {
    uint32_t h = epi_fmix32(seed + 0x9E3779B9u);
    h = epi_fmix32(h ^ pair);
    h = epi_fmix32(h ^ iter);
    return epi_fmix32(h ^ k);
}

// Floyd's algorithm: for j = n - 8 .. n - 1, r = hash % (j + 1); r unless already chosen, else j.  n >= 8.
__host__ __device__ __forceinline__ void epi_sample8(uint32_t seed, uint32_t pair, uint32_t iter, uint32_t n, uint32_t (&s)[EPI_SAMPLE]) {
#pragma unroll
    for (int k = 0; k < EPI_SAMPLE; ++k) {
        const uint32_t j = n - EPI_SAMPLE + (uint32_t)k;
        const uint32_t r = epi_hash(seed, pair, iter, (uint32_t)k) % (j + 1u);
        bool taken = false;
#pragma unroll
        for (int m = 0; m < k; ++m) taken |= s[m] == r;
        s[k] = taken ? j : r;
    }
}

// x = ((double)u - c) / f
__host__ __device__ __forceinline__ double epi_norm(float u, double c, double f) {
#pragma clang fp contract(off)
    const double x = (double)u - c;
    return x / f;
}

// The inlier rule (include/lcm.h): query (a, b, 1), train (c, d, 1), E row-major; no division, no fused multiply-add, the
// sums left to right.  The all-zero matrix has den == 0: no inlier.
__host__ __device__ __forceinline__ bool epi_inlier(const double (&e)[9], double a, double b, double c, double d, double t2) {
#pragma clang fp contract(off)
    const double p0 = e[0] * a + e[1] * b + e[2];
    const double p1 = e[3] * a + e[4] * b + e[5];
    const double p2 = e[6] * a + e[7] * b + e[8];
    const double q0 = e[0] * c + e[3] * d + e[6];
    const double q1 = e[1] * c + e[4] * d + e[7];
    const double num = c * p0 + d * p1 + p2;
    const double den = p0 * p0 + p1 * p1 + q0 * q0 + q1 * q1;
    const double lhs = num * num, rhs = t2 * den;
    return den > 0.0 && lhs <= rhs;
}

// Row of the constraint matrix for x2^T E x1 = 0: element (r, c) of the caller's 8 x 9 system lives at A[(r * 9 + c) * STRIDE]
// (STRIDE = 64 on the device: a lane-private column of LDS, so a runtime index costs nothing and no lane meets another's
// bank; 1 on the host).
template <int STRIDE>
__host__ __device__ __forceinline__ void epi_put_row(double* A, int r, double a, double b, double c, double d) {
    double* row = A + (size_t)r * 9 * STRIDE;
    row[0 * STRIDE] = c * a; row[1 * STRIDE] = c * b; row[2 * STRIDE] = c;
    row[3 * STRIDE] = d * a; row[4 * STRIDE] = d * b; row[5 * STRIDE] = d;
    row[6 * STRIDE] = a;     row[7 * STRIDE] = b;     row[8 * STRIDE] = 1.0;
}

// Projection onto the essential manifold: singular values (s1, s2, s3) -> (1, 1, 0).  One-sided Jacobi: the columns of
// G = F V are made orthogonal by plane rotations (V accumulates them); the column of the smallest norm is dropped and
// E = u_a v_a^T + u_b v_b^T over the other two, u = G's column over its norm.  false (e zeroed): no second singular value.
__host__ __device__ __forceinline__ bool epi_project(double (&e)[9]) {
    double g[3][3], v[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) { g[i][j] = e[3 * i + j]; v[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < EPI_JACOBI_SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double alpha = g[0][p] * g[0][p] + g[1][p] * g[1][p] + g[2][p] * g[2][p];
                const double beta = g[0][q] * g[0][q] + g[1][q] * g[1][q] + g[2][q] * g[2][q];
                const double gamma = g[0][p] * g[0][q] + g[1][p] * g[1][q] + g[2][p] * g[2][q];
                double cs = 1.0, sn = 0.0;
                if (gamma != 0.0 && gamma * gamma > 1e-36 * alpha * beta) {
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    cs = 1.0 / sqrt(1.0 + t * t);
                    sn = cs * t;
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double gp = g[i][p], gq = g[i][q], vp = v[i][p], vq = v[i][q];
                    g[i][p] = cs * gp - sn * gq; g[i][q] = sn * gp + cs * gq;
                    v[i][p] = cs * vp - sn * vq; v[i][q] = sn * vp + cs * vq;
                }
            }
    }
    double nrm[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) nrm[k] = sqrt(g[0][k] * g[0][k] + g[1][k] * g[1][k] + g[2][k] * g[2][k]);
    const int drop = (nrm[0] <= nrm[1] && nrm[0] <= nrm[2]) ? 0 : (nrm[1] <= nrm[2] ? 1 : 2);
    const double hi = fmax(nrm[0], fmax(nrm[1], nrm[2]));
    const double mid = drop == 0 ? fmin(nrm[1], nrm[2]) : (drop == 1 ? fmin(nrm[0], nrm[2]) : fmin(nrm[0], nrm[1]));
    const bool ok = hi > 0.0 && mid > EPI_RANK2_MIN * hi && hi < 1e300;       // also false for NaN / Inf
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s += (k == drop || !ok) ? 0.0 : (g[i][k] / nrm[k]) * v[j][k];
            e[3 * i + j] = ok ? s : 0.0;
        }
    return ok;
}

// One hypothesis from the 8 x 9 system in A (destroyed): Gauss-Jordan elimination with full pivoting leaves 8 pivot columns
// and one free column f; the null vector is x[f] = 1, x[pivot column k] = -A[k][f] / A[k][k].  It is then projected.
// A pivot below EPI_PIVOT_MIN, or a projection without a second singular value: e = 0, false.  Every loop has fixed bounds.
template <int STRIDE>
__host__ __device__ __forceinline__ bool epi_solve8(double* A, double (&e)[9]) {
    uint64_t perm = 0x876543210ull;            // nibble k: the original column now at position k
    bool ok = true;
    for (int k = 0; k < EPI_SAMPLE; ++k) {
        double best = -1.0;
        int pr = k, pc = k;
        for (int r = k; r < EPI_SAMPLE; ++r)
            for (int c = k; c < 9; ++c) {
                const double m = fabs(A[(r * 9 + c) * STRIDE]);
                if (m > best) { best = m; pr = r; pc = c; }
            }
        if (!(best >= EPI_PIVOT_MIN && best < 1e300)) { ok = false; break; }
        if (pr != k)
            for (int c = k; c < 9; ++c) {
                const double t = A[(k * 9 + c) * STRIDE];
                A[(k * 9 + c) * STRIDE] = A[(pr * 9 + c) * STRIDE];
                A[(pr * 9 + c) * STRIDE] = t;
            }
        if (pc != k) {
            for (int r = 0; r < EPI_SAMPLE; ++r) {
                const double t = A[(r * 9 + k) * STRIDE];
                A[(r * 9 + k) * STRIDE] = A[(r * 9 + pc) * STRIDE];
                A[(r * 9 + pc) * STRIDE] = t;
            }
            const uint64_t ck = (perm >> (4 * k)) & 15u, cp = (perm >> (4 * pc)) & 15u;
            perm = (perm & ~((15ull << (4 * k)) | (15ull << (4 * pc)))) | (cp << (4 * k)) | (ck << (4 * pc));
        }
        const double piv = A[(k * 9 + k) * STRIDE];
        for (int r = 0; r < EPI_SAMPLE; ++r) {
            if (r == k) continue;
            const double f = A[(r * 9 + k) * STRIDE] / piv;
            for (int c = k + 1; c < 9; ++c) A[(r * 9 + c) * STRIDE] -= f * A[(k * 9 + c) * STRIDE];
        }
    }
    if (ok) {
        double x[9];
#pragma unroll
        for (int k = 0; k < EPI_SAMPLE; ++k) x[k] = -A[(k * 9 + 8) * STRIDE] / A[(k * 9 + k) * STRIDE];
        x[8] = 1.0;
        // un-permute through row 0 of the system, which nothing needs any more
#pragma unroll
        for (int k = 0; k < 9; ++k) A[((perm >> (4 * k)) & 15u) * STRIDE] = x[k];
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] = A[k * STRIDE];
        ok = epi_project(e);
    }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] = 0.0;
    }
    return ok;
}

}  // namespace lcm
