// lcm_map_device.h — the arithmetic of the map building before the loop (include/lcm.h, lcm_map_*; src/main.cpp:1152-1351),
// stated once for the kernels (lcm_map.hip), the host (lcm_map_host.h) and the tests (tests/mapref.py restates it in numpy;
// DESIGN §9r describes the model):
//   map_displacement      one record's displacement of computeMedianDisplacement (:171-189)
//   map_system            the ten sums of M = A^T A of cv::triangulatePoints' 4 x 4 system
//   map_rotate            one Jacobi rotation of the packed 4 x 4 matrix and of the rotations' product
//   map_jacobi4           the eigenvector of M's smallest eigenvalue: cyclic Jacobi, fixed sweeps, everything in registers
//   map_parallax_cos      the cosine of the angle between the two rays (:200-222, without the acos)
//   map_reproj_error      computeSingleReprojError (:227-246)
//   map_record            one record from its four floats to its status and its lcm_map_tri, in the reference's order (:1261-1313)
// The camera point, the projection, the packed index and the rotation's angle are lcm_geom_device.h's: called, not restated.
// In double, every product and sum rounded on its own (fp contract off), sums left to right.  Every index into M and into the
// rotations' product is a compile-time constant (the pairs (p, q) and the rows are template arguments), so the 26 doubles live in
// registers and the kernel needs no scratch memory.  Everything is __host__ __device__: the host compiles the same text
// (tests/cpp/map_host_check.cpp runs it under a sanitizer).  Included by lcm_map.hip and lcm_map_host.h only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lcm_geom_device.h"

namespace lcm {

// lcm_map_status (include/lcm.h)
constexpr int MAP_NOT_INLIER = 0, MAP_NO_POINT = 1, MAP_REJ_DEPTH = 2, MAP_REJ_PARALLAX = 3, MAP_REJ_REPROJ = 4, MAP_ACCEPTED = 5,
              MAP_MERGED = 6, MAP_NEW = 7;
constexpr int MAP_STATUSES = 8;
constexpr int MAP_THREADS = 256;              // every kernel's workgroup
// tests/mapref.py's jacobi4 stops changing after 5 sweeps on every system of tests/mapcases.py's cases: one more.
constexpr int MAP_JACOBI_SWEEPS = 6;
constexpr double MAP_MIN_W = 1e-9;            // :1269
constexpr double MAP_MIN_RAY = 1e-9;          // :213
constexpr double MAP_BEHIND = 1e9;            // :237

// The device's record = lcm_map_tri (include/lcm.h; lcm_map.cpp asserts the layout); a merge writes lcm_geom_device.h's Point3 and
// Observation
struct MapTri { double X[3]; double depth1, depth2, cos_parallax, err1, err2; };
// One pair as the host planner leaves it (lcm_map_host.h, map_plan_pair): the two 3 x 4 matrices K [R | t] row-major, the poses,
// the centres, the baseline and the cosine of the smallest parallax
struct MapPair { double P1[12], P2[12], R1[9], t1[3], R2[9], t2[3], C1[3], C2[3], baseline, cos_min; };
struct MapLimits { double min_depth, max_depth, max_reproj; };

// dx = (double)(tx - qx) with the subtraction in float, dy likewise; sqrt(dx dx + dy dy)
__host__ __device__ __forceinline__ double map_displacement(float qx, float qy, float tx, float ty) {
#pragma clang fp contract(off)
    const float fx = tx - qx, fy = ty - qy;
    const double dx = (double)fx, dy = (double)fy;
    return sqrt(dx * dx + dy * dy);
}

// The rows of A: x1 P1[2] - P1[0], y1 P1[2] - P1[1], x2 P2[2] - P2[0], y2 P2[2] - P2[1]; m[sym_index<4>(i, j)] = the sum over the
// four rows, in that order, of A[r][i] A[r][j]
__host__ __device__ __forceinline__ void map_system(const double (&P1)[12], const double (&P2)[12], double x1, double y1, double x2, double y2,
                                                    double (&m)[10]) {
#pragma clang fp contract(off)
    double A[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        A[0][j] = x1 * P1[8 + j] - P1[j];
        A[1][j] = y1 * P1[8 + j] - P1[4 + j];
        A[2][j] = x2 * P2[8 + j] - P2[j];
        A[3][j] = y2 * P2[8 + j] - P2[4 + j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) {
            double s = A[0][i] * A[0][j];
#pragma unroll
            for (int r = 1; r < 4; ++r) s = s + A[r][i] * A[r][j];
            m[sym_index<4>(i, j)] = s;
        }
}

// row K of one rotation: the matrix's entries (K, P) and (K, Q) unless K is P or Q, and the product's
template <int K, int P, int Q>
__host__ __device__ __forceinline__ void map_rotate_row(double (&a)[10], double (&v)[16], double cs, double sn) {
#pragma clang fp contract(off)
    if (K != P && K != Q) {
        const double akp = a[sym_index<4>(K, P)], akq = a[sym_index<4>(K, Q)];
        a[sym_index<4>(K, P)] = cs * akp - sn * akq;
        a[sym_index<4>(K, Q)] = sn * akp + cs * akq;
    }
    const double vkp = v[4 * K + P], vkq = v[4 * K + Q];
    v[4 * K + P] = cs * vkp - sn * vkq;
    v[4 * K + Q] = sn * vkp + cs * vkq;
}

// One rotation on the pair (P, Q), skipped where jacobi_angle says so
template <int P, int Q>
__host__ __device__ __forceinline__ void map_rotate(double (&a)[10], double (&v)[16]) {
#pragma clang fp contract(off)
    const double app = a[sym_index<4>(P, P)], aqq = a[sym_index<4>(Q, Q)], apq = a[sym_index<4>(P, Q)];
    double t, cs, sn;
    if (!jacobi_angle(app, aqq, apq, t, cs, sn)) return;
    map_rotate_row<0, P, Q>(a, v, cs, sn);
    map_rotate_row<1, P, Q>(a, v, cs, sn);
    map_rotate_row<2, P, Q>(a, v, cs, sn);
    map_rotate_row<3, P, Q>(a, v, cs, sn);
    a[sym_index<4>(P, P)] = app - t * apq;
    a[sym_index<4>(Q, Q)] = aqq + t * apq;
    a[sym_index<4>(P, Q)] = 0.0;
}

// Eigenvector of the smallest eigenvalue of the packed symmetric matrix m (destroyed): MAP_JACOBI_SWEEPS sweeps over the six
// pairs in lexicographic order; the column of the smallest diagonal entry, first of equals
__host__ __device__ __forceinline__ void map_jacobi4(double (&m)[10], double (&h)[4]) {
#pragma clang fp contract(off)
    double v[16] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
#pragma clang loop unroll(disable)
    for (int sweep = 0; sweep < MAP_JACOBI_SWEEPS; ++sweep) {
        map_rotate<0, 1>(m, v); map_rotate<0, 2>(m, v); map_rotate<0, 3>(m, v);
        map_rotate<1, 2>(m, v); map_rotate<1, 3>(m, v); map_rotate<2, 3>(m, v);
    }
    double least = m[sym_index<4>(0, 0)];
    h[0] = v[0]; h[1] = v[4]; h[2] = v[8]; h[3] = v[12];
    if (m[sym_index<4>(1, 1)] < least) { least = m[sym_index<4>(1, 1)]; h[0] = v[1]; h[1] = v[5]; h[2] = v[9]; h[3] = v[13]; }
    if (m[sym_index<4>(2, 2)] < least) { least = m[sym_index<4>(2, 2)]; h[0] = v[2]; h[1] = v[6]; h[2] = v[10]; h[3] = v[14]; }
    if (m[sym_index<4>(3, 3)] < least) { least = m[sym_index<4>(3, 3)]; h[0] = v[3]; h[1] = v[7]; h[2] = v[11]; h[3] = v[15]; }
}

// The rays X - C_i; a norm below 1e-9 is parallax 0 (cosine 1); else the dot product of the normalised rays clamped to [-1, 1]
__host__ __device__ __forceinline__ double map_parallax_cos(const double (&C1)[3], const double (&C2)[3], const double (&X)[3]) {
#pragma clang fp contract(off)
    const double ax = X[0] - C1[0], ay = X[1] - C1[1], az = X[2] - C1[2];
    const double bx = X[0] - C2[0], by = X[1] - C2[1], bz = X[2] - C2[2];
    const double na = sqrt(ax * ax + ay * ay + az * az), nb = sqrt(bx * bx + by * by + bz * bz);
    if (na < MAP_MIN_RAY || nb < MAP_MIN_RAY) return 1.0;
    const double c = (ax / na) * (bx / nb) + (ay / na) * (by / nb) + (az / na) * (bz / nb);
    return c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
}

// 1e9 at z <= 0; else the distance from the projection to the pixel
__host__ __device__ __forceinline__ double map_reproj_error(const Camera& K, const double (&Xc)[3], double px, double py) {
#pragma clang fp contract(off)
    if (Xc[2] <= 0.0) return MAP_BEHIND;
    double u, v;
    pinhole_project(K, Xc, u, v);
    const double dx = u - px, dy = v - py;
    return sqrt(dx * dx + dy * dy);
}

// One record that takes part: its lcm_map_tri (all zero without a point) and its status
__host__ __device__ __forceinline__ int map_record(const MapPair& pr, const Camera& K, const MapLimits& lim, float qx, float qy, float tx,
                                                   float ty, MapTri& out) {
#pragma clang fp contract(off)
    const double x1 = (double)qx, y1 = (double)qy, x2 = (double)tx, y2 = (double)ty;
    double m[10], h[4];
    map_system(pr.P1, pr.P2, x1, y1, x2, y2, m);
    map_jacobi4(m, h);
    out = MapTri{{0.0, 0.0, 0.0}, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (fabs(h[3]) < MAP_MIN_W) return MAP_NO_POINT;
    const double X[3] = {h[0] / h[3], h[1] / h[3], h[2] / h[3]};
    double Xc1[3], Xc2[3];
    rigid_apply(pr.R1, pr.t1, X, Xc1);
    rigid_apply(pr.R2, pr.t2, X, Xc2);
    out.X[0] = X[0]; out.X[1] = X[1]; out.X[2] = X[2];
    out.depth1 = Xc1[2]; out.depth2 = Xc2[2];
    out.cos_parallax = map_parallax_cos(pr.C1, pr.C2, X);
    out.err1 = map_reproj_error(K, Xc1, x1, y1);
    out.err2 = map_reproj_error(K, Xc2, x2, y2);
    if (out.depth1 <= 0.0 || out.depth2 <= 0.0) return MAP_REJ_DEPTH;
    const double rel = out.depth1 / pr.baseline;
    if (rel < lim.min_depth || rel > lim.max_depth) return MAP_REJ_DEPTH;
    if (out.cos_parallax > pr.cos_min) return MAP_REJ_PARALLAX;
    if (out.err1 > lim.max_reproj || out.err2 > lim.max_reproj) return MAP_REJ_REPROJ;
    return MAP_ACCEPTED;
}

// ---- the kernels' arguments and launchers (lcm_map.hip)
struct MapMedianArgs { const uint4* pts; const uint64_t* off; double* median; };
struct MapTriArgs {
    const uint4* pts; const uint64_t* off; const uint8_t* mask;      // mask NULL: every record takes part
    const MapPair* pairs;
    MapTri* tri; uint8_t* status;
    uint32_t* counts;            // MAP_STATUSES words per pair, zeroed by the caller: integer sums, the same whatever the order
    Camera K; MapLimits lim;
};
struct MapMergeArgs {
    const uint4* matches; const uint4* pts; const MapTri* tri; const uint8_t* status;
    int32_t* table1; int32_t* table2;
    int32_t* winner;             // per keypoint of view 2: the largest index of an accepted record that names it, -1 = none
    uint32_t* blk_accepted; uint32_t* blk_new;     // per block of MAP_THREADS records; after the scans their exclusive prefixes
    Point3* points_out; Observation* obs_out; uint8_t* status_out;
    uint32_t n; int32_t kf1, kf2, n_points;
};
hipError_t launch_map_median(const MapMedianArgs& a, uint32_t n_pairs, hipStream_t st);                     // k_map_median
hipError_t launch_map_triangulate(const MapTriArgs& a, uint32_t n_pairs, uint32_t max_n, hipStream_t st);   // k_map_triangulate
hipError_t launch_map_merge_count(const MapMergeArgs& a, hipStream_t st);                                    // k_map_merge_count
hipError_t launch_map_merge_emit(const MapMergeArgs& a, hipStream_t st);                                     // k_map_merge_emit

}  // namespace lcm
