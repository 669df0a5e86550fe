// lcm_map_host.h — the pure host side of the map building before the loop (lcm_map.cpp): parameter and input checks, the per-pair
// plan (camera centres, baseline, the 3 x 4 matrices K [R | t], the cosine of the smallest parallax), the checks of a merge's
// lists, the keyframe gates of src/main.cpp:1156-1194 and the new keyframe's pose (:1217-1218).  No HIP call and no handle:
// tests/cpp/map_host_check.cpp compiles this text into a stand-alone program that runs under a sanitizer.  A check returns
// {0, NULL} or the status and what is wrong.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/lcm.h"
#include "lcm_map_device.h"
#include "lcm_pgo_host.h"

namespace lcm {

struct MapProblem { int code; const char* what; };       // code: LCM_OK, LCM_ERR_INVALID_ARG or LCM_ERR_CAPACITY
constexpr MapProblem MAP_FINE{LCM_OK, nullptr};
constexpr double MAP_PI = 3.14159265358979323846;

inline void map_params_default(lcm_map_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->min_parallax_deg = 1.0; p->max_reproj = 4.0; p->min_depth = 0.1; p->max_depth = 50.0;
    p->min_displacement = 20.0; p->max_displacement = 150.0; p->min_inlier_ratio = 0.3;
    p->min_tracked = 100; p->min_inliers = 50; p->min_pose_inliers = 10;
}

// mp is required: the camera matrix has no default
inline const char* map_params_problem(const lcm_map_params* mp) {
    if (!mp) return "the parameters are required (fx, fy, cx, cy have no default)";
    if (!(mp->fx > 0.0) || !(mp->fy > 0.0) || !std::isfinite(mp->fx) || !std::isfinite(mp->fy)) return "fx and fy must be finite and > 0";
    if (!std::isfinite(mp->cx) || !std::isfinite(mp->cy)) return "cx and cy must be finite";
    if (!(mp->min_parallax_deg >= 0.0) || !(mp->min_parallax_deg <= 180.0)) return "min_parallax_deg must be in [0, 180]";
    if (!(mp->max_reproj >= 0.0)) return "max_reproj must be >= 0";
    if (std::isnan(mp->min_depth) || std::isnan(mp->max_depth)) return "min_depth and max_depth must not be NaN";
    if (std::isnan(mp->min_displacement) || std::isnan(mp->max_displacement)) return "min_displacement and max_displacement must not be NaN";
    if (std::isnan(mp->min_inlier_ratio)) return "min_inlier_ratio must not be NaN";
    if (mp->min_tracked < 0 || mp->min_inliers < 0 || mp->min_pose_inliers < 0) return "min_tracked, min_inliers and min_pose_inliers must be >= 0";
    return nullptr;
}

inline double map_cos_min(double min_parallax_deg) { return std::cos(min_parallax_deg * MAP_PI / 180.0); }

// The offsets of a call walked: decided from the counts, before any record is read.  *total = offsets[n_pairs], *max_n = the
// longest pair.
inline MapProblem map_offsets_problem(const size_t* offsets, int n_pairs, size_t* total, uint32_t* max_n) {
    *total = 0; *max_n = 0;
    if (n_pairs < 0) return {LCM_ERR_INVALID_ARG, "negative pair count"};
    if (n_pairs > LCM_MAP_MAX_PAIRS) return {LCM_ERR_CAPACITY, "more pairs than LCM_MAP_MAX_PAIRS"};
    if (!offsets) return {LCM_ERR_INVALID_ARG, "NULL offsets"};
    if (offsets[0] != 0) return {LCM_ERR_INVALID_ARG, "offsets[0] must be 0"};
    for (int p = 0; p < n_pairs; ++p) {
        if (offsets[p + 1] < offsets[p]) return {LCM_ERR_INVALID_ARG, "offsets must not decrease"};
        if (offsets[p + 1] > (size_t)LCM_MAP_MAX_RECORDS) return {LCM_ERR_CAPACITY, "more records than LCM_MAP_MAX_RECORDS"};
        const size_t n = offsets[p + 1] - offsets[p];
        if (n > *max_n) *max_n = (uint32_t)n;
    }
    *total = offsets[n_pairs];
    return MAP_FINE;
}

inline const char* map_pose_problem(const lcm_pgo_pose& P) {
    if (const char* what = pgo_rotation_problem(P.R)) return what;
    return pgo_vector_problem(P.t);
}

// C = -(R^T t)
inline void map_centre(const lcm_pgo_pose& P, double (&C)[3]) {
#pragma clang fp contract(off)
    for (int k = 0; k < 3; ++k) C[k] = -(P.R[k] * P.t[0] + P.R[3 + k] * P.t[1] + P.R[6 + k] * P.t[2]);
}

// K [R | t] row-major: row 0 = fx row0 + cx row2, row 1 = fy row1 + cy row2, row 2 = row2 (K's zeros add nothing)
inline void map_projection(const lcm_map_params& mp, const lcm_pgo_pose& P, double (&M)[12]) {
#pragma clang fp contract(off)
    for (int j = 0; j < 4; ++j) {
        const double r0 = j < 3 ? P.R[j] : P.t[0], r1 = j < 3 ? P.R[3 + j] : P.t[1], r2 = j < 3 ? P.R[6 + j] : P.t[2];
        M[j] = mp.fx * r0 + mp.cx * r2;
        M[4 + j] = mp.fy * r1 + mp.cy * r2;
        M[8 + j] = r2;
    }
}

// everything the kernel needs of one pair
inline void map_plan_pair(const lcm_map_params& mp, const lcm_pgo_pose& P1, const lcm_pgo_pose& P2, MapPair* out) {
#pragma clang fp contract(off)
    MapPair& q = *out;
    map_projection(mp, P1, q.P1); map_projection(mp, P2, q.P2);
    std::memcpy(q.R1, P1.R, sizeof(q.R1)); std::memcpy(q.t1, P1.t, sizeof(q.t1));
    std::memcpy(q.R2, P2.R, sizeof(q.R2)); std::memcpy(q.t2, P2.t, sizeof(q.t2));
    map_centre(P1, q.C1); map_centre(P2, q.C2);
    const double dx = q.C2[0] - q.C1[0], dy = q.C2[1] - q.C1[1], dz = q.C2[2] - q.C1[2];
    q.baseline = std::sqrt(dx * dx + dy * dy + dz * dz);
    q.cos_min = map_cos_min(mp.min_parallax_deg);
}

// What lcm_map_merge refuses about its lists, in O(n): a status above LCM_MAP_ACCEPTED, an index outside its table, a repeated
// query_idx (among all the records), a table entry outside [-1, n_points).  seen: scratch of n_kp1 bytes.
inline const char* map_merge_problem(const lcm_dmatch* matches, const uint8_t* status, int n, const int32_t* table1, int n_kp1,
                                     const int32_t* table2, int n_kp2, int n_points, std::vector<uint8_t>& seen) {
    seen.assign((size_t)n_kp1, 0);
    for (int i = 0; i < n; ++i) {
        if (status && status[i] > LCM_MAP_ACCEPTED) return "a status byte is above LCM_MAP_ACCEPTED";
        const int q = matches[i].query_idx, t = matches[i].train_idx;
        if (q < 0 || q >= n_kp1) return "a match's query_idx is outside the last keyframe's keypoints";
        if (t < 0 || t >= n_kp2) return "a match's train_idx is outside the new keyframe's keypoints";
        if (seen[(size_t)q]) return "the list names a query_idx twice";
        seen[(size_t)q] = 1;
    }
    for (int k = 0; k < n_kp1; ++k)
        if (table1[k] < -1 || table1[k] >= n_points) return "the last keyframe's table names a point out of range";
    for (int k = 0; k < n_kp2; ++k)
        if (table2[k] < -1 || table2[k] >= n_points) return "the new keyframe's table names a point out of range";
    return nullptr;
}

// the counts a merge will produce, from host lists
inline void map_merge_counts(const lcm_dmatch* matches, const uint8_t* status, int n, const int32_t* table1, int* n_new, int* n_merged) {
    int a = 0, b = 0;
    for (int i = 0; i < n; ++i) {
        if (status[i] != LCM_MAP_ACCEPTED) continue;
        if (table1[matches[i].query_idx] == -1) ++a; else ++b;
    }
    *n_new = a; *n_merged = b;
}

// :1156-1176: the gates that need the list's length and the median alone; LCM_MAP_KEYFRAME = go on
inline int map_motion_verdict(const lcm_map_params& mp, int n_matches, double median) {
    if (n_matches < mp.min_tracked) return LCM_MAP_FEW_MATCHES;
    if (median < mp.min_displacement) return LCM_MAP_LITTLE_MOTION;
    if (median > mp.max_displacement) return LCM_MAP_MUCH_MOTION;
    return LCM_MAP_KEYFRAME;
}

// :576, :595, :611 and :1191-1194 on the pose record of the pair; *n_inliers = countNonZero(inlierMask) = n_good
inline int map_pose_verdict(const lcm_map_params& mp, int n_matches, const lcm_pose_result& pr, int* n_inliers) {
    *n_inliers = 0;
    if (n_matches < 8 || pr.status != LCM_POSE_OK || pr.n_good < mp.min_pose_inliers) return LCM_MAP_NO_POSE;
    *n_inliers = pr.n_good;
    const double ratio = (double)pr.n_good / (double)n_matches;
    if (pr.n_good < mp.min_inliers || ratio < mp.min_inlier_ratio) return LCM_MAP_FEW_INLIERS;
    return LCM_MAP_KEYFRAME;
}

// :1217-1218: R_new = R R_last, t_new = R t_last + t, every row sum left to right
inline void map_new_pose(const lcm_pose_result& pr, const lcm_pgo_pose& last, lcm_pgo_pose* out) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j)
            out->R[3 * i + j] = pr.R[3 * i] * last.R[j] + pr.R[3 * i + 1] * last.R[3 + j] + pr.R[3 * i + 2] * last.R[6 + j];
        out->t[i] = (pr.R[3 * i] * last.t[0] + pr.R[3 * i + 1] * last.t[1] + pr.R[3 * i + 2] * last.t[2]) + pr.t[i];
    }
}

}  // namespace lcm
