// lcm_ba_host.h — the pure host side of the alternating bundle adjustment (lcm_ba.cpp): parameter and input checks, the plan of one
// observation list (two stable counting sorts: camera -> observations and point -> observations, each ascending, their size
// that of the list), the spread of the camera centres that sets the outlier pass's distance threshold (:1588-1611), and the
// host-only calls (the compaction of :1633-1659, the loop's new observations of :1496-1513).  No HIP call and no handle:
// tests/cpp/ba_host_check.cpp compiles this text into a stand-alone program that runs under a sanitizer.  A check returns
// {0, NULL} or the status and what is wrong.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/lcm.h"
#include "lcm_ba_device.h"
#include "lcm_pgo_host.h"

namespace lcm {

struct BaProblem { int code; const char* what; };        // code: LCM_OK, LCM_ERR_INVALID_ARG or LCM_ERR_CAPACITY
constexpr BaProblem BA_FINE{LCM_OK, nullptr};
constexpr int BA_SECOND_OUTER_ITERS = 3;                 // :1666

inline void ba_params_default(lcm_ba_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->eps = 1e-6; p->damping = 1e-3; p->min_update = 1e-6; p->outlier_px = 5.0; p->min_spread = 10.0; p->spread_factor = 5.0;
    p->outer_iters = 5; p->inner_iters = 5; p->min_cam_obs = 10; p->min_point_obs = 2;
}

// pp is required: the camera matrix has no default
inline const char* ba_params_problem(const lcm_ba_params* pp) {
    if (!pp) return "the parameters are required (fx, fy, cx, cy have no default)";
    if (!(pp->fx > 0.0) || !(pp->fy > 0.0) || !std::isfinite(pp->fx) || !std::isfinite(pp->fy)) return "fx and fy must be finite and > 0";
    if (!std::isfinite(pp->cx) || !std::isfinite(pp->cy)) return "cx and cy must be finite";
    if (!(pp->eps > 0.0) || !std::isfinite(pp->eps)) return "eps must be finite and > 0";
    if (!(pp->damping >= 0.0) || !std::isfinite(pp->damping)) return "damping must be finite and >= 0";
    if (!(pp->min_update >= 0.0) || !std::isfinite(pp->min_update)) return "min_update must be finite and >= 0";
    if (!(pp->outlier_px >= 0.0) || !std::isfinite(pp->outlier_px)) return "outlier_px must be finite and >= 0";
    if (!(pp->min_spread >= 0.0) || !std::isfinite(pp->min_spread)) return "min_spread must be finite and >= 0";
    if (!(pp->spread_factor >= 0.0) || !std::isfinite(pp->spread_factor)) return "spread_factor must be finite and >= 0";
    if (pp->outer_iters < 1 || pp->outer_iters > LCM_BA_MAX_ITERS_PER_LOOP) return "outer_iters must be in [1, 16]";
    if (pp->inner_iters < 1 || pp->inner_iters > LCM_BA_MAX_ITERS_PER_LOOP) return "inner_iters must be in [1, 16]";
    if (pp->min_cam_obs < 0 || pp->min_point_obs < 0) return "min_cam_obs and min_point_obs must be >= 0";
    return nullptr;
}

// decided from the counts, before any buffer is read
inline BaProblem ba_counts_problem(int n_poses, int n_points, int n_obs) {
    if (n_poses < 1 || n_points < 1 || n_obs < 0) return {LCM_ERR_INVALID_ARG, "n_poses and n_points must be >= 1 and n_obs >= 0"};
    if (n_poses > LCM_BA_MAX_CAMERAS) return {LCM_ERR_CAPACITY, "more cameras than LCM_BA_MAX_CAMERAS"};
    if (n_points > LCM_BA_MAX_POINTS) return {LCM_ERR_CAPACITY, "more points than LCM_BA_MAX_POINTS"};
    if (n_obs > LCM_BA_MAX_OBS) return {LCM_ERR_CAPACITY, "more observations than LCM_BA_MAX_OBS"};
    return BA_FINE;
}

// The two tables of one observation list.  cam_obs[cam_off[c] .. cam_off[c + 1]) are the indices of camera c's observations in
// the caller's list, ascending (a stable counting sort); pt_off / pt_obs the same per point.
struct BaPlan {
    int n_cams = 0, n_points = 0, n_obs = 0;
    std::vector<uint32_t> cam_off, cam_obs, pt_off, pt_obs;
};

inline BaProblem ba_plan(const uint8_t* valid, int n_poses, int n_points, const lcm_ba_obs* obs, int n_obs, BaPlan* out) {
    BaPlan& pl = *out;
    pl = BaPlan{};
    pl.n_cams = n_poses; pl.n_points = n_points; pl.n_obs = n_obs;
    pl.cam_off.assign((size_t)n_poses + 1, 0); pl.pt_off.assign((size_t)n_points + 1, 0);
    for (int i = 0; i < n_obs; ++i) {
        const int c = obs[i].cam, p = obs[i].point;
        if (c < 0 || c >= n_poses) return {LCM_ERR_INVALID_ARG, "an observation's camera index is out of range"};
        if (p < 0 || p >= n_points) return {LCM_ERR_INVALID_ARG, "an observation's point index is out of range"};
        if (!pgo_is_valid(valid, c)) return {LCM_ERR_INVALID_ARG, "an observation of an invalid camera"};
        ++pl.cam_off[(size_t)c + 1]; ++pl.pt_off[(size_t)p + 1];
    }
    for (int c = 0; c < n_poses; ++c) pl.cam_off[(size_t)c + 1] += pl.cam_off[(size_t)c];
    for (int p = 0; p < n_points; ++p) pl.pt_off[(size_t)p + 1] += pl.pt_off[(size_t)p];
    pl.cam_obs.assign((size_t)n_obs, 0); pl.pt_obs.assign((size_t)n_obs, 0);
    std::vector<uint32_t> cf(pl.cam_off.begin(), pl.cam_off.end() - 1), pf(pl.pt_off.begin(), pl.pt_off.end() - 1);
    for (int i = 0; i < n_obs; ++i) {
        pl.cam_obs[(size_t)cf[(size_t)obs[i].cam]++] = (uint32_t)i;
        pl.pt_obs[(size_t)pf[(size_t)obs[i].point]++] = (uint32_t)i;
    }
    return BA_FINE;
}

// the values of the valid poses (an invalid pose's contents are not read), of every point and of every observation
inline const char* ba_values_problem(const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points, int n_points,
                                     const lcm_ba_obs* obs, int n_obs) {
    for (int i = 0; i < n_poses; ++i) {
        if (!pgo_is_valid(valid, i)) continue;
        if (const char* what = pgo_rotation_problem(poses[i].R)) return what;
        if (const char* what = pgo_vector_problem(poses[i].t)) return what;
    }
    for (int i = 0; i < n_points; ++i)
        if (!std::isfinite(points[i].x) || !std::isfinite(points[i].y) || !std::isfinite(points[i].z)) return "a point holds a non-finite value";
    for (int i = 0; i < n_obs; ++i)
        if (!std::isfinite(obs[i].u) || !std::isfinite(obs[i].v)) return "an observation holds a non-finite value";
    return nullptr;
}

// what a call over a map refuses, in the order it is looked at: the buffers, the parameters, the counts, the structure
// (-> *plan), the values
inline BaProblem ba_inputs_problem(const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points, int n_points,
                                   const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, BaPlan* plan) {
    if (!poses || !points || (!obs && n_obs != 0)) return {LCM_ERR_INVALID_ARG, "NULL buffer"};
    if (const char* what = ba_params_problem(pp)) return {LCM_ERR_INVALID_ARG, what};
    const BaProblem c = ba_counts_problem(n_poses, n_points, n_obs);
    if (c.what) return c;
    const BaProblem p = ba_plan(valid, n_poses, n_points, obs, n_obs, plan);
    if (p.what) return p;
    if (const char* what = ba_values_problem(poses, valid, n_poses, points, n_points, obs, n_obs)) return {LCM_ERR_INVALID_ARG, what};
    return BA_FINE;
}

// :1588-1611: the centroid of the valid cameras' centres -R^T t, the largest distance of a centre from it, and the threshold
// max(min_spread, spread_factor x that distance).  No valid camera: centroid 0, distance 0.
inline void ba_camera_spread(const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, double min_spread, double spread_factor,
                             double (&centroid)[3], double* threshold) {
#pragma clang fp contract(off)
    int count = 0;
    centroid[0] = centroid[1] = centroid[2] = 0.0;
    auto centre = [&](int i, double (&C)[3]) {
        const double* R = poses[i].R; const double* t = poses[i].t;
        for (int k = 0; k < 3; ++k) C[k] = -(R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2]);
    };
    for (int i = 0; i < n_poses; ++i) {
        if (!pgo_is_valid(valid, i)) continue;
        double C[3];
        centre(i, C);
        for (int k = 0; k < 3; ++k) centroid[k] = centroid[k] + C[k];
        ++count;
    }
    if (count > 0)
        for (int k = 0; k < 3; ++k) centroid[k] = centroid[k] / count;
    double far = 0.0;
    for (int i = 0; i < n_poses; ++i) {
        if (!pgo_is_valid(valid, i)) continue;
        double C[3];
        centre(i, C);
        const double dx = C[0] - centroid[0], dy = C[1] - centroid[1], dz = C[2] - centroid[2];
        const double d = std::sqrt(dx * dx + dy * dy + dz * dz);
        far = d > far ? d : far;
    }
    const double scaled = far * spread_factor;
    *threshold = min_spread < scaled ? scaled : min_spread;
}

// :1633-1659.  The counts; with room (cap_points, cap_obs) also the surviving points in order, the observations of surviving
// points in order with the new index, and old_to_new (n_points entries, -1 for a removed point; may be NULL).
inline void ba_compact_counts(const uint8_t* flags, int n_points, const lcm_ba_obs* obs, int n_obs, int* kept_points, int* kept_obs) {
    int np = 0, no = 0;
    for (int i = 0; i < n_points; ++i) np += flags[i] == 0;
    for (int i = 0; i < n_obs; ++i) no += flags[obs[i].point] == 0;
    *kept_points = np; *kept_obs = no;
}

inline void ba_compact(const lcm_ba_point* points, int n_points, const lcm_ba_obs* obs, int n_obs, const uint8_t* flags,
                       lcm_ba_point* points_out, lcm_ba_obs* obs_out, int32_t* old_to_new) {
    std::vector<int32_t> table((size_t)n_points, -1);
    int np = 0, no = 0;
    for (int i = 0; i < n_points; ++i)
        if (!flags[i]) { table[(size_t)i] = np; points_out[np++] = points[i]; }
    for (int i = 0; i < n_obs; ++i) {
        const int32_t to = table[(size_t)obs[i].point];
        if (to < 0) continue;
        lcm_ba_obs o = obs[i];
        o.point = to;
        obs_out[no++] = o;
    }
    if (old_to_new && n_points > 0) std::memcpy(old_to_new, table.data(), (size_t)n_points * sizeof(int32_t));
}

// :1496-1513.  what is wrong with the lists, or NULL; *n_add = the observations the call would append
inline const char* ba_loop_observations_problem(const lcm_dmatch* matches, const uint8_t* mask, int n_matches, const int32_t* past_table,
                                                int n_past_kp, int n_curr_kp, int n_points, int* n_add) {
    int n = 0;
    for (int k = 0; k < n_matches; ++k) {
        if (!mask[k]) continue;
        const int q = matches[k].query_idx, t = matches[k].train_idx;
        if (q < 0 || q >= n_curr_kp) return "a masked match's query_idx is outside the current frame's keypoints";
        if (t < 0 || t >= n_past_kp) return "a masked match's train_idx is outside the past frame's keypoints";
        const int32_t p = past_table[t];
        if (p < -1 || p >= n_points) return "the past frame's table names a point out of range";
        n += p != -1;
    }
    *n_add = n;
    return nullptr;
}

inline void ba_add_loop_observations(const lcm_dmatch* matches, const uint8_t* mask, int n_matches, const int32_t* past_table,
                                     int32_t* curr_table, const float* curr_kp, int curr, lcm_ba_obs* out) {
    int n = 0;
    for (int k = 0; k < n_matches; ++k) {
        if (!mask[k]) continue;
        const int q = matches[k].query_idx;
        const int32_t p = past_table[matches[k].train_idx];
        if (p == -1) continue;
        lcm_ba_obs o;
        std::memset(&o, 0, sizeof(o));
        o.cam = curr; o.point = p; o.u = (double)curr_kp[2 * (size_t)q]; o.v = (double)curr_kp[2 * (size_t)q + 1];
        out[n++] = o;
        curr_table[q] = p;
    }
}

// the number of elements per status (lcm_ba_info's cameras[] / points[])
inline void ba_count_statuses(const lcm_ba_elem_info* info, int n, int32_t (&count)[5]) {
    for (int k = 0; k < 5; ++k) count[k] = 0;
    for (int i = 0; i < n; ++i)
        if (info[i].status >= 0 && info[i].status < 5) ++count[info[i].status];
}

}  // namespace lcm
