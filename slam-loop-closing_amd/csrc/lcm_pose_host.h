// lcm_pose_host.h — the pure host side of the relative-pose recovery (lcm_pose.cpp): parameter checks, the pose verdict, the
// choice of the best loop among a call's candidates, the records of a call that launches nothing.  No HIP call and no handle:
// tests/cpp/pose_host_check.cpp compiles this text into a stand-alone program that runs under a sanitizer.  A check returns
// NULL or what is wrong.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "lcm_epi_host.h"

namespace lcm {

inline void pose_params_default(lcm_pose_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->max_depth = 50.0; p->min_pose_inliers = 100;
}

inline const char* pose_params_problem(const lcm_pose_params* pp) {
    if (pp && !(pp->max_depth > 0.0)) return "max_depth must be a number > 0";      // also NaN
    return nullptr;                                                                // NULL: the defaults
}

// what lcm_pose_recover_pairs needs of lcm_epi_params: the camera matrix
inline const char* pose_camera_problem(const lcm_epi_params* ep) {
    if (!ep) return "NULL lcm_epi_params (the camera matrix has no default)";
    if (!(ep->fx > 0.0) || !(ep->fy > 0.0) || !std::isfinite(ep->fx) || !std::isfinite(ep->fy)) return "fx and fy must be finite and > 0";
    if (!std::isfinite(ep->cx) || !std::isfinite(ep->cy)) return "cx and cy must be finite";
    return nullptr;
}

// src/main.cpp:1403 (first two clauses) and :1409: every comparison strict
inline int pose_loop_test(const lcm_epi_result* er, const lcm_pose_result* pr, const lcm_epi_params* ep, const lcm_pose_params* pp) {
    if (!pr || pr->status != LCM_POSE_OK) return 0;
    const int32_t limit = pp ? pp->min_pose_inliers : 100;
    return epi_loop_test(er, ep) && pr->n_good > limit;
}

// The reference's globalBest* update over n candidates walked in order: the index of the candidate with the largest
// n_inliers > floor_inliers among those that pass pose_loop_test, among equals the lowest; -1 when there is none.  A
// candidate that fails the pose test does not raise the maximum.
inline int pose_best(const lcm_epi_result* er, const lcm_pose_result* pr, size_t n, const lcm_epi_params* ep, const lcm_pose_params* pp,
                     int floor_inliers) {
    int best = -1;
    long long most = floor_inliers;
    for (size_t c = 0; c < n; ++c) {
        if ((long long)er[c].n_inliers > most && pose_loop_test(&er[c], &pr[c], ep, pp)) {
            most = er[c].n_inliers;
            best = (int)c;
        }
    }
    return best;
}

// What the kernel writes for pairs without a model (a call whose every pair is empty launches nothing)
inline void pose_empty_results(lcm_pose_result* results, size_t n) {
    for (size_t p = 0; p < n; ++p) {
        std::memset(&results[p], 0, sizeof(lcm_pose_result));
        results[p].choice = -1;
        results[p].status = LCM_POSE_NO_MODEL;
    }
}

}  // namespace lcm
