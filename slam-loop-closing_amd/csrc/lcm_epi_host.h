// lcm_epi_host.h — the pure host side of the essential-matrix RANSAC (lcm_epi.cpp): parameter checks, the loop verdict, the
// walk over a call's offsets, the records of a call that launches nothing.  No HIP call and no handle: tests/cpp/epi_host_check.cpp
// compiles this text into a stand-alone program that runs under a sanitizer.  A check returns NULL or what is wrong.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/lcm.h"

namespace lcm {

inline void epi_params_default(lcm_epi_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->threshold = 1.0; p->min_ratio = 0.6; p->iters = 1024; p->min_inliers = 200; p->seed = 0;
}

inline const char* epi_params_problem(const lcm_epi_params* ep) {
    if (!ep) return "NULL lcm_epi_params (the camera matrix has no default)";
    if (!(ep->fx > 0.0) || !(ep->fy > 0.0) || !std::isfinite(ep->fx) || !std::isfinite(ep->fy)) return "fx and fy must be finite and > 0";
    if (!std::isfinite(ep->cx) || !std::isfinite(ep->cy)) return "cx and cy must be finite";
    if (!(ep->threshold >= 0.0) || !std::isfinite(ep->threshold)) return "threshold must be finite and >= 0";
    if (std::isnan(ep->min_ratio)) return "min_ratio must be a number";
    if (ep->iters < 64 || ep->iters > 65536 || ep->iters % 64 != 0) return "iters must be a multiple of 64 in [64, 65536]";
    return nullptr;
}

// OpenCV's scaling of the pixel threshold into normalised coordinates, squared
inline double epi_t2(const lcm_epi_params& ep) {
    const double t = ep.threshold / ((ep.fx + ep.fy) / 2.0);
    return t * t;
}

// src/main.cpp:1403, first two clauses: both comparisons strict
inline int epi_loop_test(const lcm_epi_result* r, const lcm_epi_params* ep) {
    if (!r || !ep || r->n_points <= 0) return 0;
    return r->n_inliers > ep->min_inliers && (double)r->n_inliers / (double)r->n_points > ep->min_ratio;
}

// offsets[0] == 0, non-decreasing, at most max_points records per pair: *total = offsets[n_pairs], *max_n = the longest pair
inline const char* epi_offsets_problem(const size_t* offsets, int n_pairs, size_t max_points, size_t* total, uint32_t* max_n, bool* capacity) {
    *total = 0; *max_n = 0; *capacity = false;
    if (n_pairs < 0) return "negative pair count";
    if (!offsets) return "NULL offsets";
    if (offsets[0] != 0) return "offsets[0] must be 0";
    for (int p = 0; p < n_pairs; ++p) {
        if (offsets[p + 1] < offsets[p]) return "offsets must not decrease";
        const size_t n = offsets[p + 1] - offsets[p];
        if (n > max_points) { *capacity = true; return "a pair holds at most 65535 point records"; }
        if (n > *max_n) *max_n = (uint32_t)n;
    }
    *total = offsets[n_pairs];
    return nullptr;
}

// What the kernels write for pairs without records (a call whose every pair is empty launches nothing)
inline void epi_empty_results(lcm_epi_result* results, size_t n) {
    for (size_t p = 0; p < n; ++p) {
        std::memset(&results[p], 0, sizeof(lcm_epi_result));
        results[p].status = LCM_EPI_TOO_FEW;
    }
}

}  // namespace lcm
