// lcm_lo_host.h — the pure host side of the RANSAC's local optimisation (lcm_lo.cpp): the parameters' defaults and checks,
// the check of a caller's counts, the records of a call that launches nothing.  No HIP call and no handle:
// tests/cpp/lo_host_check.cpp compiles this text into a stand-alone program that runs under a sanitizer.  A check returns
// NULL or what is wrong.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/lcm.h"

namespace lcm {

inline void lo_params_default(lcm_lo_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->rounds = 4; p->seeds = LCM_LO_SEEDS;
    p->mult[0] = 3.0; p->mult[1] = 2.0; p->mult[2] = 1.5; p->mult[3] = 1.0;
}

// NULL is the defaults
inline const char* lo_params_problem(const lcm_lo_params* lp) {
    if (!lp) return nullptr;
    if (lp->rounds < 1 || lp->rounds > 8) return "rounds must be in [1, 8]";
    if (lp->seeds != LCM_LO_SEEDS) return "seeds must be 64";
    for (int r = 0; r < lp->rounds; ++r)
        if (!(lp->mult[r] >= 1.0) || !std::isfinite(lp->mult[r])) return "every round's multiplier must be finite and >= 1";
    return nullptr;
}

inline const char* lo_mult_problem(double mult) {
    return (mult >= 1.0 && std::isfinite(mult)) ? nullptr : "the multiplier must be finite and >= 1";
}

// lcm_lo_select's input: a count is an inlier count of at most 65 535 records
inline const char* lo_counts_problem(const int32_t* counts, int iters) {
    if (iters < 64 || iters > 65536 || iters % 64 != 0) return "iters must be a multiple of 64 in [64, 65536]";
    if (!counts) return "NULL counts";
    for (int it = 0; it < iters; ++it)
        if (counts[it] < 0 || counts[it] > 65535) return "a count must be in [0, 65535]";
    return nullptr;
}

// What the kernels write for pairs without records (a call whose every pair is empty launches nothing)
inline void lo_empty_info(lcm_lo_info* info, size_t n) {
    for (size_t p = 0; p < n; ++p) {
        info[p].seed_iter = 0; info[p].round = -1; info[p].n_inliers_ransac = 0; info[p].status = LCM_LO_TOO_FEW;
    }
}

}  // namespace lcm
