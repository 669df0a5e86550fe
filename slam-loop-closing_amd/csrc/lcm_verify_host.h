// lcm_verify_host.h — the loop verification's plan and its pure host side (lcm_verify.cpp): which stages a call runs, where
// their outputs go, what the call must be given, the records of a call that launches nothing.  No HIP call and no handle:
// tests/cpp/verify_host_check.cpp compiles this text into a stand-alone program that runs under a sanitizer.  A check returns
// NULL or what is wrong.
#pragma once
#include "lcm_epi_host.h"
#include "lcm_lo_host.h"
#include "lcm_pose_host.h"

namespace lcm {

// One call's verification: the RANSAC always, then the local optimisation (lo) and the pose recovery (pose) where wanted.
// ep is the caller's pointer: when it is checked decides the order of a call's refusals, so verify_plan_problem does it.
// lp / pp are checked copies, the defaults for NULL (verify_params_checked); they mean nothing for a stage that is off.
struct VerifyPlan {
    const lcm_epi_params* ep;
    bool lo, pose;
    lcm_epi_result* results; uint8_t* mask;                                    // the RANSAC's (optimised) records and inlier mask
    lcm_lo_info* info = nullptr;                                               // lo
    lcm_pose_result* pose_results = nullptr; uint8_t* pose_mask = nullptr;     // pose
    lcm_lo_params lp{};
    lcm_pose_params pp{};
};

// What a store call with a plan refuses: bad RANSAC parameters, then a missing buffer among those that n_outputs records per
// stage need (n_outputs: the call's pairs, or the room for candidates; the masks are optional).  pts: the call's point pairs.
inline const char* verify_plan_problem(const VerifyPlan& plan, const void* pts, size_t n_outputs) {
    if (const char* what = epi_params_problem(plan.ep)) return what;
    if (!pts || (n_outputs > 0 && !plan.results)) return "the verification needs pts and results";
    if (plan.pose && n_outputs > 0 && !plan.pose_results) return "the pose recovery needs pose_results";
    if (plan.lo && n_outputs > 0 && !plan.info) return "the optimisation needs info";
    return nullptr;
}

// What the stages' kernels write for pairs without records (a call whose every pair is empty launches nothing)
inline void verify_empty(const VerifyPlan& plan, size_t n_pairs) {
    epi_empty_results(plan.results, n_pairs);
    if (plan.lo) lo_empty_info(plan.info, n_pairs);
    if (plan.pose) pose_empty_results(plan.pose_results, n_pairs);
}

}  // namespace lcm
