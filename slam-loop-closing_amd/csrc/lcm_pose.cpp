// lcm_pose.cpp — the host side of the relative-pose recovery (include/lcm.h, lcm_pose_*): src/main.cpp:1405-1421 over point
// lists.  The kernel is lcm_pose.hip's, the arithmetic lcm_pose_device.h's, the pure checks and the choice of the best loop
// lcm_pose_host.h's.  The store's forms (lcm_pose_db_*) live in lcm_l2_db.cpp beside the RANSAC whose records they read; there the
// stage runs through lcm_verify.cpp's pipeline.  Part of liblcm_hip.so's host side; shared state and helpers: lcm_internal.h.
#include "lcm_internal.h"

#include "lcm_epi_device.h"
#include "lcm_pose_device.h"

static_assert(sizeof(lcm_pose_result) == 128 && sizeof(lcm::PoseResult) == 128 && sizeof(lcm_pose_params) == 32, "record sizes");
static_assert(offsetof(lcm_pose_result, t) == 72 && offsetof(lcm::PoseResult, t) == 72 && offsetof(lcm_pose_result, counts) == 96 &&
              offsetof(lcm::PoseResult, counts) == 96 && offsetof(lcm_pose_result, n_used) == 112 && offsetof(lcm::PoseResult, n_used) == 112 &&
              offsetof(lcm_pose_result, status) == 124 && offsetof(lcm::PoseResult, status) == 124, "record layout");
static_assert(sizeof(lcm_epi_result) == 11 * sizeof(double) && offsetof(lcm_epi_result, E) == 0, "the RANSAC's records as a matrix array");

namespace lcm {

int pose_params_checked(const lcm_pose_params* pp, lcm_pose_params* out) {
    if (const char* what = pose_params_problem(pp)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    if (pp) *out = *pp; else pose_params_default(out);
    return LCM_OK;
}

static PoseArgs pose_args(lcm_handle* h, const uint4* d_pts, const uint64_t* d_off, const double* d_E, uint32_t e_stride,
                          const uint8_t* d_mask_in, const lcm_epi_params& ep, const lcm_pose_params& pp) {
    return PoseArgs{d_pts, d_off, d_E, e_stride, d_mask_in, h->pose.d_res, h->pose.d_mask, nullptr, nullptr,
                    ep.fx, ep.fy, ep.cx, ep.cy, pp.max_depth, 0u};
}

static int pose_launch(lcm_handle* h, const PoseArgs& a, size_t n_pairs, uint32_t* launches) {
    const hipError_t e = launch_pose_recover(a, (uint32_t)n_pairs, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "pose kernel launch failed: %s", hipGetErrorString(e));
    return pair_slices(n_pairs, launches);
}

int pose_enqueue(lcm_handle* h, const uint4* d_pts, const uint64_t* d_off, size_t n_pairs, size_t total, const double* d_E,
                 uint32_t e_stride, const uint8_t* d_mask_in, const lcm_epi_params& ep, const lcm_pose_params& pp, uint32_t* launches) {
    *launches = 0;
    if (n_pairs == 0) return LCM_OK;
    if (n_pairs > 0x7FFFFFFFull) return fail(LCM_ERR_CAPACITY, "too many pairs for one call");
    auto& s = h->pose;
    int rc = ensure_dev(s.d_res, s.d_res_n, n_pairs); if (rc) return rc;
    rc = ensure_dev(s.d_mask, s.d_mask_n, total); if (rc) return rc;
    return pose_launch(h, pose_args(h, d_pts, d_off, d_E, e_stride, d_mask_in, ep, pp), n_pairs, launches);
}

int pose_download(lcm_handle* h, size_t n_pairs, size_t total, lcm_pose_result* results, uint8_t* mask) {
    if (n_pairs) HIP_TRY(hipMemcpyAsync(results, h->pose.d_res, n_pairs * sizeof(lcm_pose_result), hipMemcpyDeviceToHost, h->stream));
    if (mask && total) HIP_TRY(hipMemcpyAsync(mask, h->pose.d_mask, total, hipMemcpyDeviceToHost, h->stream));
    return LCM_OK;
}

}  // namespace lcm

namespace {

int pose_recover_pairs_impl(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs, const double* E,
                            const uint8_t* mask_in, const lcm_epi_params* ep, const lcm_pose_params* pp_in, lcm_pose_result* results,
                            uint8_t* mask_out) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (const char* what = lcm::pose_camera_problem(ep)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    lcm_pose_params pp;
    int rc = lcm::pose_params_checked(pp_in, &pp); if (rc) return rc;
    size_t total = 0;
    uint32_t max_n = 0;
    rc = lcm::offsets_checked(offsets, n_pairs, &total, &max_n); if (rc) return rc;
    if ((n_pairs > 0 && (!results || !E)) || (total > 0 && !pts)) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    if (n_pairs == 0) return LCM_OK;
    rc = set_device(h); if (rc) return rc;
    const size_t P = (size_t)n_pairs;
    auto& s = h->pose;
    rc = lcm::epi_upload_points(h, pts, offsets, P, total); if (rc) return rc;
    rc = ensure_dev(s.d_E, s.d_E_n, P * 9); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(s.d_E, E, P * 9 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (mask_in && total) {
        rc = ensure_dev(s.d_mask_in, s.d_mask_in_n, total); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(s.d_mask_in, mask_in, total, hipMemcpyHostToDevice, h->stream));
    }
    uint32_t launches = 0;
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    rc = lcm::pose_enqueue(h, h->epi.d_pts, h->epi.d_off, P, total, s.d_E, 9, mask_in ? s.d_mask_in : nullptr, *ep, pp, &launches);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    h->info_pending = true;
    h->info.workgroups = (uint32_t)P; h->info.route = LCM_ROUTE_PLAIN; h->info.launches = launches;
    h->info.pairs = P; h->info.distances = (uint64_t)total * 5;       // depth tests: four in the first pass, one in the second
    h->info.algo_bytes = total * 34 + P * (9 * sizeof(double) + sizeof(lcm_pose_result));
    rc = lcm::pose_download(h, P, total, results, mask_out); if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return LCM_OK;
}

int pose_candidates_impl(lcm_handle* h, const double* E, int n_models, double* R4, double* t4, int32_t* status) {
    if (!h || n_models < 0) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (n_models > 0 && (!E || !R4 || !t4 || !status)) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    if (n_models == 0) return LCM_OK;
    int rc = set_device(h); if (rc) return rc;
    const size_t P = (size_t)n_models;
    auto& s = h->pose;
    rc = ensure_dev(s.d_E, s.d_E_n, P * 9); if (rc) return rc;
    rc = ensure_dev(s.d_cand, s.d_cand_n, P * 48); if (rc) return rc;
    rc = ensure_dev(s.d_res, s.d_res_n, P); if (rc) return rc;
    rc = ensure_dev(s.d_mask, s.d_mask_n, 0); if (rc) return rc;
    rc = ensure_dev(h->epi.d_off, h->epi.d_off_n, P + 1); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(s.d_E, E, P * 9 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(h->epi.d_off, 0, (P + 1) * sizeof(uint64_t), h->stream));      // no records: the decomposition alone
    lcm_epi_params unit{};
    unit.fx = unit.fy = 1.0;
    lcm_pose_params pp;
    lcm::pose_params_default(&pp);
    lcm::PoseArgs a = lcm::pose_args(h, nullptr, h->epi.d_off, s.d_E, 9, nullptr, unit, pp);
    a.cand_R = s.d_cand; a.cand_t = s.d_cand + P * 36;
    uint32_t launches = 0;
    rc = lcm::pose_launch(h, a, P, &launches); if (rc) return rc;
    std::vector<lcm_pose_result> res(P);
    HIP_TRY(hipMemcpyAsync(R4, a.cand_R, P * 36 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(t4, a.cand_t, P * 12 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(res.data(), s.d_res, P * sizeof(lcm_pose_result), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t m = 0; m < P; ++m) status[m] = res[m].status;
    return LCM_OK;
}

}  // namespace

extern "C" {

void lcm_pose_params_default(lcm_pose_params* p) { if (p) lcm::pose_params_default(p); }
int lcm_pose_loop_test(const lcm_epi_result* er, const lcm_pose_result* pr, const lcm_epi_params* ep, const lcm_pose_params* pp) {
    return lcm::pose_loop_test(er, pr, ep, pp);
}
int lcm_pose_best(const lcm_epi_result* epi_results, const lcm_pose_result* pose_results, int n, const lcm_epi_params* ep,
                  const lcm_pose_params* pp, int floor_inliers, int* best) {
    if (!best || n < 0 || !ep || (n > 0 && (!epi_results || !pose_results))) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (const char* what = lcm::pose_params_problem(pp)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    *best = lcm::pose_best(epi_results, pose_results, (size_t)n, ep, pp, floor_inliers);
    return LCM_OK;
}
int lcm_pose_recover_pairs(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs, const double* E,
                           const uint8_t* mask_in, const lcm_epi_params* ep, const lcm_pose_params* pp, lcm_pose_result* results,
                           uint8_t* mask_out) {
    return guarded([&] { return pose_recover_pairs_impl(h, pts, offsets, n_pairs, E, mask_in, ep, pp, results, mask_out); });
}
int lcm_pose_candidates(lcm_handle* h, const double* E, int n_models, double* R4, double* t4, int32_t* status) {
    return guarded([&] { return pose_candidates_impl(h, E, n_models, R4, t4, status); });
}

}  // extern "C"
