// lcm_verify.cpp — the loop verification as one staged pipeline over a lcm::VerifyPlan (lcm_verify_host.h): the RANSAC
// (lcm_epi.cpp), the local optimisation (lcm_lo.cpp) and the pose recovery (lcm_pose.cpp), each enqueued behind the one
// before on the same point records.  The store's list calls (lcm_l2_db.cpp, store_lists) and the host-list calls
// lcm_epi_verify_pairs / lcm_lo_verify_pairs run their plan through verify_enqueue and verify_download; a new stage is a flag
// of the plan and its lines in verify_empty, verify_enqueue and verify_download.  Part of liblcm_hip.so's host side; shared
// state and helpers: lcm_internal.h.
#include "lcm_internal.h"

#include "lcm_epi_device.h"
#include "lcm_lo_device.h"

namespace lcm {

int pair_slices(size_t n_pairs, uint32_t* slices) {
    uint32_t lim = 1;
    const hipError_t e = grid_y_limit(&lim);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "grid limit: %s", hipGetErrorString(e));
    *slices = (uint32_t)((n_pairs + lim - 1) / lim);
    return LCM_OK;
}

int offsets_checked(const size_t* offsets, int n_pairs, size_t* total, uint32_t* max_n) {
    bool capacity = false;
    const char* what = epi_offsets_problem(offsets, n_pairs, EPI_MAX_POINTS, total, max_n, &capacity);
    return what ? fail(capacity ? LCM_ERR_CAPACITY : LCM_ERR_INVALID_ARG, "%s", what) : LCM_OK;
}

int verify_params_checked(VerifyPlan* plan, const lcm_lo_params* lp, const lcm_pose_params* pp) {
    if (plan->pose) { const int rc = pose_params_checked(pp, &plan->pp); if (rc) return rc; }
    return plan->lo ? lo_params_checked(lp, &plan->lp) : LCM_OK;
}

int verify_enqueue(lcm_handle* h, const VerifyPlan& plan, const uint4* d_pts, const uint64_t* d_off, size_t n_pairs, uint32_t max_n,
                   size_t total, uint32_t* launches) {
    uint32_t more = 0;
    int rc = epi_enqueue(h, d_pts, d_off, n_pairs, max_n, total, *plan.ep, launches, plan.lo); if (rc) return rc;
    if (plan.lo) {
        rc = lo_enqueue(h, d_pts, d_off, n_pairs, *plan.ep, plan.lp, &more); if (rc) return rc;
        *launches += more;
    }
    if (plan.pose) {        // on the device's results[].E and the device's mask: the optimised ones behind lo_enqueue
        static_assert(sizeof(lcm_epi_result) == 11 * sizeof(double) && offsetof(lcm_epi_result, E) == 0, "results[].E as a matrix array");
        rc = pose_enqueue(h, d_pts, d_off, n_pairs, total, reinterpret_cast<const double*>(h->epi.d_res), 11, h->epi.d_mask, *plan.ep,
                          plan.pp, &more); if (rc) return rc;
        *launches += more;
    }
    return LCM_OK;
}

int verify_download(lcm_handle* h, const VerifyPlan& plan, size_t n_pairs, size_t total) {
    int rc = epi_download(h, n_pairs, total, plan.results, plan.mask); if (rc) return rc;
    if (plan.lo) { rc = lo_download(h, n_pairs, plan.info); if (rc) return rc; }
    return plan.pose ? pose_download(h, n_pairs, total, plan.pose_results, plan.pose_mask) : LCM_OK;
}

int verify_pairs(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs, VerifyPlan* plan, const lcm_lo_params* lp) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    int rc = epi_params_checked(plan->ep); if (rc) return rc;
    rc = verify_params_checked(plan, lp, nullptr); if (rc) return rc;
    size_t total = 0;
    uint32_t max_n = 0;
    rc = offsets_checked(offsets, n_pairs, &total, &max_n); if (rc) return rc;
    if ((n_pairs > 0 && (!plan->results || (plan->lo && !plan->info))) || (total > 0 && !pts)) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    if (n_pairs == 0) return LCM_OK;
    rc = set_device(h); if (rc) return rc;
    const size_t P = (size_t)n_pairs;
    const uint64_t iters = (uint64_t)plan->ep->iters, lo = plan->lo ? 1 : 0;
    rc = epi_upload_points(h, pts, offsets, P, total); if (rc) return rc;
    uint32_t launches = 0;
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    rc = verify_enqueue(h, *plan, h->epi.d_pts, h->epi.d_off, P, max_n, total, &launches); if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    h->info_pending = true;
    h->info.workgroups = (uint32_t)(P * (size_t)((iters + 255) / 256)); h->info.route = LCM_ROUTE_PLAIN; h->info.launches = launches;
    h->info.pairs = P;
    // the optimisation: 4 passes over the records per seed and round; a count word per hypothesis and an info record per pair
    h->info.distances = (uint64_t)total * (iters + lo * (uint64_t)LO_SEEDS * 4u * (uint64_t)plan->lp.rounds);
    h->info.algo_bytes = total * 17 + P * (iters * (104 + lo * 4) + sizeof(lcm_epi_result) + lo * sizeof(lcm_lo_info));
    rc = verify_download(h, *plan, P, total); if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return LCM_OK;
}

}  // namespace lcm
