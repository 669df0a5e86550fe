// lcm_epi.cpp — the host side of the essential-matrix RANSAC (include/lcm.h, lcm_epi_*): src/main.cpp:1395-1403 over point
// lists.  The kernels are lcm_epi.hip's, the arithmetic lcm_epi_device.h's, the pure checks lcm_epi_host.h's.  The stage runs
// through lcm_verify.cpp's pipeline: lcm_epi_verify_pairs here, the store's forms (lcm_epi_db_*) in lcm_l2_db.cpp beside the list
// kernels whose records they read.
// Part of liblcm_hip.so's host side; shared state and helpers: lcm_internal.h.
#include "lcm_internal.h"

#include "lcm_epi_device.h"

static_assert(sizeof(lcm_epi_result) == 88 && sizeof(lcm::EpiResult) == 88 && sizeof(lcm_epi_params) == 64, "record sizes");
static_assert(offsetof(lcm_epi_result, n_points) == 72 && offsetof(lcm::EpiResult, n_points) == 72 &&
              offsetof(lcm_epi_result, status) == 84 && offsetof(lcm::EpiResult, status) == 84, "record layout");
static_assert(sizeof(lcm_point_pair) == sizeof(uint4) && sizeof(size_t) == sizeof(uint64_t), "record sizes");

namespace lcm {

int epi_params_checked(const lcm_epi_params* ep) {
    const char* what = epi_params_problem(ep);
    return what ? fail(LCM_ERR_INVALID_ARG, "%s", what) : LCM_OK;
}

static EpiArgs epi_args(lcm_handle* h, const uint4* d_pts, const uint64_t* d_off, const lcm_epi_params& ep, uint32_t iters) {
    auto& s = h->epi;
    return EpiArgs{d_pts, d_off, s.d_samples, s.d_E, s.d_best, nullptr, s.d_res, s.d_mask, ep.fx, ep.fy, ep.cx, ep.cy, epi_t2(ep),
                   iters, ep.seed, 0u, 0u};
}

// the hypothesis buffers of n_pairs pairs x iters
static int epi_reserve(lcm_handle* h, size_t n_pairs, size_t iters, size_t total) {
    if (n_pairs * iters > ((size_t)1 << 31)) return fail(LCM_ERR_CAPACITY, "%zu pairs x %zu hypotheses: at most 2^31 per call", n_pairs, iters);
    auto& s = h->epi;
    int rc = ensure_dev(s.d_samples, s.d_samples_n, n_pairs * iters * EPI_SAMPLE); if (rc) return rc;
    rc = ensure_dev(s.d_E, s.d_E_n, n_pairs * iters * 9); if (rc) return rc;
    rc = ensure_dev(s.d_best, s.d_best_n, n_pairs); if (rc) return rc;
    rc = ensure_dev(s.d_res, s.d_res_n, n_pairs); if (rc) return rc;
    return ensure_dev(s.d_mask, s.d_mask_n, total);
}

int epi_enqueue(lcm_handle* h, const uint4* d_pts, const uint64_t* d_off, size_t n_pairs, uint32_t max_n, size_t total,
                const lcm_epi_params& ep, uint32_t* launches, bool want_counts) {
    *launches = 0;
    if (n_pairs == 0) return LCM_OK;
    if (n_pairs > 0x7FFFFFFFull) return fail(LCM_ERR_CAPACITY, "too many pairs for one call");
    int rc = epi_reserve(h, n_pairs, (size_t)ep.iters, total); if (rc) return rc;
    EpiArgs a = epi_args(h, d_pts, d_off, ep, (uint32_t)ep.iters);
    if (want_counts) {
        rc = ensure_dev(h->epi.d_counts, h->epi.d_counts_n, n_pairs * (size_t)ep.iters); if (rc) return rc;
        a.counts = h->epi.d_counts;
    }
    HIP_TRY(hipMemsetAsync(a.best, 0, n_pairs * sizeof(uint32_t), h->stream));
    hipError_t e = launch_epi_solve(a, (uint32_t)n_pairs, h->stream);
    if (e == hipSuccess) e = launch_epi_score(a, (uint32_t)n_pairs, h->stream);
    if (e == hipSuccess) e = launch_epi_mask(a, (uint32_t)n_pairs, max_n, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "RANSAC kernels: launch failed: %s", hipGetErrorString(e));
    uint32_t slices = 0;
    rc = pair_slices(n_pairs, &slices); if (rc) return rc;
    *launches = 3u * slices;
    return LCM_OK;
}

int epi_download(lcm_handle* h, size_t n_pairs, size_t total, lcm_epi_result* results, uint8_t* mask) {
    if (n_pairs) HIP_TRY(hipMemcpyAsync(results, h->epi.d_res, n_pairs * sizeof(lcm_epi_result), hipMemcpyDeviceToHost, h->stream));
    if (mask && total) HIP_TRY(hipMemcpyAsync(mask, h->epi.d_mask, total, hipMemcpyDeviceToHost, h->stream));
    return LCM_OK;
}

// A host call's records and offsets -> h->epi.d_pts / d_off, enqueued (the sources are pageable: the caller waits)
int epi_upload_points(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, size_t n_pairs, size_t total) {
    auto& s = h->epi;
    int rc = ensure_dev(s.d_pts, s.d_pts_n, total); if (rc) return rc;
    rc = ensure_dev(s.d_off, s.d_off_n, n_pairs + 1); if (rc) return rc;
    if (total) HIP_TRY(hipMemcpyAsync(s.d_pts, pts, total * sizeof(uint4), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(s.d_off, offsets, (n_pairs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    return LCM_OK;
}

}  // namespace lcm

namespace {
using lcm::epi_upload_points;

// what the two seams check alike; one pair of n records at h->epi.d_pts / d_off on return
int seam_pair(lcm_handle* h, const lcm_point_pair* pts, int n, const lcm_epi_params* ep) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    int rc = lcm::epi_params_checked(ep); if (rc) return rc;
    if (n < 0 || (n > 0 && !pts)) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if ((uint32_t)n > lcm::EPI_MAX_POINTS) return fail(LCM_ERR_CAPACITY, "a pair holds at most %u point records", lcm::EPI_MAX_POINTS);
    return set_device(h);
}

int epi_hypotheses_impl(lcm_handle* h, const lcm_point_pair* pts, int n, uint32_t pair_index, const lcm_epi_params* ep,
                        int32_t* samples, double* E) {
    int rc = seam_pair(h, pts, n, ep); if (rc) return rc;
    if (!samples || !E) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    const size_t offsets[2] = {0, (size_t)n}, iters = (size_t)ep->iters;
    rc = epi_upload_points(h, pts, offsets, 1, (size_t)n); if (rc) return rc;
    rc = lcm::epi_reserve(h, 1, iters, (size_t)n); if (rc) return rc;
    lcm::EpiArgs a = lcm::epi_args(h, h->epi.d_pts, h->epi.d_off, *ep, (uint32_t)iters);
    a.pair_seed0 = pair_index;
    const hipError_t e = lcm::launch_epi_solve(a, 1, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "solver kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(samples, a.samples, iters * lcm::EPI_SAMPLE * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(E, a.E, iters * 9 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return LCM_OK;
}

int epi_score_models_impl(lcm_handle* h, const lcm_point_pair* pts, int n, const double* E, int n_models, const lcm_epi_params* ep,
                          int32_t* counts) {
    int rc = seam_pair(h, pts, n, ep); if (rc) return rc;
    if (n_models < 1 || (uint32_t)n_models > lcm::EPI_MAX_ITERS) return fail(LCM_ERR_INVALID_ARG, "n_models must be in [1, %u]", lcm::EPI_MAX_ITERS);
    if (!E || !counts) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    const size_t offsets[2] = {0, (size_t)n}, padded = ((size_t)n_models + 63) / 64 * 64;      // whole waves: the pad scores zero matrices
    rc = epi_upload_points(h, pts, offsets, 1, (size_t)n); if (rc) return rc;
    rc = lcm::epi_reserve(h, 1, padded, (size_t)n); if (rc) return rc;
    rc = ensure_dev(h->epi.d_counts, h->epi.d_counts_n, padded); if (rc) return rc;
    lcm::EpiArgs a = lcm::epi_args(h, h->epi.d_pts, h->epi.d_off, *ep, (uint32_t)padded);
    a.counts = h->epi.d_counts;
    HIP_TRY(hipMemsetAsync(a.E, 0, padded * 9 * sizeof(double), h->stream));
    HIP_TRY(hipMemcpyAsync(a.E, E, (size_t)n_models * 9 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(a.best, 0, sizeof(uint32_t), h->stream));
    const hipError_t e = lcm::launch_epi_score(a, 1, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "scoring kernel launch failed: %s", hipGetErrorString(e));
    static_assert(sizeof(int32_t) == sizeof(uint32_t), "counts");
    HIP_TRY(hipMemcpyAsync(counts, a.counts, (size_t)n_models * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return LCM_OK;
}

}  // namespace

extern "C" {

void lcm_epi_params_default(lcm_epi_params* p) { if (p) lcm::epi_params_default(p); }
int lcm_epi_loop_test(const lcm_epi_result* r, const lcm_epi_params* ep) { return lcm::epi_loop_test(r, ep); }
int lcm_epi_verify_pairs(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs, const lcm_epi_params* ep,
                         lcm_epi_result* results, uint8_t* mask) {
    return guarded([&] {
        lcm::VerifyPlan plan{ep, false, false, results, mask};
        return lcm::verify_pairs(h, pts, offsets, n_pairs, &plan, nullptr);
    });
}
int lcm_epi_hypotheses(lcm_handle* h, const lcm_point_pair* pts, int n, uint32_t pair_index, const lcm_epi_params* ep, int32_t* samples,
                       double* E) {
    return guarded([&] { return epi_hypotheses_impl(h, pts, n, pair_index, ep, samples, E); });
}
int lcm_epi_score_models(lcm_handle* h, const lcm_point_pair* pts, int n, const double* E, int n_models, const lcm_epi_params* ep,
                         int32_t* counts) {
    return guarded([&] { return epi_score_models_impl(h, pts, n, E, n_models, ep, counts); });
}

}  // extern "C"
