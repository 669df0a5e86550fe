// lcm_lo.cpp — the host side of the RANSAC's local optimisation (include/lcm.h, lcm_lo_*): the refit of the 64 best
// hypotheses on their inliers, between the RANSAC (lcm_epi.cpp) and the pose recovery (lcm_pose.cpp).  The kernels are
// lcm_lo.hip's, the arithmetic lcm_lo_device.h's, the pure checks lcm_lo_host.h's.  The stage runs through lcm_verify.cpp's
// pipeline: lcm_lo_verify_pairs here, the store's forms (lcm_lo_db_*) in lcm_l2_db.cpp.  Part of liblcm_hip.so's host side;
// shared state and helpers: lcm_internal.h.
#include "lcm_internal.h"

#include "lcm_lo_device.h"

static_assert(sizeof(lcm_lo_info) == 16 && sizeof(lcm::LoInfo) == 16 && sizeof(lcm_lo_params) == 96, "record sizes");
static_assert(offsetof(lcm_lo_info, round) == 4 && offsetof(lcm::LoInfo, round) == 4 && offsetof(lcm_lo_info, status) == 12 &&
              offsetof(lcm::LoInfo, status) == 12 && offsetof(lcm_lo_params, mult) == 8, "record layout");
static_assert(LCM_LO_SEEDS == lcm::LO_SEEDS && LCM_LO_OK == lcm::LO_OK && LCM_LO_TOO_FEW == lcm::LO_TOO_FEW &&
              LCM_LO_DEGENERATE == lcm::LO_DEGENERATE && LCM_LO_NO_MODEL == lcm::LO_NO_MODEL && (int)LCM_LO_TOO_FEW == (int)LCM_EPI_TOO_FEW,
              "the header's constants are the device's");

namespace lcm {

int lo_params_checked(const lcm_lo_params* lp, lcm_lo_params* out) {
    if (const char* what = lo_params_problem(lp)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    if (lp) *out = *lp; else lo_params_default(out);
    return LCM_OK;
}

static LoArgs lo_args(lcm_handle* h, const uint4* d_pts, const uint64_t* d_off, const lcm_epi_params& ep, uint32_t iters) {
    LoArgs a{};
    a.pts = d_pts; a.offsets = d_off; a.E = h->epi.d_E; a.counts = h->epi.d_counts; a.seeds = h->lo.d_seeds;
    a.results = h->epi.d_res; a.mask = h->epi.d_mask; a.info = h->lo.d_info;
    a.fx = ep.fx; a.fy = ep.fy; a.cx = ep.cx; a.cy = ep.cy; a.t = ep.threshold / ((ep.fx + ep.fy) / 2.0);      // epi_t2's t
    a.iters = iters; a.rounds = 1;
    return a;
}

int lo_enqueue(lcm_handle* h, const uint4* d_pts, const uint64_t* d_off, size_t n_pairs, const lcm_epi_params& ep,
               const lcm_lo_params& lp, uint32_t* launches) {
    *launches = 0;
    if (n_pairs == 0) return LCM_OK;
    auto& s = h->lo;
    int rc = ensure_dev(s.d_seeds, s.d_seeds_n, n_pairs * LO_SEEDS); if (rc) return rc;
    rc = ensure_dev(s.d_info, s.d_info_n, n_pairs); if (rc) return rc;
    LoArgs a = lo_args(h, d_pts, d_off, ep, (uint32_t)ep.iters);
    a.rounds = (uint32_t)lp.rounds;
    for (int r = 0; r < LO_MAX_ROUNDS; ++r) a.mult[r] = r < lp.rounds ? lp.mult[r] : 1.0;
    hipError_t e = launch_lo_select(a, (uint32_t)n_pairs, h->stream);
    if (e == hipSuccess) e = launch_lo_refine(a, (uint32_t)n_pairs, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "optimisation kernels: launch failed: %s", hipGetErrorString(e));
    uint32_t slices = 0;
    rc = pair_slices(n_pairs, &slices); if (rc) return rc;
    *launches = 2u * slices;
    return LCM_OK;
}

int lo_download(lcm_handle* h, size_t n_pairs, lcm_lo_info* info) {
    if (n_pairs) HIP_TRY(hipMemcpyAsync(info, h->lo.d_info, n_pairs * sizeof(lcm_lo_info), hipMemcpyDeviceToHost, h->stream));
    return LCM_OK;
}

}  // namespace lcm

namespace {

int lo_select_impl(lcm_handle* h, const int32_t* counts, int iters, int32_t* seeds_out) {
    if (!h || !seeds_out) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (const char* what = lcm::lo_counts_problem(counts, iters)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    int rc = set_device(h); if (rc) return rc;
    rc = ensure_dev(h->epi.d_counts, h->epi.d_counts_n, (size_t)iters); if (rc) return rc;
    rc = ensure_dev(h->lo.d_seeds, h->lo.d_seeds_n, (size_t)lcm::LO_SEEDS); if (rc) return rc;
    static_assert(sizeof(int32_t) == sizeof(uint32_t), "counts");
    HIP_TRY(hipMemcpyAsync(h->epi.d_counts, counts, (size_t)iters * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    lcm::LoArgs a{};
    a.counts = h->epi.d_counts; a.seeds = h->lo.d_seeds; a.iters = (uint32_t)iters;
    const hipError_t e = lcm::launch_lo_select(a, 1, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "selection kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(seeds_out, a.seeds, (size_t)lcm::LO_SEEDS * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return LCM_OK;
}

int lo_refit_models_impl(lcm_handle* h, const lcm_point_pair* pts, int n, const double* E_in, int n_models, double mult,
                         const lcm_epi_params* ep, double* E_out, int32_t* n_selected, int32_t* status) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    int rc = lcm::epi_params_checked(ep); if (rc) return rc;
    if (const char* what = lcm::lo_mult_problem(mult)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    if (n < 0 || (n > 0 && !pts)) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if ((uint32_t)n > lcm::EPI_MAX_POINTS) return fail(LCM_ERR_CAPACITY, "a pair holds at most %u point records", lcm::EPI_MAX_POINTS);
    if (n_models < 1 || n_models > lcm::LO_SEEDS) return fail(LCM_ERR_INVALID_ARG, "n_models must be in [1, %d]", lcm::LO_SEEDS);
    if (!E_in || !E_out || !n_selected || !status) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    rc = set_device(h); if (rc) return rc;
    const size_t offsets[2] = {0, (size_t)n}, M = (size_t)n_models, S = (size_t)lcm::LO_SEEDS;
    auto& s = h->lo;
    rc = lcm::epi_upload_points(h, pts, offsets, 1, (size_t)n); if (rc) return rc;
    rc = ensure_dev(s.d_models, s.d_models_n, 2 * S * 9); if (rc) return rc;
    rc = ensure_dev(s.d_seam, s.d_seam_n, 2 * S); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(s.d_models, E_in, M * 9 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    lcm::LoArgs a = lcm::lo_args(h, h->epi.d_pts, h->epi.d_off, *ep, (uint32_t)S);
    a.E = s.d_models; a.counts = nullptr; a.seeds = nullptr; a.results = nullptr; a.mask = nullptr; a.info = nullptr;
    a.refit_E = s.d_models + S * 9; a.refit_n = s.d_seam; a.refit_status = s.d_seam + S;
    a.n_models = (uint32_t)n_models; a.mult[0] = mult;
    const hipError_t e = lcm::launch_lo_refine(a, 1, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "refinement kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(E_out, a.refit_E, M * 9 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(n_selected, a.refit_n, M * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(status, a.refit_status, M * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return LCM_OK;
}

}  // namespace

extern "C" {

void lcm_lo_params_default(lcm_lo_params* p) { if (p) lcm::lo_params_default(p); }
int lcm_lo_verify_pairs(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs, const lcm_epi_params* ep,
                        const lcm_lo_params* lp, lcm_epi_result* results, lcm_lo_info* info, uint8_t* mask) {
    return guarded([&] {
        lcm::VerifyPlan plan{ep, true, false, results, mask, info};
        return lcm::verify_pairs(h, pts, offsets, n_pairs, &plan, lp);
    });
}
int lcm_lo_select(lcm_handle* h, const int32_t* counts, int iters, int32_t* seeds_out) {
    return guarded([&] { return lo_select_impl(h, counts, iters, seeds_out); });
}
int lcm_lo_refit_models(lcm_handle* h, const lcm_point_pair* pts, int n, const double* E_in, int n_models, double mult,
                        const lcm_epi_params* ep, double* E_out, int32_t* n_selected, int32_t* status) {
    return guarded([&] { return lo_refit_models_impl(h, pts, n, E_in, n_models, mult, ep, E_out, n_selected, status); });
}

}  // extern "C"
