// lcm_ba.cpp — the host side of the alternating bundle adjustment and the outlier removal (include/lcm.h, lcm_ba_*):
// src/main.cpp:1494-1669.  The kernels are lcm_ba.hip's, the arithmetic lcm_ba_device.h's, the checks, the plan and the host-only
// calls lcm_ba_host.h's.  Here: the staging of one map, the launches of a run (every phase of every outer iteration enqueued back
// to back, every decision on the device), the download, and the C exports.  Part of liblcm_hip.so's host side; shared state and
// helpers: lcm_internal.h.
#include "lcm_internal.h"

#include "lcm_ba_host.h"

static_assert(sizeof(lcm_ba_point) == 24 && sizeof(lcm::Point3) == 24 && sizeof(lcm_ba_obs) == 24 && sizeof(lcm::Observation) == 24 &&
              sizeof(lcm_ba_elem_info) == 24 && sizeof(lcm::BaElemInfo) == 24 && sizeof(lcm_ba_params) == 112 &&
              sizeof(lcm_ba_info) == 184 && sizeof(lcm_ba_map_report) == 56, "record sizes");
static_assert(offsetof(lcm_ba_obs, point) == 4 && offsetof(lcm::Observation, point) == 4 && offsetof(lcm_ba_obs, u) == 8 &&
              offsetof(lcm::Observation, u) == 8 && offsetof(lcm_ba_obs, v) == 16 && offsetof(lcm::Observation, v) == 16, "observation layout");
static_assert(offsetof(lcm_ba_elem_info, cost) == 8 && offsetof(lcm::BaElemInfo, cost) == 8 && offsetof(lcm_ba_elem_info, iterations) == 16 &&
              offsetof(lcm::BaElemInfo, iterations) == 16 && offsetof(lcm_ba_elem_info, status) == 20 && offsetof(lcm::BaElemInfo, status) == 20,
              "element info layout");
static_assert(offsetof(lcm_ba_params, eps) == 32 && offsetof(lcm_ba_params, outlier_px) == 56 && offsetof(lcm_ba_params, spread_factor) == 72 &&
              offsetof(lcm_ba_params, outer_iters) == 80 && offsetof(lcm_ba_params, min_point_obs) == 92 && offsetof(lcm_ba_params, reserved) == 96,
              "parameter layout");
static_assert(offsetof(lcm_ba_info, outer_iters) == 136 && offsetof(lcm_ba_info, cameras) == 140 && offsetof(lcm_ba_info, points) == 160 &&
              offsetof(lcm_ba_map_report, threshold) == 32 && offsetof(lcm_ba_map_report, n_outliers) == 40 && offsetof(lcm_ba_map_report, n_obs) == 48,
              "info layout");
static_assert(LCM_BA_CONVERGED == lcm::BA_CONVERGED && LCM_BA_MAX_ITERS == lcm::BA_MAX_ITERS && LCM_BA_SOLVE_FAILED == lcm::BA_SOLVE_FAILED &&
              LCM_BA_HALF_TURN == lcm::BA_HALF_TURN && LCM_BA_SKIPPED == lcm::BA_SKIPPED, "statuses");

namespace {

enum BaMode { BA_ERROR, BA_CAMERAS, BA_POINTS, BA_STEP_CAMERAS, BA_STEP_POINTS, BA_OPTIMIZE, BA_OUTLIERS };

struct BaMap {
    const lcm_pgo_pose* poses; const uint8_t* valid; int n_poses;
    const lcm_ba_point* points; int n_points;
    const lcm_ba_obs* obs; int n_obs;
};

struct BaOut {                                // what a mode returns; the pointers it does not use stay NULL
    double* mean = nullptr; double* obs_err = nullptr;
    lcm_pgo_pose* poses = nullptr; lcm_ba_point* points = nullptr;
    lcm_ba_elem_info* cam_info = nullptr; lcm_ba_elem_info* pt_info = nullptr;
    double* r = nullptr; double* J = nullptr; double* H = nullptr; double* g = nullptr; double* dp = nullptr;
    lcm_ba_info* info = nullptr;
    uint8_t* flags = nullptr; double* max_err = nullptr; double* threshold = nullptr; int* n_outliers = nullptr;
};

bool ba_outputs_missing(BaMode mode, const BaOut& o) {
    switch (mode) {
        case BA_ERROR: return !o.mean;
        case BA_CAMERAS: return !o.poses || !o.cam_info;
        case BA_POINTS: return !o.points || !o.pt_info;
        case BA_STEP_CAMERAS: return !o.r || !o.J || !o.H || !o.g || !o.dp || !o.cam_info;
        case BA_STEP_POINTS: return !o.r || !o.J || !o.H || !o.g || !o.dp || !o.pt_info;
        case BA_OPTIMIZE: return !o.poses || !o.points || !o.info;
        case BA_OUTLIERS: return !o.flags || !o.n_outliers;
    }
    return true;
}

// One call over one map: the checks, the staging, the mode's launches, the download.
int ba_run(lcm_handle* h, const BaMap& m, const lcm_ba_params* pp_in, BaMode mode, const BaOut& o) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (ba_outputs_missing(mode, o)) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    lcm::BaPlan pl;
    const lcm::BaProblem prob = lcm::ba_inputs_problem(m.poses, m.valid, m.n_poses, m.points, m.n_points, m.obs, m.n_obs, pp_in, &pl);
    if (prob.what) return fail(prob.code, "%s", prob.what);
    const lcm_ba_params pp = *pp_in;
    int rc = set_device(h); if (rc) return rc;

    // the map in one block: [poses | points | observations | the plan's four tables | valid], uploaded once; behind it what the
    // kernels write
    const size_t NC = (size_t)m.n_poses, NP = (size_t)m.n_points, NO = (size_t)m.n_obs;
    const size_t n_partials = NO ? (NO + lcm::BA_ERROR_THREADS - 1) / lcm::BA_ERROR_THREADS : 1;
    const bool step_cam = mode == BA_STEP_CAMERAS, step_pt = mode == BA_STEP_POINTS, seam = step_cam || step_pt;
    const size_t width = step_cam ? 6 : 3, n_elem = step_cam ? NC : NP;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o_ = at; at += up16(bytes); return o_; };
    const size_t o_poses = take(NC * sizeof(lcm_pgo_pose)), o_points = take(NP * sizeof(lcm_ba_point)), o_obs = take(NO * sizeof(lcm_ba_obs));
    const size_t o_cam_off = take((NC + 1) * 4), o_cam_obs = take(NO * 4), o_pt_off = take((NP + 1) * 4), o_pt_obs = take(NO * 4);
    const size_t o_valid = take(NC), upload = at;
    const size_t o_cam_info = take(NC * sizeof(lcm_ba_elem_info)), o_pt_info = take(NP * sizeof(lcm_ba_elem_info));
    const size_t o_means = take(17 * sizeof(double)), o_partial = take(n_partials * sizeof(double));
    const size_t o_obs_err = take(mode == BA_ERROR && o.obs_err ? NO * sizeof(double) : 0);
    const size_t o_flags = take(mode == BA_OUTLIERS ? NP : 0), o_max_err = take(mode == BA_OUTLIERS ? NP * sizeof(double) : 0);
    const size_t o_seam = at;
    const size_t o_r = take(seam ? 2 * NO * sizeof(double) : 0), o_J = take(seam ? 2 * width * NO * sizeof(double) : 0);
    const size_t o_H = take(seam ? width * width * n_elem * sizeof(double) : 0), o_g = take(seam ? width * n_elem * sizeof(double) : 0);
    const size_t o_dp = take(seam ? width * n_elem * sizeof(double) : 0), total = at;

    std::vector<uint8_t> stage(upload, 0);
    std::memcpy(stage.data() + o_poses, m.poses, NC * sizeof(lcm_pgo_pose));
    std::memcpy(stage.data() + o_points, m.points, NP * sizeof(lcm_ba_point));
    if (NO) {
        std::memcpy(stage.data() + o_obs, m.obs, NO * sizeof(lcm_ba_obs));
        std::memcpy(stage.data() + o_cam_obs, pl.cam_obs.data(), NO * 4);
        std::memcpy(stage.data() + o_pt_obs, pl.pt_obs.data(), NO * 4);
    }
    std::memcpy(stage.data() + o_cam_off, pl.cam_off.data(), (NC + 1) * 4);
    std::memcpy(stage.data() + o_pt_off, pl.pt_off.data(), (NP + 1) * 4);
    for (size_t c = 0; c < NC; ++c) stage[o_valid + c] = lcm::pgo_is_valid(m.valid, (int)c) ? 1 : 0;
    auto& s = h->ba;
    rc = ensure_dev(s.d_map, s.d_map_n, total); if (rc) return rc;
    uint8_t* d = s.d_map;
    HIP_TRY(hipMemcpyAsync(d, stage.data(), upload, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(d + o_cam_info, 0, o_partial - o_cam_info, h->stream));           // the infos and the 17 means
    if (seam) HIP_TRY(hipMemsetAsync(d + o_seam, 0, total - o_seam, h->stream));

    lcm::BaArgs a{};
    a.poses = reinterpret_cast<lcm::Pose*>(d + o_poses); a.points = reinterpret_cast<lcm::Point3*>(d + o_points);
    a.valid = d + o_valid; a.obs = reinterpret_cast<const lcm::Observation*>(d + o_obs);
    a.cam_off = reinterpret_cast<const uint32_t*>(d + o_cam_off); a.cam_obs = reinterpret_cast<const uint32_t*>(d + o_cam_obs);
    a.pt_off = reinterpret_cast<const uint32_t*>(d + o_pt_off); a.pt_obs = reinterpret_cast<const uint32_t*>(d + o_pt_obs);
    a.cam_info = reinterpret_cast<lcm::BaElemInfo*>(d + o_cam_info); a.pt_info = reinterpret_cast<lcm::BaElemInfo*>(d + o_pt_info);
    double* means = reinterpret_cast<double*>(d + o_means);
    a.partial = reinterpret_cast<double*>(d + o_partial); a.mean_out = means;
    if (mode == BA_ERROR && o.obs_err) a.obs_err = reinterpret_cast<double*>(d + o_obs_err);
    if (mode == BA_OUTLIERS) { a.flags = d + o_flags; a.max_err = reinterpret_cast<double*>(d + o_max_err); }
    if (seam) {
        a.seam_r = reinterpret_cast<double*>(d + o_r); a.seam_J = reinterpret_cast<double*>(d + o_J); a.seam_H = reinterpret_cast<double*>(d + o_H);
        a.seam_g = reinterpret_cast<double*>(d + o_g); a.seam_dp = reinterpret_cast<double*>(d + o_dp);
    }
    a.n_cams = (uint32_t)NC; a.n_points = (uint32_t)NP; a.n_obs = (uint32_t)NO; a.n_partials = (uint32_t)n_partials;
    a.K = lcm::Camera{pp.fx, pp.fy, pp.cx, pp.cy};
    a.eps = pp.eps; a.damping = pp.damping; a.min_update = pp.min_update; a.outlier_px = pp.outlier_px;
    a.inner_iters = seam ? 1 : pp.inner_iters; a.min_cam_obs = pp.min_cam_obs; a.min_point_obs = pp.min_point_obs;
    double threshold = 0.0;
    if (mode == BA_OUTLIERS) {
        lcm::ba_camera_spread(m.poses, m.valid, m.n_poses, pp.min_spread, pp.spread_factor, a.centroid, &threshold);
        a.max_dist = threshold;
    }

    uint32_t launches = 0;
    hipError_t e = hipSuccess;
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    switch (mode) {
        case BA_ERROR: e = lcm::launch_ba_error(a, h->stream); launches = 2; break;
        case BA_CAMERAS: case BA_STEP_CAMERAS: e = lcm::launch_ba_cameras(a, h->stream); launches = 1; break;
        case BA_POINTS: case BA_STEP_POINTS: e = lcm::launch_ba_points(a, h->stream); launches = 1; break;
        case BA_OUTLIERS: e = lcm::launch_ba_outliers(a, h->stream); launches = 1; break;
        case BA_OPTIMIZE:
            e = lcm::launch_ba_error(a, h->stream); launches = 2;
            for (int it = 1; it <= pp.outer_iters && e == hipSuccess; ++it) {
                if ((e = lcm::launch_ba_cameras(a, h->stream)) != hipSuccess) break;
                if ((e = lcm::launch_ba_points(a, h->stream)) != hipSuccess) break;
                a.mean_out = means + it;
                e = lcm::launch_ba_error(a, h->stream);
                launches += 4;
            }
            break;
    }
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "bundle-adjustment kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    h->info_pending = true;
    h->info.launches = launches;
    h->info.workgroups = (uint32_t)std::max({NC, (NP + 63) / 64, n_partials}); h->info.route = LCM_ROUTE_PLAIN;
    h->info.pairs = NO; h->info.distances = 0;
    h->info.algo_bytes = upload;

    // the download, straight into the caller's buffers: every check is behind us and every input is staged, so an output may
    // alias an input
    std::vector<lcm_ba_elem_info> cam_info, pt_info;
    double mean_buf[17] = {0.0};
    int n_flagged = 0;
    switch (mode) {
        case BA_ERROR:
            HIP_TRY(hipMemcpyAsync(mean_buf, means, sizeof(double), hipMemcpyDeviceToHost, h->stream));
            if (o.obs_err && NO) HIP_TRY(hipMemcpyAsync(o.obs_err, a.obs_err, NO * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            break;
        case BA_CAMERAS:
            HIP_TRY(hipMemcpyAsync(o.poses, a.poses, NC * sizeof(lcm_pgo_pose), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(o.cam_info, a.cam_info, NC * sizeof(lcm_ba_elem_info), hipMemcpyDeviceToHost, h->stream));
            break;
        case BA_POINTS:
            HIP_TRY(hipMemcpyAsync(o.points, a.points, NP * sizeof(lcm_ba_point), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(o.pt_info, a.pt_info, NP * sizeof(lcm_ba_elem_info), hipMemcpyDeviceToHost, h->stream));
            break;
        case BA_STEP_CAMERAS: case BA_STEP_POINTS:
            if (NO) {
                HIP_TRY(hipMemcpyAsync(o.r, a.seam_r, 2 * NO * sizeof(double), hipMemcpyDeviceToHost, h->stream));
                HIP_TRY(hipMemcpyAsync(o.J, a.seam_J, 2 * width * NO * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            }
            HIP_TRY(hipMemcpyAsync(o.H, a.seam_H, width * width * n_elem * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(o.g, a.seam_g, width * n_elem * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(o.dp, a.seam_dp, width * n_elem * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(step_cam ? o.cam_info : o.pt_info, step_cam ? a.cam_info : a.pt_info, n_elem * sizeof(lcm_ba_elem_info),
                                   hipMemcpyDeviceToHost, h->stream));
            break;
        case BA_OPTIMIZE:
            cam_info.resize(NC); pt_info.resize(NP);
            HIP_TRY(hipMemcpyAsync(o.poses, a.poses, NC * sizeof(lcm_pgo_pose), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(o.points, a.points, NP * sizeof(lcm_ba_point), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(cam_info.data(), a.cam_info, NC * sizeof(lcm_ba_elem_info), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(pt_info.data(), a.pt_info, NP * sizeof(lcm_ba_elem_info), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(mean_buf, means, sizeof(mean_buf), hipMemcpyDeviceToHost, h->stream));
            break;
        case BA_OUTLIERS:
            HIP_TRY(hipMemcpyAsync(o.flags, a.flags, NP, hipMemcpyDeviceToHost, h->stream));
            if (o.max_err) HIP_TRY(hipMemcpyAsync(o.max_err, a.max_err, NP * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            break;
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (mode == BA_ERROR) *o.mean = mean_buf[0];
    if (mode == BA_OPTIMIZE) {
        lcm_ba_info got;
        std::memset(&got, 0, sizeof(got));
        std::memcpy(got.mean_error, mean_buf, sizeof(mean_buf));
        got.outer_iters = pp.outer_iters;
        lcm::ba_count_statuses(cam_info.data(), m.n_poses, got.cameras);
        lcm::ba_count_statuses(pt_info.data(), m.n_points, got.points);
        *o.info = got;
        if (o.cam_info) std::memcpy(o.cam_info, cam_info.data(), NC * sizeof(lcm_ba_elem_info));
        if (o.pt_info) std::memcpy(o.pt_info, pt_info.data(), NP * sizeof(lcm_ba_elem_info));
    }
    if (mode == BA_OUTLIERS) {
        for (size_t p = 0; p < NP; ++p) n_flagged += o.flags[p] != 0;
        *o.n_outliers = n_flagged;
        if (o.threshold) *o.threshold = threshold;
    }
    return LCM_OK;
}

int ba_compact_impl(const lcm_ba_point* points, int n_points, const lcm_ba_obs* obs, int n_obs, const uint8_t* flags, lcm_ba_point* points_out,
                    int cap_points, lcm_ba_obs* obs_out, int cap_obs, int32_t* old_to_new, int* n_points_out, int* n_obs_out) {
    if (n_points < 0 || n_obs < 0 || cap_points < 0 || cap_obs < 0 || !n_points_out || !n_obs_out) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if ((n_points && (!points || !flags)) || (n_obs && !obs) || (cap_points && !points_out) || (cap_obs && !obs_out))
        return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    for (int i = 0; i < n_obs; ++i)
        if (obs[i].point < 0 || obs[i].point >= n_points) return fail(LCM_ERR_INVALID_ARG, "an observation's point index is out of range");
    int kp = 0, ko = 0;
    lcm::ba_compact_counts(flags, n_points, obs, n_obs, &kp, &ko);
    *n_points_out = kp; *n_obs_out = ko;
    if (kp > cap_points || ko > cap_obs) return fail(LCM_ERR_CAPACITY, "%d points and %d observations but room for %d and %d", kp, ko, cap_points, cap_obs);
    lcm::ba_compact(points, n_points, obs, n_obs, flags, points_out, obs_out, old_to_new);
    return LCM_OK;
}

int ba_add_loop_impl(const lcm_dmatch* matches, const uint8_t* mask, int n_matches, const int32_t* past_table, int n_past_kp, int32_t* curr_table,
                     const float* curr_kp, int n_curr_kp, int curr, int n_points, lcm_ba_obs* obs, int n_obs, int cap, int* n_added) {
    if (n_matches < 0 || n_past_kp < 0 || n_curr_kp < 0 || curr < 0 || n_points < 0 || n_obs < 0 || cap < n_obs || !n_added)
        return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if ((n_matches && (!matches || !mask)) || (n_past_kp && !past_table) || (n_curr_kp && (!curr_table || !curr_kp)) || (cap && !obs))
        return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    int n = 0;
    if (const char* what = lcm::ba_loop_observations_problem(matches, mask, n_matches, past_table, n_past_kp, n_curr_kp, n_points, &n))
        return fail(LCM_ERR_INVALID_ARG, "%s", what);
    *n_added = n;
    if (n > cap - n_obs) return fail(LCM_ERR_CAPACITY, "%d new observations but room for %d", n, cap - n_obs);
    lcm::ba_add_loop_observations(matches, mask, n_matches, past_table, curr_table, curr_kp, curr, obs + n_obs);
    return LCM_OK;
}

int ba_refine_map_impl(lcm_handle* h, const BaMap& m, const lcm_ba_params* pp, int second, lcm_pgo_pose* poses_out, lcm_ba_point* points_out,
                       lcm_ba_obs* obs_out, int32_t* old_to_new, lcm_ba_map_report* report) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (!poses_out || !points_out || (!obs_out && m.n_obs > 0) || !report) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    if (second > LCM_BA_MAX_ITERS_PER_LOOP) return fail(LCM_ERR_INVALID_ARG, "second_outer_iters must be at most 16");
    lcm_ba_map_report rep;
    std::memset(&rep, 0, sizeof(rep));
    lcm_ba_info info;
    BaOut o;
    o.poses = poses_out; o.info = &info;
    std::vector<lcm_ba_point> pts((size_t)std::max(m.n_points, 1));
    o.points = pts.data();
    int rc = ba_run(h, m, pp, BA_OPTIMIZE, o);                     // every refusal happens here, before anything is written
    if (rc) return rc;
    rep.error_before = info.mean_error[0]; rep.error_after = info.mean_error[info.outer_iters];
    const BaMap after{poses_out, m.valid, m.n_poses, pts.data(), m.n_points, m.obs, m.n_obs};
    std::vector<uint8_t> flags((size_t)m.n_points);
    BaOut f;
    f.flags = flags.data(); f.threshold = &rep.threshold; f.n_outliers = &rep.n_outliers;
    if ((rc = ba_run(h, after, pp, BA_OUTLIERS, f)) != 0) return rc;
    int kp = 0, ko = 0;
    rc = ba_compact_impl(pts.data(), m.n_points, m.obs, m.n_obs, flags.data(), points_out, m.n_points, obs_out, m.n_obs, old_to_new, &kp, &ko);
    if (rc) return rc;
    rep.n_points = kp; rep.n_obs = ko;
    if (kp > 0) {
        lcm_ba_params p2 = *pp;
        p2.outer_iters = second > 0 ? second : lcm::BA_SECOND_OUTER_ITERS;
        const BaMap kept{poses_out, m.valid, m.n_poses, points_out, kp, obs_out, ko};
        BaOut o2;
        o2.poses = poses_out; o2.points = points_out; o2.info = &info;
        if ((rc = ba_run(h, kept, &p2, BA_OPTIMIZE, o2)) != 0) return rc;
        rep.error_filtered = info.mean_error[0]; rep.error_final = info.mean_error[info.outer_iters];
    }
    *report = rep;
    return LCM_OK;
}

}  // namespace

extern "C" {

void lcm_ba_params_default(lcm_ba_params* p) { if (p) lcm::ba_params_default(p); }
int lcm_ba_error(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points, int n_points,
                 const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, double* mean, double* obs_err) {
    BaOut o; o.mean = mean; o.obs_err = obs_err;
    return guarded([&] { return ba_run(h, BaMap{poses, valid, n_poses, points, n_points, obs, n_obs}, pp, BA_ERROR, o); });
}
int lcm_ba_refine_cameras(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points, int n_points,
                          const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, lcm_pgo_pose* poses_out, lcm_ba_elem_info* info) {
    BaOut o; o.poses = poses_out; o.cam_info = info;
    return guarded([&] { return ba_run(h, BaMap{poses, valid, n_poses, points, n_points, obs, n_obs}, pp, BA_CAMERAS, o); });
}
int lcm_ba_refine_points(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points, int n_points,
                         const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, lcm_ba_point* points_out, lcm_ba_elem_info* info) {
    BaOut o; o.points = points_out; o.pt_info = info;
    return guarded([&] { return ba_run(h, BaMap{poses, valid, n_poses, points, n_points, obs, n_obs}, pp, BA_POINTS, o); });
}
int lcm_ba_step_cameras(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points, int n_points,
                        const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, double* r, double* J, double* H, double* g, double* dp,
                        lcm_ba_elem_info* info) {
    BaOut o; o.r = r; o.J = J; o.H = H; o.g = g; o.dp = dp; o.cam_info = info;
    return guarded([&] { return ba_run(h, BaMap{poses, valid, n_poses, points, n_points, obs, n_obs}, pp, BA_STEP_CAMERAS, o); });
}
int lcm_ba_step_points(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points, int n_points,
                       const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, double* r, double* J, double* H, double* g, double* dp,
                       lcm_ba_elem_info* info) {
    BaOut o; o.r = r; o.J = J; o.H = H; o.g = g; o.dp = dp; o.pt_info = info;
    return guarded([&] { return ba_run(h, BaMap{poses, valid, n_poses, points, n_points, obs, n_obs}, pp, BA_STEP_POINTS, o); });
}
int lcm_ba_optimize(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points, int n_points,
                    const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, lcm_pgo_pose* poses_out, lcm_ba_point* points_out,
                    lcm_ba_elem_info* cam_info, lcm_ba_elem_info* pt_info, lcm_ba_info* info) {
    BaOut o; o.poses = poses_out; o.points = points_out; o.cam_info = cam_info; o.pt_info = pt_info; o.info = info;
    return guarded([&] { return ba_run(h, BaMap{poses, valid, n_poses, points, n_points, obs, n_obs}, pp, BA_OPTIMIZE, o); });
}
int lcm_ba_outliers(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points, int n_points,
                    const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, uint8_t* flags, double* max_err, double* threshold, int* n_outliers) {
    BaOut o; o.flags = flags; o.max_err = max_err; o.threshold = threshold; o.n_outliers = n_outliers;
    return guarded([&] { return ba_run(h, BaMap{poses, valid, n_poses, points, n_points, obs, n_obs}, pp, BA_OUTLIERS, o); });
}
int lcm_ba_compact(const lcm_ba_point* points, int n_points, const lcm_ba_obs* obs, int n_obs, const uint8_t* flags, lcm_ba_point* points_out,
                   int cap_points, lcm_ba_obs* obs_out, int cap_obs, int32_t* old_to_new, int* n_points_out, int* n_obs_out) {
    return guarded([&] { return ba_compact_impl(points, n_points, obs, n_obs, flags, points_out, cap_points, obs_out, cap_obs, old_to_new,
                                                n_points_out, n_obs_out); });
}
int lcm_ba_add_loop_observations(const lcm_dmatch* matches, const uint8_t* mask, int n_matches, const int32_t* past_table, int n_past_kp,
                                 int32_t* curr_table, const float* curr_kp, int n_curr_kp, int curr, int n_points, lcm_ba_obs* obs, int n_obs,
                                 int cap, int* n_added) {
    return guarded([&] { return ba_add_loop_impl(matches, mask, n_matches, past_table, n_past_kp, curr_table, curr_kp, n_curr_kp, curr, n_points,
                                                 obs, n_obs, cap, n_added); });
}
int lcm_ba_refine_map(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_ba_point* points, int n_points,
                      const lcm_ba_obs* obs, int n_obs, const lcm_ba_params* pp, int second_outer_iters, lcm_pgo_pose* poses_out,
                      lcm_ba_point* points_out, lcm_ba_obs* obs_out, int32_t* old_to_new, lcm_ba_map_report* report) {
    return guarded([&] { return ba_refine_map_impl(h, BaMap{poses, valid, n_poses, points, n_points, obs, n_obs}, pp, second_outer_iters, poses_out,
                                                   points_out, obs_out, old_to_new, report); });
}

}  // extern "C"
