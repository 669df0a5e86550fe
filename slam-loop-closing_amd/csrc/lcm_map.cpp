// lcm_map.cpp — the host side of the map building before the loop (include/lcm.h, lcm_map_*): src/main.cpp:1152-1351.  The kernels
// are lcm_map.hip's, the arithmetic lcm_map_device.h's, the checks, the per-pair plan and the gates lcm_map_host.h's.  Here: the
// staging, the launches and the downloads of the median, the triangulation and the merge, each also as a stage over records that
// are on the device already (map_median_enqueue, map_tri_enqueue, map_merge_run), and the keyframe call that chains them behind
// the loop verification's pipeline (lcm_verify.cpp) with only the small verdict values read back in between.  Part of
// liblcm_hip.so's host side; shared state and helpers: lcm_internal.h.
#include "lcm_internal.h"

#include "lcm_epi_device.h"
#include "lcm_map_host.h"

static_assert(sizeof(lcm_map_params) == 112 && sizeof(lcm_map_tri) == 64 && sizeof(lcm::MapTri) == 64 && sizeof(lcm_map_pair_info) == 48 &&
              sizeof(lcm_map_keyframe_report) == 168 && sizeof(lcm::MapPair) == 448, "record sizes");
static_assert(offsetof(lcm_map_tri, depth1) == 24 && offsetof(lcm::MapTri, depth1) == 24 && offsetof(lcm_map_tri, err2) == 56 &&
              offsetof(lcm::MapTri, err2) == 56 && offsetof(lcm_map_params, min_parallax_deg) == 32 && offsetof(lcm_map_params, min_tracked) == 88 &&
              offsetof(lcm_map_params, reserved) == 100 && offsetof(lcm_map_pair_info, counts) == 16 &&
              offsetof(lcm_map_keyframe_report, median) == 96 && offsetof(lcm_map_keyframe_report, verdict) == 112 &&
              offsetof(lcm_map_keyframe_report, counts) == 136, "record layouts");
static_assert(LCM_MAP_NOT_INLIER == lcm::MAP_NOT_INLIER && LCM_MAP_NO_POINT == lcm::MAP_NO_POINT && LCM_MAP_REJ_DEPTH == lcm::MAP_REJ_DEPTH &&
              LCM_MAP_REJ_PARALLAX == lcm::MAP_REJ_PARALLAX && LCM_MAP_REJ_REPROJ == lcm::MAP_REJ_REPROJ && LCM_MAP_ACCEPTED == lcm::MAP_ACCEPTED &&
              LCM_MAP_MERGED == lcm::MAP_MERGED && LCM_MAP_NEW == lcm::MAP_NEW, "statuses");
static_assert(sizeof(lcm_point_pair) == sizeof(uint4) && sizeof(lcm_dmatch) == sizeof(uint4) && sizeof(size_t) == sizeof(uint64_t), "record sizes");

namespace lcm {

int map_median_enqueue(lcm_handle* h, const uint4* d_pts, const uint64_t* d_off, size_t n_pairs) {
    auto& s = h->map;
    const int rc = ensure_dev(s.d_median, s.d_median_n, n_pairs); if (rc) return rc;
    const hipError_t e = launch_map_median(MapMedianArgs{d_pts, d_off, s.d_median}, (uint32_t)n_pairs, h->stream);
    return e == hipSuccess ? LCM_OK : fail(LCM_ERR_HIP, "median kernel launch failed: %s", hipGetErrorString(e));
}

int map_tri_enqueue(lcm_handle* h, const uint4* d_pts, const uint64_t* d_off, size_t n_pairs, uint32_t max_n, size_t total,
                    const uint8_t* d_mask, const MapPair* pairs, const lcm_map_params& mp) {
    auto& s = h->map;
    int rc = ensure_dev(s.d_pairs, s.d_pairs_n, n_pairs); if (rc) return rc;
    rc = ensure_dev(s.d_counts, s.d_counts_n, n_pairs * MAP_STATUSES); if (rc) return rc;
    rc = ensure_dev(s.d_tri, s.d_tri_n, total); if (rc) return rc;
    rc = ensure_dev(s.d_status, s.d_status_n, total); if (rc) return rc;
    if (n_pairs == 0) return LCM_OK;
    HIP_TRY(hipMemcpyAsync(s.d_pairs, pairs, n_pairs * sizeof(MapPair), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(s.d_counts, 0, n_pairs * MAP_STATUSES * sizeof(uint32_t), h->stream));
    const MapTriArgs a{d_pts, d_off, d_mask, s.d_pairs, s.d_tri, s.d_status, s.d_counts, Camera{mp.fx, mp.fy, mp.cx, mp.cy},
                       MapLimits{mp.min_depth, mp.max_depth, mp.max_reproj}};
    const hipError_t e = launch_map_triangulate(a, (uint32_t)n_pairs, max_n, h->stream);
    return e == hipSuccess ? LCM_OK : fail(LCM_ERR_HIP, "triangulation kernel launch failed: %s", hipGetErrorString(e));
}

int map_merge_run(lcm_handle* h, const MapMergeIO& io, int* n_new, int* n_merged, uint32_t* launches) {
    *launches = 0;
    auto& s = h->map;
    const size_t n = io.n, K1 = (size_t)io.n_kp1, K2 = (size_t)io.n_kp2, n_blocks = (n + MAP_THREADS - 1) / MAP_THREADS;
    if (n == 0) { *n_new = 0; *n_merged = 0; return LCM_OK; }
    int rc = ensure_dev(s.d_tab, s.d_tab_n, K1 + 2 * K2); if (rc) return rc;
    rc = ensure_dev(s.d_blocks, s.d_blocks_n, 2 * (n_blocks + 1)); if (rc) return rc;
    rc = ensure_dev(s.d_status_out, s.d_status_out_n, n); if (rc) return rc;
    int32_t* d_t1 = s.d_tab; int32_t* d_t2 = s.d_tab + K1; int32_t* d_win = s.d_tab + K1 + K2;
    uint32_t* d_acc = s.d_blocks; uint32_t* d_new = s.d_blocks + n_blocks + 1;
    if (K1) HIP_TRY(hipMemcpyAsync(d_t1, io.table1, K1 * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if (K2) HIP_TRY(hipMemcpyAsync(d_t2, io.table2, K2 * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if (K2) HIP_TRY(hipMemsetAsync(d_win, 0xFF, K2 * sizeof(int32_t), h->stream));
    MapMergeArgs a{io.d_matches, io.d_pts, io.d_tri, io.d_status, d_t1, d_t2, d_win, d_acc, d_new, nullptr, nullptr, s.d_status_out,
                   (uint32_t)n, io.kf1, io.kf2, io.n_points};
    hipError_t e = launch_map_merge_count(a, h->stream);
    if (e == hipSuccess) e = launch_block_scan(d_acc, (uint32_t)n_blocks, d_acc + n_blocks, h->stream);
    if (e == hipSuccess) e = launch_block_scan(d_new, (uint32_t)n_blocks, d_new + n_blocks, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "merge count kernels: launch failed: %s", hipGetErrorString(e));
    *launches = 3;
    uint32_t totals[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&totals[0], d_acc + n_blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&totals[1], d_new + n_blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));                // also: the tables (pageable) have been consumed
    if (totals[1] > totals[0] || totals[0] > n) return fail(LCM_ERR_HIP, "merge counts %u / %u exceed the %zu records", totals[1], totals[0], n);
    const size_t fresh = totals[1], merged = totals[0] - totals[1], n_obs = 2 * fresh + merged;
    *n_new = (int)fresh; *n_merged = (int)merged;
    if (fresh > (size_t)io.cap_points || n_obs > (size_t)io.cap_obs)
        return fail(LCM_ERR_CAPACITY, "%zu new points and %zu new observations but room for %d and %d", fresh, n_obs, io.cap_points, io.cap_obs);
    rc = ensure_dev(s.d_points, s.d_points_n, fresh); if (rc) return rc;
    rc = ensure_dev(s.d_obs, s.d_obs_n, n_obs); if (rc) return rc;
    a.points_out = s.d_points; a.obs_out = s.d_obs;
    e = launch_map_merge_emit(a, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "merge kernel launch failed: %s", hipGetErrorString(e));
    *launches = 4;
    return LCM_OK;
}

int map_merge_download(lcm_handle* h, const MapMergeIO& io, int n_new, int n_merged) {
    auto& s = h->map;
    const size_t n_obs = 2 * (size_t)n_new + (size_t)n_merged;
    if (io.n == 0) return LCM_OK;
    if (n_new) HIP_TRY(hipMemcpyAsync(io.points_out, s.d_points, (size_t)n_new * sizeof(Point3), hipMemcpyDeviceToHost, h->stream));
    if (n_obs) HIP_TRY(hipMemcpyAsync(io.obs_out, s.d_obs, n_obs * sizeof(Observation), hipMemcpyDeviceToHost, h->stream));
    if (io.status_out) HIP_TRY(hipMemcpyAsync(io.status_out, s.d_status_out, io.n, hipMemcpyDeviceToHost, h->stream));
    if (io.n_kp1) HIP_TRY(hipMemcpyAsync(io.table1, s.d_tab, (size_t)io.n_kp1 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (io.n_kp2) HIP_TRY(hipMemcpyAsync(io.table2, s.d_tab + io.n_kp1, (size_t)io.n_kp2 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    return LCM_OK;
}

}  // namespace lcm

namespace {
using lcm::MapMergeIO;
using lcm::MapPair;

int map_problem(const lcm::MapProblem& p) { return p.what ? fail(p.code, "%s", p.what) : LCM_OK; }

void map_set_info(lcm_handle* h, uint32_t launches, size_t workgroups, size_t records, size_t bytes) {
    h->info_pending = true;
    h->info.launches = launches; h->info.workgroups = (uint32_t)workgroups; h->info.route = LCM_ROUTE_PLAIN;
    h->info.pairs = records; h->info.distances = 0; h->info.algo_bytes = bytes;
}

int map_median_impl(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs, double* median) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    size_t total = 0;
    uint32_t max_n = 0;
    int rc = map_problem(lcm::map_offsets_problem(offsets, n_pairs, &total, &max_n)); if (rc) return rc;
    if ((n_pairs > 0 && !median) || (total > 0 && !pts)) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    if (n_pairs == 0) return LCM_OK;
    rc = set_device(h); if (rc) return rc;
    const size_t P = (size_t)n_pairs;
    rc = lcm::epi_upload_points(h, pts, offsets, P, total); if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    rc = lcm::map_median_enqueue(h, h->epi.d_pts, h->epi.d_off, P); if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    map_set_info(h, 1, P, total, total * 16 * 8 + P * 24);
    HIP_TRY(hipMemcpyAsync(median, h->map.d_median, P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return LCM_OK;
}

int map_triangulate_impl(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs, const uint8_t* mask,
                         const lcm_pgo_pose* poses1, const lcm_pgo_pose* poses2, const lcm_map_params* mp, lcm_map_tri* tri, uint8_t* status,
                         lcm_map_pair_info* info) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (const char* what = lcm::map_params_problem(mp)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    size_t total = 0;
    uint32_t max_n = 0;
    int rc = map_problem(lcm::map_offsets_problem(offsets, n_pairs, &total, &max_n)); if (rc) return rc;
    if ((n_pairs > 0 && (!poses1 || !poses2 || !info)) || (total > 0 && (!pts || !tri || !status))) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    const size_t P = (size_t)n_pairs;
    for (size_t p = 0; p < P; ++p) {
        if (const char* what = lcm::map_pose_problem(poses1[p])) return fail(LCM_ERR_INVALID_ARG, "pair %zu, view 1: %s", p, what);
        if (const char* what = lcm::map_pose_problem(poses2[p])) return fail(LCM_ERR_INVALID_ARG, "pair %zu, view 2: %s", p, what);
    }
    if (n_pairs == 0) return LCM_OK;
    std::vector<MapPair> pairs(P);
    for (size_t p = 0; p < P; ++p) lcm::map_plan_pair(*mp, poses1[p], poses2[p], &pairs[p]);
    rc = set_device(h); if (rc) return rc;
    auto& s = h->map;
    rc = lcm::epi_upload_points(h, pts, offsets, P, total); if (rc) return rc;
    if (mask && total) {
        rc = ensure_dev(s.d_mask, s.d_mask_n, total); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(s.d_mask, mask, total, hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    rc = lcm::map_tri_enqueue(h, h->epi.d_pts, h->epi.d_off, P, max_n, total, mask ? s.d_mask : nullptr, pairs.data(), *mp); if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    map_set_info(h, max_n ? 1 : 0, (size_t)((max_n + lcm::MAP_THREADS - 1) / lcm::MAP_THREADS) * P, total,
                 total * (16 + 1 + 64 + 1) + P * (sizeof(MapPair) + 16 + 32));
    std::vector<uint32_t> counts(P * lcm::MAP_STATUSES);
    if (total) {
        HIP_TRY(hipMemcpyAsync(tri, s.d_tri, total * sizeof(lcm_map_tri), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(status, s.d_status, total, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipMemcpyAsync(counts.data(), s.d_counts, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t p = 0; p < P; ++p) {
        std::memset(&info[p], 0, sizeof(info[p]));
        info[p].baseline = pairs[p].baseline; info[p].cos_min = pairs[p].cos_min;
        for (int k = 0; k < lcm::MAP_STATUSES; ++k) info[p].counts[k] = (int32_t)counts[p * lcm::MAP_STATUSES + (size_t)k];
    }
    return LCM_OK;
}

// what lcm_map_merge and lcm_map_add_keyframe check alike about the map's side of a merge
int map_merge_args_checked(const lcm_dmatch* matches, const uint8_t* status, int n, int kf1, int kf2, const int32_t* table1, int n_kp1,
                           const int32_t* table2, int n_kp2, int n_points, const lcm_ba_point* points_out, int cap_points,
                           const lcm_ba_obs* obs_out, int cap_obs) {
    if (n < 0 || kf1 < 0 || kf2 < 0 || n_kp1 < 0 || n_kp2 < 0 || n_points < 0 || cap_points < 0 || cap_obs < 0) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (n > LCM_MAP_MAX_RECORDS) return fail(LCM_ERR_CAPACITY, "more records than LCM_MAP_MAX_RECORDS");
    if ((n > 0 && !matches) || (n_kp1 > 0 && !table1) || (n_kp2 > 0 && !table2) || (cap_points > 0 && !points_out) || (cap_obs > 0 && !obs_out))
        return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    if ((long long)n_points + n > 0x7FFFFFFFll) return fail(LCM_ERR_CAPACITY, "the map's point indices would pass 2^31");
    std::vector<uint8_t> seen;
    if (const char* what = lcm::map_merge_problem(matches, status, n, table1, n_kp1, table2, n_kp2, n_points, seen)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    return LCM_OK;
}

int map_merge_impl(lcm_handle* h, const lcm_dmatch* matches, const lcm_point_pair* pts, const lcm_map_tri* tri, const uint8_t* status, int n,
                   int kf1, int kf2, int32_t* table1, int n_kp1, int32_t* table2, int n_kp2, int n_points, lcm_ba_point* points_out,
                   int cap_points, lcm_ba_obs* obs_out, int cap_obs, uint8_t* status_out, int* n_new, int* n_merged) {
    if (!h || !n_new || !n_merged) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (n > 0 && (!pts || !tri || !status || !status_out)) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    int rc = map_merge_args_checked(matches, status, n, kf1, kf2, table1, n_kp1, table2, n_kp2, n_points, points_out, cap_points, obs_out, cap_obs);
    if (rc) return rc;
    if (n == 0) { *n_new = 0; *n_merged = 0; return LCM_OK; }
    rc = set_device(h); if (rc) return rc;
    auto& s = h->map;
    const size_t N = (size_t)n, offsets[2] = {0, N};
    rc = lcm::epi_upload_points(h, pts, offsets, 1, N); if (rc) return rc;
    rc = ensure_dev(s.d_matches, s.d_matches_n, N); if (rc) return rc;
    rc = ensure_dev(s.d_tri, s.d_tri_n, N); if (rc) return rc;
    rc = ensure_dev(s.d_status, s.d_status_n, N); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(s.d_matches, matches, N * sizeof(uint4), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(s.d_tri, tri, N * sizeof(lcm_map_tri), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(s.d_status, status, N, hipMemcpyHostToDevice, h->stream));
    const MapMergeIO io{s.d_matches, h->epi.d_pts, s.d_tri, s.d_status, (uint32_t)n, kf1, kf2, table1, n_kp1, table2, n_kp2, n_points,
                        points_out, cap_points, obs_out, cap_obs, status_out};
    uint32_t launches = 0;
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    rc = lcm::map_merge_run(h, io, n_new, n_merged, &launches);
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    map_set_info(h, launches, (N + lcm::MAP_THREADS - 1) / lcm::MAP_THREADS, N, N * (2 * 17 + 16 + 1) + ((size_t)n_kp1 + 2 * (size_t)n_kp2) * 8);
    if (rc) return rc;
    rc = lcm::map_merge_download(h, io, *n_new, *n_merged); if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return LCM_OK;
}

}  // namespace

namespace lcm {

int map_track_checked(lcm_handle* h, const MapTrack& t, int n_matches) {
    if (!h || !t.report) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (const char* what = map_params_problem(t.mp)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    if (!t.pose_last) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    if (const char* what = map_pose_problem(*t.pose_last)) return fail(LCM_ERR_INVALID_ARG, "the last keyframe's pose: %s", what);
    if (n_matches < 0) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    return map_merge_args_checked(nullptr, nullptr, 0, t.kf_last, t.kf_new, t.table_last, t.n_kp_last, t.table_new, t.n_kp_new, t.n_points,
                                  t.points_out, t.cap_points, t.obs_out, t.cap_obs);
}

void map_report_start(const MapTrack& t, int n_matches) {
    std::memset(t.report, 0, sizeof(*t.report));
    t.report->n_matches = n_matches;
    t.report->verdict = n_matches < t.mp->min_tracked ? LCM_MAP_FEW_MATCHES : LCM_MAP_KEYFRAME;         // :1156, before the points are looked at
}

// The stages behind the verification of ONE pair whose n records, matches and pose record are on the device (the pipeline ran
// with the pose stage): the pose gates, the new pose, the triangulation under the pose's mask and the merge.  pr: the pair's pose
// record, read back by the caller.  On LCM_OK with the verdict LCM_MAP_KEYFRAME the downloads are enqueued and not waited for.
int map_keyframe_stages(lcm_handle* h, const MapTrack& t, const uint4* d_pts, const uint64_t* d_off, const uint4* d_matches,
                        const uint8_t* d_pose_mask, uint32_t n, const lcm_pose_result& pr, uint32_t* launches) {
    lcm_map_keyframe_report& rep = *t.report;
    *launches = 0;
    rep.verdict = map_pose_verdict(*t.mp, (int)n, pr, &rep.n_inliers);
    if (rep.verdict != LCM_MAP_KEYFRAME) return LCM_OK;
    lcm_pgo_pose pose_new;
    map_new_pose(pr, *t.pose_last, &pose_new);
    MapPair pair;
    map_plan_pair(*t.mp, *t.pose_last, pose_new, &pair);
    int rc = map_tri_enqueue(h, d_pts, d_off, 1, n, n, d_pose_mask, &pair, *t.mp); if (rc) return rc;
    auto& s = h->map;
    const MapMergeIO io{d_matches, d_pts + 0, s.d_tri, s.d_status, n, t.kf_last, t.kf_new, t.table_last, t.n_kp_last, t.table_new, t.n_kp_new,
                        t.n_points, t.points_out, t.cap_points, t.obs_out, t.cap_obs, t.status_out};
    uint32_t more = 0;
    rc = map_merge_run(h, io, &rep.n_new, &rep.n_merged, &more);      // waits: `pair` (pageable) has been consumed
    *launches = 1 + more;
    if (rc) { if (rc != LCM_ERR_CAPACITY) { rep.n_new = 0; rep.n_merged = 0; } return rc; }
    uint32_t counts[MAP_STATUSES] = {0};
    HIP_TRY(hipMemcpyAsync(counts, s.d_counts, sizeof(counts), hipMemcpyDeviceToHost, h->stream));
    rc = map_merge_download(h, io, rep.n_new, rep.n_merged); if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int k = 0; k < MAP_STATUSES; ++k) rep.counts[k] = (int32_t)counts[k];
    rep.counts[MAP_ACCEPTED] = 0; rep.counts[MAP_MERGED] = rep.n_merged; rep.counts[MAP_NEW] = rep.n_new;
    rep.pose = pose_new; rep.baseline = pair.baseline;
    return LCM_OK;
}

// The whole of the map's side behind a verification (with the pose stage) that is enqueued and not yet read: the median, the
// pose record read back with it, the gates in the reference's order, then map_keyframe_stages.  n == 0: nothing is launched.
int map_track_stages(lcm_handle* h, const MapTrack& t, const uint4* d_pts, const uint64_t* d_off, const uint4* d_matches, uint32_t n,
                     uint32_t* launches) {
    *launches = 0;
    map_report_start(t, (int)n);
    lcm_map_keyframe_report& rep = *t.report;
    if (rep.verdict != LCM_MAP_KEYFRAME) return LCM_OK;
    lcm_pose_result pr;
    pose_empty_results(&pr, 1);
    if (n > 0) {
        int rc = map_median_enqueue(h, d_pts, d_off, 1); if (rc) return rc;
        *launches = 1;
        HIP_TRY(hipMemcpyAsync(&rep.median, h->map.d_median, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(&pr, h->pose.d_res, sizeof(pr), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    rep.verdict = map_motion_verdict(*t.mp, (int)n, rep.median);
    if (rep.verdict != LCM_MAP_KEYFRAME) return LCM_OK;
    uint32_t more = 0;
    const int rc = map_keyframe_stages(h, t, d_pts, d_off, d_matches, h->pose.d_mask, n, pr, &more);
    *launches += more;
    return rc;
}

}  // namespace lcm

namespace {

int map_add_keyframe_impl(lcm_handle* h, const lcm_dmatch* matches, const lcm_point_pair* pts, int n_matches, const lcm::MapTrack& t,
                          const lcm_epi_params* ep, const lcm_lo_params* lp, const lcm_pose_params* pp) {
    int rc = lcm::map_track_checked(h, t, n_matches); if (rc) return rc;
    rc = lcm::epi_params_checked(ep); if (rc) return rc;
    lcm_epi_result er;
    lcm_lo_info li;
    lcm_pose_result pr;
    lcm::VerifyPlan plan{ep, lp != nullptr, true, &er, nullptr, &li, &pr, nullptr};
    rc = lcm::verify_params_checked(&plan, lp, pp); if (rc) return rc;
    if ((uint32_t)n_matches > lcm::EPI_MAX_POINTS) return fail(LCM_ERR_CAPACITY, "a pair holds at most %u point records", lcm::EPI_MAX_POINTS);
    if (n_matches > 0 && !pts) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    rc = map_merge_args_checked(matches, nullptr, n_matches, t.kf_last, t.kf_new, t.table_last, t.n_kp_last, t.table_new, t.n_kp_new, t.n_points,
                                t.points_out, t.cap_points, t.obs_out, t.cap_obs);
    if (rc) return rc;
    lcm_map_keyframe_report& rep = *t.report;
    lcm::map_report_start(t, n_matches);
    if (rep.verdict != LCM_MAP_KEYFRAME) return LCM_OK;
    rc = set_device(h); if (rc) return rc;
    const size_t N = (size_t)n_matches, offsets[2] = {0, N};
    rc = lcm::epi_upload_points(h, pts, offsets, 1, N); if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    rc = lcm::map_median_enqueue(h, h->epi.d_pts, h->epi.d_off, 1); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(&rep.median, h->map.d_median, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    uint32_t launches = 1, more = 0;
    rep.verdict = lcm::map_motion_verdict(*t.mp, n_matches, rep.median);
    if (rep.verdict == LCM_MAP_KEYFRAME) {
        auto& s = h->map;
        rc = ensure_dev(s.d_matches, s.d_matches_n, N); if (rc) return rc;
        if (N) HIP_TRY(hipMemcpyAsync(s.d_matches, matches, N * sizeof(uint4), hipMemcpyHostToDevice, h->stream));
        rc = lcm::verify_enqueue(h, plan, h->epi.d_pts, h->epi.d_off, 1, (uint32_t)n_matches, N, &more); if (rc) return rc;
        launches += more;
        HIP_TRY(hipMemcpyAsync(&pr, h->pose.d_res, sizeof(pr), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        rc = lcm::map_keyframe_stages(h, t, h->epi.d_pts, h->epi.d_off, s.d_matches, h->pose.d_mask, (uint32_t)n_matches, pr, &more);
        launches += more;
    }
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    map_set_info(h, launches, (N + lcm::MAP_THREADS - 1) / lcm::MAP_THREADS, N, N * 16);
    return rc;
}

}  // namespace

extern "C" {

void lcm_map_params_default(lcm_map_params* p) { if (p) lcm::map_params_default(p); }
int lcm_map_median_displacement(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs, double* median) {
    return guarded([&] { return map_median_impl(h, pts, offsets, n_pairs, median); });
}
int lcm_map_triangulate_pairs(lcm_handle* h, const lcm_point_pair* pts, const size_t* offsets, int n_pairs, const uint8_t* mask,
                              const lcm_pgo_pose* poses1, const lcm_pgo_pose* poses2, const lcm_map_params* mp, lcm_map_tri* tri, uint8_t* status,
                              lcm_map_pair_info* info) {
    return guarded([&] { return map_triangulate_impl(h, pts, offsets, n_pairs, mask, poses1, poses2, mp, tri, status, info); });
}
int lcm_map_merge(lcm_handle* h, const lcm_dmatch* matches, const lcm_point_pair* pts, const lcm_map_tri* tri, const uint8_t* status, int n,
                  int kf1, int kf2, int32_t* table1, int n_kp1, int32_t* table2, int n_kp2, int n_points, lcm_ba_point* points_out,
                  int cap_points, lcm_ba_obs* obs_out, int cap_obs, uint8_t* status_out, int* n_new, int* n_merged) {
    return guarded([&] {
        return map_merge_impl(h, matches, pts, tri, status, n, kf1, kf2, table1, n_kp1, table2, n_kp2, n_points, points_out, cap_points, obs_out,
                              cap_obs, status_out, n_new, n_merged);
    });
}
int lcm_map_add_keyframe(lcm_handle* h, const lcm_dmatch* matches, const lcm_point_pair* pts, int n_matches, int kf_last,
                         const lcm_pgo_pose* pose_last, int32_t* table_last, int n_kp_last, int kf_new, int32_t* table_new, int n_kp_new,
                         int n_points, const lcm_map_params* mp, const lcm_epi_params* ep, const lcm_lo_params* lp, const lcm_pose_params* pp,
                         lcm_ba_point* points_out, int cap_points, lcm_ba_obs* obs_out, int cap_obs, uint8_t* status_out,
                         lcm_map_keyframe_report* report) {
    return guarded([&] {
        const lcm::MapTrack t{mp, kf_last, kf_new, pose_last, table_last, n_kp_last, table_new, n_kp_new, n_points, points_out, cap_points,
                              obs_out, cap_obs, status_out, report};
        return map_add_keyframe_impl(h, matches, pts, n_matches, t, ep, lp, pp);
    });
}

}  // extern "C"
