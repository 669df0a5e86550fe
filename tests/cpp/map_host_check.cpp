// The pure host side of the map building before the loop (csrc/lcm_map_host.h: parameter and offset checks, the per-pair plan, the
// checks of a merge's lists, the keyframe gates, the new keyframe's pose) and the arithmetic of csrc/lcm_map_device.h compiled for
// the host, as a stand-alone program: tests/test_map_abi_host.py builds it with -fsanitize=address,undefined and runs it on the
// CPU.  No device.  Exit status 0 = every check held.
#include <cstdio>
#include <limits>
#include <vector>

#include "lcm_map_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static_assert(sizeof(lcm::MapTri) == sizeof(lcm_map_tri) && sizeof(lcm_map_tri) == 64, "tri");
static_assert(sizeof(lcm::Point3) == sizeof(lcm_ba_point) && sizeof(lcm::Observation) == sizeof(lcm_ba_obs), "map records");
static_assert(sizeof(lcm_map_params) == 112 && sizeof(lcm_map_pair_info) == 48 && sizeof(lcm_map_keyframe_report) == 168 && sizeof(lcm::MapPair) == 448, "records");
static_assert(lcm::sym_index<4>(0, 0) == 0 && lcm::sym_index<4>(0, 3) == 3 && lcm::sym_index<4>(1, 1) == 4 && lcm::sym_index<4>(3, 1) == 6 && lcm::sym_index<4>(2, 2) == 7 &&
              lcm::sym_index<4>(2, 3) == 8 && lcm::sym_index<4>(3, 3) == 9, "packed upper triangle");

static const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

static lcm_pgo_pose pose_at(double x, double y, double z) {
    lcm_pgo_pose p;
    std::memcpy(p.R, I3, sizeof(I3));
    p.t[0] = -x; p.t[1] = -y; p.t[2] = -z;                              // centre -R^T t = (x, y, z)
    return p;
}

static lcm_map_params good_params() {
    lcm_map_params p;
    lcm::map_params_default(&p);
    p.fx = p.fy = 1000.0; p.cx = 640.0; p.cy = 360.0;
    return p;
}

static void check_params() {
    lcm_map_params p;
    std::memset(&p, 0xFF, sizeof(p));
    lcm::map_params_default(&p);
    CHECK(p.fx == 0 && p.fy == 0 && p.cx == 0 && p.cy == 0 && p.min_parallax_deg == 1.0 && p.max_reproj == 4.0 && p.min_depth == 0.1);
    CHECK(p.max_depth == 50.0 && p.min_displacement == 20.0 && p.max_displacement == 150.0 && p.min_inlier_ratio == 0.3);
    CHECK(p.min_tracked == 100 && p.min_inliers == 50 && p.min_pose_inliers == 10 && p.reserved[0] == 0 && p.reserved[2] == 0);
    CHECK(lcm::map_params_problem(&p) != nullptr && lcm::map_params_problem(nullptr) != nullptr);      // K has no default
    p = good_params();
    CHECK(lcm::map_params_problem(&p) == nullptr);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    lcm_map_params q = p; q.fx = 0.0; CHECK(lcm::map_params_problem(&q));
    q = p; q.fy = -1.0; CHECK(lcm::map_params_problem(&q));
    q = p; q.fx = nan; CHECK(lcm::map_params_problem(&q));
    q = p; q.cx = inf; CHECK(lcm::map_params_problem(&q));
    q = p; q.min_parallax_deg = -1.0; CHECK(lcm::map_params_problem(&q));
    q = p; q.min_parallax_deg = 181.0; CHECK(lcm::map_params_problem(&q));
    q = p; q.min_parallax_deg = nan; CHECK(lcm::map_params_problem(&q));
    q = p; q.min_parallax_deg = 0.0; CHECK(!lcm::map_params_problem(&q));
    q = p; q.max_reproj = -0.5; CHECK(lcm::map_params_problem(&q));
    q = p; q.max_reproj = inf; CHECK(!lcm::map_params_problem(&q));
    q = p; q.min_depth = nan; CHECK(lcm::map_params_problem(&q));
    q = p; q.max_displacement = nan; CHECK(lcm::map_params_problem(&q));
    q = p; q.min_inlier_ratio = nan; CHECK(lcm::map_params_problem(&q));
    q = p; q.min_tracked = -1; CHECK(lcm::map_params_problem(&q));
    q = p; q.min_pose_inliers = -1; CHECK(lcm::map_params_problem(&q));
    CHECK(lcm::map_cos_min(0.0) == 1.0 && lcm::map_cos_min(60.0) > 0.4999999 && lcm::map_cos_min(60.0) < 0.5000001 && lcm::map_cos_min(180.0) == -1.0);
}

static void check_offsets() {
    size_t total = 9;
    uint32_t max_n = 9;
    const size_t a[4] = {0, 5, 5, 12};
    lcm::MapProblem r = lcm::map_offsets_problem(a, 3, &total, &max_n);
    CHECK(!r.what && r.code == LCM_OK && total == 12 && max_n == 7);
    r = lcm::map_offsets_problem(a, 0, &total, &max_n);
    CHECK(!r.what && total == 0 && max_n == 0);
    CHECK(lcm::map_offsets_problem(a, -1, &total, &max_n).code == LCM_ERR_INVALID_ARG);
    CHECK(lcm::map_offsets_problem(nullptr, 1, &total, &max_n).code == LCM_ERR_INVALID_ARG);
    CHECK(lcm::map_offsets_problem(nullptr, LCM_MAP_MAX_PAIRS + 1, &total, &max_n).code == LCM_ERR_CAPACITY);      // from the count alone
    const size_t b[3] = {1, 2, 3}, c[3] = {0, 4, 3}, d[2] = {0, (size_t)LCM_MAP_MAX_RECORDS + 1}, e[2] = {0, (size_t)LCM_MAP_MAX_RECORDS};
    CHECK(lcm::map_offsets_problem(b, 2, &total, &max_n).code == LCM_ERR_INVALID_ARG);
    CHECK(lcm::map_offsets_problem(c, 2, &total, &max_n).code == LCM_ERR_INVALID_ARG);
    CHECK(lcm::map_offsets_problem(d, 1, &total, &max_n).code == LCM_ERR_CAPACITY);
    CHECK(!lcm::map_offsets_problem(e, 1, &total, &max_n).what && total == (size_t)LCM_MAP_MAX_RECORDS && max_n == (uint32_t)LCM_MAP_MAX_RECORDS);
    std::vector<size_t> many((size_t)LCM_MAP_MAX_PAIRS + 1, 0);
    CHECK(!lcm::map_offsets_problem(many.data(), LCM_MAP_MAX_PAIRS, &total, &max_n).what && total == 0);
}

static void check_plan_and_record() {
    const lcm_map_params mp = good_params();
    const lcm_pgo_pose P1 = pose_at(0, 0, 0), P2 = pose_at(1, 0, 0);
    CHECK(!lcm::map_pose_problem(P1) && !lcm::map_pose_problem(P2));
    lcm_pgo_pose bad = P1; bad.R[0] = 2.0; CHECK(lcm::map_pose_problem(bad));
    bad = P1; bad.t[1] = std::numeric_limits<double>::infinity(); CHECK(lcm::map_pose_problem(bad));
    lcm::MapPair pr;
    lcm::map_plan_pair(mp, P1, P2, &pr);
    CHECK(pr.baseline == 1.0 && pr.C1[0] == 0.0 && pr.C2[0] == 1.0 && pr.C2[1] == 0.0 && pr.cos_min == lcm::map_cos_min(1.0));
    CHECK(pr.P1[0] == 1000.0 && pr.P1[2] == 640.0 && pr.P1[3] == 0.0 && pr.P1[5] == 1000.0 && pr.P1[6] == 360.0 && pr.P1[10] == 1.0);
    CHECK(pr.P2[3] == -1000.0 && pr.P2[7] == 0.0 && pr.P2[11] == 0.0 && pr.t2[0] == -1.0 && pr.R2[4] == 1.0);
    const lcm::Camera K{mp.fx, mp.fy, mp.cx, mp.cy};
    const lcm::MapLimits lim{mp.min_depth, mp.max_depth, mp.max_reproj};
    lcm::MapTri t;
    // the point (0.5, 0.25, 5): pixels 740, 410 and 540, 410, all floats
    CHECK(lcm::map_record(pr, K, lim, 740.f, 410.f, 540.f, 410.f, t) == lcm::MAP_ACCEPTED);
    CHECK(std::fabs(t.X[0] - 0.5) < 1e-12 && std::fabs(t.X[1] - 0.25) < 1e-12 && std::fabs(t.X[2] - 5.0) < 1e-11);
    CHECK(std::fabs(t.depth1 - 5.0) < 1e-11 && std::fabs(t.depth2 - 5.0) < 1e-11 && t.err1 < 1e-9 && t.err2 < 1e-9 && t.cos_parallax < 0.99);
    // the same pixel in both views: a point at infinity, exactly w = 0
    CHECK(lcm::map_record(pr, K, lim, 700.f, 300.f, 700.f, 300.f, t) == lcm::MAP_NO_POINT);
    CHECK(t.X[0] == 0 && t.X[1] == 0 && t.X[2] == 0 && t.depth1 == 0 && t.depth2 == 0 && t.cos_parallax == 0 && t.err1 == 0 && t.err2 == 0);
    // crossed rays: the point lies behind both cameras
    CHECK(lcm::map_record(pr, K, lim, 540.f, 410.f, 740.f, 410.f, t) == lcm::MAP_REJ_DEPTH && t.depth1 < 0 && t.err1 == lcm::MAP_BEHIND);
    // 100 baselines away: beyond max_depth; 30 away with 0.5 degrees wanted: fine; with 5 degrees wanted: too little parallax
    CHECK(lcm::map_record(pr, K, lim, 640.f, 360.f, 630.f, 360.f, t) == lcm::MAP_REJ_DEPTH && std::fabs(t.depth1 - 100.0) < 1e-8);
    lcm_map_params wide = mp; wide.min_parallax_deg = 5.0;
    lcm::MapPair pw;
    lcm::map_plan_pair(wide, P1, P2, &pw);
    CHECK(lcm::map_record(pw, K, lim, 640.f, 360.f, 600.f, 360.f, t) == lcm::MAP_REJ_PARALLAX && std::fabs(t.depth1 - 25.0) < 1e-9);
    CHECK(lcm::map_record(pr, K, lim, 640.f, 360.f, 600.f, 360.f, t) == lcm::MAP_ACCEPTED);
    // the train pixel 20 px off the epipolar line
    CHECK(lcm::map_record(pr, K, lim, 740.f, 410.f, 540.f, 430.f, t) == lcm::MAP_REJ_REPROJ && t.err1 > 4.0 && t.err2 > 4.0);
    // baseline 0 and no rotation: IEEE decides, nothing traps
    lcm::MapPair p0;
    lcm::map_plan_pair(mp, P1, P1, &p0);
    CHECK(p0.baseline == 0.0);
    (void)lcm::map_record(p0, K, lim, 740.f, 410.f, 540.f, 410.f, t);
    CHECK(lcm::map_displacement(1.f, 2.f, 4.f, 6.f) == 5.0 && lcm::map_displacement(7.f, 7.f, 7.f, 7.f) == 0.0);
}

static lcm_dmatch dm(int q, int t) { lcm_dmatch m; std::memset(&m, 0, sizeof(m)); m.query_idx = q; m.train_idx = t; return m; }

static void check_merge_lists() {
    std::vector<lcm_dmatch> m{dm(0, 3), dm(2, 1), dm(1, 3)};
    std::vector<uint8_t> st{LCM_MAP_ACCEPTED, LCM_MAP_REJ_DEPTH, LCM_MAP_ACCEPTED}, seen;
    std::vector<int32_t> t1{-1, 4, -1}, t2{-1, -1, -1, -1};
    CHECK(!lcm::map_merge_problem(m.data(), st.data(), 3, t1.data(), 3, t2.data(), 4, 5, seen));
    CHECK(!lcm::map_merge_problem(m.data(), nullptr, 3, t1.data(), 3, t2.data(), 4, 5, seen));
    CHECK(!lcm::map_merge_problem(nullptr, nullptr, 0, nullptr, 0, nullptr, 0, 0, seen));
    int a = -1, b = -1;
    lcm::map_merge_counts(m.data(), st.data(), 3, t1.data(), &a, &b);
    CHECK(a == 1 && b == 1);
    auto with = [&](int i, lcm_dmatch v) { std::vector<lcm_dmatch> c = m; c[(size_t)i] = v; return c; };
    CHECK(lcm::map_merge_problem(with(2, dm(0, 2)).data(), st.data(), 3, t1.data(), 3, t2.data(), 4, 5, seen));      // query_idx twice
    CHECK(lcm::map_merge_problem(with(1, dm(0, 2)).data(), st.data(), 3, t1.data(), 3, t2.data(), 4, 5, seen));      // ... a rejected record's too
    CHECK(lcm::map_merge_problem(with(0, dm(3, 0)).data(), st.data(), 3, t1.data(), 3, t2.data(), 4, 5, seen));
    CHECK(lcm::map_merge_problem(with(0, dm(-1, 0)).data(), st.data(), 3, t1.data(), 3, t2.data(), 4, 5, seen));
    CHECK(lcm::map_merge_problem(with(0, dm(0, 4)).data(), st.data(), 3, t1.data(), 3, t2.data(), 4, 5, seen));
    CHECK(lcm::map_merge_problem(m.data(), st.data(), 3, t1.data(), 3, t2.data(), 4, 4, seen));                      // table1 names point 4 of 4
    std::vector<int32_t> low{-2, 4, -1}, t2bad{-1, 7, -1, -1};
    CHECK(lcm::map_merge_problem(m.data(), st.data(), 3, low.data(), 3, t2.data(), 4, 5, seen));
    CHECK(lcm::map_merge_problem(m.data(), st.data(), 3, t1.data(), 3, t2bad.data(), 4, 5, seen));
    std::vector<uint8_t> merged{LCM_MAP_ACCEPTED, LCM_MAP_MERGED, LCM_MAP_ACCEPTED};
    CHECK(lcm::map_merge_problem(m.data(), merged.data(), 3, t1.data(), 3, t2.data(), 4, 5, seen));
}

static void check_gates_and_pose() {
    const lcm_map_params mp = good_params();
    CHECK(lcm::map_motion_verdict(mp, 99, 50.0) == LCM_MAP_FEW_MATCHES && lcm::map_motion_verdict(mp, 100, 50.0) == LCM_MAP_KEYFRAME);
    CHECK(lcm::map_motion_verdict(mp, 100, 19.999) == LCM_MAP_LITTLE_MOTION && lcm::map_motion_verdict(mp, 100, 20.0) == LCM_MAP_KEYFRAME);
    CHECK(lcm::map_motion_verdict(mp, 100, 150.0) == LCM_MAP_KEYFRAME && lcm::map_motion_verdict(mp, 100, 150.001) == LCM_MAP_MUCH_MOTION);
    lcm_pose_result pr;
    std::memset(&pr, 0, sizeof(pr));
    int n = -1;
    pr.status = LCM_POSE_NO_MODEL; pr.n_good = 500;
    CHECK(lcm::map_pose_verdict(mp, 1000, pr, &n) == LCM_MAP_NO_POSE && n == 0);
    pr.status = LCM_POSE_OK; pr.n_good = 9;
    CHECK(lcm::map_pose_verdict(mp, 1000, pr, &n) == LCM_MAP_NO_POSE);
    pr.n_good = 7;
    CHECK(lcm::map_pose_verdict(mp, 7, pr, &n) == LCM_MAP_NO_POSE);
    pr.n_good = 49;
    CHECK(lcm::map_pose_verdict(mp, 100, pr, &n) == LCM_MAP_FEW_INLIERS && n == 49);
    pr.n_good = 50;
    CHECK(lcm::map_pose_verdict(mp, 100, pr, &n) == LCM_MAP_KEYFRAME && n == 50);
    CHECK(lcm::map_pose_verdict(mp, 167, pr, &n) == LCM_MAP_FEW_INLIERS);                        // 50 / 167 < 0.3
    CHECK(lcm::map_pose_verdict(mp, 166, pr, &n) == LCM_MAP_KEYFRAME);
    // R_new = R R_last, t_new = R t_last + t with a quarter turn about z
    const double Rz[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(pr.R, Rz, sizeof(Rz));
    pr.t[0] = 1; pr.t[1] = 0; pr.t[2] = 0;
    lcm_pgo_pose last = pose_at(0, 0, 0), out;
    std::memcpy(last.R, Rz, sizeof(Rz));
    last.t[0] = 2; last.t[1] = 3; last.t[2] = 4;
    lcm::map_new_pose(pr, last, &out);
    const double want[9] = {-1, 0, 0, 0, -1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k) CHECK(out.R[k] == want[k]);
    CHECK(out.t[0] == -3 + 1 && out.t[1] == 2 && out.t[2] == 4);
}

int main() {
    check_params();
    check_offsets();
    check_plan_and_record();
    check_merge_lists();
    check_gates_and_pose();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all held\n");
    return 0;
}
