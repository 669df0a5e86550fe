// The pure host side of the bundle adjustment (csrc/lcm_ba_host.h: parameter and input checks, the plan of one observation list,
// the cameras' spread, the compaction, the loop's new observations) and the arithmetic of csrc/lcm_ba_device.h compiled for the
// host, as a stand-alone program: tests/test_ba_abi_host.py builds it with -fsanitize=address,undefined and runs it on the CPU.
// No device.  Exit status 0 = every check held.
#include <cstdio>
#include <limits>
#include <vector>

#include "lcm_ba_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static_assert(sizeof(lcm::Point3) == sizeof(lcm_ba_point) && sizeof(lcm_ba_point) == 24, "point");
static_assert(sizeof(lcm::Observation) == sizeof(lcm_ba_obs) && sizeof(lcm_ba_obs) == 24, "observation");
static_assert(sizeof(lcm::BaElemInfo) == sizeof(lcm_ba_elem_info) && sizeof(lcm_ba_elem_info) == 24, "element info");
static_assert(sizeof(lcm_ba_params) == 112 && sizeof(lcm_ba_info) == 184 && sizeof(lcm_ba_map_report) == 56, "records");

using U32 = std::vector<uint32_t>;
static const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

static lcm_pgo_pose pose_at(double x, double y, double z) {
    lcm_pgo_pose p;
    std::memcpy(p.R, I3, sizeof(I3));
    p.t[0] = -x; p.t[1] = -y; p.t[2] = -z;                              // centre -R^T t = (x, y, z)
    return p;
}

static lcm_ba_obs ob(int cam, int point, double u = 1.0, double v = 2.0) {
    lcm_ba_obs o;
    std::memset(&o, 0, sizeof(o));
    o.cam = cam; o.point = point; o.u = u; o.v = v;
    return o;
}

static lcm_ba_params good_params() {
    lcm_ba_params p;
    lcm::ba_params_default(&p);
    p.fx = p.fy = 1000.0; p.cx = 640.0; p.cy = 360.0;
    return p;
}

static void check_params() {
    lcm_ba_params p;
    std::memset(&p, 0xFF, sizeof(p));
    lcm::ba_params_default(&p);
    CHECK(p.fx == 0 && p.fy == 0 && p.cx == 0 && p.cy == 0 && p.eps == 1e-6 && p.damping == 1e-3 && p.min_update == 1e-6);
    CHECK(p.outlier_px == 5.0 && p.min_spread == 10.0 && p.spread_factor == 5.0 && p.outer_iters == 5 && p.inner_iters == 5);
    CHECK(p.min_cam_obs == 10 && p.min_point_obs == 2 && p.reserved[0] == 0 && p.reserved[3] == 0);
    CHECK(lcm::ba_params_problem(&p) != nullptr && lcm::ba_params_problem(nullptr) != nullptr);          // K has no default
    p = good_params();
    CHECK(lcm::ba_params_problem(&p) == nullptr);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    lcm_ba_params q = p; q.fx = 0.0; CHECK(lcm::ba_params_problem(&q));
    q = p; q.fy = -1.0; CHECK(lcm::ba_params_problem(&q));
    q = p; q.fx = nan; CHECK(lcm::ba_params_problem(&q));
    q = p; q.cy = inf; CHECK(lcm::ba_params_problem(&q));
    q = p; q.eps = 0.0; CHECK(lcm::ba_params_problem(&q));
    q = p; q.damping = -1e-9; CHECK(lcm::ba_params_problem(&q));
    q = p; q.min_update = 0.0; CHECK(!lcm::ba_params_problem(&q));
    q = p; q.min_update = nan; CHECK(lcm::ba_params_problem(&q));
    q = p; q.outlier_px = -1.0; CHECK(lcm::ba_params_problem(&q));
    q = p; q.outer_iters = 0; CHECK(lcm::ba_params_problem(&q));
    q = p; q.outer_iters = 16; CHECK(!lcm::ba_params_problem(&q));
    q = p; q.inner_iters = 17; CHECK(lcm::ba_params_problem(&q));
    q = p; q.min_cam_obs = -1; CHECK(lcm::ba_params_problem(&q));
    CHECK(lcm::ba_counts_problem(1, 1, 0).what == nullptr && lcm::ba_counts_problem(0, 1, 0).code == LCM_ERR_INVALID_ARG);
    CHECK(lcm::ba_counts_problem(1, 0, 0).code == LCM_ERR_INVALID_ARG && lcm::ba_counts_problem(1, 1, -1).code == LCM_ERR_INVALID_ARG);
    CHECK(lcm::ba_counts_problem(4096, 1 << 24, 1 << 24).what == nullptr && lcm::ba_counts_problem(4097, 1, 1).code == LCM_ERR_CAPACITY);
    CHECK(lcm::ba_counts_problem(1, (1 << 24) + 1, 1).code == LCM_ERR_CAPACITY && lcm::ba_counts_problem(1, 1, (1 << 24) + 1).code == LCM_ERR_CAPACITY);
}

static void check_plan_and_inputs() {
    // 3 cameras, 4 points, a shuffled list with a point seen twice by one camera
    const std::vector<lcm_ba_obs> obs = {ob(2, 1), ob(0, 3), ob(2, 0), ob(0, 1), ob(2, 1), ob(0, 0)};
    lcm::BaPlan pl;
    CHECK(!lcm::ba_plan(nullptr, 3, 4, obs.data(), 6, &pl).what);
    CHECK((pl.cam_off == U32{0, 3, 3, 6}) && (pl.cam_obs == U32{1, 3, 5, 0, 2, 4}));
    CHECK((pl.pt_off == U32{0, 2, 5, 5, 6}) && (pl.pt_obs == U32{2, 5, 0, 3, 4, 1}));
    CHECK(!lcm::ba_plan(nullptr, 3, 4, nullptr, 0, &pl).what && (pl.cam_off == U32{0, 0, 0, 0}) && pl.cam_obs.empty() && pl.pt_off.size() == 5);
    const uint8_t valid[3] = {1, 0, 1};
    CHECK(!lcm::ba_plan(valid, 3, 4, obs.data(), 6, &pl).what);
    std::vector<lcm_ba_obs> bad = obs;
    bad[2].cam = 1; CHECK(lcm::ba_plan(valid, 3, 4, bad.data(), 6, &pl).code == LCM_ERR_INVALID_ARG);            // an invalid camera
    bad = obs; bad[5].cam = 3; CHECK(lcm::ba_plan(nullptr, 3, 4, bad.data(), 6, &pl).what);
    bad = obs; bad[5].cam = -1; CHECK(lcm::ba_plan(nullptr, 3, 4, bad.data(), 6, &pl).what);
    bad = obs; bad[0].point = 4; CHECK(lcm::ba_plan(nullptr, 3, 4, bad.data(), 6, &pl).what);
    bad = obs; bad[0].point = -2; CHECK(lcm::ba_plan(nullptr, 3, 4, bad.data(), 6, &pl).what);

    std::vector<lcm_pgo_pose> poses = {pose_at(0, 0, 0), pose_at(1, 0, 0), pose_at(0, 2, 0)};
    std::vector<lcm_ba_point> points = {{0, 0, 5}, {1, 0, 5}, {0, 1, 5}, {1, 1, 5}};
    const lcm_ba_params p = good_params();
    CHECK(!lcm::ba_inputs_problem(poses.data(), valid, 3, points.data(), 4, obs.data(), 6, &p, &pl).what);
    CHECK(lcm::ba_inputs_problem(nullptr, valid, 3, points.data(), 4, obs.data(), 6, &p, &pl).what);
    CHECK(lcm::ba_inputs_problem(poses.data(), valid, 3, nullptr, 4, obs.data(), 6, &p, &pl).what);
    CHECK(lcm::ba_inputs_problem(poses.data(), valid, 3, points.data(), 4, nullptr, 6, &p, &pl).what);
    CHECK(!lcm::ba_inputs_problem(poses.data(), valid, 3, points.data(), 4, nullptr, 0, &p, &pl).what);
    CHECK(lcm::ba_inputs_problem(poses.data(), valid, 3, points.data(), 4, obs.data(), 6, nullptr, &pl).what);
    CHECK(lcm::ba_inputs_problem(poses.data(), valid, 4097, points.data(), 4, obs.data(), 6, &p, &pl).code == LCM_ERR_CAPACITY);   // nothing is read
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<lcm_pgo_pose> q = poses;
    q[1].t[0] = nan; CHECK(!lcm::ba_inputs_problem(q.data(), valid, 3, points.data(), 4, obs.data(), 6, &p, &pl).what);          // invalid: not read
    q[2].t[0] = nan; CHECK(lcm::ba_inputs_problem(q.data(), valid, 3, points.data(), 4, obs.data(), 6, &p, &pl).what);
    q = poses; q[0].R[0] = 1.001; CHECK(lcm::ba_inputs_problem(q.data(), valid, 3, points.data(), 4, obs.data(), 6, &p, &pl).what);
    q = poses; q[0].R[0] = -1.0; CHECK(lcm::ba_inputs_problem(q.data(), valid, 3, points.data(), 4, obs.data(), 6, &p, &pl).what);  // a reflection
    std::vector<lcm_ba_point> x = points;
    x[3].z = nan; CHECK(lcm::ba_inputs_problem(poses.data(), valid, 3, x.data(), 4, obs.data(), 6, &p, &pl).what);
    bad = obs; bad[4].v = std::numeric_limits<double>::infinity();
    CHECK(lcm::ba_inputs_problem(poses.data(), valid, 3, points.data(), 4, bad.data(), 6, &p, &pl).what);

    // the spread: centres (0,0,0), (1,0,0) [invalid], (0,2,0): centroid (0,1,0), distance 1, threshold max(10, 5) and max(2, 5)
    double c[3], thr = 0;
    lcm::ba_camera_spread(poses.data(), valid, 3, 10.0, 5.0, c, &thr);
    CHECK(c[0] == 0 && c[1] == 1 && c[2] == 0 && thr == 10.0);
    lcm::ba_camera_spread(poses.data(), valid, 3, 2.0, 5.0, c, &thr);
    CHECK(thr == 5.0);
    lcm::ba_camera_spread(poses.data(), nullptr, 3, 0.0, 3.0, c, &thr);
    CHECK(c[0] == 1.0 / 3 && c[1] == 2.0 / 3 && thr > 3.0 * 1.37 && thr < 3.0 * 1.38);
    const uint8_t none[3] = {0, 0, 0};
    lcm::ba_camera_spread(poses.data(), none, 3, 10.0, 5.0, c, &thr);
    CHECK(c[0] == 0 && c[1] == 0 && c[2] == 0 && thr == 10.0);
}

static void check_compaction_and_loop_observations() {
    const std::vector<lcm_ba_point> points = {{0, 0, 0}, {1, 1, 1}, {2, 2, 2}, {3, 3, 3}};
    const std::vector<lcm_ba_obs> obs = {ob(0, 3, 30, 31), ob(1, 1, 10, 11), ob(0, 0, 0, 1), ob(2, 3, 32, 33), ob(1, 2, 20, 21)};
    const uint8_t flags[4] = {0, 1, 0, 0};
    int kp = -1, ko = -1;
    lcm::ba_compact_counts(flags, 4, obs.data(), 5, &kp, &ko);
    CHECK(kp == 3 && ko == 4);
    std::vector<lcm_ba_point> xo(3);
    std::vector<lcm_ba_obs> oo(4);
    int32_t table[4];
    lcm::ba_compact(points.data(), 4, obs.data(), 5, flags, xo.data(), oo.data(), table);
    CHECK(table[0] == 0 && table[1] == -1 && table[2] == 1 && table[3] == 2 && xo[1].x == 2 && xo[2].z == 3);
    CHECK(oo[0].point == 2 && oo[0].cam == 0 && oo[0].u == 30 && oo[1].point == 0 && oo[2].point == 2 && oo[2].cam == 2 && oo[3].point == 1 && oo[3].v == 21);
    lcm::ba_compact(points.data(), 4, obs.data(), 5, flags, xo.data(), oo.data(), nullptr);
    const uint8_t all[4] = {1, 1, 1, 1};
    lcm::ba_compact_counts(all, 4, obs.data(), 5, &kp, &ko);
    CHECK(kp == 0 && ko == 0);
    lcm::ba_compact(points.data(), 4, obs.data(), 5, all, nullptr, nullptr, table);
    CHECK(table[0] == -1 && table[3] == -1);

    // :1496-1513
    std::vector<lcm_dmatch> matches(4);
    const int q[4] = {2, 0, 1, 3}, t[4] = {1, 2, 0, 3};
    for (int k = 0; k < 4; ++k) { matches[k].query_idx = q[k]; matches[k].train_idx = t[k]; matches[k].img_idx = 0; matches[k].distance = 0.f; }
    const uint8_t mask[4] = {1, 1, 0, 1};
    const int32_t past[4] = {7, 5, -1, 9};
    int32_t curr[4] = {-1, -1, 4, -1};
    const float kpts[8] = {0.5f, 1.5f, 2.5f, 3.5f, 4.5f, 5.5f, 6.5f, 7.5f};
    int n = -1;
    CHECK(!lcm::ba_loop_observations_problem(matches.data(), mask, 4, past, 4, 4, 10, &n) && n == 2);
    std::vector<lcm_ba_obs> out(2);
    lcm::ba_add_loop_observations(matches.data(), mask, 4, past, curr, kpts, 6, out.data());
    CHECK(out[0].cam == 6 && out[0].point == 5 && out[0].u == 4.5 && out[0].v == 5.5 && out[1].point == 9 && out[1].u == 6.5);
    CHECK(curr[0] == -1 && curr[1] == -1 && curr[2] == 5 && curr[3] == 9);
    CHECK(lcm::ba_loop_observations_problem(matches.data(), mask, 4, past, 4, 4, 9, &n));       // point 9 is out of range
    CHECK(lcm::ba_loop_observations_problem(matches.data(), mask, 4, past, 3, 4, 10, &n));      // train_idx 3
    CHECK(lcm::ba_loop_observations_problem(matches.data(), mask, 4, past, 4, 3, 10, &n));      // query_idx 3
    matches[2].query_idx = 99;                                                                   // not masked: not looked at
    CHECK(!lcm::ba_loop_observations_problem(matches.data(), mask, 4, past, 4, 4, 10, &n) && n == 2);
    CHECK(!lcm::ba_loop_observations_problem(nullptr, nullptr, 0, nullptr, 0, 0, 0, &n) && n == 0);
    lcm_ba_elem_info infos[4] = {{0, 0, 0, 4}, {0, 0, 1, 0}, {0, 0, 5, 1}, {0, 0, 0, 4}};
    int32_t count[5];
    lcm::ba_count_statuses(infos, 4, count);
    CHECK(count[0] == 1 && count[1] == 1 && count[2] == 0 && count[3] == 0 && count[4] == 2);
}

// the camera point, the projection, exp / log and the Cholesky solves: tests/cpp/geom_host_check.cpp
static void check_arithmetic() {
    // the residual on exact numbers: Xc = (2, 2, 4), u = 1000 * 2 / 4 + 640, v likewise + 360
    const lcm::Camera K{1000.0, 1000.0, 640.0, 360.0};
    const double Xc[3] = {2, 2, 4};
    double r[2];
    lcm::ba_residual(K, Xc, 1140.0, 857.0, r);
    CHECK(r[0] == 0.0 && r[1] == 3.0 && lcm::ba_error(r) == 3.0);
    const double zero[3] = {2, 2, 0};
    lcm::ba_residual(K, zero, 0.0, 0.0, r);
    CHECK(std::isinf(r[0]) && std::isinf(r[1]));
    const double rp[2] = {3.0, 1.0}, rm[2] = {1.0, 2.0};
    double col[2];
    lcm::ba_column(rp, rm, 0.5 / 0.25, col);
    CHECK(col[0] == 4.0 && col[1] == -2.0);
    // the running sums: two rows of one observation
    const double Ju[3] = {1, 2, 3}, Jv[3] = {0, 1, -1}, rr[2] = {2, 3};
    double H[6] = {0}, g[3] = {0}, cost = 0;
    lcm::ba_accumulate<3>(Ju, Jv, rr, H, g, cost);
    CHECK(H[0] == 1 && H[1] == 2 && H[2] == 5 && H[3] == 3 && H[4] == 5 && H[5] == 10 && g[0] == 2 && g[1] == 7 && g[2] == 3 && cost == 13);
}

int main() {
    check_params();
    check_plan_and_inputs();
    check_compaction_and_loop_observations();
    check_arithmetic();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all held\n");
    return 0;
}
