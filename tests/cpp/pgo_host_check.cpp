// The pure host side of the pose-graph correction (csrc/lcm_pgo_host.h: parameter and input checks, the plan of one graph, the
// host-only calls) and the edge residual of csrc/lcm_pgo_device.h compiled for the host, as a stand-alone program:
// tests/test_pgo_abi_host.py builds it with -fsanitize=address,undefined and runs it on the CPU.  No device.  Whole plans are
// compared with literals for the graph shapes of tests/test_gpu_pgo.py.  Exit status 0 = every check held.
#include <cstdio>
#include <limits>
#include <utility>
#include <vector>

#include "lcm_pgo_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static_assert(sizeof(lcm::Pose) == sizeof(lcm_pgo_pose) && sizeof(lcm_pgo_pose) == 96, "pose");
static_assert(sizeof(lcm::PgoEdge) == sizeof(lcm_pgo_edge) && sizeof(lcm_pgo_edge) == 112, "edge");
static_assert(sizeof(lcm_pgo_params) == 64 && sizeof(lcm_pgo_info) == 48 && offsetof(lcm::PgoState, done) == 48, "records");

using Ints = std::vector<int32_t>;
using Ends = std::vector<std::pair<int, int>>;

static const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

static std::vector<lcm_pgo_edge> edges_of(const Ends& ends) {
    std::vector<lcm_pgo_edge> e(ends.size());
    for (size_t k = 0; k < ends.size(); ++k) {
        std::memset(&e[k], 0, sizeof(e[k]));
        std::memcpy(e[k].R, I3, sizeof(I3));
        e[k].weight = 1.0; e[k].from = ends[k].first; e[k].to = ends[k].second;
    }
    return e;
}

static lcm::PgoProblem plan_of(const Ends& ends, int n_poses, const std::vector<uint8_t>& valid, lcm::PgoPlan* pl) {
    const std::vector<lcm_pgo_edge> e = edges_of(ends);
    return lcm::pgo_plan(valid.empty() ? nullptr : valid.data(), n_poses, e.data(), (int)e.size(), pl);
}

static Ends chain(int n) {
    Ends e;
    for (int i = 1; i < n; ++i) e.push_back({i - 1, i});
    return e;
}

static void check_plans() {
    lcm::PgoPlan pl;
    // 2 poses, one edge from pose 0: one block, no coupling, no border
    CHECK(!plan_of({{0, 1}}, 2, {}, &pl).what);
    CHECK(pl.n_int == 1 && pl.n_border == 0 && pl.n_loops == 0 && pl.ncols == 1);
    CHECK((pl.slot == Ints{-1, 0}) && (pl.int_pose == Ints{1}) && pl.border_pose.empty());
    CHECK((pl.seg_first == Ints{0}) && (pl.seg_len == Ints{1}));
    CHECK((pl.pose_off == Ints{0, 1, 2}) && (pl.pose_edge == Ints{0, 1}));
    CHECK(pl.blk_doubles == 36 && pl.b_doubles == 0 && pl.w_doubles == 6 && pl.s_doubles == 0 && pl.t_doubles == 0 && pl.g_doubles == 6);
    CHECK(pl.tab_off == 2 && pl.tab_edge == 5 && pl.tab_int == 7 && pl.tab_border == 8 && pl.tab_words == 8);
    Ints tab;
    lcm::pgo_plan_table(pl, &tab);
    CHECK((tab == Ints{-1, 0, 0, 1, 2, 0, 1, 1}));
    // 3 poses, a loop edge ending in pose 0: no border pose for that end
    CHECK(!plan_of({{0, 1}, {1, 2}, {0, 2}}, 3, {}, &pl).what);
    CHECK(pl.n_int == 1 && pl.n_border == 1 && pl.n_loops == 1 && pl.ncols == 7);
    CHECK((pl.slot == Ints{-1, 0, 1}) && (pl.int_pose == Ints{1}) && (pl.border_pose == Ints{2}));
    CHECK((pl.pose_off == Ints{0, 2, 4, 6}) && (pl.pose_edge == Ints{0, 4, 1, 2, 3, 5}));
    CHECK(pl.b_doubles == 36 && pl.w_doubles == 42 && pl.s_doubles == 36 && pl.t_doubles == 42 && pl.g_doubles == 12);
    // an invalid pose in the middle: two interior segments, the far one reached only through the loop edge
    CHECK(!plan_of({{0, 1}, {1, 2}, {4, 5}, {1, 4}}, 6, {1, 1, 1, 0, 1, 1}, &pl).what);
    CHECK(pl.n_int == 2 && pl.n_border == 2 && pl.n_loops == 1);
    CHECK((pl.slot == Ints{-1, 2, 0, -1, 3, 1}) && (pl.int_pose == Ints{2, 5}) && (pl.border_pose == Ints{1, 4}));
    CHECK((pl.seg_first == Ints{0, 1}) && (pl.seg_len == Ints{1, 1}));
    CHECK((pl.pose_off == Ints{0, 1, 4, 5, 5, 7, 8}) && (pl.pose_edge == Ints{0, 1, 2, 6, 3, 4, 7, 5}));
    // two loop edges sharing an endpoint, two border poses adjacent in index, a border pose at n_poses - 2 and an interior one behind
    Ends e = chain(8);
    e.push_back({2, 6}); e.push_back({2, 5});
    CHECK(!plan_of(e, 8, {}, &pl).what);
    CHECK(pl.n_int == 4 && pl.n_border == 3 && pl.n_loops == 2 && pl.ncols == 19);
    CHECK((pl.slot == Ints{-1, 0, 4, 1, 2, 5, 6, 3}) && (pl.int_pose == Ints{1, 3, 4, 7}) && (pl.border_pose == Ints{2, 5, 6}));
    CHECK((pl.seg_first == Ints{0, 1, 3}) && (pl.seg_len == Ints{1, 2, 1}));
    CHECK(pl.pose_off[2] == 3 && pl.pose_off[3] == 7 && pl.pose_edge[3] == 3 && pl.pose_edge[4] == 4 && pl.pose_edge[5] == 14 && pl.pose_edge[6] == 16);
    // a border pose at index 1 and at n_poses - 1; a valid pose no edge reaches; duplicate edges
    e = {{0, 1}, {1, 2}, {4, 5}, {1, 5}, {1, 5}, {4, 5}};
    CHECK(!plan_of(e, 6, {}, &pl).what);
    CHECK(pl.n_loops == 2 && (pl.border_pose == Ints{1, 5}) && (pl.int_pose == Ints{2, 3, 4}) && (pl.seg_len == Ints{3}));
    CHECK(pl.pose_off[3] == pl.pose_off[4]);                     // pose 3: valid, unreached, still an unknown
    // 8 loop edges with 16 distinct border poses: the largest border
    e = chain(40);
    for (int k = 0; k < 8; ++k) e.push_back({1 + 2 * k, 38 - 2 * k});
    CHECK(!plan_of(e, 40, {}, &pl).what);
    CHECK(pl.n_loops == 8 && pl.n_border == 16 && pl.n_int == 23 && pl.ncols == 97);
    CHECK(pl.s_doubles == 96 * 96 && pl.t_doubles == 96 * 97 && pl.b_doubles == 23u * 6 * 96 && pl.w_doubles == 23u * 6 * 97);
    e.push_back({0, 20});
    const lcm::PgoProblem nine = plan_of(e, 40, {}, &pl);
    CHECK(nine.code == LCM_ERR_CAPACITY && nine.what);
    // the pose limit, and what device memory it costs with the largest border
    e = chain(LCM_PGO_MAX_POSES);
    for (int k = 0; k < 8; ++k) e.push_back({10 + 2 * k, 4000 - 2 * k});
    CHECK(!plan_of(e, LCM_PGO_MAX_POSES, {}, &pl).what);
    CHECK(pl.n_int == 4095 - 16 && pl.w_doubles * sizeof(double) < 19000000 && pl.b_doubles < pl.w_doubles);
    CHECK(plan_of(chain(LCM_PGO_MAX_POSES + 1), LCM_PGO_MAX_POSES + 1, {}, &pl).code == LCM_ERR_CAPACITY);
    // refusals of the structure
    CHECK(plan_of({{0, 1}}, 1, {}, &pl).code == LCM_ERR_INVALID_ARG);
    CHECK(plan_of({}, 2, {}, &pl).code == LCM_ERR_INVALID_ARG);
    CHECK(plan_of({{0, 1}}, 2, {0, 1}, &pl).code == LCM_ERR_INVALID_ARG);              // pose 0 invalid
    CHECK(plan_of({{0, 1}, {1, 1}}, 3, {}, &pl).code == LCM_ERR_INVALID_ARG);          // from == to
    CHECK(plan_of({{0, 1}, {1, 3}}, 3, {}, &pl).code == LCM_ERR_INVALID_ARG);          // out of range
    CHECK(plan_of({{0, 1}, {-1, 2}}, 3, {}, &pl).code == LCM_ERR_INVALID_ARG);
    CHECK(plan_of({{0, 1}, {1, 2}}, 3, {1, 1, 0}, &pl).code == LCM_ERR_INVALID_ARG);   // an invalid endpoint
}

static void check_params_and_values() {
    lcm_pgo_params p;
    std::memset(&p, 0xFF, sizeof(p));
    lcm::pgo_params_default(&p);
    CHECK(p.eps == 1e-6 && p.damping == 1e-4 && p.min_update == 1e-6 && p.loop_weight == 10.0 && p.max_iters == 20 && p.loop_direction == 0);
    for (int k = 0; k < 6; ++k) CHECK(p.reserved[k] == 0);
    CHECK(!lcm::pgo_params_problem(nullptr) && !lcm::pgo_params_problem(&p));
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    lcm_pgo_params q = p;
    q.eps = 0.0; CHECK(lcm::pgo_params_problem(&q)); q.eps = nan; CHECK(lcm::pgo_params_problem(&q)); q.eps = inf; CHECK(lcm::pgo_params_problem(&q));
    q = p; q.damping = -1e-9; CHECK(lcm::pgo_params_problem(&q)); q.damping = 0.0; CHECK(!lcm::pgo_params_problem(&q));
    q = p; q.min_update = nan; CHECK(lcm::pgo_params_problem(&q)); q.min_update = 0.0; CHECK(!lcm::pgo_params_problem(&q));
    q = p; q.loop_weight = -1.0; CHECK(lcm::pgo_params_problem(&q)); q.loop_weight = inf; CHECK(lcm::pgo_params_problem(&q));
    q = p; q.max_iters = 0; CHECK(lcm::pgo_params_problem(&q)); q.max_iters = 101; CHECK(lcm::pgo_params_problem(&q));
    q.max_iters = 100; CHECK(!lcm::pgo_params_problem(&q)); q.max_iters = 1; CHECK(!lcm::pgo_params_problem(&q));
    q = p; q.loop_direction = 2; CHECK(lcm::pgo_params_problem(&q)); q.loop_direction = 1; CHECK(!lcm::pgo_params_problem(&q));

    double R[9];
    std::memcpy(R, I3, sizeof(R));
    CHECK(!lcm::pgo_rotation_problem(R));
    R[1] = 9e-7; CHECK(!lcm::pgo_rotation_problem(R));
    R[1] = 2e-6; CHECK(lcm::pgo_rotation_problem(R));
    R[1] = 0.0; R[8] = -1.0; CHECK(lcm::pgo_rotation_problem(R));                      // a reflection
    R[8] = nan; CHECK(lcm::pgo_rotation_problem(R));
    std::vector<lcm_pgo_pose> poses(3);
    for (auto& ps : poses) { std::memset(&ps, 0, sizeof(ps)); std::memcpy(ps.R, I3, sizeof(I3)); }
    std::vector<lcm_pgo_edge> e = edges_of({{0, 1}, {1, 2}});
    CHECK(!lcm::pgo_values_problem(poses.data(), nullptr, 3, e.data(), 2));
    e[1].weight = -0.5; CHECK(lcm::pgo_values_problem(poses.data(), nullptr, 3, e.data(), 2));
    e[1].weight = nan; CHECK(lcm::pgo_values_problem(poses.data(), nullptr, 3, e.data(), 2));
    e[1].weight = 0.0; CHECK(!lcm::pgo_values_problem(poses.data(), nullptr, 3, e.data(), 2));
    e[0].t[2] = inf; CHECK(lcm::pgo_values_problem(poses.data(), nullptr, 3, e.data(), 2));
    e[0].t[2] = 0.0; poses[2].t[0] = nan;
    CHECK(lcm::pgo_values_problem(poses.data(), nullptr, 3, e.data(), 2));
    const uint8_t valid[3] = {1, 1, 0};
    CHECK(!lcm::pgo_values_problem(poses.data(), valid, 3, e.data(), 1));              // an invalid pose's contents are not read
    lcm::PgoPlan pl;
    CHECK(lcm::pgo_inputs_problem(nullptr, nullptr, 3, e.data(), 2, nullptr, &pl).code == LCM_ERR_INVALID_ARG);
    CHECK(lcm::pgo_inputs_problem(poses.data(), nullptr, 3, nullptr, 2, nullptr, &pl).code == LCM_ERR_INVALID_ARG);
    poses[2].t[0] = 0.0;
    CHECK(lcm::pgo_inputs_problem(poses.data(), nullptr, 3, e.data(), 2, nullptr, &pl).code == LCM_OK && pl.n_int == 2);
}

// exp, log, the products and the 6 x 6 Cholesky: tests/cpp/geom_host_check.cpp
static void check_arithmetic_and_host_calls() {
    // the graph of :1441-1470 over four poses, pose 2 invalid; the drift and the linear correction of a known rotation
    std::vector<lcm_pgo_pose> poses(4);
    for (int i = 0; i < 4; ++i) {
        const double ri[3] = {0.0, 0.1 * i, 0.0};
        std::memset(&poses[i], 0, sizeof(poses[i]));
        lcm::so3_exp(ri, poses[i].R);
        poses[i].t[0] = i; poses[i].t[2] = -2.0 * i;
    }
    const uint8_t valid[4] = {1, 1, 0, 1};
    const double tl[3] = {1, 2, 3};
    std::vector<lcm_pgo_edge> out(4);
    CHECK(lcm::pgo_build_graph(poses.data(), valid, 4, 0, 3, I3, tl, 10.0, nullptr, 0) == 2);
    CHECK(lcm::pgo_build_graph(poses.data(), nullptr, 4, 0, 3, I3, tl, 10.0, out.data(), 4) == 4);
    CHECK(out[0].from == 0 && out[0].to == 1 && out[2].from == 2 && out[2].to == 3 && out[0].weight == 1.0);
    CHECK(out[3].from == 0 && out[3].to == 3 && out[3].weight == 10.0 && out[3].t[1] == 2.0 && std::memcmp(out[3].R, I3, sizeof(I3)) == 0);
    {
        double Rf[9], tf[3], Rt[9], tt[3], Rr[9], tr[3], res[6];            // a sequential edge's residual starts at (nearly) zero
        std::memcpy(Rf, poses[0].R, 72); std::memcpy(tf, poses[0].t, 24); std::memcpy(Rt, poses[1].R, 72); std::memcpy(tt, poses[1].t, 24);
        std::memcpy(Rr, out[0].R, 72); std::memcpy(tr, out[0].t, 24);
        CHECK(lcm::pgo_edge_residual(Rr, tr, 1.0, Rf, tf, Rt, tt, res));
        for (int k = 0; k < 6; ++k) CHECK(std::fabs(res[k]) < 1e-15);
    }
    CHECK(!lcm::pgo_loop_ends_problem(valid, 4, 0, 3) && lcm::pgo_loop_ends_problem(valid, 4, 0, 2) && lcm::pgo_loop_ends_problem(valid, 4, 3, 3) &&
          lcm::pgo_loop_ends_problem(valid, 4, 0, 4) && lcm::pgo_loop_ends_problem(nullptr, 4, -1, 2));
    CHECK(std::fabs(lcm::pgo_rotation_drift(poses.data(), 0, 3, I3) - 0.3) < 1e-15);
    CHECK(std::fabs(lcm::pgo_rotation_drift(poses.data(), 0, 3, poses[3].R)) < 1e-15);
    std::vector<lcm_pgo_pose> fixed(4);
    CHECK(lcm::pgo_linear_correct(poses.data(), valid, 4, 0, 3, I3, fixed.data()));
    CHECK(std::memcmp(&fixed[0], &poses[0], 96) == 0 && std::memcmp(&fixed[2], &poses[2], 96) == 0);
    CHECK(std::fabs(lcm::pgo_rotation_drift(fixed.data(), 0, 3, I3)) < 1e-15);          // the whole error taken out at curr
    double r1[3];
    CHECK(lcm::so3_log(fixed[1].R, r1) && std::fabs(r1[1] - 0.0) < 1e-15);              // pose 1: 0.1 - 0.3 / 3
    CHECK(lcm::pgo_linear_correct(poses.data(), valid, 4, 0, 3, I3, poses.data()) && std::memcmp(poses.data(), fixed.data(), 4 * 96) == 0);
}

int main() {
    check_plans();
    check_params_and_values();
    check_arithmetic_and_host_calls();
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all held\n");
    return 0;
}
