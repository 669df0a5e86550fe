// lcm_pgo.cpp — the host side of the pose-graph correction (include/lcm.h, lcm_pgo_*): src/main.cpp:1429-1491.  The kernels are
// lcm_pgo.hip's, the arithmetic lcm_pgo_device.h's, the checks, the plan and the host-only calls lcm_pgo_host.h's.  Here: the
// staging of one graph, the launches of a run (every iteration enqueued back to back, the decision to stop on the device), the
// download, and the C exports.  Part of liblcm_hip.so's host side; shared state and helpers: lcm_internal.h.
#include "lcm_internal.h"

#include "lcm_pgo_host.h"

static_assert(sizeof(lcm_pgo_pose) == 96 && sizeof(lcm::Pose) == 96 && sizeof(lcm_pgo_edge) == 112 && sizeof(lcm::PgoEdge) == 112 &&
              sizeof(lcm_pgo_params) == 64 && sizeof(lcm_pgo_info) == 48, "record sizes");
static_assert(offsetof(lcm_pgo_pose, t) == 72 && offsetof(lcm::Pose, t) == 72 && offsetof(lcm_pgo_edge, t) == 72 &&
              offsetof(lcm::PgoEdge, t) == 72 && offsetof(lcm_pgo_edge, weight) == 96 && offsetof(lcm::PgoEdge, weight) == 96 &&
              offsetof(lcm_pgo_edge, from) == 104 && offsetof(lcm::PgoEdge, from) == 104 && offsetof(lcm_pgo_edge, to) == 108 &&
              offsetof(lcm::PgoEdge, to) == 108, "record layout");
static_assert(offsetof(lcm_pgo_params, loop_weight) == 24 && offsetof(lcm_pgo_params, max_iters) == 32 &&
              offsetof(lcm_pgo_params, loop_direction) == 36 && offsetof(lcm_pgo_params, reserved) == 40, "parameter layout");
static_assert(offsetof(lcm_pgo_info, lambda) == 24 && offsetof(lcm_pgo_info, iterations) == 32 && offsetof(lcm_pgo_info, status) == 36 &&
              offsetof(lcm_pgo_info, n_params) == 40 && offsetof(lcm_pgo_info, n_border) == 44, "info layout");
static_assert(offsetof(lcm::PgoState, lambda) == 24 && offsetof(lcm::PgoState, iterations) == 32 && offsetof(lcm::PgoState, n_border) == 44 &&
              offsetof(lcm::PgoState, done) == sizeof(lcm_pgo_info), "the device's state begins with lcm_pgo_info");

namespace {

struct PgoSeam { double* params; double* res; double* jac; double* dp; };      // lcm_pgo_step's outputs

// One run: `iters` iterations enqueued over the staged graph.  seam == NULL: lcm_pgo_optimize (poses_out), else lcm_pgo_step.
int pgo_run(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_pgo_edge* edges, int n_edges,
            const lcm_pgo_params* pp_in, lcm_pgo_pose* poses_out, lcm_pgo_info* info, const PgoSeam* seam) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (!info || (!seam && !poses_out) || (seam && (!seam->params || !seam->res || !seam->jac || !seam->dp)))
        return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    lcm::PgoPlan pl;
    const lcm::PgoProblem prob = lcm::pgo_inputs_problem(poses, valid, n_poses, edges, n_edges, pp_in, &pl);
    if (prob.what) return fail(prob.code, "%s", prob.what);
    lcm_pgo_params pp;
    if (pp_in) pp = *pp_in; else lcm::pgo_params_default(&pp);
    const int iters = seam ? 1 : pp.max_iters;
    int rc = set_device(h); if (rc) return rc;

    // the graph in one block: [poses | edges | table | valid], uploaded once; behind it the returned poses and the state
    const size_t NP = (size_t)n_poses, NE = (size_t)n_edges;
    const size_t o_edges = NP * sizeof(lcm_pgo_pose), o_tab = o_edges + NE * sizeof(lcm_pgo_edge);
    const size_t o_valid = o_tab + up16(pl.tab_words * sizeof(int32_t)), o_out = o_valid + up16(NP);
    const size_t o_state = o_out + NP * sizeof(lcm_pgo_pose), in_bytes = o_state + up16(sizeof(lcm::PgoState));
    std::vector<uint8_t> stage(o_out, 0);
    std::memcpy(stage.data(), poses, o_edges);
    std::memcpy(stage.data() + o_edges, edges, NE * sizeof(lcm_pgo_edge));
    std::vector<int32_t> tab;
    lcm::pgo_plan_table(pl, &tab);
    std::memcpy(stage.data() + o_tab, tab.data(), tab.size() * sizeof(int32_t));
    for (size_t p = 0; p < NP; ++p) stage[o_valid + p] = lcm::pgo_is_valid(valid, (int)p) ? 1 : 0;
    auto& s = h->pgo;
    rc = ensure_dev(s.d_in, s.d_in_n, in_bytes); if (rc) return rc;
    // ... and every array of doubles in one block, in PgoArgs' order
    const size_t sizes[] = {6 * NP, 6 * NE, 72 * NE, pl.blk_doubles, pl.blk_doubles, pl.blk_doubles, pl.blk_doubles, pl.b_doubles,
                            pl.w_doubles, pl.s_doubles, pl.t_doubles, pl.g_doubles, pl.g_doubles, pl.g_doubles / 6, 6 * (NP - 1)};
    size_t off[16] = {0};
    for (int k = 0; k < 15; ++k) off[k + 1] = off[k] + sizes[k] + (sizes[k] & 1);
    rc = ensure_dev(s.d_work, s.d_work_n, off[15]); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(s.d_in, stage.data(), o_out, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(s.d_in + o_state, 0, sizeof(lcm::PgoState), h->stream));
    double* w = s.d_work;
    HIP_TRY(hipMemsetAsync(w + off[14], 0, sizes[14] * sizeof(double), h->stream));

    lcm::PgoArgs a{};
    a.poses = reinterpret_cast<const lcm::Pose*>(s.d_in); a.edges = reinterpret_cast<const lcm::PgoEdge*>(s.d_in + o_edges);
    a.tab = reinterpret_cast<const int32_t*>(s.d_in + o_tab); a.valid = s.d_in + o_valid;
    a.poses_out = reinterpret_cast<lcm::Pose*>(s.d_in + o_out); a.st = reinterpret_cast<lcm::PgoState*>(s.d_in + o_state);
    a.params = w + off[0]; a.res = w + off[1]; a.jac = w + off[2]; a.D = w + off[3]; a.C = w + off[4]; a.L = w + off[5]; a.M = w + off[6];
    a.B = w + off[7]; a.W = w + off[8]; a.S = w + off[9]; a.T = w + off[10]; a.g = w + off[11]; a.dpu = w + off[12]; a.tr = w + off[13];
    a.dp_out = w + off[14];
    a.n_poses = (uint32_t)n_poses; a.n_edges = (uint32_t)n_edges; a.n_int = (uint32_t)pl.n_int; a.n_border = (uint32_t)pl.n_border;
    a.tab_off = (uint32_t)pl.tab_off; a.tab_edge = (uint32_t)pl.tab_edge; a.tab_int = (uint32_t)pl.tab_int; a.tab_border = (uint32_t)pl.tab_border;
    a.eps = pp.eps; a.damping = pp.damping; a.min_update = pp.min_update; a.max_iters = iters;

    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    hipError_t e = lcm::launch_pgo_params(a, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "pose-graph kernel launch failed: %s", hipGetErrorString(e));
    if (seam) HIP_TRY(hipMemcpyAsync(seam->params, a.params, 6 * NP * sizeof(double), hipMemcpyDeviceToHost, h->stream));   // before the update
    for (int it = 0; it < iters; ++it) {
        e = lcm::launch_pgo_iteration(a, h->stream);
        if (e != hipSuccess) return fail(LCM_ERR_HIP, "pose-graph kernel launch failed: %s", hipGetErrorString(e));
    }
    e = lcm::launch_pgo_writeback(a, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "pose-graph kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    h->info_pending = true;
    h->info.launches = (uint32_t)(2 + lcm::PGO_KERNELS_PER_ITERATION * iters);
    h->info.workgroups = (uint32_t)n_poses; h->info.route = LCM_ROUTE_PLAIN;
    h->info.pairs = NE; h->info.distances = 25 * NE * (uint64_t)iters;          // residual evaluations: 1 + 2 x 12 per edge
    h->info.algo_bytes = o_out + NP * sizeof(lcm_pgo_pose) + sizeof(lcm_pgo_info);

    lcm_pgo_info got;
    HIP_TRY(hipMemcpyAsync(&got, a.st, sizeof(got), hipMemcpyDeviceToHost, h->stream));
    if (seam) {
        HIP_TRY(hipMemcpyAsync(seam->res, a.res, 6 * NE * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(seam->jac, a.jac, 72 * NE * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(seam->dp, a.dp_out, 6 * (NP - 1) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    } else {
        HIP_TRY(hipMemcpyAsync(poses_out, a.poses_out, NP * sizeof(lcm_pgo_pose), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    got.n_params = 6 * (pl.n_int + pl.n_border); got.n_border = pl.n_border;
    *info = got;
    return LCM_OK;
}

int pgo_loop_args_problem(const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, int past, int curr, const double* R_loop) {
    if (!poses || !R_loop) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    if (const char* what = lcm::pgo_loop_ends_problem(valid, n_poses, past, curr)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    for (const int i : {past, curr})
        if (const char* what = lcm::pgo_rotation_problem(poses[i].R)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    if (const char* what = lcm::pgo_rotation_problem(R_loop)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    return LCM_OK;
}

int pgo_build_graph_impl(const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, int past, int curr, const double* R_loop,
                         const double* t_loop, const lcm_pgo_params* pp, lcm_pgo_edge* edges_out, int cap, int* n_edges) {
    if (!poses || !R_loop || !t_loop || !n_edges || cap < 0 || (cap > 0 && !edges_out)) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (const char* what = lcm::pgo_params_problem(pp)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    if (const char* what = lcm::pgo_loop_ends_problem(valid, n_poses, past, curr)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    const double weight = pp ? pp->loop_weight : 10.0;
    const int n = lcm::pgo_build_graph(poses, valid, n_poses, past, curr, R_loop, t_loop, weight, nullptr, 0);
    *n_edges = n;
    if (n > cap) return fail(LCM_ERR_CAPACITY, "%d edges but room for %d", n, cap);
    lcm::pgo_build_graph(poses, valid, n_poses, past, curr, R_loop, t_loop, weight, edges_out, cap);
    return LCM_OK;
}

int pgo_close_loop_impl(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, int past, int curr,
                        const lcm_pose_result* pr, const lcm_pgo_params* pp, lcm_pgo_pose* poses_out, lcm_pgo_info* info) {
    if (!h) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (!poses || !pr || !poses_out || !info) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    if (pr->status != LCM_POSE_OK) return fail(LCM_ERR_INVALID_ARG, "the relative pose's status is not LCM_POSE_OK");
    if (const char* what = lcm::pgo_params_problem(pp)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    if (n_poses > LCM_PGO_MAX_POSES) return fail(LCM_ERR_CAPACITY, "more poses than LCM_PGO_MAX_POSES");
    if (const char* what = lcm::pgo_loop_ends_problem(valid, n_poses, past, curr)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
    double R[9], t[3];
    std::memcpy(R, pr->R, sizeof(R)); std::memcpy(t, pr->t, sizeof(t));
    if (pp && pp->loop_direction == LCM_PGO_LOOP_INVERTED) {             // (R^T, -R^T t)
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) R[3 * i + j] = pr->R[3 * j + i];
            t[i] = -(pr->R[i] * pr->t[0] + pr->R[3 + i] * pr->t[1] + pr->R[6 + i] * pr->t[2]);
        }
    }
    std::vector<lcm_pgo_edge> edges((size_t)n_poses);
    int n_edges = 0;
    const int rc = pgo_build_graph_impl(poses, valid, n_poses, past, curr, R, t, pp, edges.data(), n_poses, &n_edges);
    if (rc) return rc;
    return pgo_run(h, poses, valid, n_poses, edges.data(), n_edges, pp, poses_out, info, nullptr);
}

}  // namespace

extern "C" {

void lcm_pgo_params_default(lcm_pgo_params* p) { if (p) lcm::pgo_params_default(p); }
int lcm_pgo_optimize(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_pgo_edge* edges, int n_edges,
                     const lcm_pgo_params* pp, lcm_pgo_pose* poses_out, lcm_pgo_info* info) {
    return guarded([&] { return pgo_run(h, poses, valid, n_poses, edges, n_edges, pp, poses_out, info, nullptr); });
}
int lcm_pgo_step(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_pgo_edge* edges, int n_edges,
                 const lcm_pgo_params* pp, double* params_out, double* residuals, double* jac, double* dp, lcm_pgo_info* info) {
    const PgoSeam seam{params_out, residuals, jac, dp};
    return guarded([&] { return pgo_run(h, poses, valid, n_poses, edges, n_edges, pp, nullptr, info, &seam); });
}
int lcm_pgo_build_graph(const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, int past, int curr, const double* R_loop,
                        const double* t_loop, const lcm_pgo_params* pp, lcm_pgo_edge* edges_out, int cap, int* n_edges) {
    return guarded([&] { return pgo_build_graph_impl(poses, valid, n_poses, past, curr, R_loop, t_loop, pp, edges_out, cap, n_edges); });
}
int lcm_pgo_rotation_drift(const lcm_pgo_pose* poses, int n_poses, int past, int curr, const double* R_loop, double* angle) {
    return guarded([&] {
        if (!angle) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
        if (const int rc = pgo_loop_args_problem(poses, nullptr, n_poses, past, curr, R_loop)) return rc;
        *angle = lcm::pgo_rotation_drift(poses, past, curr, R_loop);
        return (int)LCM_OK;
    });
}
int lcm_pgo_linear_correct(const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, int past, int curr, const double* R_loop,
                           lcm_pgo_pose* poses_out) {
    return guarded([&] {
        if (!poses_out) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
        if (const int rc = pgo_loop_args_problem(poses, valid, n_poses, past, curr, R_loop)) return rc;
        if (past > curr) return fail(LCM_ERR_INVALID_ARG, "past must come before curr");
        for (int f = past + 1; f < curr; ++f)
            if (lcm::pgo_is_valid(valid, f))
                if (const char* what = lcm::pgo_rotation_problem(poses[f].R)) return fail(LCM_ERR_INVALID_ARG, "%s", what);
        if (!lcm::pgo_linear_correct(poses, valid, n_poses, past, curr, R_loop, poses_out))
            return fail(LCM_ERR_INVALID_ARG, "the rotation error is half a turn: it has no rotation vector");
        return (int)LCM_OK;
    });
}
int lcm_pgo_close_loop(lcm_handle* h, const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, int past, int curr,
                       const lcm_pose_result* pr, const lcm_pgo_params* pp, lcm_pgo_pose* poses_out, lcm_pgo_info* info) {
    return guarded([&] { return pgo_close_loop_impl(h, poses, valid, n_poses, past, curr, pr, pp, poses_out, info); });
}

}  // extern "C"
