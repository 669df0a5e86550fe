// lcm_pgo_host.h — the pure host side of the pose-graph correction (lcm_pgo.cpp): parameter and input checks, the classification
// of the edges, the border list, the interior segments, the pose -> edges table and the sizes of every device buffer as ONE plan
// value; and the host-only calls (the graph of :1441-1470, the drift of :1476-1480, simplePoseCorrection), which use the exp / log
// and the products of lcm_pgo_device.h.  No HIP call and no handle: tests/cpp/pgo_host_check.cpp compiles this text into a
// stand-alone program that runs under a sanitizer.  A check returns {0, NULL} or the status and what is wrong.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/lcm.h"
#include "lcm_pgo_device.h"

namespace lcm {

struct PgoProblem { int code; const char* what; };      // code: LCM_OK, LCM_ERR_INVALID_ARG or LCM_ERR_CAPACITY
constexpr PgoProblem PGO_FINE{LCM_OK, nullptr};
constexpr int PGO_MAX_BORDER = 2 * LCM_PGO_MAX_LOOPS;
constexpr double PGO_ROTATION_TOL = 1e-6;               // max |R R^T - I| of an accepted rotation

inline void pgo_params_default(lcm_pgo_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->eps = 1e-6; p->damping = 1e-4; p->min_update = 1e-6; p->loop_weight = 10.0; p->max_iters = 20;
    p->loop_direction = LCM_PGO_LOOP_AS_WRITTEN;
}

inline const char* pgo_params_problem(const lcm_pgo_params* pp) {
    if (!pp) return nullptr;                                                      // NULL: the defaults
    if (!(pp->eps > 0.0) || !std::isfinite(pp->eps)) return "eps must be finite and > 0";
    if (!(pp->damping >= 0.0) || !std::isfinite(pp->damping)) return "damping must be finite and >= 0";
    if (!(pp->min_update >= 0.0) || !std::isfinite(pp->min_update)) return "min_update must be finite and >= 0";
    if (!(pp->loop_weight >= 0.0) || !std::isfinite(pp->loop_weight)) return "loop_weight must be finite and >= 0";
    if (pp->max_iters < 1 || pp->max_iters > 100) return "max_iters must be in [1, 100]";
    if (pp->loop_direction != LCM_PGO_LOOP_AS_WRITTEN && pp->loop_direction != LCM_PGO_LOOP_INVERTED) return "loop_direction must be 0 or 1";
    return nullptr;
}

inline bool pgo_is_valid(const uint8_t* valid, int i) { return !valid || valid[i] != 0; }

// a rotation as the calls accept it: finite, max |R R^T - I| <= 1e-6, determinant not negative
inline const char* pgo_rotation_problem(const double* R) {
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(R[k])) return "a rotation holds a non-finite value";
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double d = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0);
            if (!(std::fabs(d) <= PGO_ROTATION_TOL)) return "a rotation is not orthonormal (max |R R^T - I| > 1e-6)";
        }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (!(det > 0.0)) return "a rotation has a negative determinant";
    return nullptr;
}

inline const char* pgo_vector_problem(const double* t) {
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(t[k])) return "a translation holds a non-finite value";
    return nullptr;
}

// the values of the valid poses and of every edge (an invalid pose's contents are not read)
inline const char* pgo_values_problem(const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_pgo_edge* edges, int n_edges) {
    for (int i = 0; i < n_poses; ++i) {
        if (!pgo_is_valid(valid, i)) continue;
        if (const char* what = pgo_rotation_problem(poses[i].R)) return what;
        if (const char* what = pgo_vector_problem(poses[i].t)) return what;
    }
    for (int e = 0; e < n_edges; ++e) {
        if (!(edges[e].weight >= 0.0) || !std::isfinite(edges[e].weight)) return "an edge's weight must be finite and >= 0";
        if (const char* what = pgo_rotation_problem(edges[e].R)) return what;
        if (const char* what = pgo_vector_problem(edges[e].t)) return what;
    }
    return nullptr;
}

// Everything the host decides about one graph.  The unknowns are the valid poses >= 1: the interior ones (those that end no loop
// edge) in index order, slots [0, n_int), then the border in index order, slots [n_int, n_int + n_border).  One int32 table goes
// to the device: [slot (n_poses) | pose_off (n_poses + 1) | pose_edge (2 n_edges) | int_pose (n_int) | border_pose (n_border)].
struct PgoPlan {
    int n_poses = 0, n_edges = 0, n_int = 0, n_border = 0, n_loops = 0;
    std::vector<int32_t> slot;            // per pose: its unknown's slot, -1 for pose 0 and for an invalid pose
    std::vector<int32_t> int_pose;        // per interior slot: its pose
    std::vector<int32_t> border_pose;     // per border slot - n_int: its pose
    std::vector<int32_t> seg_first, seg_len;   // interior segments: maximal runs of interior slots whose poses are consecutive
    std::vector<int32_t> pose_off;        // pose p's entries are pose_edge[pose_off[p] .. pose_off[p + 1])
    std::vector<int32_t> pose_edge;       // 2 e + side (0: p is e's `from`, 1: its `to`), ascending
    // table offsets (int32 words) and buffer sizes (doubles)
    size_t tab_slot = 0, tab_off = 0, tab_edge = 0, tab_int = 0, tab_border = 0, tab_words = 0;
    size_t ncols = 1;                     // 6 n_border + 1: the border's columns and the right-hand side
    size_t blk_doubles = 0;               // D, C, L and M: 36 per interior slot each
    size_t b_doubles = 0;                 // B: n_int x 6 x 6 n_border
    size_t w_doubles = 0;                 // W | y: n_int x 6 x ncols
    size_t s_doubles = 0;                 // S: (6 n_border)^2;  T (the Schur system | its right-hand side): 6 n_border x ncols
    size_t t_doubles = 0;
    size_t g_doubles = 0;                 // g, dp and the traces: per unknown
};

inline PgoProblem pgo_plan(const uint8_t* valid, int n_poses, const lcm_pgo_edge* edges, int n_edges, PgoPlan* out) {
    if (n_poses < 2) return {LCM_ERR_INVALID_ARG, "a pose graph needs at least 2 poses"};
    if (n_edges < 1) return {LCM_ERR_INVALID_ARG, "a pose graph needs at least 1 edge"};
    if (n_poses > LCM_PGO_MAX_POSES) return {LCM_ERR_CAPACITY, "more poses than LCM_PGO_MAX_POSES"};
    if (!pgo_is_valid(valid, 0)) return {LCM_ERR_INVALID_ARG, "pose 0 is the fixed pose and must be valid"};
    PgoPlan& pl = *out;
    pl = PgoPlan{};
    pl.n_poses = n_poses; pl.n_edges = n_edges;
    std::vector<uint8_t> border((size_t)n_poses, 0);
    std::vector<int32_t> count((size_t)n_poses + 1, 0);
    for (int e = 0; e < n_edges; ++e) {
        const int f = edges[e].from, t = edges[e].to;
        if (f < 0 || f >= n_poses || t < 0 || t >= n_poses) return {LCM_ERR_INVALID_ARG, "an edge's pose index is out of range"};
        if (f == t) return {LCM_ERR_INVALID_ARG, "an edge joins a pose to itself"};
        if (!pgo_is_valid(valid, f) || !pgo_is_valid(valid, t)) return {LCM_ERR_INVALID_ARG, "an edge ends in an invalid pose"};
        if (f - t != 1 && t - f != 1) {
            ++pl.n_loops;
            border[(size_t)f] = f > 0; border[(size_t)t] = t > 0;
        }
        ++count[(size_t)f]; ++count[(size_t)t];
    }
    if (pl.n_loops > LCM_PGO_MAX_LOOPS) return {LCM_ERR_CAPACITY, "more loop edges than LCM_PGO_MAX_LOOPS"};
    pl.slot.assign((size_t)n_poses, -1);
    for (int p = 1; p < n_poses; ++p)
        if (pgo_is_valid(valid, p) && !border[(size_t)p]) {
            const int s = (int)pl.int_pose.size();
            if (s > 0 && pl.int_pose.back() == p - 1) ++pl.seg_len.back();
            else { pl.seg_first.push_back(s); pl.seg_len.push_back(1); }
            pl.slot[(size_t)p] = s;
            pl.int_pose.push_back(p);
        }
    pl.n_int = (int)pl.int_pose.size();
    for (int p = 1; p < n_poses; ++p)
        if (border[(size_t)p]) {
            pl.slot[(size_t)p] = pl.n_int + (int)pl.border_pose.size();
            pl.border_pose.push_back(p);
        }
    pl.n_border = (int)pl.border_pose.size();
    pl.pose_off.assign((size_t)n_poses + 1, 0);
    for (int p = 0; p < n_poses; ++p) pl.pose_off[(size_t)p + 1] = pl.pose_off[(size_t)p] + count[(size_t)p];
    pl.pose_edge.assign(2 * (size_t)n_edges, 0);
    std::vector<int32_t> fill(pl.pose_off.begin(), pl.pose_off.end() - 1);
    for (int e = 0; e < n_edges; ++e) {
        pl.pose_edge[(size_t)fill[(size_t)edges[e].from]++] = 2 * e;
        pl.pose_edge[(size_t)fill[(size_t)edges[e].to]++] = 2 * e + 1;
    }
    const size_t np = (size_t)n_poses, ni = (size_t)pl.n_int, nb = (size_t)pl.n_border;
    pl.tab_slot = 0; pl.tab_off = np; pl.tab_edge = 2 * np + 1; pl.tab_int = pl.tab_edge + 2 * (size_t)n_edges;
    pl.tab_border = pl.tab_int + ni; pl.tab_words = pl.tab_border + nb;
    pl.ncols = 6 * nb + 1;
    pl.blk_doubles = 36 * ni; pl.b_doubles = ni * 6 * 6 * nb; pl.w_doubles = ni * 6 * pl.ncols;
    pl.s_doubles = 36 * nb * nb; pl.t_doubles = 6 * nb * pl.ncols; pl.g_doubles = 6 * (ni + nb);
    return PGO_FINE;
}

inline void pgo_plan_table(const PgoPlan& pl, std::vector<int32_t>* tab) {
    tab->clear();
    tab->reserve(pl.tab_words);
    tab->insert(tab->end(), pl.slot.begin(), pl.slot.end());
    tab->insert(tab->end(), pl.pose_off.begin(), pl.pose_off.end());
    tab->insert(tab->end(), pl.pose_edge.begin(), pl.pose_edge.end());
    tab->insert(tab->end(), pl.int_pose.begin(), pl.int_pose.end());
    tab->insert(tab->end(), pl.border_pose.begin(), pl.border_pose.end());
}

// what a graph call refuses, in the order it is looked at: the parameters, the structure (-> *plan), the values
inline PgoProblem pgo_inputs_problem(const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, const lcm_pgo_edge* edges, int n_edges,
                                     const lcm_pgo_params* pp, PgoPlan* plan) {
    if (!poses || !edges) return {LCM_ERR_INVALID_ARG, "NULL buffer"};
    if (const char* what = pgo_params_problem(pp)) return {LCM_ERR_INVALID_ARG, what};
    const PgoProblem p = pgo_plan(valid, n_poses, edges, n_edges, plan);
    if (p.what) return p;
    if (const char* what = pgo_values_problem(poses, valid, n_poses, edges, n_edges)) return {LCM_ERR_INVALID_ARG, what};
    return PGO_FINE;
}

// ---- the host-only calls ---------------------------------------------------------------------------------------------------
inline const char* pgo_loop_ends_problem(const uint8_t* valid, int n_poses, int past, int curr) {
    if (n_poses < 2) return "a pose graph needs at least 2 poses";
    if (past < 0 || past >= n_poses || curr < 0 || curr >= n_poses) return "past / curr out of range";
    if (past == curr) return "past and curr are the same pose";
    if (!pgo_is_valid(valid, past) || !pgo_is_valid(valid, curr)) return "past / curr is an invalid pose";
    return nullptr;
}

// the edges of :1441-1470 in order; returns their number and writes at most cap of them (all or none is the caller's rule)
inline int pgo_build_graph(const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, int past, int curr, const double* R_loop,
                           const double* t_loop, double loop_weight, lcm_pgo_edge* out, int cap) {
#pragma clang fp contract(off)
    int n = 0;
    for (int i = 1; i < n_poses; ++i) {
        if (!pgo_is_valid(valid, i - 1) || !pgo_is_valid(valid, i)) continue;
        if (n < cap) {
            lcm_pgo_edge& e = out[n];
            std::memset(&e, 0, sizeof(e));
            double Ra[9], Rb[9], ta[3], rt[3];
            std::memcpy(Ra, poses[i - 1].R, sizeof(Ra)); std::memcpy(Rb, poses[i].R, sizeof(Rb)); std::memcpy(ta, poses[i - 1].t, sizeof(ta));
            mat3_mul_nt(Rb, Ra, e.R);
            mat3_apply(e.R, ta, rt);
            for (int k = 0; k < 3; ++k) e.t[k] = poses[i].t[k] - rt[k];
            e.weight = 1.0; e.from = i - 1; e.to = i;
        }
        ++n;
    }
    if (n < cap) {
        lcm_pgo_edge& e = out[n];
        std::memset(&e, 0, sizeof(e));
        std::memcpy(e.R, R_loop, sizeof(e.R)); std::memcpy(e.t, t_loop, sizeof(e.t));
        e.weight = loop_weight; e.from = past; e.to = curr;
    }
    return n + 1;
}

// log(R_loop (R_curr R_past^T)^T); false at half a turn
inline bool pgo_loop_error(const lcm_pgo_pose* poses, int past, int curr, const double* R_loop, double (&rvec)[3]) {
    double Rp[9], Rc[9], Rl[9], Rseq[9], Rerr[9];
    std::memcpy(Rp, poses[past].R, sizeof(Rp)); std::memcpy(Rc, poses[curr].R, sizeof(Rc)); std::memcpy(Rl, R_loop, sizeof(Rl));
    mat3_mul_nt(Rc, Rp, Rseq);
    mat3_mul_nt(Rl, Rseq, Rerr);
    return so3_log(Rerr, rvec);
}

inline double pgo_rotation_drift(const lcm_pgo_pose* poses, int past, int curr, const double* R_loop) {
#pragma clang fp contract(off)
    double rv[3];
    if (pgo_loop_error(poses, past, curr, R_loop, rv)) return std::sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
    double Rp[9], Rc[9], Rl[9], Rseq[9], Rerr[9];      // half a turn: rv is v, the angle atan2(|v|, c)
    std::memcpy(Rp, poses[past].R, sizeof(Rp)); std::memcpy(Rc, poses[curr].R, sizeof(Rc)); std::memcpy(Rl, R_loop, sizeof(Rl));
    mat3_mul_nt(Rc, Rp, Rseq);
    mat3_mul_nt(Rl, Rseq, Rerr);
    double c = 0.5 * (Rerr[0] + Rerr[4] + Rerr[8] - 1.0);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    return std::atan2(std::sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]), c);
}

// simplePoseCorrection (:451-492); false: the error is half a turn and nothing was written
inline bool pgo_linear_correct(const lcm_pgo_pose* poses, const uint8_t* valid, int n_poses, int past, int curr, const double* R_loop,
                               lcm_pgo_pose* out) {
#pragma clang fp contract(off)
    double rv[3];
    if (!pgo_loop_error(poses, past, curr, R_loop, rv)) return false;
    if (out != poses) std::memmove(out, poses, (size_t)n_poses * sizeof(lcm_pgo_pose));
    const int span = curr - past;
    for (int f = past + 1; f <= curr; ++f) {
        if (!pgo_is_valid(valid, f)) continue;
        const double alpha = (double)(f - past) / span;
        const double ra[3] = {alpha * rv[0], alpha * rv[1], alpha * rv[2]};
        double Rc[9], Rf[9], Rn[9];
        so3_exp(ra, Rc);
        std::memcpy(Rf, out[f].R, sizeof(Rf));
        mat3_mul(Rc, Rf, Rn);
        std::memcpy(out[f].R, Rn, sizeof(Rn));
    }
    return true;
}

}  // namespace lcm
