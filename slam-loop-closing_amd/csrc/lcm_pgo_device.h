// lcm_pgo_device.h — the arithmetic of the pose-graph correction (lcm_pgo.hip), stated once for the kernels, the two host-only
// helpers of lcm_pgo_host.h and the tests (tests/pgoref.py restates it in numpy; include/lcm.h and DESIGN §9p describe the model):
//   pgo_edge_residual  the six residuals of one edge (src/main.cpp:358-381)
// The rotation's exp and log, the 3 x 3 products and the 6 x 6 Cholesky with its two solves are lcm_geom_device.h's: called, not
// restated.  In double, every product and sum rounded on its own (fp contract off), sums left to right.  Everything is
// __host__ __device__: the host compiles the same text (a stand-alone program runs it under a sanitizer).
// Included by lcm_pgo.hip and, for so3_exp / so3_log and the products, by lcm_pgo_host.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lcm_geom_device.h"

namespace lcm {

// The device's edge record = lcm_pgo_edge (include/lcm.h; lcm_pgo.cpp asserts the layouts); a pose is lcm_geom_device.h's Pose
struct PgoEdge { double R[9]; double t[3]; double weight; int32_t from, to; };

// The residual of one edge between (Rf, tf) and (Rt, tt): w log((R_rel Rf)^T Rt), w (tt - (R_rel tf + t_rel)), w = sqrt(weight).
// false: the rotational error is half a turn (r[0..3) is then w v).
__host__ __device__ __forceinline__ bool pgo_edge_residual(const double (&Rrel)[9], const double (&trel)[3], double w,
                                                           const double (&Rf)[9], const double (&tf)[3], const double (&Rt)[9],
                                                           const double (&tt)[3], double (&r)[6]) {
#pragma clang fp contract(off)
    double Rexp[9], Rerr[9], rv[3], te[3];
    mat3_mul(Rrel, Rf, Rexp);
    mat3_mul_tn(Rexp, Rt, Rerr);
    const bool ok = so3_log(Rerr, rv);
    mat3_apply(Rrel, tf, te);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r[k] = w * rv[k];
        r[3 + k] = w * (tt[k] - (te[k] + trel[k]));
    }
    return ok;
}

// ---- what lcm_pgo.cpp hands to lcm_pgo.hip ----------------------------------------------------------------------------------
// The run's state on the device: the first 48 bytes are lcm_pgo_info.  `done` ends the run: every kernel of a later iteration
// that finds it set does nothing.  `half_turn` is raised by any log that has no rotation vector.
struct PgoState {
    double cost_first, cost_last, max_update, lambda;
    int32_t iterations, status, n_params, n_border;
    int32_t done, half_turn;
};

// The unknowns' order, the tables and the buffers are lcm_pgo_host.h's plan (PgoPlan): interior slots [0, n_int), border slots
// behind them.  D, C, L, M: 36 doubles per interior slot (C[i] couples slot i to slot i + 1; L packed, tri_index); B: n_int x 6 x
// 6 n_border; W: n_int x 6 x ncols, the last column the right-hand side; S: the border's square; T: 6 n_border x ncols, the
// Schur system and its right-hand side; g, dpu: 6 per slot; tr: the trace of a slot's diagonal block.
struct PgoArgs {
    const Pose* poses; const uint8_t* valid; const PgoEdge* edges; const int32_t* tab;
    double* params; double* res; double* jac;
    double* D; double* C; double* L; double* M; double* B; double* W; double* S; double* T; double* g; double* dpu; double* tr;
    double* dp_out; Pose* poses_out; PgoState* st;
    uint32_t n_poses, n_edges, n_int, n_border;
    uint32_t tab_off, tab_edge, tab_int, tab_border;
    double eps, damping, min_update;
    int32_t max_iters;
};

constexpr int PGO_KERNELS_PER_ITERATION = 5;
hipError_t launch_pgo_params(const PgoArgs& a, hipStream_t st);         // k_pgo_params
hipError_t launch_pgo_iteration(const PgoArgs& a, hipStream_t st);      // k_pgo_linearise, _assemble, _sweep, _schur, _finish
hipError_t launch_pgo_writeback(const PgoArgs& a, hipStream_t st);      // k_pgo_writeback

}  // namespace lcm
