// lcm_pgo.hip — the reference's optimizePoseGraph (src/main.cpp:282-445) on the device, with every step's arithmetic defined in
// lcm_pgo_device.h and, where other stages share it, lcm_geom_device.h: the block-sparse central-difference linearisation, the
// normal equations in the plan's order (interior poses, then the border: lcm_pgo_host.h) and an exact block Cholesky of them.
// No floating-point atomic anywhere: every sum has one owner and a fixed order, so the same call gives the same bytes.  The
// convergence decision stays on the device: the host enqueues the iterations back to back, and a kernel that finds
// PgoState::done set returns at once.
//
// k_pgo_params     one thread per pose, once per run: the parameters (log R, t) of every valid pose; zeros for an invalid one.
// k_pgo_linearise  16 lanes per edge, four edges per wave, 256 threads per workgroup, the grid over the edges.  Lanes 0 .. 11 own
//                  one Jacobian column each (the six parameters of `from`, then of `to`): both endpoints' poses from the
//                  parameters, the owned parameter moved by +eps and by -eps, pgo_edge_residual twice, the column written.
//                  Lane 0 also writes the edge's residual.  A column of pose 0 is zero.
// k_pgo_assemble   one workgroup of 64 threads per pose: lanes 0 .. 35 own one entry (a, b) of every 6 x 6 block, lanes 36 .. 41
//                  one entry of g.  The pose's edges are walked in ascending order through the plan's pose -> edges table: the
//                  diagonal block, g, the coupling to the next interior slot (C) and the couplings to border poses (a row of B
//                  for an interior pose, a block row of S for a border pose), the last two as read-modify-write of words only
//                  this workgroup touches.  Lane 0 sums the block's trace.
// k_pgo_sweep      ONE workgroup of 128 threads.  cost = r . r and trace(H), each as 128 strided partial sums added left to
//                  right; lambda.  Then the forward sweep over the interior slots: every thread factors the damped 6 x 6 pivot
//                  block in registers (the same bytes in every lane, so the loop has no barrier), thread c < 6 n_border + 1
//                  carries column c of W = L^-1 B (the last column: L^-1 (-g)) and stores it; thread 0 stores L and M.
// k_pgo_schur      one thread per entry of the lower triangle of the border's Schur complement S + lambda I - W^T W and of its
//                  right-hand side -g_b - W^T y, each one running sum over the interior slots.
// k_pgo_finish     ONE workgroup of 256 threads: the Cholesky of the Schur system (at most 96 x 96, in place in device memory, one
//                  thread per row), its two substitutions through 96 doubles of LDS, z = y - W x_b in parallel, the backward
//                  recurrence over the interior slots in wave 0, p += dp, max |dp|, the iteration count and the status.
// k_pgo_writeback  one thread per pose, once per run: exp of the rotation parameters and t; pose 0 and invalid poses (and every
//                  pose after a half turn before any update) byte for byte.
//
// Budget (tests/test_kernel_metadata_pgo.py): no scratch, no spills.  k_pgo_params, k_pgo_linearise and k_pgo_writeback at most
// 128 VGPRs and no LDS; k_pgo_assemble at most 64 VGPRs and no LDS; k_pgo_sweep at most 256 VGPRs and 2048 bytes of LDS;
// k_pgo_schur at most 64 VGPRs and no LDS; k_pgo_finish at most 128 VGPRs and 2824 bytes of LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcm_pgo_device.h"

namespace lcm {

namespace {

// pose `idx` under the parameters, parameter k (0 .. 5, or -1: none) moved by delta; pose 0 is the given pose itself
__device__ __forceinline__ void pgo_pose_at(const PgoArgs& a, uint32_t idx, int k, double delta, double (&R)[9], double (&t)[3]) {
#pragma clang fp contract(off)
    if (idx == 0) {
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = a.poses[0].R[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = a.poses[0].t[j];
        return;
    }
    const double* p = a.params + 6 * (size_t)idx;
    double r[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        r[j] = (j == k) ? p[j] + delta : p[j];
        t[j] = (j + 3 == k) ? p[j + 3] + delta : p[j + 3];
    }
    so3_exp(r, R);
}

}  // namespace

__global__ __launch_bounds__(256) void k_pgo_params(PgoArgs a) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.n_poses) return;
    double* out = a.params + 6 * (size_t)p;
    if (!a.valid[p]) {
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = 0.0;
        return;
    }
    double R[9], r[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a.poses[p].R[k];
    if (!so3_log(R, r) && p != 0) a.st->half_turn = 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) { out[k] = r[k]; out[3 + k] = a.poses[p].t[k]; }
}

__global__ __launch_bounds__(256) void k_pgo_linearise(PgoArgs a) {
#pragma clang fp contract(off)
    if (a.st->done) return;
    const uint32_t gid = blockIdx.x * 256 + threadIdx.x, e = gid >> 4, col = gid & 15;
    if (e >= a.n_edges || col >= 12) return;
    const PgoEdge& ed = a.edges[e];
    double Rrel[9], trel[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rrel[k] = ed.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) trel[k] = ed.t[k];
    const double w = sqrt(ed.weight);
    const uint32_t from = (uint32_t)ed.from, to = (uint32_t)ed.to;
    const bool own_from = col < 6;
    const int k = (int)(own_from ? col : col - 6);
    double Rf[9], tf[3], Rt[9], tt[3], rp[6], rm[6];
    bool ok = true;
    if (col == 0) {
        pgo_pose_at(a, from, -1, 0.0, Rf, tf);
        pgo_pose_at(a, to, -1, 0.0, Rt, tt);
        ok = pgo_edge_residual(Rrel, trel, w, Rf, tf, Rt, tt, rp);
#pragma unroll
        for (int m = 0; m < 6; ++m) a.res[6 * (size_t)e + m] = rp[m];
    }
    double* jc = a.jac + 72 * (size_t)e + col;
    if ((own_from ? from : to) == 0) {
#pragma unroll
        for (int m = 0; m < 6; ++m) jc[12 * m] = 0.0;
    } else {
        pgo_pose_at(a, from, own_from ? k : -1, a.eps, Rf, tf);
        pgo_pose_at(a, to, own_from ? -1 : k, a.eps, Rt, tt);
        ok = pgo_edge_residual(Rrel, trel, w, Rf, tf, Rt, tt, rp) && ok;
        pgo_pose_at(a, from, own_from ? k : -1, -a.eps, Rf, tf);
        pgo_pose_at(a, to, own_from ? -1 : k, -a.eps, Rt, tt);
        ok = pgo_edge_residual(Rrel, trel, w, Rf, tf, Rt, tt, rm) && ok;
        const double two_eps = 2.0 * a.eps;
#pragma unroll
        for (int m = 0; m < 6; ++m) jc[12 * m] = (rp[m] - rm[m]) / two_eps;
    }
    if (!ok) a.st->half_turn = 1;
}

__global__ __launch_bounds__(64) void k_pgo_assemble(PgoArgs a) {
#pragma clang fp contract(off)
    if (a.st->done) return;
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    const int32_t* slot = a.tab;
    const int32_t u = slot[p];
    if (u < 0) return;
    const bool interior = (uint32_t)u < a.n_int;
    const uint32_t ld = 6 * a.n_border, b = interior ? 0u : (uint32_t)u - a.n_int;
    double* row = interior ? a.B + (size_t)u * 6 * ld : a.S + (size_t)b * 6 * ld;      // this pose's six rows of B or of S
    for (uint32_t k = lane; k < 6 * ld; k += 64) row[k] = 0.0;
    __syncthreads();
    const uint32_t ra = lane < 36 ? lane / 6 : lane - 36, cb = lane % 6;      // lanes 0 .. 35: entry (ra, cb); 36 .. 41: g[ra]
    double acc_d = 0.0, acc_c = 0.0, acc_g = 0.0;
    const uint32_t e0 = (uint32_t)a.tab[a.tab_off + p], e1 = (uint32_t)a.tab[a.tab_off + p + 1];
    for (uint32_t i = e0; i < e1; ++i) {
        const uint32_t code = (uint32_t)a.tab[a.tab_edge + i], e = code >> 1, side = code & 1;
        const double* J = a.jac + 72 * (size_t)e;
        const uint32_t mine = 6 * side, other = 6 - mine;
        const uint32_t q = (uint32_t)(side ? a.edges[e].from : a.edges[e].to);
        const int32_t uq = slot[q];
        if (lane < 36) {
#pragma unroll
            for (int m = 0; m < 6; ++m) acc_d = acc_d + J[12 * m + mine + ra] * J[12 * m + mine + cb];
            if (uq >= 0) {
                const bool q_interior = (uint32_t)uq < a.n_int;
                if (interior && q_interior) {
                    if (uq == u + 1) {
#pragma unroll
                        for (int m = 0; m < 6; ++m) acc_c = acc_c + J[12 * m + mine + ra] * J[12 * m + other + cb];
                    }
                } else if (!q_interior) {
                    double* cell = row + (size_t)ra * ld + 6 * ((uint32_t)uq - a.n_int) + cb;
                    double s = *cell;
#pragma unroll
                    for (int m = 0; m < 6; ++m) s = s + J[12 * m + mine + ra] * J[12 * m + other + cb];
                    *cell = s;
                }
            }
        } else if (lane < 42) {
#pragma unroll
            for (int m = 0; m < 6; ++m) acc_g = acc_g + J[12 * m + mine + ra] * a.res[6 * (size_t)e + m];
        }
    }
    double* diag = interior ? a.D + 36 * (size_t)u : nullptr;
    if (lane < 36) {
        if (interior) { diag[lane] = acc_d; a.C[36 * (size_t)u + lane] = acc_c; }
        else row[(size_t)ra * ld + 6 * b + cb] = acc_d;
    } else if (lane < 42) {
        a.g[6 * (size_t)u + ra] = acc_g;
    }
    __syncthreads();
    if (lane == 0) {
        double t = 0.0;
        for (uint32_t k = 0; k < 6; ++k) t = t + (interior ? diag[7 * k] : row[(size_t)k * ld + 6 * b + k]);
        a.tr[u] = t;
    }
}

__global__ __launch_bounds__(128) void k_pgo_sweep(PgoArgs a) {
#pragma clang fp contract(off)
    __shared__ double part[2][128];
    const uint32_t tid = threadIdx.x;
    PgoState* st = a.st;
    const int done = st->done, half = st->half_turn, iterations = st->iterations;
    __syncthreads();
    if (done) return;
    if (half) {
        if (tid == 0) { st->status = 3; st->done = 1; }                  // LCM_PGO_HALF_TURN
        return;
    }
    double c = 0.0, t = 0.0;
    for (uint32_t i = tid; i < 6 * a.n_edges; i += 128) c = c + a.res[i] * a.res[i];
    for (uint32_t i = tid; i < a.n_int + a.n_border; i += 128) t = t + a.tr[i];
    part[0][tid] = c; part[1][tid] = t;
    __syncthreads();
    double cost = part[0][0], trace = part[1][0];
    for (uint32_t k = 1; k < 128; ++k) { cost = cost + part[0][k]; trace = trace + part[1][k]; }
    const double lambda = a.damping * trace / (6.0 * (double)(a.n_poses - 1));
    if (tid == 0) {
        if (iterations == 0) st->cost_first = cost;
        st->cost_last = cost; st->lambda = lambda;
    }
    const uint32_t nb6 = 6 * a.n_border, ncols = nb6 + 1;
    const bool active = tid < ncols;
    double Lp[21], wp[6], M[36];
#pragma unroll
    for (int k = 0; k < 21; ++k) Lp[k] = 1.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) wp[k] = 0.0;
    bool ok = true;
    for (uint32_t i = 0; i < a.n_int && ok; ++i) {
        const double* Di = a.D + 36 * (size_t)i;
        double Lc[21], w[6];
        if (i > 0) {
            const double* Cp = a.C + 36 * (size_t)(i - 1);
#pragma unroll
            for (int r = 0; r < 6; ++r) {                                 // row r of M = L^-1 (column r of C): M L^T = C^T
                double x[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) x[j] = Cp[6 * j + r];
                lower_solve<6>(Lp, x);
#pragma unroll
                for (int j = 0; j < 6; ++j) M[6 * r + j] = x[j];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 36; ++k) M[k] = 0.0;
        }
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int cc = 0; cc <= r; ++cc) {
                double s = (r == cc) ? Di[6 * r + cc] + lambda : Di[6 * r + cc];
#pragma unroll
                for (int k = 0; k < 6; ++k) s = s - M[6 * r + k] * M[6 * cc + k];
                Lc[tri_index(r, cc)] = s;
            }
        ok = chol<6>(Lc);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            double s = 0.0;
            if (active) s = tid < nb6 ? a.B[((size_t)i * 6 + k) * nb6 + tid] : -a.g[6 * (size_t)i + k];
#pragma unroll
            for (int j = 0; j < 6; ++j) s = s - M[6 * k + j] * wp[j];
            w[k] = s;
        }
        lower_solve<6>(Lc, w);
        if (active && ok) {
#pragma unroll
            for (int k = 0; k < 6; ++k) a.W[((size_t)i * 6 + k) * ncols + tid] = w[k];
        }
        if (tid == 0 && ok) {
#pragma unroll
            for (int k = 0; k < 21; ++k) a.L[36 * (size_t)i + k] = Lc[k];
#pragma unroll
            for (int k = 0; k < 36; ++k) a.M[36 * (size_t)i + k] = M[k];
        }
#pragma unroll
        for (int k = 0; k < 21; ++k) Lp[k] = Lc[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) wp[k] = w[k];
    }
    if (!ok && tid == 0) { st->status = 2; st->done = 1; }               // LCM_PGO_SOLVE_FAILED
}

__global__ __launch_bounds__(256) void k_pgo_schur(PgoArgs a) {
#pragma clang fp contract(off)
    if (a.st->done) return;
    const uint32_t nb6 = 6 * a.n_border, ncols = nb6 + 1;
    const uint32_t id = blockIdx.x * 256 + threadIdx.x, r = id / ncols, c = id % ncols;
    if (r >= nb6 || (c < nb6 && c > r)) return;
    double acc = 0.0;
    const double* W = a.W;
    for (uint32_t k = 0; k < 6 * a.n_int; ++k) acc = acc + W[(size_t)k * ncols + r] * W[(size_t)k * ncols + c];
    double base;
    if (c == nb6) base = -a.g[6 * (size_t)a.n_int + r];
    else base = (r == c) ? a.S[(size_t)r * nb6 + c] + a.st->lambda : a.S[(size_t)r * nb6 + c];
    a.T[(size_t)r * ncols + c] = base - acc;
}

__global__ __launch_bounds__(256) void k_pgo_finish(PgoArgs a) {
#pragma clang fp contract(off)
    __shared__ double v[96];
    __shared__ double red[256];
    __shared__ int pivot_ok;
    const uint32_t tid = threadIdx.x;
    PgoState* st = a.st;
    if (st->done) return;
    const uint32_t n = 6 * a.n_border, ncols = n + 1;
    double* T = a.T;
    for (uint32_t j = 0; j < n; ++j) {
        double s = 0.0;
        if (tid >= j && tid < n) {
            s = T[(size_t)tid * ncols + j];
            for (uint32_t k = 0; k < j; ++k) s = s - T[(size_t)tid * ncols + k] * T[(size_t)j * ncols + k];
        }
        if (tid == j) { pivot_ok = s > 0.0; T[(size_t)j * ncols + j] = sqrt(s); }
        __syncthreads();
        if (!pivot_ok) {                                                 // the same word for every thread
            if (tid == 0) { st->status = 2; st->done = 1; }              // LCM_PGO_SOLVE_FAILED
            return;
        }
        if (tid > j && tid < n) T[(size_t)tid * ncols + j] = s / T[(size_t)j * ncols + j];
        __syncthreads();
    }
    if (tid < n) v[tid] = T[(size_t)tid * ncols + n];
    __syncthreads();
    for (uint32_t j = 0; j < n; ++j) {
        if (tid == j) v[j] = v[j] / T[(size_t)j * ncols + j];
        __syncthreads();
        if (tid > j && tid < n) v[tid] = v[tid] - T[(size_t)tid * ncols + j] * v[j];
        __syncthreads();
    }
    for (uint32_t jj = n; jj > 0; --jj) {
        const uint32_t j = jj - 1;
        if (tid == j) v[j] = v[j] / T[(size_t)j * ncols + j];
        __syncthreads();
        if (tid < j) v[tid] = v[tid] - T[(size_t)j * ncols + tid] * v[j];
        __syncthreads();
    }
    // z = y - W x_b, every interior component on its own
    for (uint32_t idx = tid; idx < 6 * a.n_int; idx += 256) {
        const double* Wr = a.W + (size_t)idx * ncols;
        double s = Wr[n];
        for (uint32_t c = 0; c < n; ++c) s = s - Wr[c] * v[c];
        a.dpu[idx] = s;
    }
    if (tid < n) a.dpu[6 * (size_t)a.n_int + tid] = v[tid];
    __syncthreads();
    // x_i = L_i^-T (z_i - M_{i+1}^T x_{i+1}), from the last interior slot down; the same bytes in every lane of wave 0
    if (tid < 64) {
        double xn[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) xn[k] = 0.0;
        for (uint32_t ii = a.n_int; ii > 0; --ii) {
            const uint32_t i = ii - 1;
            double x[6], Lc[21];
#pragma unroll
            for (int k = 0; k < 6; ++k) x[k] = a.dpu[6 * (size_t)i + k];
            if (ii < a.n_int) {
                const double* Mn = a.M + 36 * (size_t)ii;
#pragma unroll
                for (int k = 0; k < 6; ++k)
#pragma unroll
                    for (int j = 0; j < 6; ++j) x[k] = x[k] - Mn[6 * j + k] * xn[j];
            }
#pragma unroll
            for (int k = 0; k < 21; ++k) Lc[k] = a.L[36 * (size_t)i + k];
            upper_solve<6>(Lc, x);
            if (tid == 0) {
#pragma unroll
                for (int k = 0; k < 6; ++k) a.dpu[6 * (size_t)i + k] = x[k];
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) xn[k] = x[k];
        }
    }
    __syncthreads();
    double m = 0.0;
    for (uint32_t idx = tid; idx < 6 * (a.n_int + a.n_border); idx += 256) {
        const uint32_t u = idx / 6, k = idx % 6;
        const uint32_t pose = (uint32_t)(u < a.n_int ? a.tab[a.tab_int + u] : a.tab[a.tab_border + (u - a.n_int)]);
        const double d = a.dpu[idx];
        a.params[6 * (size_t)pose + k] = a.params[6 * (size_t)pose + k] + d;
        a.dp_out[6 * (size_t)(pose - 1) + k] = d;
        const double ad = fabs(d);
        m = ad > m ? ad : m;
    }
    red[tid] = m;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t k = 1; k < 256; ++k) m = red[k] > m ? red[k] : m;
        const int it = st->iterations + 1;
        st->iterations = it; st->max_update = m;
        if (m < a.min_update) { st->status = 0; st->done = 1; }          // LCM_PGO_CONVERGED
        else if (it >= a.max_iters) { st->status = 1; st->done = 1; }    // LCM_PGO_MAX_ITERS
    }
}

__global__ __launch_bounds__(256) void k_pgo_writeback(PgoArgs a) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.n_poses) return;
    const bool untouched = a.st->status == 3 && a.st->iterations == 0;
    Pose out = a.poses[p];
    if (p != 0 && a.valid[p] && !untouched) {
        const double* q = a.params + 6 * (size_t)p;
        const double r[3] = {q[0], q[1], q[2]};
        so3_exp(r, out.R);
#pragma unroll
        for (int k = 0; k < 3; ++k) out.t[k] = q[3 + k];
    }
    a.poses_out[p] = out;
}

hipError_t launch_pgo_params(const PgoArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_pgo_params, dim3((a.n_poses + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_pgo_iteration(const PgoArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_pgo_linearise, dim3((a.n_edges + 15) / 16), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pgo_assemble, dim3(a.n_poses), dim3(64), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_pgo_sweep, dim3(1), dim3(128), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const uint32_t entries = 6 * a.n_border * (6 * a.n_border + 1);
    hipLaunchKernelGGL(k_pgo_schur, dim3(entries / 256 + 1), dim3(256), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_pgo_finish, dim3(1), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_pgo_writeback(const PgoArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_pgo_writeback, dim3((a.n_poses + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace lcm
