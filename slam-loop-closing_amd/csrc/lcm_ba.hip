// lcm_ba.hip — the reference's alternatingBundleAdjustment (src/main.cpp:905-943: refineCameraPoseGN :632-743, refinePointGN
// :757-858), computeReprojectionError (:871-896) and the outlier flags of :1563-1619 on the device, with every step's arithmetic
// defined in lcm_ba_device.h and, where other stages share it, lcm_geom_device.h.  With the points fixed every camera is
// independent of every other, with the poses fixed so is every point: a phase runs all its elements at once and gives what the
// reference's sequential loops give.  No floating-point atomic anywhere: every sum has one owner and a fixed order, so the same
// call gives the same bytes, and an element's k-th iteration depends neither on min_update nor on inner_iters.
//
// k_ba_cameras   one workgroup of 256 threads per camera, every inner iteration inside the kernel.  Per iteration lanes 0 .. 6
//                build the seven distinct rotations of the thirteen parameter vectors into LDS (p, p + eps e_k and p - eps e_k for
//                the three rotation parameters; the six translation vectors have the rotation of p itself, the same input and so
//                the same bytes), once per camera and iteration.  Lane l takes the camera's observations l, l + 256, ... of the
//                plan's camera -> observations table (ascending index of the caller's list): thirteen projections each, R X shared
//                by the residual and the six translation columns.  Each lane keeps 21 + 6 + 1 running sums (the packed lower
//                triangle of H, g, r . r), in the order of ba_accumulate.  Summation order over a camera's observations: lane l's
//                own sum in ascending table position; then, through LDS, the 32 lanes of chunk c = l / 32 added left to right
//                (threads 0 .. 223, one per sum and chunk); then the 8 chunk sums added left to right by lane 0, which damps,
//                factors, solves, updates the parameters and publishes the decision.
// k_ba_points    one lane per point, 64 threads per workgroup: the point's observations in ascending table position through the
//                plan's point -> observations table, the poses gathered (at most 384 KiB, cache resident); seven projections per
//                observation; H, g, the 3 x 3 solve and the loop over the iterations in registers.  Summation order: one running
//                sum per entry in table order.
// k_ba_error     one thread per observation, 256 threads per workgroup: sqrt(dx dx + dy dy), optionally stored; the workgroup's
//                256 errors (0 beyond the list) summed as 8 chunks of 32 left to right, then the 8 chunk sums left to right.
// k_ba_mean      ONE workgroup of 256 threads: thread t adds the partial sums t, t + 256, ... in ascending order, the 256 sums
//                combined as in k_ba_error, the total divided by the count (0.0 for no observation).
// k_ba_outliers  one lane per point, 64 threads per workgroup: depth <= 0 flags and does not enter the maximum, else the error
//                enters max_err and flags above outlier_px; then the distance from the cameras' centroid against the threshold
//                (both from the host: lcm_ba_host.h).
//
// Budget (tests/test_kernel_metadata_ba.py): no scratch, no spills.  k_ba_cameras at most 256 VGPRs and 61488 bytes of LDS (two
// workgroups per compute unit by either limit); k_ba_points at most 160 VGPRs and no LDS; k_ba_outliers at most 64 VGPRs and no
// LDS; k_ba_error and k_ba_mean at most 64 VGPRs and 2176 bytes of LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcm_ba_device.h"

namespace lcm {

namespace {

constexpr int BA_PAD = BA_CAMERA_CHUNK + 1;                            // a chunk's stride in LDS: 33 doubles, off the bank period
constexpr int BA_CHUNKS = BA_CAMERA_THREADS / BA_CAMERA_CHUNK;         // 8

// 256 values, one per thread, summed as 8 chunks of 32 left to right and the 8 chunk sums left to right; the result in every
// thread.  buf: 8 x 33 doubles, chunk: 8 doubles.
__device__ __forceinline__ double ba_block_sum(double v, double* buf, double* chunk, uint32_t tid) {
#pragma clang fp contract(off)
    buf[(tid >> 5) * BA_PAD + (tid & 31)] = v;
    __syncthreads();
    if (tid < BA_CHUNKS) {
        double s = buf[tid * BA_PAD];
        for (int j = 1; j < BA_CAMERA_CHUNK; ++j) s = s + buf[tid * BA_PAD + j];
        chunk[tid] = s;
    }
    __syncthreads();
    double total = chunk[0];
    for (int c = 1; c < BA_CHUNKS; ++c) total = total + chunk[c];
    __syncthreads();
    return total;
}

}  // namespace

__global__ __launch_bounds__(256) void k_ba_cameras(BaArgs a) {
#pragma clang fp contract(off)
    __shared__ double part[BA_CAMERA_SUMS * BA_CHUNKS * BA_PAD];       // [sum][chunk][lane of the chunk], padded
    __shared__ double part2[BA_CAMERA_SUMS * BA_CHUNKS];               // [sum][chunk]
    __shared__ double rot[7 * 9];                                      // R(p), R(p + eps e_k), R(p - eps e_k), k < 3
    __shared__ double par[6];
    __shared__ int32_t word[2];                                        // [0]: the camera is refined; [1]: the iterations end
    const uint32_t cam = blockIdx.x, tid = threadIdx.x;
    const uint32_t e0 = a.cam_off[cam], e1 = a.cam_off[cam + 1];
    BaElemInfo info{0.0, 0.0, 0, BA_SKIPPED};
    if (!a.valid[cam] || e1 - e0 < (uint32_t)a.min_cam_obs) {          // the pose stays as it is, byte for byte
        if (tid == 0) a.cam_info[cam] = info;
        return;
    }
    if (tid == 0) {
        double R[9], r[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = a.poses[cam].R[k];
        const bool ok = so3_log(R, r);
#pragma unroll
        for (int k = 0; k < 3; ++k) { par[k] = r[k]; par[3 + k] = a.poses[cam].t[k]; }
        word[0] = ok; word[1] = 0;
    }
    __syncthreads();
    if (!word[0]) {
        if (tid == 0) { info.status = BA_HALF_TURN; a.cam_info[cam] = info; }
        return;
    }
    info.status = BA_MAX_ITERS;
    const double half_inv_eps = 0.5 / a.eps;
    for (int it = 0; it < a.inner_iters; ++it) {
        if (tid < 7) {
            double r[3] = {par[0], par[1], par[2]}, R[9];
            if (tid >= 1 && tid <= 3) r[tid - 1] = r[tid - 1] + a.eps;
            if (tid >= 4) r[tid - 4] = r[tid - 4] - a.eps;
            so3_exp(r, R);
#pragma unroll
            for (int k = 0; k < 9; ++k) rot[9 * tid + k] = R[k];
        }
        __syncthreads();
        double t[3], tp[3], tm[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { t[k] = par[3 + k]; tp[k] = t[k] + a.eps; tm[k] = t[k] - a.eps; }
        double H[21], g[6], cost = 0.0;
#pragma unroll
        for (int k = 0; k < 21; ++k) H[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = 0.0;
        for (uint32_t i = e0 + tid; i < e1; i += BA_CAMERA_THREADS) {
            const uint32_t oi = a.cam_obs[i];
            const Observation ob = a.obs[oi];
            const Point3 P = a.points[ob.point];
            const double X[3] = {P.x, P.y, P.z};
            double R[9], Y0[3], Y[3], Xc[3], r[2], rp[2], rm[2], col[2], Ju[6], Jv[6];
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = rot[k];
            mat3_apply(R, X, Y0);
#pragma unroll
            for (int k = 0; k < 3; ++k) Xc[k] = Y0[k] + t[k];
            ba_residual(a.K, Xc, ob.u, ob.v, r);
#pragma unroll
            for (int c = 0; c < 3; ++c) {                              // the rotation columns: their own R, the translation of p
#pragma unroll
                for (int k = 0; k < 9; ++k) R[k] = rot[9 * (1 + c) + k];
                mat3_apply(R, X, Y);
#pragma unroll
                for (int k = 0; k < 3; ++k) Xc[k] = Y[k] + t[k];
                ba_residual(a.K, Xc, ob.u, ob.v, rp);
#pragma unroll
                for (int k = 0; k < 9; ++k) R[k] = rot[9 * (4 + c) + k];
                mat3_apply(R, X, Y);
#pragma unroll
                for (int k = 0; k < 3; ++k) Xc[k] = Y[k] + t[k];
                ba_residual(a.K, Xc, ob.u, ob.v, rm);
                ba_column(rp, rm, half_inv_eps, col);
                Ju[c] = col[0]; Jv[c] = col[1];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {                              // the translation columns: R X of p, t[c] moved
#pragma unroll
                for (int k = 0; k < 3; ++k) Xc[k] = Y0[k] + (k == c ? tp[k] : t[k]);
                ba_residual(a.K, Xc, ob.u, ob.v, rp);
#pragma unroll
                for (int k = 0; k < 3; ++k) Xc[k] = Y0[k] + (k == c ? tm[k] : t[k]);
                ba_residual(a.K, Xc, ob.u, ob.v, rm);
                ba_column(rp, rm, half_inv_eps, col);
                Ju[3 + c] = col[0]; Jv[3 + c] = col[1];
            }
            if (a.seam_r) {
                a.seam_r[2 * (size_t)oi] = r[0]; a.seam_r[2 * (size_t)oi + 1] = r[1];
#pragma unroll
                for (int k = 0; k < 6; ++k) { a.seam_J[12 * (size_t)oi + k] = Ju[k]; a.seam_J[12 * (size_t)oi + 6 + k] = Jv[k]; }
            }
            ba_accumulate<6>(Ju, Jv, r, H, g, cost);
        }
        const uint32_t mine = (tid >> 5) * BA_PAD + (tid & 31);
#pragma unroll
        for (int k = 0; k < 21; ++k) part[k * (BA_CHUNKS * BA_PAD) + mine] = H[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) part[(21 + k) * (BA_CHUNKS * BA_PAD) + mine] = g[k];
        part[27 * (BA_CHUNKS * BA_PAD) + mine] = cost;
        __syncthreads();
        if (tid < BA_CAMERA_SUMS * BA_CHUNKS) {
            const double* src = part + (tid >> 3) * (BA_CHUNKS * BA_PAD) + (tid & 7) * BA_PAD;
            double s = src[0];
            for (int j = 1; j < BA_CAMERA_CHUNK; ++j) s = s + src[j];
            part2[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            double dp[6];
#pragma unroll
            for (int k = 0; k < BA_CAMERA_SUMS; ++k) {
                double s = part2[BA_CHUNKS * k];
#pragma unroll
                for (int c = 1; c < BA_CHUNKS; ++c) s = s + part2[BA_CHUNKS * k + c];
                if (k < 21) H[k] = s; else if (k < 27) g[k - 21] = s; else cost = s;
            }
            info.cost = cost;
            const bool ok = solve_damped<6>(H, g, a.damping, dp);
            if (a.seam_H) {
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = 0; c < 6; ++c) a.seam_H[36 * (size_t)cam + 6 * r + c] = H[r >= c ? tri_index(r, c) : tri_index(c, r)];
#pragma unroll
                for (int k = 0; k < 6; ++k) { a.seam_g[6 * (size_t)cam + k] = g[k]; a.seam_dp[6 * (size_t)cam + k] = ok ? dp[k] : 0.0; }
            }
            if (!ok) {
                info.status = BA_SOLVE_FAILED; word[1] = 1;
            } else {
                double m = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    par[k] = par[k] + dp[k];
                    const double ad = fabs(dp[k]);
                    m = ad > m ? ad : m;
                }
                info.iterations = it + 1; info.last_update = m;
                if (m < a.min_update) { info.status = BA_CONVERGED; word[1] = 1; }
            }
        }
        __syncthreads();
        if (word[1]) break;
    }
    if (tid == 0) {
        const double r[3] = {par[0], par[1], par[2]};
        double R[9];
        so3_exp(r, R);
#pragma unroll
        for (int k = 0; k < 9; ++k) a.poses[cam].R[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) a.poses[cam].t[k] = par[3 + k];
        a.cam_info[cam] = info;
    }
}

__global__ __launch_bounds__(64) void k_ba_points(BaArgs a) {
#pragma clang fp contract(off)
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= a.n_points) return;
    const uint32_t e0 = a.pt_off[p], e1 = a.pt_off[p + 1];
    BaElemInfo info{0.0, 0.0, 0, BA_SKIPPED};
    if (e1 - e0 < (uint32_t)a.min_point_obs) {                         // the point stays as it is, byte for byte
        a.pt_info[p] = info;
        return;
    }
    double X[3] = {a.points[p].x, a.points[p].y, a.points[p].z};
    const double half_inv_eps = 0.5 / a.eps;
    info.status = BA_MAX_ITERS;
    for (int it = 0; it < a.inner_iters; ++it) {
        double H[6], g[3], dp[3], cost = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) H[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = 0.0;
        for (uint32_t i = e0; i < e1; ++i) {
            const uint32_t oi = a.pt_obs[i];
            const Observation ob = a.obs[oi];
            const Pose& pose = a.poses[ob.cam];
            double R[9], t[3], Xc[3], r[2], rp[2], rm[2], col[2], Ju[3], Jv[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = pose.R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = pose.t[k];
            rigid_apply(R, t, X, Xc);
            ba_residual(a.K, Xc, ob.u, ob.v, r);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double Xp[3] = {X[0], X[1], X[2]}, Xm[3] = {X[0], X[1], X[2]};
                Xp[c] = Xp[c] + a.eps; Xm[c] = Xm[c] - a.eps;
                rigid_apply(R, t, Xp, Xc);
                ba_residual(a.K, Xc, ob.u, ob.v, rp);
                rigid_apply(R, t, Xm, Xc);
                ba_residual(a.K, Xc, ob.u, ob.v, rm);
                ba_column(rp, rm, half_inv_eps, col);
                Ju[c] = col[0]; Jv[c] = col[1];
            }
            if (a.seam_r) {
                a.seam_r[2 * (size_t)oi] = r[0]; a.seam_r[2 * (size_t)oi + 1] = r[1];
#pragma unroll
                for (int k = 0; k < 3; ++k) { a.seam_J[6 * (size_t)oi + k] = Ju[k]; a.seam_J[6 * (size_t)oi + 3 + k] = Jv[k]; }
            }
            ba_accumulate<3>(Ju, Jv, r, H, g, cost);
        }
        info.cost = cost;
        const bool ok = solve_damped<3>(H, g, a.damping, dp);
        if (a.seam_H) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) a.seam_H[9 * (size_t)p + 3 * r + c] = H[r >= c ? tri_index(r, c) : tri_index(c, r)];
#pragma unroll
            for (int k = 0; k < 3; ++k) { a.seam_g[3 * (size_t)p + k] = g[k]; a.seam_dp[3 * (size_t)p + k] = ok ? dp[k] : 0.0; }
        }
        if (!ok) { info.status = BA_SOLVE_FAILED; break; }
        double m = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            X[k] = X[k] + dp[k];
            const double ad = fabs(dp[k]);
            m = ad > m ? ad : m;
        }
        info.iterations = it + 1; info.last_update = m;
        if (m < a.min_update) { info.status = BA_CONVERGED; break; }
    }
    a.points[p].x = X[0]; a.points[p].y = X[1]; a.points[p].z = X[2];
    a.pt_info[p] = info;
}

__global__ __launch_bounds__(256) void k_ba_error(BaArgs a) {
#pragma clang fp contract(off)
    __shared__ double buf[BA_CHUNKS * BA_PAD];
    __shared__ double chunk[BA_CHUNKS];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * BA_ERROR_THREADS + tid;
    double err = 0.0;
    if (i < a.n_obs) {
        const Observation ob = a.obs[i];
        const Pose& pose = a.poses[ob.cam];
        const Point3 P = a.points[ob.point];
        const double X[3] = {P.x, P.y, P.z};
        double R[9], t[3], Xc[3], r[2];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = pose.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = pose.t[k];
        rigid_apply(R, t, X, Xc);
        ba_residual(a.K, Xc, ob.u, ob.v, r);
        err = ba_error(r);
        if (a.obs_err) a.obs_err[i] = err;
    }
    const double total = ba_block_sum(err, buf, chunk, tid);
    if (tid == 0) a.partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_ba_mean(BaArgs a) {
#pragma clang fp contract(off)
    __shared__ double buf[BA_CHUNKS * BA_PAD];
    __shared__ double chunk[BA_CHUNKS];
    const uint32_t tid = threadIdx.x;
    double s = 0.0;
    for (uint32_t i = tid; i < a.n_partials; i += 256) s = s + a.partial[i];
    const double total = ba_block_sum(s, buf, chunk, tid);
    if (tid == 0) a.mean_out[0] = a.n_obs ? total / (double)a.n_obs : 0.0;
}

__global__ __launch_bounds__(64) void k_ba_outliers(BaArgs a) {
#pragma clang fp contract(off)
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= a.n_points) return;
    const double X[3] = {a.points[p].x, a.points[p].y, a.points[p].z};
    bool flag = false;
    double worst = 0.0;
    for (uint32_t i = a.pt_off[p]; i < a.pt_off[p + 1]; ++i) {
        const Observation ob = a.obs[a.pt_obs[i]];
        const Pose& pose = a.poses[ob.cam];
        double R[9], t[3], Xc[3], r[2];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = pose.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = pose.t[k];
        rigid_apply(R, t, X, Xc);
        if (Xc[2] <= 0.0) { flag = true; continue; }
        ba_residual(a.K, Xc, ob.u, ob.v, r);
        const double err = ba_error(r);
        worst = err > worst ? err : worst;                             // std::max(worst, err): a NaN error leaves it
        if (err > a.outlier_px) flag = true;
    }
    const double dx = X[0] - a.centroid[0], dy = X[1] - a.centroid[1], dz = X[2] - a.centroid[2];
    if (sqrt(dx * dx + dy * dy + dz * dz) > a.max_dist) flag = true;
    a.flags[p] = flag ? 1 : 0;
    a.max_err[p] = worst;
}

hipError_t launch_ba_cameras(const BaArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_ba_cameras, dim3(a.n_cams), dim3(BA_CAMERA_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_ba_points(const BaArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_ba_points, dim3((a.n_points + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_ba_error(const BaArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_ba_error, dim3(a.n_partials), dim3(BA_ERROR_THREADS), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ba_mean, dim3(1), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_ba_outliers(const BaArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_ba_outliers, dim3((a.n_points + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace lcm
