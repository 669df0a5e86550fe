// lcm_pose.hip — the reference's cv::recoverPose(E, ptsCurr, ptsPast, K, R_loop, t_loop, mask) (src/main.cpp:1405-1409) on
// the device, with every step defined in lcm_pose_device.h: the closed-form decomposition of E into two rotations and a unit
// translation, the division-free depth test, and the selection among the four (R, t).  It runs on the point records, the
// matrices and the inlier mask k_epi_mask has just written (lcm_pose_db_*), or on a caller's (lcm_pose_recover_pairs).
// The pair comes from blockIdx.y, in slices (launch_y_sliced, lcm_kernels.h) as k_epi_mask's does.
//
// k_pose_recover  one workgroup of 256 threads per pair.  E is read at a wave-uniform address and EVERY thread decomposes
//                 it (about 150 double operations; the alternative, one lane and a broadcast through LDS behind a barrier,
//                 saves no register: Ra, Rb and t stay live through pass 1 either way).  Pass 1 strides over the pair's
//                 records: those whose input mask byte is non-zero are normalised and put to the depth test under the four
//                 hypotheses, four running counts (and the number of records used) in registers.  The counts are summed by
//                 __shfl_xor within the wave and through 4 waves x 5 words of LDS; every thread then derives the same choice.
//                 Pass 2 recomputes the chosen hypothesis's verdict per record and writes one byte each: a pair holds up to
//                 65 535 records, which no register file keeps.  Thread 0 writes the pair's 128-byte result record and, for
//                 the test seam, the four candidates.  A matrix without a model: zero record, choice -1, zero mask.
//
// Budget (tests/test_kernel_metadata_pose.py): no scratch, no spills; k_pose_recover at most 96 VGPRs and 80 bytes of LDS
// (the compiler gives 90: five waves per SIMD).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lcm_kernels.h"
#include "lcm_pose_device.h"

namespace lcm {

__global__ __launch_bounds__(256) void k_pose_recover(PoseArgs a) {
    __shared__ uint32_t wave_cnt[4][5];
    const uint32_t p = a.pair_base + blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t first = a.offsets[p];
    const uint32_t n = (uint32_t)(a.offsets[p + 1] - first);
    const double* eb = a.E + (size_t)p * a.e_stride;
    double e[9], ra[9], rb[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = eb[k];
    const bool ok = pose_decompose(e, ra, rb, t);              // the same for every thread of the workgroup
    PoseResult* res = reinterpret_cast<PoseResult*>(a.results) + p;
    if (threadIdx.x == 0 && a.cand_R) {
        double* cr = a.cand_R + (size_t)p * 36;
        double* ct = a.cand_t + (size_t)p * 12;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double r[9], tk[3];
            pose_candidate(k, ra, rb, t, r, tk);
#pragma unroll
            for (int i = 0; i < 9; ++i) cr[9 * k + i] = r[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) ct[3 * k + i] = ok ? tk[i] : 0.0;      // not -0.0
        }
    }
    if (!ok) {                                                 // the whole workgroup
        for (uint32_t i = threadIdx.x; i < n; i += 256) a.mask_out[first + i] = 0;
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) res->R[i] = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) res->t[i] = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) res->counts[k] = 0;
            res->n_used = 0; res->n_good = 0; res->choice = -1; res->status = 1;      // LCM_POSE_NO_MODEL
        }
        return;
    }
    // pass 1: the four counts
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, used = 0;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        if (a.mask_in && a.mask_in[first + i] == 0) continue;
        const uint4 r = a.pts[first + i];
        const double x1 = epi_norm(__uint_as_float(r.x), a.cx, a.fx), y1 = epi_norm(__uint_as_float(r.y), a.cy, a.fy);
        const double x2 = epi_norm(__uint_as_float(r.z), a.cx, a.fx), y2 = epi_norm(__uint_as_float(r.w), a.cy, a.fy);
        c0 += pose_in_front(ra, t[0], t[1], t[2], x1, y1, x2, y2, a.max_depth) ? 1u : 0u;
        c1 += pose_in_front(rb, t[0], t[1], t[2], x1, y1, x2, y2, a.max_depth) ? 1u : 0u;
        c2 += pose_in_front(ra, -t[0], -t[1], -t[2], x1, y1, x2, y2, a.max_depth) ? 1u : 0u;
        c3 += pose_in_front(rb, -t[0], -t[1], -t[2], x1, y1, x2, y2, a.max_depth) ? 1u : 0u;
        used += 1u;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        c0 += (uint32_t)__shfl_xor((int)c0, o, 64);
        c1 += (uint32_t)__shfl_xor((int)c1, o, 64);
        c2 += (uint32_t)__shfl_xor((int)c2, o, 64);
        c3 += (uint32_t)__shfl_xor((int)c3, o, 64);
        used += (uint32_t)__shfl_xor((int)used, o, 64);
    }
    if (lane == 0) { wave_cnt[wave][0] = c0; wave_cnt[wave][1] = c1; wave_cnt[wave][2] = c2; wave_cnt[wave][3] = c3; wave_cnt[wave][4] = used; }
    __syncthreads();
    c0 = wave_cnt[0][0] + wave_cnt[1][0] + wave_cnt[2][0] + wave_cnt[3][0];
    c1 = wave_cnt[0][1] + wave_cnt[1][1] + wave_cnt[2][1] + wave_cnt[3][1];
    c2 = wave_cnt[0][2] + wave_cnt[1][2] + wave_cnt[2][2] + wave_cnt[3][2];
    c3 = wave_cnt[0][3] + wave_cnt[1][3] + wave_cnt[2][3] + wave_cnt[3][3];
    used = wave_cnt[0][4] + wave_cnt[1][4] + wave_cnt[2][4] + wave_cnt[3][4];
    const int choice = pose_choose(c0, c1, c2, c3);
    double rk[9], tk[3];
    pose_candidate(choice, ra, rb, t, rk, tk);
    // pass 2: the chosen hypothesis's verdict per record
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        bool in = false;
        if (!a.mask_in || a.mask_in[first + i] != 0) {
            const uint4 r = a.pts[first + i];
            in = pose_in_front(rk, tk[0], tk[1], tk[2], epi_norm(__uint_as_float(r.x), a.cx, a.fx), epi_norm(__uint_as_float(r.y), a.cy, a.fy),
                               epi_norm(__uint_as_float(r.z), a.cx, a.fx), epi_norm(__uint_as_float(r.w), a.cy, a.fy), a.max_depth);
        }
        a.mask_out[first + i] = in ? 1 : 0;
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) res->R[i] = rk[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) res->t[i] = tk[i];
        res->counts[0] = (int32_t)c0; res->counts[1] = (int32_t)c1; res->counts[2] = (int32_t)c2; res->counts[3] = (int32_t)c3;
        res->n_used = (int32_t)used;
        res->n_good = (int32_t)(choice == 0 ? c0 : (choice == 1 ? c1 : (choice == 2 ? c2 : c3)));
        res->choice = choice; res->status = 0;                // LCM_POSE_OK
    }
}

hipError_t launch_pose_recover(const PoseArgs& a, uint32_t n_pairs, hipStream_t st) {
    return launch_y_sliced(k_pose_recover, a, &PoseArgs::pair_base, n_pairs, 1, 256, st);
}

}  // namespace lcm
