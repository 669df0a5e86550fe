// lcm_epi.hip — the reference's loop verification on the device: cv::findEssentialMat(ptsCurr, ptsPast, K, RANSAC) and
// the inlier count (src/main.cpp:1395-1400), as a RANSAC whose every step is defined in lcm_epi_device.h: a counter-based
// sampler, the linear eight-point solver on normalised coordinates, a fixed number of hypotheses, first-of-equals selection.
// The kernels run on the point records k_l2_emit has just written (lcm_epi_db_*), or on a caller's (lcm_epi_verify_pairs).
// The pair comes from blockIdx.y, in slices (launch_y_sliced, lcm_kernels.h) as k_l2_fold's does.
//
// k_epi_solve   one lane per (pair, hypothesis), one wave per workgroup: the lane draws its 8 indices, normalises those 8
//               records, lays the 8 x 9 system into its own column of LDS (72 doubles x 64 lanes: runtime row and column
//               indices of the pivoting address LDS, not registers), eliminates, projects, and writes 8 indices + 9 doubles.
//               A pair with fewer than 8 records gets indices -1 and zero matrices.
// k_epi_score   four waves per workgroup, one lane per hypothesis: E in 18 VGPRs, one running count.  The workgroup
//               normalises 512 records at a time into LDS, once, and every lane reads them back at the same address (a
//               broadcast); the count goes by epi_inlier.  Per pair the maximum of (count << 16 | 0xFFFF - hypothesis) is
//               taken in the wave, in LDS over the four waves, and by one atomic maximum per workgroup into best[pair]:
//               the largest count, among equals the lowest hypothesis, whatever the order the workgroups run in.
// k_epi_mask    one thread per record: the same verdict against the pair's winning E -> one byte; thread 0 of the pair's
//               first workgroup writes the pair's result record.
//
// Budget (tests/test_kernel_metadata_epi.py): no scratch, no spills; k_epi_solve at most 192 VGPRs and 36 864 bytes of
// LDS, k_epi_score at most 64 VGPRs and 16 400 bytes (512 records x 32 + the four waves' keys), k_epi_mask at most 64
// VGPRs and no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lcm_epi_device.h"
#include "lcm_kernels.h"

namespace lcm {

constexpr int EPI_CHUNK = 512;                // records normalised into LDS per pass of k_epi_score

__global__ __launch_bounds__(64) void k_epi_solve(EpiArgs a) {
    __shared__ double sys[EPI_SAMPLE * 9 * 64];
    const uint32_t p = a.pair_base + blockIdx.y, lane = threadIdx.x, it = blockIdx.x * 64u + lane;
    const uint64_t first = a.offsets[p];
    const uint64_t n = a.offsets[p + 1] - first;
    const size_t hyp = (size_t)p * a.iters + it;
    int32_t* so = a.samples + hyp * EPI_SAMPLE;
    double* eo = a.E + hyp * 9;
    double e[9];
    if (n < (uint64_t)EPI_SAMPLE) {              // the whole workgroup
#pragma unroll
        for (int k = 0; k < EPI_SAMPLE; ++k) so[k] = -1;
#pragma unroll
        for (int k = 0; k < 9; ++k) eo[k] = 0.0;
        return;
    }
    uint32_t s[EPI_SAMPLE];
    epi_sample8(a.seed, a.pair_seed0 + p, it, (uint32_t)n, s);
    double* A = sys + lane;
#pragma unroll
    for (int k = 0; k < EPI_SAMPLE; ++k) {
        const uint4 r = a.pts[first + s[k]];
        epi_put_row<64>(A, k, epi_norm(__uint_as_float(r.x), a.cx, a.fx), epi_norm(__uint_as_float(r.y), a.cy, a.fy),
                        epi_norm(__uint_as_float(r.z), a.cx, a.fx), epi_norm(__uint_as_float(r.w), a.cy, a.fy));
        so[k] = (int32_t)s[k];
    }
    epi_solve8<64>(A, e);
#pragma unroll
    for (int k = 0; k < 9; ++k) eo[k] = e[k];
}

__global__ __launch_bounds__(256) void k_epi_score(EpiArgs a) {
    __shared__ double rec[EPI_CHUNK * 4];
    __shared__ uint32_t wave_key[4];
    const uint32_t p = a.pair_base + blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t it = (blockIdx.x * 4u + wave) * 64u + lane;
    const bool active = it < a.iters;            // wave-uniform: iters is a multiple of 64
    const uint64_t first = a.offsets[p];
    const uint32_t n = (uint32_t)(a.offsets[p + 1] - first);
    const size_t hyp = (size_t)p * a.iters + it;
    double e[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = active ? a.E[hyp * 9 + k] : 0.0;
    uint32_t count = 0;
    for (uint32_t base = 0; base < n; base += EPI_CHUNK) {
        const uint32_t m = min((uint32_t)EPI_CHUNK, n - base);
        __syncthreads();                         // the previous chunk has been read by every wave
        for (uint32_t i = threadIdx.x; i < m; i += 256) {
            const uint4 r = a.pts[first + base + i];
            rec[4 * i + 0] = epi_norm(__uint_as_float(r.x), a.cx, a.fx);
            rec[4 * i + 1] = epi_norm(__uint_as_float(r.y), a.cy, a.fy);
            rec[4 * i + 2] = epi_norm(__uint_as_float(r.z), a.cx, a.fx);
            rec[4 * i + 3] = epi_norm(__uint_as_float(r.w), a.cy, a.fy);
        }
        __syncthreads();
        if (active)
            for (uint32_t i = 0; i < m; ++i)
                count += epi_inlier(e, rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3], a.t2) ? 1u : 0u;
    }
    if (active && a.counts) a.counts[hyp] = count;
    uint32_t key = active ? (count << 16 | (0xFFFFu - it)) : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, o, 64));
    if (lane == 0) wave_key[wave] = key;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(a.best + p, max(max(wave_key[0], wave_key[1]), max(wave_key[2], wave_key[3])));
}

__global__ __launch_bounds__(256) void k_epi_mask(EpiArgs a) {
    const uint32_t p = a.pair_base + blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    const uint64_t first = a.offsets[p];
    const uint32_t n = (uint32_t)(a.offsets[p + 1] - first);
    if (blockIdx.x * 256u >= n && blockIdx.x != 0) return;     // whole workgroup: the grid's x is the longest pair's
    const uint32_t key = a.best[p], it = min(0xFFFFu - (key & 0xFFFFu), a.iters - 1u);     // k_epi_score left a key of a hypothesis < iters
    const double* eb = a.E + ((size_t)p * a.iters + it) * 9;
    double e[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = eb[k];
    if (i == 0) {
        EpiResult* r = reinterpret_cast<EpiResult*>(a.results) + p;
#pragma unroll
        for (int k = 0; k < 9; ++k) r->E[k] = e[k];
        r->n_points = (int32_t)n; r->n_inliers = (int32_t)(key >> 16); r->best_iter = (int32_t)it;
        r->status = n < (uint32_t)EPI_SAMPLE ? 1 : 0;          // LCM_EPI_TOO_FEW : LCM_EPI_OK
    }
    if (i >= n) return;
    const uint4 r = a.pts[first + i];
    const bool in = epi_inlier(e, epi_norm(__uint_as_float(r.x), a.cx, a.fx), epi_norm(__uint_as_float(r.y), a.cy, a.fy),
                               epi_norm(__uint_as_float(r.z), a.cx, a.fx), epi_norm(__uint_as_float(r.w), a.cy, a.fy), a.t2);
    a.mask[first + i] = in ? 1 : 0;
}

hipError_t launch_epi_solve(const EpiArgs& a, uint32_t n_pairs, hipStream_t st) {
    return launch_y_sliced(k_epi_solve, a, &EpiArgs::pair_base, n_pairs, a.iters / 64u, 64, st);
}

hipError_t launch_epi_score(const EpiArgs& a, uint32_t n_pairs, hipStream_t st) {
    return launch_y_sliced(k_epi_score, a, &EpiArgs::pair_base, n_pairs, (a.iters + 255u) / 256u, 256, st);
}

hipError_t launch_epi_mask(const EpiArgs& a, uint32_t n_pairs, uint32_t max_n, hipStream_t st) {
    return launch_y_sliced(k_epi_mask, a, &EpiArgs::pair_base, n_pairs, std::max(1u, (max_n + 255u) / 256u), 256, st);
}

}  // namespace lcm
