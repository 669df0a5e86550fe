// lcm_l2_emit.hip — the last step of the reference's loop search on SIFT rows, on the device: Lowe's ratio test over the
// folded neighbours, the survivors compacted in query order, and their keypoints gathered (src/main.cpp:524-531 inside
// matchFeatures, :551-555 extractMatchedPoints; called at :1386-1392).  lcm_l2_db_match_points and
// lcm_l2_db_detect_loops_points run it over the SIFT keyframe store, whose fourth arena keeps a frame's keypoints.
//
// The kernels read final_keys, (D1, idx1, D2, idx2) per query row of every job, and therefore run AFTER k_l2_rescan, which
// rewrites the rows whose second neighbour may share a float root with a rival.  A job's query rows are cut into blocks of
// 256 (lcm_kernels.h, L2EmitArgs); the job comes from blockIdx.y, in slices (launch_y_sliced) as k_l2_fold's does.
//
// k_l2_emit_count    one workgroup per block: the survivors of l2_ratio_pass (lcm_l2_count_device.h: the one verdict, the
//                    host's bit for bit) among its rows -> blocks[block].  A row without a second neighbour is dropped.
//                    k_block_scan (lcm_kernels.hip) then turns the counts of the whole call into exclusive prefixes.
// k_l2_emit_offsets  one thread per pair of the call: offsets[p] = prefix of the first block at or after pair p (64-bit).
// k_l2_emit          the verdict again; a survivor's rank inside its block comes from the wave's ballot (popcount of the
//                    lower lanes) plus the counts of the waves before it, so record blocks[block] + rank is in query order by
//                    construction, whatever the order the workgroups run in.  One 16-byte store of {query row, idx1, 0,
//                    sqrtf(D1)}; with points a second one of the two 8-byte keypoints, which are moved as bits (no
//                    arithmetic touches them: NaN and -0.0 survive).
// HBM-bound: 16 bytes read per query row, twice; 16 or 32 bytes written and 16 gathered per survivor.
//
// Budget (tests/test_kernel_metadata_l2_emit.py): no scratch, no spills, at most 128 VGPRs, 16 bytes of LDS (the four
// waves' counts) in k_l2_emit_count and k_l2_emit, none in k_l2_emit_offsets.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lcm_kernels.h"
#include "lcm_l2_count_device.h"

namespace lcm {

// row r of the job: does it survive?  k = its (D1, idx1, D2, idx2)
__device__ __forceinline__ bool l2_emit_verdict(const L2EmitArgs& a, const L2Job& jb, uint32_t r, uint4& k) {
    if (r >= jb.nq) return false;
    k = a.final_keys[(size_t)jb.out_row0 + r];
    return k.w != L2_NONE && l2_ratio_pass(k.x, k.z, a.ratio);
}

__global__ __launch_bounds__(256) void k_l2_emit_count(L2EmitArgs a) {
    __shared__ uint32_t wave_n[4];
    const L2Job jb = a.jobs[a.job_base + blockIdx.y];
    if (blockIdx.x * 256u >= jb.nq) return;                    // whole workgroup: the grid's x is the longest job's
    uint4 k;
    const bool pass = l2_emit_verdict(a, jb, blockIdx.x * 256u + threadIdx.x, k);
    const uint64_t m = __ballot(pass);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) a.blocks[jb.reserved + blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

__global__ __launch_bounds__(256) void k_l2_emit_offsets(const uint32_t* blocks, const uint32_t* pair_block, uint64_t* offsets, uint32_t n) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < n) offsets[p] = blocks[pair_block[p]];
}

__global__ __launch_bounds__(256) void k_l2_emit(L2EmitArgs a) {
    __shared__ uint32_t wave_n[4];
    const L2Job jb = a.jobs[a.job_base + blockIdx.y];
    if (blockIdx.x * 256u >= jb.nq) return;
    const uint32_t r = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint4 k;
    const bool pass = l2_emit_verdict(a, jb, r, k);
    const uint64_t m = __ballot(pass);
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!pass) return;
    uint32_t at = a.blocks[jb.reserved + blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; ++w) at += wave_n[w];
    if (at >= a.n_out) return;                                 // never: n_out is the scan's total over these verdicts
    a.out[at] = make_uint4(r, k.y, 0u, __float_as_uint(l2_root(k.x)));
    if (a.pts) {
        const uint2 q = a.pts[(size_t)jb.q_tile * L2_TILE_ROWS + r], t = a.pts[(size_t)jb.t_tile * L2_TILE_ROWS + k.y];
        a.out_pts[at] = make_uint4(q.x, q.y, t.x, t.y);
    }
}

hipError_t launch_l2_emit_count(const L2EmitArgs& a, uint32_t n_jobs, uint32_t max_nq, hipStream_t st) {
    if (n_jobs == 0 || max_nq == 0) return hipSuccess;
    return launch_y_sliced(k_l2_emit_count, a, &L2EmitArgs::job_base, n_jobs, (max_nq + 255) / 256, 256, st);
}

hipError_t launch_l2_emit(const L2EmitArgs& a, uint32_t n_jobs, uint32_t max_nq, hipStream_t st) {
    if (n_jobs == 0 || max_nq == 0) return hipSuccess;
    return launch_y_sliced(k_l2_emit, a, &L2EmitArgs::job_base, n_jobs, (max_nq + 255) / 256, 256, st);
}

hipError_t launch_l2_emit_offsets(const uint32_t* blocks, const uint32_t* pair_block, uint64_t* offsets, uint32_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_l2_emit_offsets, dim3((n + 255) / 256), dim3(256), 0, st, blocks, pair_block, offsets, n);
    return hipGetLastError();
}

}  // namespace lcm
