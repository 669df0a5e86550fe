// lcm_l2_store.hip — the ratio-test count of lcm_l2_count.hip over the device-resident SIFT keyframe store
// (lcm_l2_db_loop_search, lcm_l2_db_detect_loops; src/main.cpp:1375-1388 keyframe by keyframe or in bulk).
//
// k_l2_count<QT> reads a 32-byte item per workgroup from a table the host builds and uploads per call: pairs x chunks
// entries.  With the matrices stored, a loop search is fully described by tables that grow with the number of FRAMES:
// the store's frame table {first tile, rows} per slot (kept current at append), one ascending list of admitted slots, and
// one 24-byte entry per run (a `curr` and how many leading entries of the list are its pasts): lcm_kernels.h, L2StoreRun.
//
// k_l2_count_store<QT>  one workgroup (4 waves) = one (pair, query chunk) item that it derives itself:
//                  run u = the last run with first_wg <= blockIdx.x (binary search; blockIdx.x is workgroup-uniform, so
//                  the probes are scalar loads and every branch is uniform), l = blockIdx.x - first_wg, pair k = l / chunks,
//                  chunk c = l % chunks, train matrix = frames[past[k]].  Then l2_count_item (lcm_l2_count_device.h), the
//                  body that k_l2_count runs: the verdict, the roots and the top-2 update exist once.  The decode is a
//                  handful of scalar loads and one 32-bit division per workgroup beside a train matrix of MFMA work.
//
// Budget (tests/test_kernel_metadata_l2_store.py): no scratch, no spills, no LDS; k_l2_count_store<1> at most 128 VGPRs
// (4 waves per SIMD), <2> at most 168 (3 waves per SIMD).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcm_kernels.h"
#include "lcm_l2_count_device.h"

namespace lcm {

template <int QT>
__global__ __launch_bounds__(256, QT == 1 ? 4 : 3) void k_l2_count_store(L2StoreArgs a) {
    const uint32_t wg = blockIdx.x;
    uint32_t lo = 0, hi = a.n_runs;                             // runs[lo].first_wg <= wg < runs[hi].first_wg (hi = n_runs: the grid's end)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.runs[mid].first_wg <= wg) lo = mid; else hi = mid;
    }
    const L2StoreRun run = a.runs[lo];
    const uint32_t local = wg - run.first_wg, k = local / run.chunks, c = local - k * run.chunks;
    if (k >= run.n_past) return;                                // never: the grid ends with the last run
    const uint2 train = a.frames[a.past[k]];
    const uint32_t chunk_rows = (uint32_t)(QT * 4 * L2_TILE_ROWS);
    l2_count_item<QT>(a.img, a.tw, run.q_tile + c * (uint32_t)(QT * 4), min(chunk_rows, run.q_rows - c * chunk_rows), train.x, train.y,
                      reinterpret_cast<uint32_t*>(a.scores + run.first_pair + k), a.ratio);
}

hipError_t launch_l2_count_store(const L2StoreArgs& a, uint32_t n_workgroups, hipStream_t st) {
    if (n_workgroups == 0 || a.n_runs == 0) return hipSuccess;
    if (a.chunk_rows == 128) hipLaunchKernelGGL(k_l2_count_store<1>, dim3(n_workgroups), dim3(256), 0, st, a);
    else if (a.chunk_rows == 256) hipLaunchKernelGGL(k_l2_count_store<2>, dim3(n_workgroups), dim3(256), 0, st, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace lcm
