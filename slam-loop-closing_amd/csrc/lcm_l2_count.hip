// lcm_l2_count.hip — the loop search's score on SIFT rows: per (query matrix, train matrix) pair the NUMBER of query rows
// that pass Lowe's ratio test after BFMatcher(NORM_L2).knnMatch(k = 2), which is all the reference looks at
// (src/main.cpp:1375-1388: matchFeatures(desc[curr], desc[past], matches, 0.7), then matches.size() >= 300).
//
// THE COUNT NEEDS NO INDICES.  The verdict (double)s1 < ratio * (double)s2 depends on the row's two smallest float
// distances only; sqrtf is monotone, so they are the roots of the two smallest D as a MULTISET.  Which train row is
// reported among equal roots (the (s, index) rule above 2^22 that lcm_l2.hip's rescan settles) never changes (s1, s2).
// So one workgroup walks a pair's whole train matrix with the running keys in registers: no per-segment scratch, no fold,
// no flag list, no rescan, 8 bytes per pair leave the device.
//
// k_l2_count_init  (good_count, min_dist_sq) <- (0, 0xFFFFFFFF) for every pair of the call, on the stream, every call.
// k_l2_count<QT>   one workgroup (4 waves) = one item: a chunk of 128 * QT query rows of one pair against ALL train tiles of
//                  the pair.  Operand image, per-row words, MFMA tile loop and the exact top-2 update are k_l2_score's
//                  (lcm_l2.hip, lcm_l2_device.h).  The keys stay D << 9 | index inside the row's 512-row segment: rows of
//                  different segments can now meet with EQUAL keys in one running list, which the update treats as a
//                  multiset (two rows with equal D are first and second neighbour).  The padding trap applies to the one
//                  partial last tile of the matrix (checked epilogue, wave-uniform branch).
//                  End of the item: the two lanes of a query row merge; with QT = 2 lane half h then takes query tile h, so
//                  the wave evaluates 32 * QT rows in ONE pass: D -> the exact float roots -> the double comparison, one
//                  ballot, one atomicAdd (good_count) and one atomicMin (min_dist_sq) per wave.  Integer vector atomics:
//                  the result does not depend on the order of the workgroups.  Nothing crosses waves: no LDS.
// k_l2_ratio_test  diagnostic: l2_ratio_pass over host-given (D1, D2) pairs, the function the count kernel calls.
//
// THE ROOTS ARE EXACT.  For every integer D in [0, 8 323 200], (float)sqrt((double)D) has the bits of sqrtf((float)D): the
// double root is correctly rounded (53 bits), and it lies at least 2^-39 from every midpoint between two floats (a
// midpoint m below 4096 is a multiple of 2^-13, m^2 of 2^-26, and |sqrt(D) - m| = |D - m^2| / (sqrt(D) + m)), four double
// ulps at the top of the range, so the second rounding to 24 bits cannot cross one.  The comparison is one double multiply
// and one compare: nothing to contract, and the build passes no fast-math flag (contraction is switched off here anyway).
//
// Budget (tests/test_kernel_metadata_l2_count.py): no scratch, no spills, no LDS; k_l2_count<1> at most 128 VGPRs (4 waves
// per SIMD), <2> at most 168 (3 waves per SIMD).  The accumulators are read by compiler-visible code only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lcm_kernels.h"
#include "lcm_l2_count_device.h"

namespace lcm {

__global__ __launch_bounds__(256) void k_l2_count_init(uint2* scores, uint32_t n_pairs) {
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n_pairs; p += gridDim.x * 256u) scores[p] = make_uint2(0u, L2_NONE);
}

hipError_t launch_l2_count_init(uint2* scores, uint32_t n_pairs, hipStream_t st) {
    if (n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_l2_count_init, dim3(std::min((n_pairs + 255u) / 256u, 1024u)), dim3(256), 0, st, scores, n_pairs);
    return hipGetLastError();
}

template <int QT>
__global__ __launch_bounds__(256, QT == 1 ? 4 : 3) void k_l2_count(L2CountArgs a) {
    const L2CountItem it = a.items[blockIdx.x];
    l2_count_item<QT>(a.img, a.tw, it.q_tile, it.q_rows, it.t_tile, it.t_rows, reinterpret_cast<uint32_t*>(a.scores + it.pair), a.ratio);
}

hipError_t launch_l2_count(const L2CountArgs& a, uint32_t n_items, hipStream_t st) {
    if (n_items == 0) return hipSuccess;
    if (a.chunk_rows == 128) hipLaunchKernelGGL(k_l2_count<1>, dim3(n_items), dim3(256), 0, st, a);
    else if (a.chunk_rows == 256) hipLaunchKernelGGL(k_l2_count<2>, dim3(n_items), dim3(256), 0, st, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_l2_ratio_test(const uint32_t* d1, const uint32_t* d2, size_t n, double ratio, uint8_t* pass) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u)
        pass[i] = l2_ratio_pass(d1[i], d2[i], ratio) ? 1 : 0;
}

hipError_t launch_l2_ratio_test(const uint32_t* d1, const uint32_t* d2, size_t n, double ratio, uint8_t* pass, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_l2_ratio_test, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st, d1, d2, n, ratio, pass);
    return hipGetLastError();
}

}  // namespace lcm
