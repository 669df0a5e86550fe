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
#include "lcm_l2_device.h"

namespace lcm {

// OpenCV's distance of a squared distance D <= L2_MAX_DSQ: sqrtf((float)D), bit for bit (see above)
__device__ __forceinline__ float l2_root(uint32_t D) { return (float)sqrt((double)D); }

// Lowe's ratio test on the two smallest squared distances of a query row (src/main.cpp:524-531), as lcm_l2.cpp's host
// list runs it: strict, in IEEE double.
__device__ __forceinline__ bool l2_ratio_pass(uint32_t D1, uint32_t D2, double ratio) {
#pragma clang fp contract(off)
    const double s1 = (double)l2_root(D1), s2 = (double)l2_root(D2);
    const double lim = ratio * s2;
    return s1 < lim;
}

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
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const uint32_t qt0 = wave * QT;
    if (qt0 * L2_TILE_ROWS >= it.q_rows) return;               // whole wave, no barrier in this kernel
    const uint4* img = reinterpret_cast<const uint4*>(a.img);

    // B operands: this wave's query tiles x 4 k-steps, resident for the whole item (tiles past the chunk: zeros, unused)
    l2_v4i b[QT][4];
    uint32_t qterm[QT], b1[QT], b2[QT];
#pragma unroll
    for (int j = 0; j < QT; ++j) {
        const bool have = (qt0 + j) * L2_TILE_ROWS < it.q_rows;
        const size_t tile = (size_t)it.q_tile + qt0 + j;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            uint4 x = make_uint4(0, 0, 0, 0);
            if (have) x = img[tile * 256 + ks * 64 + lane];
            b[j][ks] = l2_v4i{(int)x.x, (int)x.y, (int)x.z, (int)x.w};
        }
        qterm[j] = have ? (a.tw[tile * L2_TILE_ROWS + r] & ~((1u << L2_KEY_SHIFT) - 1u)) : 0u;
        b1[j] = b2[j] = L2_NONE;
    }

    // every train tile of the matrix, the next one's fragments in flight; the running keys live across all of them
    const uint32_t nt = it.t_rows, nt_tiles = (nt + L2_TILE_ROWS - 1) / L2_TILE_ROWS;
    const uint4* timg = img + (size_t)it.t_tile * 256 + lane;
    const uint4* ttw = reinterpret_cast<const uint4*>(a.tw + (size_t)it.t_tile * L2_TILE_ROWS) + h;
    uint4 cur[4], nxt[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) cur[ks] = nxt[ks] = timg[ks * 64];
    for (uint32_t t = 0; t < nt_tiles; ++t) {
        if (t + 1 < nt_tiles) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) nxt[ks] = timg[(size_t)(t + 1) * 256 + ks * 64];
        }
        // this lane's 16 train rows of the tile: rows 8 g + 4 h + {0..3} = registers 4 g + {0..3}
        uint32_t tw[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint4 x = ttw[(size_t)t * 8 + 2 * g];
            tw[4 * g] = x.x; tw[4 * g + 1] = x.y; tw[4 * g + 2] = x.z; tw[4 * g + 3] = x.w;
        }
        const bool partial = (t + 1) * L2_TILE_ROWS > nt;       // wave-uniform: only the matrix's last tile
#pragma unroll
        for (int j = 0; j < QT; ++j) {
            l2_v16i acc = {0};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(l2_v4i{(int)cur[ks].x, (int)cur[ks].y, (int)cur[ks].z, (int)cur[ks].w},
                                                            b[j][ks], acc, 0, 0, 0);
            if (partial) l2_epilogue<true>(acc, tw, qterm[j], b1[j], b2[j], t * L2_TILE_ROWS + 4 * h, nt);
            else l2_epilogue<false>(acc, tw, qterm[j], b1[j], b2[j], 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) cur[ks] = nxt[ks];
    }

    // lanes l and l + 32 hold the same query rows over different train rows: after the merge BOTH hold the row's list
#pragma unroll
    for (int j = 0; j < QT; ++j) {
        const uint32_t o1 = (uint32_t)__shfl_xor((int)b1[j], 32, 64), o2 = (uint32_t)__shfl_xor((int)b2[j], 32, 64);
        l2_top2_insert(b1[j], b2[j], o1);
        l2_top2_insert(b1[j], b2[j], o2);
    }
    // lane half h evaluates query tile h (QT = 2), half 0 the only tile (QT = 1); rows past the chunk are excluded
    const uint32_t mine = QT == 2 ? h : 0u;
    const uint32_t k1 = mine ? b1[QT - 1] : b1[0], k2 = mine ? b2[QT - 1] : b2[0];
    const uint32_t row = (qt0 + mine) * L2_TILE_ROWS + r;
    const bool live = (QT == 2 || h == 0) && row < it.q_rows;
    const uint32_t D1 = k1 >> L2_KEY_SHIFT, D2 = k2 >> L2_KEY_SHIFT;
    const bool pass = live && k2 != L2_NONE && l2_ratio_pass(D1, D2, a.ratio);     // fewer than 2 neighbours: not counted
    const uint32_t good = (uint32_t)__popcll(__ballot(pass));
    uint32_t dmin = live && k1 != L2_NONE ? D1 : L2_NONE;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) dmin = min(dmin, (uint32_t)__shfl_xor((int)dmin, o, 64));
    if (lane == 0) {
        uint32_t* rec = reinterpret_cast<uint32_t*>(a.scores + it.pair);
        if (good) atomicAdd(rec, good);
        if (dmin != L2_NONE) atomicMin(rec + 1, dmin);
    }
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
