// lcm_knn.hip — pair mode with TWO neighbours per query row: cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2), the matcher the
// reference actually runs before Lowe's ratio test (src/main.cpp:509-534).
//
// OpenCV's batchDistance with K = 2 scans the train rows in ascending order, admits a candidate only if d < dist[K-1] and
// shifts it past entries with dist[k] > d (strict): a query row's neighbours are the TWO SMALLEST packed keys
// dist << 22 | train_idx — ascending by distance, lower index first among equal distances.
//
// k_knn2_rowlane is the pair mode's keyed kernel (lcm_kernels.hip, k_score_rowlane with ARGMIN_MODE 2) with a second
// running key per query row: lanes own query rows in VGPRs, train rows arrive wave-uniform through s_load, one packed key
// per distance, xors at priority 0 and everything else inside s_setprio 3 ... s_setprio 0.  Each query row keeps two keys
// b1 <= b2; two new keys k0, k1 update them exactly in three quarter-rate instructions:
//     m  = med3(b1, k0, k1);  b2 = min(b2, m);  b1 = min3(b1, k0, k1)
// (the second smallest of {b1, b2, k0, k1} with b1 <= b2 is min(b2, median(b1, k0, k1))).
//
// What k = 1 never had to care about: the train role is padded with COPIES of a matrix's last row (to a multiple of 4 rows,
// plus 4 for the prefetch) and the last loop trip reads them.  For k = 1 a copy never wins (same distance, higher index);
// for k = 2 it would be the SECOND neighbour whenever the last row is the best.  Rows >= nt of an item therefore get
// 0xFFFFFFFF as the index operand of v_lshl_or_b32: the key becomes 0xFFFFFFFF, above every real key (at most
// 256 << 22 | 0x3FFFFF), at no extra instruction — the row index is wave-uniform and selected on the scalar unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lcm_kernels.h"

namespace lcm {

typedef const uint32_t __attribute__((address_space(4))) * knn_sptr_t;   // constant AS => SMEM (s_load) when uniform

constexpr uint32_t KNN_NONE = 0xFFFFFFFFu;     // "no neighbour": above every real key

// One (xor, xor | popcount, popcount) phase of the two chains: word SA of train row 0, word SB of train row 1, word QV of
// the query row; ACC0 / ACC1 = what the popcounts add to ("0" in the first phase).
#define LCM_KNN_PHASE(SA, SB, QV, ACC0, ACC1)                                                                  \
    "v_xor_b32_e32 %4, %" #SA ", %" #QV "\n\tv_xor_b32_e32 %5, %" #SB ", %" #QV "\n\ts_setprio 3\n\t"           \
    "v_bcnt_u32_b32 %2, %4, " ACC0 "\n\tv_bcnt_u32_b32 %3, %5, " ACC1 "\n\t"

// One query row (8 VGPRs) against TWO train rows (16 SGPRs): both distances, both packed keys (i0 / i1 = the rows' indices
// inside the item, or KNN_NONE for a padding row) and the exact top-2 update, as ONE asm statement so that the instruction
// order is exactly the one below.  Operands: %0 b1, %1 b2, %2 %3 the two distances / keys, %4 %5 temporaries,
// %6..%13 train row 0, %14..%21 train row 1, %22..%29 the query row, %30 %31 the index operands.
__device__ __forceinline__ void fold2_knn(uint32_t& b1, uint32_t& b2, const uint32_t (&q)[8], const uint32_t* s, uint32_t i0, uint32_t i1) {
    uint32_t d0, d1, x0, x1;
    asm volatile(
        LCM_KNN_PHASE(6, 14, 22, "0", "0") "s_setprio 0\n\t"
        LCM_KNN_PHASE(7, 15, 23, "%2", "%3") "s_setprio 0\n\t"
        LCM_KNN_PHASE(8, 16, 24, "%2", "%3") "s_setprio 0\n\t"
        LCM_KNN_PHASE(9, 17, 25, "%2", "%3") "s_setprio 0\n\t"
        LCM_KNN_PHASE(10, 18, 26, "%2", "%3") "s_setprio 0\n\t"
        LCM_KNN_PHASE(11, 19, 27, "%2", "%3") "s_setprio 0\n\t"
        LCM_KNN_PHASE(12, 20, 28, "%2", "%3") "s_setprio 0\n\t"
        LCM_KNN_PHASE(13, 21, 29, "%2", "%3")
        "v_lshl_or_b32 %2, %2, 22, %30\n\t"
        "v_lshl_or_b32 %3, %3, 22, %31\n\t"
        "v_med3_u32 %4, %0, %2, %3\n\t"
        "v_min_u32_e32 %1, %4, %1\n\t"
        "v_min3_u32 %0, %0, %2, %3\n\ts_setprio 0"
        : "+v"(b1), "+v"(b2), "=&v"(d0), "=&v"(d1), "=&v"(x0), "=&v"(x1)
        : "s"(s[0]), "s"(s[1]), "s"(s[2]), "s"(s[3]), "s"(s[4]), "s"(s[5]), "s"(s[6]), "s"(s[7]),
          "s"(s[8]), "s"(s[9]), "s"(s[10]), "s"(s[11]), "s"(s[12]), "s"(s[13]), "s"(s[14]), "s"(s[15]),
          "v"(q[0]), "v"(q[1]), "v"(q[2]), "v"(q[3]), "v"(q[4]), "v"(q[5]), "v"(q[6]), "v"(q[7]),
          "s"(i0), "s"(i1));
}
#undef LCM_KNN_PHASE

// One workgroup = one PairItem: <= THREADS * QPT query rows against one segment of a train matrix.  Writes the two
// smallest keys (segment-local train indices) of every query row: keys[(out_offset * keys_stride + row) * 2 + {0, 1}].
// 5 waves per SIMD (96 VGPRs), the budget of the k = 1 keyed kernel: 64 hold the query rows and 16 the running keys of
// the 8-rows-per-lane shape, which comes to 91.
template <int THREADS, int QPT>
__global__ __launch_bounds__(THREADS, 5) void k_knn2_rowlane(Knn2Args a) {
    const int tid = threadIdx.x;
    const PairItem pi = a.items[blockIdx.x];
    const int nq = (int)(pi.nq_nt & 0xFFFu);
    const uint32_t nt = pi.nq_nt >> 12;

    // ---- this lane's query rows: row = j * THREADS + tid (consecutive lanes -> consecutive 32-byte rows)
    uint32_t q[QPT][8];
    const uint4* qbase = reinterpret_cast<const uint4*>(a.q_rows + (size_t)pi.q_row * 8);
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const int row = j * THREADS + tid;
        uint4 lo = make_uint4(0, 0, 0, 0), hi = make_uint4(0, 0, 0, 0);
        if (row < nq) { lo = qbase[row * 2]; hi = qbase[row * 2 + 1]; }
        q[j][0] = lo.x; q[j][1] = lo.y; q[j][2] = lo.z; q[j][3] = lo.w;
        q[j][4] = hi.x; q[j][5] = hi.y; q[j][6] = hi.z; q[j][7] = hi.w;
    }

    uint32_t b1[QPT], b2[QPT];
#pragma unroll
    for (int j = 0; j < QPT; ++j) b1[j] = b2[j] = KNN_NONE;

    // Same train-row pipeline as k_score_rowlane: two 16-dword SGPR buffers (2 rows each) ping-pong, the s_load of the
    // next 2 rows in flight while the VALU works on the current 2.  The last trip reads up to 6 rows past nt: the
    // matrix's padding rows, or the next segment's rows — their keys are KNN_NONE either way.
    if (nt > 0) {
        knn_sptr_t T = (knn_sptr_t)(a.t_rows + (size_t)pi.t_row * 8);
        auto idx = [&](uint32_t r) { return r < nt ? r : KNN_NONE; };     // wave-uniform: s_cmp + s_cselect
        uint32_t A[16], B[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) A[k] = T[k];
        __builtin_amdgcn_s_waitcnt(0xC07F);
        for (uint32_t t = 0; t < nt; t += 4) {
#pragma unroll
            for (int k = 0; k < 16; ++k) B[k] = T[(t + 2) * 8 + k];
            __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ABOVE the VALU block it overlaps
            {
                const uint32_t i0 = idx(t), i1 = idx(t + 1);
#pragma unroll
                for (int j = 0; j < QPT; ++j) fold2_knn(b1[j], b2[j], q[j], A, i0, i1);
            }
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): B landed while A was being consumed
#pragma unroll
            for (int k = 0; k < 16; ++k) A[k] = T[(t + 4) * 8 + k];
            __builtin_amdgcn_sched_barrier(0);
            {
                const uint32_t i2 = idx(t + 2), i3 = idx(t + 3);
#pragma unroll
                for (int j = 0; j < QPT; ++j) fold2_knn(b1[j], b2[j], q[j], B, i2, i3);
            }
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0xC07F);  // A (rows t+4, t+5) landed while B was being consumed
        }
    }

    uint2* out = reinterpret_cast<uint2*>(a.keys) + (size_t)pi.out_offset * a.keys_stride;
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const int row = j * THREADS + tid;
        if (row < nq) out[row] = make_uint2(b1[j], b2[j]);
    }
}

template <int THREADS, int QPT>
static hipError_t launch_knn2(const Knn2Args& a, uint32_t n_items, hipStream_t st) {
    if (n_items == 0) return hipSuccess;
    hipLaunchKernelGGL((k_knn2_rowlane<THREADS, QPT>), dim3(n_items), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_knn2_pairs_small(const Knn2Args& a, uint32_t n_items, hipStream_t st) {
    return launch_knn2<256, 2>(a, n_items, st);
}

hipError_t launch_knn2_pairs(const Knn2Args& a, uint32_t n_items, int max_query_rows, hipStream_t st) {
    if (max_query_rows <= 512) return launch_knn2<64, 8>(a, n_items, st);
    if (max_query_rows <= 1024) return launch_knn2<128, 8>(a, n_items, st);
    if (max_query_rows <= 1536) return launch_knn2<192, 8>(a, n_items, st);
    if (max_query_rows <= 2048) return launch_knn2<256, 8>(a, n_items, st);
    return hipErrorInvalidValue;
}

// (b1, b2) <- the two smallest of {b1, b2, k}
__device__ __forceinline__ void top2_insert(uint32_t& b1, uint32_t& b2, uint32_t k) {
    b2 = min(b2, max(b1, k));
    b1 = min(b1, k);
}

// The twin of k_fold_pair_keys: 32 query rows per workgroup, 8 threads per row; thread (row, part) merges the top-2 lists
// of segments part, part + 8, ... (the segment base g * seg_rows is added to a key only when it is not KNN_NONE), the 8
// partial lists meet in LDS.  Keys of different segments never compare equal, so the merge is exact.
__global__ __launch_bounds__(256) void k_fold_pair_keys2(FoldArgs a) {
    __shared__ uint2 part_top[8][32];
    const PairDesc p = a.pairs[a.pair_base + blockIdx.y];
    const uint32_t rr = threadIdx.x & 31u, part = threadIdx.x >> 5;
    const uint32_t r = blockIdx.x * 32u + rr;
    const uint32_t CR = a.chunk_rows ? a.chunk_rows : (uint32_t)MAX_FUSED_QUERY_ROWS;
    uint32_t b1 = KNN_NONE, b2 = KNN_NONE;
    if (r < p.nq) {
        const uint32_t c = r / CR, lr = r % CR;
        const uint2* src = reinterpret_cast<const uint2*>(a.seg_keys) + ((size_t)p.first_item + (size_t)c * p.n_seg) * CR + lr;
        for (uint32_t g = part; g < p.n_seg; g += 8) {
            const uint2 k = src[(size_t)g * CR];
            const uint32_t base = g * p.seg_rows;
            top2_insert(b1, b2, k.x == KNN_NONE ? KNN_NONE : k.x + base);
            top2_insert(b1, b2, k.y == KNN_NONE ? KNN_NONE : k.y + base);
        }
    }
    part_top[part][rr] = make_uint2(b1, b2);
    __syncthreads();
    if (part == 0 && r < p.nq) {
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            const uint2 o = part_top[k][rr];
            top2_insert(b1, b2, o.x);
            top2_insert(b1, b2, o.y);
        }
        reinterpret_cast<uint2*>(a.final_keys)[p.out_row0 + r] = make_uint2(b1, b2);
    }
}

hipError_t launch_fold_pair_keys2(const FoldArgs& a, uint32_t max_nq, hipStream_t st) {
    if (a.n_pairs == 0 || max_nq == 0) return hipSuccess;
    return launch_y_sliced(k_fold_pair_keys2, a, &FoldArgs::pair_base, a.n_pairs, (max_nq + 31) / 32, 256, st);
}

}  // namespace lcm
