// lcm_ratio.hip — the bulk / online loop search scored with Lowe's ratio test: per (query frame, stored frame) pair the
// NUMBER of query rows whose best neighbour passes best.distance < ratio * second.distance — the size of the list that
// matchFeatures(desc[curr], desc[past], matches, 0.7) returns and that the reference's loop search compares with its
// threshold (src/main.cpp:1375-1388) — as the usual 8-byte lcm_score record.
//
// k_ratio_rowlane is k_score_rowlane's plain bulk route (lcm_kernels.hip) with a second running minimum per query row:
// one workgroup = one WorkItem (one query frame against a run of stored slots), lanes own 8 query rows in VGPRs, stored
// rows arrive wave-uniform through two ping-pong SGPR buffers, xors at priority 0 and everything else inside
// s_setprio 3 ... s_setprio 0.  Each query row keeps two plain DISTANCES b1 <= b2 (no keys: the count needs no train
// index, and equal distances count with multiplicity as knnMatch's two entries do); two new distances d0, d1 update
// them exactly in three quarter-rate instructions:
//     m  = med3(b1, d0, d1);  b2 = min(b2, m);  b1 = min3(b1, d0, d1)
// 8 x 2 popcounts + 3 = 19 quarter-rate instructions per two distances (the distance-only fold2_min: 17).
//
// Padding rows: a stored frame is padded to a multiple of 4 rows with COPIES of its last row and the last loop trip
// reads them (and 2 rows further: the next slot, or the arena's slack).  A copy of the best row would be a fake second
// neighbour at d2 = d1.  Rows >= nt therefore start their popcount chain from RATIO_PAD_BIAS instead of 0: the chain's
// first v_bcnt_u32_b32 adds to an SGPR that the scalar unit selects per row (s_cmp + s_cselect on the wave-uniform row
// index), so the vector pipe pays nothing.  A biased distance (>= 4096) can never displace a real one (<= 256); the
// epilogue reads b2 > 256 as "no second neighbour".
//
// Ratio test: the host tabulates lim[d2] = number of integers d1 in 0..256 with (double)d1 < ratio * (double)d2; the set
// is downward closed in d1, so d1 < lim[d2] IS the reference's IEEE-double comparison.  The table travels as a kernel
// argument and is copied to LDS once per workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcm_kernels.h"

namespace lcm {

typedef const uint32_t __attribute__((address_space(4))) * ratio_sptr_t;   // constant AS => SMEM (s_load) when uniform
typedef const int32_t __attribute__((address_space(4))) * ratio_siptr_t;

constexpr uint32_t RATIO_PAD_BIAS = 4096;      // start of a padding row's popcount chain: above every real distance
constexpr uint32_t RATIO_NONE = 0xFFFFFFFFu;   // initial b1 / b2: "no neighbour yet"

// One (xor, xor | popcount, popcount) phase of the two chains: word SA of stored row 0, word SB of stored row 1, word QV
// of the query row; ACC0 / ACC1 = what the popcounts add to (the bias SGPRs in the first phase).
#define LCM_RATIO_PHASE(SA, SB, QV, ACC0, ACC1)                                                                \
    "v_xor_b32_e32 %4, %" #SA ", %" #QV "\n\tv_xor_b32_e32 %5, %" #SB ", %" #QV "\n\ts_setprio 3\n\t"           \
    "v_bcnt_u32_b32 %2, %4, " ACC0 "\n\tv_bcnt_u32_b32 %3, %5, " ACC1 "\n\t"

// One query row (8 VGPRs) against TWO stored rows (16 SGPRs): both distances (+ bias0 / bias1: 0 for a real row,
// RATIO_PAD_BIAS for a padding row) and the exact top-2 update, as ONE asm statement so that the instruction order is
// exactly the one below.  Operands: %0 b1, %1 b2, %2 %3 the two distances, %4 %5 temporaries, %6..%13 stored row 0,
// %14..%21 stored row 1, %22..%29 the query row, %30 %31 the biases.
__device__ __forceinline__ void fold2_ratio(uint32_t& b1, uint32_t& b2, const uint32_t (&q)[8], const uint32_t* s,
                                            uint32_t bias0, uint32_t bias1) {
    uint32_t d0, d1, x0, x1;
    asm volatile(
        LCM_RATIO_PHASE(6, 14, 22, "%30", "%31") "s_setprio 0\n\t"
        LCM_RATIO_PHASE(7, 15, 23, "%2", "%3") "s_setprio 0\n\t"
        LCM_RATIO_PHASE(8, 16, 24, "%2", "%3") "s_setprio 0\n\t"
        LCM_RATIO_PHASE(9, 17, 25, "%2", "%3") "s_setprio 0\n\t"
        LCM_RATIO_PHASE(10, 18, 26, "%2", "%3") "s_setprio 0\n\t"
        LCM_RATIO_PHASE(11, 19, 27, "%2", "%3") "s_setprio 0\n\t"
        LCM_RATIO_PHASE(12, 20, 28, "%2", "%3") "s_setprio 0\n\t"
        LCM_RATIO_PHASE(13, 21, 29, "%2", "%3")
        "v_med3_u32 %4, %0, %2, %3\n\t"
        "v_min_u32_e32 %1, %4, %1\n\t"
        "v_min3_u32 %0, %0, %2, %3\n\ts_setprio 0"
        : "+v"(b1), "+v"(b2), "=&v"(d0), "=&v"(d1), "=&v"(x0), "=&v"(x1)
        : "s"(s[0]), "s"(s[1]), "s"(s[2]), "s"(s[3]), "s"(s[4]), "s"(s[5]), "s"(s[6]), "s"(s[7]),
          "s"(s[8]), "s"(s[9]), "s"(s[10]), "s"(s[11]), "s"(s[12]), "s"(s[13]), "s"(s[14]), "s"(s[15]),
          "v"(q[0]), "v"(q[1]), "v"(q[2]), "v"(q[3]), "v"(q[4]), "v"(q[5]), "v"(q[6]), "v"(q[7]),
          "s"(bias0), "s"(bias1));
}
#undef LCM_RATIO_PHASE

// 5 waves per SIMD (96 VGPRs), the budget of k_knn2_rowlane: 64 registers hold the query rows and 16 the running
// distances of the 8-rows-per-lane shape.
template <int THREADS, int QPT>
__global__ __launch_bounds__(THREADS, 5) void k_ratio_rowlane(RatioArgs a) {
    __shared__ uint32_t red_min[2];
    __shared__ uint32_t red_sum[2];
    __shared__ uint16_t lim_s[RATIO_LIM_ENTRIES];

    const int tid = threadIdx.x;
    if (tid == 0) { red_min[0] = red_min[1] = 0xFFFFFFFFu; red_sum[0] = red_sum[1] = 0u; }
    for (int i = tid; i < RATIO_LIM_ENTRIES; i += THREADS) lim_s[i] = a.lim[i];
    __syncthreads();

    WorkItem it;
    int nq;
    if (a.items) {
        it = a.items[blockIdx.x];
        nq = a.q_counts[it.q_frame];
    } else {                                   // implicit item (online query): run blockIdx.x of imp_spi stored slots
        it.q_frame = 0;
        it.slot_begin = blockIdx.x * a.imp_spi;
        it.n_slots = min(a.imp_spi, a.imp_total - it.slot_begin);
        it.out_offset = it.slot_begin;
        nq = a.imp_nq;
    }

    // ---- this lane's query rows: row = j * THREADS + tid (consecutive lanes -> consecutive 32-byte rows)
    uint32_t q[QPT][8];
    auto valid = [&](int j) { return j * THREADS + tid < nq; };     // recomputed where needed: no register held for it
    const uint4* qbase = reinterpret_cast<const uint4*>(a.q_rows + (size_t)it.q_frame * a.q_stride_words);
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const int row = j * THREADS + tid;
        uint4 lo = make_uint4(0, 0, 0, 0), hi = make_uint4(0, 0, 0, 0);
        if (row < nq) { lo = qbase[row * 2]; hi = qbase[row * 2 + 1]; }
        q[j][0] = lo.x; q[j][1] = lo.y; q[j][2] = lo.z; q[j][3] = lo.w;
        q[j][4] = hi.x; q[j][5] = hi.y; q[j][6] = hi.z; q[j][7] = hi.w;
    }

    for (uint32_t s = 0; s < it.n_slots; ++s) {
        const uint32_t slot = it.slot_begin + s;
        const uint32_t nt = (uint32_t)((ratio_siptr_t)a.db_counts)[slot];
        ratio_sptr_t T = (ratio_sptr_t)(a.db_rows + (size_t)slot * a.db_stride_words);

        uint32_t b1[QPT], b2[QPT];             // reset per stored slot
#pragma unroll
        for (int j = 0; j < QPT; ++j) b1[j] = b2[j] = RATIO_NONE;

        // k_score_rowlane's stored-row pipeline: two 16-dword SGPR buffers (2 rows each) ping-pong, the s_load of the next
        // 2 rows in flight while the VALU works on the current 2 (SMEM returns out of order: the only legal wait is
        // lgkmcnt(0)).  The last trip reads up to 6 rows past nt; their chains start from RATIO_PAD_BIAS.
        if (nt > 0) {
            auto bias = [&](uint32_t r) { return r < nt ? 0u : RATIO_PAD_BIAS; };     // wave-uniform: s_cmp + s_cselect
            uint32_t A[16], B[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) A[k] = T[k];
            __builtin_amdgcn_s_waitcnt(0xC07F);
            for (uint32_t t = 0; t < nt; t += 4) {
#pragma unroll
                for (int k = 0; k < 16; ++k) B[k] = T[(t + 2) * 8 + k];
                __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ABOVE the VALU block it overlaps
                {
                    const uint32_t c0 = bias(t), c1 = bias(t + 1);
#pragma unroll
                    for (int j = 0; j < QPT; ++j) fold2_ratio(b1[j], b2[j], q[j], A, c0, c1);
                }
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): B landed while A was being consumed
#pragma unroll
                for (int k = 0; k < 16; ++k) A[k] = T[(t + 4) * 8 + k];
                __builtin_amdgcn_sched_barrier(0);
                {
                    const uint32_t c2 = bias(t + 2), c3 = bias(t + 3);
#pragma unroll
                    for (int j = 0; j < QPT; ++j) fold2_ratio(b1[j], b2[j], q[j], B, c2, c3);
                }
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_waitcnt(0xC07F);  // A (rows t+4, t+5) landed while B was being consumed
            }
        }

        // ---- pair epilogue: min of the best distances, count of the ratio-test survivors, one score record.  Per-lane
        // partials folded with LDS atomics on one word per pair parity, as k_score_rowlane does; the count does not
        // depend on the pair's minimum here, so one barrier per pair is enough: thread 0 re-arms the OTHER parity's words
        // before the barrier (their last readers and writers finished before the previous pair's barrier, and the next
        // pair's atomics come after this one).
        const int par = s & 1;
        if (tid == 0) { red_min[par ^ 1] = 0xFFFFFFFFu; red_sum[par ^ 1] = 0u; }
        uint32_t dmin = 0xFFFFFFFFu, cnt = 0;
#pragma unroll
        for (int j = 0; j < QPT; ++j) {
            if (!valid(j)) continue;
            dmin = min(dmin, b1[j]);
            // b2 > 256: no second neighbour (one stored row, or none): the row does not count
            const uint32_t l = lim_s[min(b2[j], (uint32_t)(RATIO_LIM_ENTRIES - 1))];
            cnt += (b2[j] <= 256u && b1[j] < l) ? 1u : 0u;
        }
        atomicMin(&red_min[par], dmin);
        atomicAdd(&red_sum[par], cnt);
        __syncthreads();
        if (tid == 0) {
            const bool empty = (nq <= 0) || (nt == 0);
            uint2 rec;
            rec.x = empty ? 0u : red_sum[par];
            rec.y = (empty ? 0xFFFFu : (red_min[par] & 0xFFFFu)) | ((nt & 0xFFFFu) << 16);
            reinterpret_cast<uint2*>(a.scores)[(size_t)it.out_offset + s] = rec;
        }
    }
}

template <int THREADS>
static hipError_t launch_ratio_shape(const RatioArgs& a, uint32_t n_items, hipStream_t st) {
    hipLaunchKernelGGL((k_ratio_rowlane<THREADS, 8>), dim3(n_items), dim3(THREADS), 0, st, a);
    return hipGetLastError();
}

// workgroup shape by the largest query frame, as launch_score picks it
hipError_t launch_score_ratio(const RatioArgs& a, uint32_t n_items, int max_query_rows, hipStream_t st) {
    if (n_items == 0) return hipSuccess;
    if (max_query_rows <= 512) return launch_ratio_shape<64>(a, n_items, st);
    if (max_query_rows <= 1024) return launch_ratio_shape<128>(a, n_items, st);
    if (max_query_rows <= 1536) return launch_ratio_shape<192>(a, n_items, st);
    if (max_query_rows <= 2048) return launch_ratio_shape<256>(a, n_items, st);
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------------
// The reference's loop rule (src/main.cpp:1379-1388) over the finished score array, candidates compacted IN PAIR ORDER =
// (current id, matched id) ascending, as k_loop_count / k_block_scan / k_loop_emit do for README.md:123-126
// (lcm_kernels.hip): verdict per pair + candidates per 256-pair block, exclusive prefix of the block counts (the SAME
// k_block_scan), verdict again + rank inside the block by wave ballots + write.  The division is IEEE double (no
// fast-math), so the record equals the host's lcm_ratio_loop_test bit for bit.  HBM-bound: 2 x 8 bytes read per pair (+ one
// cached row count) + 24 bytes written per candidate.
// ---------------------------------------------------------------------------------------------------
struct RatioCandidateRec { int32_t cur, matched, num; int32_t pad; double sim; };
static_assert(sizeof(RatioCandidateRec) == 24, "lcm_loop_candidate layout");

__device__ __forceinline__ bool ratio_loop_verdict(const RatioLoopArgs& a, uint32_t p, RatioCandidateRec& r) {
    if (p >= a.n_pairs) return false;
    // query frame of pair p: last c with offsets[c] <= p
    uint32_t lo = 0, hi = a.n_q;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.offsets[mid] <= p) lo = mid; else hi = mid;
    }
    const uint32_t c = lo, slot = p - a.offsets[c];
    const uint2 rec = reinterpret_cast<const uint2*>(a.scores)[p];
    const uint32_t good = rec.x;
    const int rows_c = a.q_rows[c], rows_s = (int)(rec.y >> 16);
    if (rows_c < a.min_rows || rows_s < a.min_rows || (int64_t)good < (int64_t)a.min_matches) return false;
    const int den = min(rows_c, rows_s);
    r.cur = a.q_ids[c]; r.matched = a.db_ids[slot]; r.num = (int32_t)good; r.pad = 0;
    r.sim = den > 0 ? (double)good / (double)den : 0.0;
    return true;
}

__global__ __launch_bounds__(256) void k_ratio_loop_count(RatioLoopArgs a) {
    RatioCandidateRec r;
    const bool pass = ratio_loop_verdict(a, blockIdx.x * 256u + threadIdx.x, r);
    const int n = __syncthreads_count(pass ? 1 : 0);
    if (threadIdx.x == 0) a.block_counts[blockIdx.x] = (uint32_t)n;
}

__global__ __launch_bounds__(256) void k_ratio_loop_emit(RatioLoopArgs a) {
    __shared__ uint32_t wave_n[4];
    RatioCandidateRec r;
    const bool pass = ratio_loop_verdict(a, blockIdx.x * 256u + threadIdx.x, r);
    const uint64_t m = __ballot(pass);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!pass) return;
    uint32_t k = a.block_counts[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) k += wave_n[w];
    if (k < a.cap) reinterpret_cast<RatioCandidateRec*>(a.out)[k] = r;
}

hipError_t launch_ratio_loop_count(const RatioLoopArgs& a, hipStream_t st) {
    if (a.n_pairs == 0) return hipSuccess;
    const uint32_t n_blocks = (a.n_pairs + 255) / 256;
    hipLaunchKernelGGL(k_ratio_loop_count, dim3(n_blocks), dim3(256), 0, st, a);
    return launch_block_scan(a.block_counts, n_blocks, a.counter, st);
}

hipError_t launch_ratio_loop_emit(const RatioLoopArgs& a, hipStream_t st) {
    if (a.n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ratio_loop_emit, dim3((a.n_pairs + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace lcm
