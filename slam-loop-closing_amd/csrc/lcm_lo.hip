// lcm_lo.hip — the local optimisation of the essential-matrix RANSAC (include/lcm.h, lcm_lo_*): the 64 best
// hypotheses of every pair are refitted on their own inliers, in rounds under a shrinking threshold, and a refit replaces the
// RANSAC's record only when it holds strictly more inliers.  Every step is defined in lcm_lo_device.h; the inlier rule, the
// camera normalisation, the constraint row and the projection are lcm_epi_device.h's.  The kernels run after k_epi_mask on
// the same records, hypotheses and counts.  The pair comes from blockIdx.y, in slices (launch_y_sliced) as k_epi_mask's.
//
// k_lo_select   one workgroup of 256 threads per pair: the exact 64 largest of the pair's `iters` keys (count << 16 |
//               0xFFFF - hypothesis; unique).  Four passes of an 8-bit radix select over the keys (a 256-bin histogram in LDS
//               by integer atomics, the bin holding the 64th largest found by thread 0) give the 64th largest key itself; the
//               64 keys at or above it are collected and each is placed at its rank: seeds[lane] = the lane-th largest.
// k_lo_refine   one wave per pair, lane = seed.  A pass walks the pair's records in tiles of 2016: the wave normalises a tile
//               into LDS once and every lane reads it back at the same address (a broadcast, k_epi_score's pattern).  A round
//               is four passes: the selected set's count and coordinate sums; its squared distances to the means; the 45
//               moments of the Hartley-normalised constraint rows, in registers; and, after the eigen step, the refit's inlier
//               count under the model's own threshold, which also is the next round's first pass (the same matrix, the next
//               multiplier): 3 rounds + 1 passes in all.  Between the third and the fourth the tile's LDS becomes 64
//               lane-private columns (stride 64 doubles): 45 moments + the 9 x 9 product of the Jacobi rotations, so the
//               runtime indices address LDS, not registers.  All sums run in record order within a lane: no atomics, the
//               same bytes every time.  Epilogue: the winning lane by a wave maximum of (count << 6 | 63 - lane); where its
//               round is >= 0, lane 0 rewrites the pair's result record and the wave its mask bytes; lane 0 writes the info
//               record.  A pair with fewer than 8 records or without spread on a side writes its info record alone.
//               The refit seam (LoArgs.refit_E) runs one round per caller-supplied model and writes E', |S| and the status.
//
// Budget (tests/test_kernel_metadata_lo.py): no scratch, no spills; k_lo_select at most 64 VGPRs and 1 292 bytes of LDS
// (the compiler gives 58), k_lo_refine at most 256 VGPRs and 64 512 bytes of LDS (the compiler gives 236: two waves per
// SIMD; 126 doubles x 64 lanes: two workgroups per CU, so the LDS and not the register file bounds the occupancy).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lcm_kernels.h"
#include "lcm_lo_device.h"

namespace lcm {

constexpr uint32_t LO_TILE = LO_WORK * 64 / 4;          // records per tile: the eigen workspace's bytes, 4 doubles a record

__global__ __launch_bounds__(256) void k_lo_select(LoArgs a) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t list[LO_SEEDS];
    __shared__ uint32_t s_prefix, s_need, s_n;
    const uint32_t p = a.pair_base + blockIdx.y, tid = threadIdx.x;
    const uint32_t* cnt = a.counts + (size_t)p * a.iters;
    uint32_t prefix = 0, need = LO_SEEDS;               // among the keys that share `prefix` above the digit: the need-th largest
    for (int shift = 24; shift >= 0; shift -= 8) {
        const uint32_t above = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        hist[tid] = 0;
        __syncthreads();
        for (uint32_t it = tid; it < a.iters; it += 256) {
            const uint32_t key = cnt[it] << 16 | (0xFFFFu - it);
            if ((key & above) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t acc = 0, digit = 0, left = need;
            for (int b = 255; b >= 0; --b) {
                if (acc + hist[b] >= need) { digit = (uint32_t)b; left = need - acc; break; }
                acc += hist[b];
            }
            s_prefix = prefix | digit << shift; s_need = left; s_n = 0;
        }
        __syncthreads();
        prefix = s_prefix; need = s_need;
    }
    for (uint32_t it = tid; it < a.iters; it += 256) {  // prefix = the 64th largest key: exactly 64 keys are at or above it
        const uint32_t key = cnt[it] << 16 | (0xFFFFu - it);
        if (key >= prefix) {
            const uint32_t pos = atomicAdd(&s_n, 1u);
            if (pos < (uint32_t)LO_SEEDS) list[pos] = key;
        }
    }
    __syncthreads();
    if (tid < (uint32_t)LO_SEEDS) {
        const uint32_t key = list[tid];
        uint32_t rank = 0;
        for (int j = 0; j < LO_SEEDS; ++j) rank += list[j] > key ? 1u : 0u;
        a.seeds[(size_t)p * LO_SEEDS + rank] = (int32_t)(0xFFFFu - (key & 0xFFFFu));
    }
}

// One pass over the pair's records: fn(a, b, c, d) per record, in record order, for every lane alike
template <typename F>
__device__ __forceinline__ void lo_pass(const LoArgs& a, uint64_t first, uint32_t n, double* tile, uint32_t lane, F&& fn) {
    for (uint32_t base = 0; base < n; base += LO_TILE) {
        const uint32_t m = min(LO_TILE, n - base);
        __syncthreads();                                // the previous tile, or the eigen columns, have been read
        for (uint32_t i = lane; i < m; i += 64) {
            const uint4 r = a.pts[first + base + i];
            tile[4 * i + 0] = epi_norm(__uint_as_float(r.x), a.cx, a.fx);
            tile[4 * i + 1] = epi_norm(__uint_as_float(r.y), a.cy, a.fy);
            tile[4 * i + 2] = epi_norm(__uint_as_float(r.z), a.cx, a.fx);
            tile[4 * i + 3] = epi_norm(__uint_as_float(r.w), a.cy, a.fy);
        }
        __syncthreads();
#pragma unroll 2
        for (uint32_t i = 0; i < m; ++i) fn(tile[4 * i], tile[4 * i + 1], tile[4 * i + 2], tile[4 * i + 3]);
    }
}

__device__ __forceinline__ double lo_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

// Do ALL the pair's records have a spread on both sides?  (If not, no subset has: no seed could be refitted.)
__device__ __forceinline__ bool lo_pair_spread(const LoArgs& a, uint64_t first, uint32_t n, uint32_t lane) {
    double sa = 0.0, sb = 0.0, sc = 0.0, sd = 0.0;
    for (uint32_t i = lane; i < n; i += 64) {
        const uint4 r = a.pts[first + i];
        sa = sa + epi_norm(__uint_as_float(r.x), a.cx, a.fx); sb = sb + epi_norm(__uint_as_float(r.y), a.cy, a.fy);
        sc = sc + epi_norm(__uint_as_float(r.z), a.cx, a.fx); sd = sd + epi_norm(__uint_as_float(r.w), a.cy, a.fy);
    }
    const double nn = (double)n;
    const double m1x = lo_wave_sum(sa) / nn, m1y = lo_wave_sum(sb) / nn, m2x = lo_wave_sum(sc) / nn, m2y = lo_wave_sum(sd) / nn;
    double v1 = 0.0, v2 = 0.0;
    for (uint32_t i = lane; i < n; i += 64) {
        const uint4 r = a.pts[first + i];
        v1 = v1 + lo_sqdist(epi_norm(__uint_as_float(r.x), a.cx, a.fx), epi_norm(__uint_as_float(r.y), a.cy, a.fy), m1x, m1y);
        v2 = v2 + lo_sqdist(epi_norm(__uint_as_float(r.z), a.cx, a.fx), epi_norm(__uint_as_float(r.w), a.cy, a.fy), m2x, m2y);
    }
    double s1, s2;
    const bool ok1 = lo_hartley_scale(lo_wave_sum(v1), nn, &s1), ok2 = lo_hartley_scale(lo_wave_sum(v2), nn, &s2);
    return ok1 && ok2;
}

__global__ __launch_bounds__(64) void k_lo_refine(LoArgs a) {
    __shared__ double ws[LO_WORK * 64];
    const uint32_t p = a.pair_base + blockIdx.y, lane = threadIdx.x;
    const uint64_t first = a.offsets[p];
    const uint32_t n = (uint32_t)(a.offsets[p + 1] - first);
    const bool seam = a.refit_E != nullptr;
    EpiResult* res = reinterpret_cast<EpiResult*>(a.results) + p;
    LoInfo* info = reinterpret_cast<LoInfo*>(a.info) + p;
    int32_t ransac_inliers = 0;
    if (!seam) {                                        // the whole wave
        ransac_inliers = res->n_inliers;
        int32_t status = n < (uint32_t)EPI_SAMPLE ? LO_TOO_FEW : LO_OK;
        if (status == LO_OK && !lo_pair_spread(a, first, n, lane)) status = LO_DEGENERATE;
        if (status != LO_OK) {
            if (lane == 0) *info = LoInfo{res->best_iter, -1, ransac_inliers, status};
            return;
        }
    }
    uint32_t seed = lane, best_cnt = 0, n_sel = 0;
    bool alive = true;
    double cur[9], best_e[9];
    if (seam) {
        alive = lane < a.n_models;
#pragma unroll
        for (int k = 0; k < 9; ++k) cur[k] = alive ? a.E[(size_t)lane * 9 + k] : 0.0;
    } else {
        seed = min((uint32_t)a.seeds[(size_t)p * LO_SEEDS + lane], a.iters - 1u);      // k_lo_select left a hypothesis < iters
        const size_t hyp = (size_t)p * a.iters + seed;
#pragma unroll
        for (int k = 0; k < 9; ++k) cur[k] = a.E[hyp * 9 + k];
        best_cnt = a.counts[hyp];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) best_e[k] = cur[k];
    int32_t best_round = -1, status = LO_OK;
    const double t2 = lo_threshold2(a.t, 1.0);
    const uint32_t rounds = seam ? 1u : a.rounds;
    // the selected set's count and coordinate sums: round 0's here, a later round's with the round before's last pass
    uint32_t cnt = 0;
    double sa = 0.0, sb = 0.0, sc = 0.0, sd = 0.0;
    {
        const double t2m = lo_threshold2(a.t, a.mult[0]);
        lo_pass(a, first, n, ws, lane, [&](double qa, double qb, double qc, double qd) {
            if (alive && epi_inlier(cur, qa, qb, qc, qd, t2m)) { ++cnt; sa = sa + qa; sb = sb + qb; sc = sc + qc; sd = sd + qd; }
        });
        n_sel = cnt;
    }
    for (uint32_t r = 0; r < rounds; ++r) {
        if (!__any(alive)) break;                       // wave-uniform
        const double t2m = lo_threshold2(a.t, a.mult[r]);
        if (alive && cnt < (uint32_t)EPI_SAMPLE) { alive = false; status = LO_TOO_FEW; }
        const double nn = (double)cnt;
        const double m1x = sa / nn, m1y = sb / nn, m2x = sc / nn, m2y = sd / nn;
        double v1 = 0.0, v2 = 0.0;
        lo_pass(a, first, n, ws, lane, [&](double qa, double qb, double qc, double qd) {
            if (alive && epi_inlier(cur, qa, qb, qc, qd, t2m)) { v1 = v1 + lo_sqdist(qa, qb, m1x, m1y); v2 = v2 + lo_sqdist(qc, qd, m2x, m2y); }
        });
        double s1, s2;
        const bool ok1 = lo_hartley_scale(v1, nn, &s1), ok2 = lo_hartley_scale(v2, nn, &s2);
        if (alive && !(ok1 && ok2)) { alive = false; status = LO_DEGENERATE; }
        double m[LO_MOMENTS];
#pragma unroll
        for (int k = 0; k < LO_MOMENTS; ++k) m[k] = 0.0;
        lo_pass(a, first, n, ws, lane, [&](double qa, double qb, double qc, double qd) {
            if (alive && epi_inlier(cur, qa, qb, qc, qd, t2m))
                lo_add_moments(m, lo_centre(qa, m1x, s1), lo_centre(qb, m1y, s1), lo_centre(qc, m2x, s2), lo_centre(qd, m2y, s2));
        });
        __syncthreads();                                // the last tile has been read: its LDS becomes the lanes' columns
        if (alive) {
            double* W = ws + lane;
#pragma unroll
            for (int k = 0; k < LO_MOMENTS; ++k) W[k * 64] = m[k];
            double f[9];
            lo_eig9<64>(W, f);
            lo_denormalise(f, m1x, m1y, s1, m2x, m2y, s2);
            if (epi_project(f)) {
#pragma unroll
                for (int k = 0; k < 9; ++k) cur[k] = f[k];
            } else {
                alive = false; status = LO_NO_MODEL;
            }
        }
        if (seam) break;
        // the refit's count under the model's own threshold and, on the same records, the next round's selected set
        const double t2n = lo_threshold2(a.t, a.mult[min(r + 1u, rounds - 1u)]);
        uint32_t c2 = 0;
        cnt = 0; sa = 0.0; sb = 0.0; sc = 0.0; sd = 0.0;
        lo_pass(a, first, n, ws, lane, [&](double qa, double qb, double qc, double qd) {
            if (alive && epi_inlier(cur, qa, qb, qc, qd, t2)) ++c2;
            if (alive && epi_inlier(cur, qa, qb, qc, qd, t2n)) { ++cnt; sa = sa + qa; sb = sb + qb; sc = sc + qc; sd = sd + qd; }
        });
        if (alive && lo_accepts(c2, best_cnt)) {
            best_cnt = c2; best_round = (int32_t)r;
#pragma unroll
            for (int k = 0; k < 9; ++k) best_e[k] = cur[k];
        }
    }
    if (seam) {
        if (lane < a.n_models) {
#pragma unroll
            for (int k = 0; k < 9; ++k) a.refit_E[(size_t)lane * 9 + k] = status == LO_OK ? cur[k] : 0.0;
            a.refit_n[lane] = (int32_t)n_sel; a.refit_status[lane] = status;
        }
        return;
    }
    uint32_t key = lo_lane_key(best_cnt, lane);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, o, 64));
    const int win = (int)(63u - (key & 63u));
    const int32_t win_round = __shfl(best_round, win, 64), win_seed = __shfl((int)seed, win, 64);
    if (lane == 0) *info = LoInfo{win_seed, win_round, ransac_inliers, LO_OK};
    if (win_round < 0) return;                          // the whole wave: the RANSAC's record and mask stay as they are
    double we[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) we[k] = __shfl(best_e[k], win, 64);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) res->E[k] = we[k];
        res->n_inliers = (int32_t)(key >> 6); res->best_iter = win_seed;
    }
    for (uint32_t i = lane; i < n; i += 64) {
        const uint4 r = a.pts[first + i];
        const bool in = epi_inlier(we, epi_norm(__uint_as_float(r.x), a.cx, a.fx), epi_norm(__uint_as_float(r.y), a.cy, a.fy),
                                   epi_norm(__uint_as_float(r.z), a.cx, a.fx), epi_norm(__uint_as_float(r.w), a.cy, a.fy), t2);
        a.mask[first + i] = in ? 1 : 0;
    }
}

hipError_t launch_lo_select(const LoArgs& a, uint32_t n_pairs, hipStream_t st) {
    return launch_y_sliced(k_lo_select, a, &LoArgs::pair_base, n_pairs, 1, 256, st);
}

hipError_t launch_lo_refine(const LoArgs& a, uint32_t n_pairs, hipStream_t st) {
    return launch_y_sliced(k_lo_refine, a, &LoArgs::pair_base, n_pairs, 1, 64, st);
}

}  // namespace lcm
