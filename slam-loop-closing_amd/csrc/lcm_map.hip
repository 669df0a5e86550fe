// lcm_map.hip — the reference's map building before the loop (src/main.cpp:1152-1351) on the device: the median displacement of the
// keyframe gate (:171-189), cv::triangulatePoints with the depth, parallax and reprojection filters (:1250-1313) and the merge of a
// keyframe's points into the map (:1315-1340), with every step's arithmetic defined in lcm_map_device.h (the shared part in
// lcm_geom_device.h).  The loop over the matches looks sequential but is a filter per record, an ordered compaction and a
// last-writer scatter: a knnMatch list holds every query_idx once.  No floating-point atomic anywhere: the integer atomics below
// count or take a maximum, which no order changes, so the same call gives the same bytes.
//
// k_map_median       one workgroup of 256 threads per pair: the exact element n / 2 of the pair's sorted displacements by a radix
//                    select over the doubles' 64-bit patterns (non-negative doubles order as their patterns do): eight passes of
//                    8 bits from the top, each a 256-bin histogram in LDS by integer atomics over the records whose higher bits
//                    equal the prefix found so far, the bin holding the wanted rank found by thread 0.  The displacements are
//                    recomputed from the records in every pass (16 bytes read, a square root) and never stored or sorted.
// k_map_triangulate  one lane per record, 256 records per workgroup, the pair from blockIdx.y: the pair's 56 doubles come through
//                    uniform loads, the 4 x 4 system and the rotations' product live in registers (every index a compile-time
//                    constant, the six pairs unrolled, a loop over the sweeps), one 64-byte record and one status byte out; the
//                    per-pair counts per status by one integer atomic per wave and status.
// k_map_merge_count  one lane per record, 256 per workgroup: the accepted records and, among them, those whose query keypoint has
//                    no point yet, counted per block by wave ballots; an integer maximum of the record index per train keypoint
//                    says which accepted record writes that keypoint's table entry (the last in list order).  k_block_scan
//                    (lcm_kernels.hip) then turns both block counts into exclusive prefixes and totals.
// k_map_merge_emit   the verdict again; a record's rank among the accepted and among the new records of its block from the
//                    wave's ballot (popcount of the lower lanes) plus the waves before it, so point n_points + rank and the
//                    observations at (accepted before) + (new before) are in list order by construction, whatever the order the
//                    workgroups run in.  A new record writes its point (the 24 bytes of tri's X moved as they are), two
//                    observations and table1[query_idx]; a merged one one observation; the winner of a train keypoint table2.
//
// Budget (tests/test_kernel_metadata_map.py): no scratch, no spills.  k_map_triangulate at most 128 VGPRs and no LDS; k_map_median
// at most 64 VGPRs and 1040 bytes of LDS; k_map_merge_count and k_map_merge_emit at most 64 VGPRs and 32 bytes of LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcm_map_device.h"

namespace lcm {

__global__ __launch_bounds__(256) void k_map_median(MapMedianArgs a) {
#pragma clang fp contract(off)
    __shared__ uint32_t hist[256];
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_need;
    const uint32_t p = blockIdx.x, tid = threadIdx.x;
    const uint64_t first = a.off[p];
    const uint32_t n = (uint32_t)(a.off[p + 1] - first);
    if (n == 0) {                                            // whole workgroup
        if (tid == 0) a.median[p] = 0.0;
        return;
    }
    uint64_t prefix = 0;
    uint32_t need = n / 2;                                   // among the values that share `prefix` above the digit: rank `need`, ascending
    for (int shift = 56; shift >= 0; shift -= 8) {
        const uint64_t above = shift == 56 ? 0ull : ~0ull << (shift + 8);
        hist[tid] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += 256) {
            const uint4 r = a.pts[first + i];
            const uint64_t key = (uint64_t)__double_as_longlong(
                map_displacement(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w)));
            if ((key & above) == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t acc = 0, digit = 255, left = 0;
            for (uint32_t b = 0; b < 256; ++b) {
                if (acc + hist[b] > need) { digit = b; left = need - acc; break; }
                acc += hist[b];
            }
            s_prefix = prefix | (uint64_t)digit << shift; s_need = left;
        }
        __syncthreads();
        prefix = s_prefix; need = s_need;
    }
    if (tid == 0) a.median[p] = __longlong_as_double((long long)prefix);
}

__global__ __launch_bounds__(256) void k_map_triangulate(MapTriArgs a) {
#pragma clang fp contract(off)
    const uint32_t p = blockIdx.y;
    const uint64_t first = a.off[p];
    const uint32_t n = (uint32_t)(a.off[p + 1] - first);
    if (blockIdx.x * 256u >= n) return;                      // whole workgroup: the grid's x is the longest pair's
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    int status = -1;                                         // beyond the pair's records
    if (i < n) {
        MapTri t = MapTri{{0.0, 0.0, 0.0}, 0.0, 0.0, 0.0, 0.0, 0.0};
        status = MAP_NOT_INLIER;
        if (!a.mask || a.mask[first + i]) {
            const uint4 r = a.pts[first + i];
            status = map_record(a.pairs[p], a.K, a.lim, __uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z),
                                __uint_as_float(r.w), t);
        }
        a.tri[first + i] = t;
        a.status[first + i] = (uint8_t)status;
    }
#pragma unroll
    for (int s = 0; s <= MAP_ACCEPTED; ++s) {
        const uint64_t m = __ballot(status == s);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.counts[(size_t)p * MAP_STATUSES + s], (uint32_t)__popcll(m));
    }
}

// record i of the list: is it accepted, and if so, does its query keypoint lack a point?
__device__ __forceinline__ bool map_merge_verdict(const MapMergeArgs& a, uint32_t i, uint4& mt, bool& is_new) {
    is_new = false;
    if (i >= a.n || a.status[i] != MAP_ACCEPTED) return false;
    mt = a.matches[i];
    is_new = a.table1[mt.x] == -1;
    return true;
}

__global__ __launch_bounds__(256) void k_map_merge_count(MapMergeArgs a) {
    __shared__ uint32_t wave_acc[4], wave_new[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint4 mt;
    bool is_new;
    const bool acc = map_merge_verdict(a, i, mt, is_new);
    if (acc) atomicMax(&a.winner[mt.y], (int32_t)i);
    const uint64_t ma = __ballot(acc), mn = __ballot(is_new);
    if ((threadIdx.x & 63) == 0) { wave_acc[threadIdx.x >> 6] = (uint32_t)__popcll(ma); wave_new[threadIdx.x >> 6] = (uint32_t)__popcll(mn); }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.blk_accepted[blockIdx.x] = wave_acc[0] + wave_acc[1] + wave_acc[2] + wave_acc[3];
        a.blk_new[blockIdx.x] = wave_new[0] + wave_new[1] + wave_new[2] + wave_new[3];
    }
}

__global__ __launch_bounds__(256) void k_map_merge_emit(MapMergeArgs a) {
    __shared__ uint32_t wave_acc[4], wave_new[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint4 mt;
    bool is_new;
    const bool acc = map_merge_verdict(a, i, mt, is_new);
    const uint64_t ma = __ballot(acc), mn = __ballot(is_new);
    if (lane == 0) { wave_acc[wave] = (uint32_t)__popcll(ma); wave_new[wave] = (uint32_t)__popcll(mn); }
    __syncthreads();
    if (i >= a.n) return;
    if (!acc) { a.status_out[i] = a.status[i]; return; }
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t r_acc = a.blk_accepted[blockIdx.x] + (uint32_t)__popcll(ma & below), r_new = a.blk_new[blockIdx.x] + (uint32_t)__popcll(mn & below);
    for (uint32_t w = 0; w < wave; ++w) { r_acc += wave_acc[w]; r_new += wave_new[w]; }
    const uint4 px = a.pts[i];
    const double qx = (double)__uint_as_float(px.x), qy = (double)__uint_as_float(px.y);
    const double tx = (double)__uint_as_float(px.z), ty = (double)__uint_as_float(px.w);
    uint32_t at = r_acc + r_new;                             // one observation per accepted record before, one more per new one
    int32_t point;
    if (is_new) {
        point = a.n_points + (int32_t)r_new;
        const MapTri t = a.tri[i];
        a.points_out[r_new] = Point3{t.X[0], t.X[1], t.X[2]};
        a.obs_out[at++] = Observation{a.kf1, point, qx, qy};
        a.table1[mt.x] = point;
    } else {
        point = a.table1[mt.x];
    }
    a.obs_out[at] = Observation{a.kf2, point, tx, ty};
    if (a.winner[mt.y] == (int32_t)i) a.table2[mt.y] = point;
    a.status_out[i] = (uint8_t)(is_new ? MAP_NEW : MAP_MERGED);
}

hipError_t launch_map_median(const MapMedianArgs& a, uint32_t n_pairs, hipStream_t st) {
    if (n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_map_median, dim3(n_pairs), dim3(MAP_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_map_triangulate(const MapTriArgs& a, uint32_t n_pairs, uint32_t max_n, hipStream_t st) {
    if (n_pairs == 0 || max_n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_map_triangulate, dim3((max_n + MAP_THREADS - 1) / MAP_THREADS, n_pairs), dim3(MAP_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_map_merge_count(const MapMergeArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_map_merge_count, dim3((a.n + MAP_THREADS - 1) / MAP_THREADS), dim3(MAP_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_map_merge_emit(const MapMergeArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_map_merge_emit, dim3((a.n + MAP_THREADS - 1) / MAP_THREADS), dim3(MAP_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace lcm
