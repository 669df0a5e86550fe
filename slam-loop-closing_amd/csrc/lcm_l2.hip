// lcm_l2.hip — pair mode on SIFT rows: cv::BFMatcher(NORM_L2).knnMatch(k = 2) over 128-byte descriptors, the matcher call
// the reference executes (src/main.cpp:497-504 cv::SIFT::create(4000), :517 BFMatcher(NORM_L2, false), :520 knnMatch).
//
// EXACTNESS.  OpenCV's SIFT stores saturate_cast<uchar> values, so a row is 128 integers 0..255 and the squared distance
// D = sum (q_i - t_i)^2 is an integer <= 128 * 255^2 = 8 323 200 < 2^24: OpenCV's float accumulation is exact in any order
// and its distance is s = sqrtf(D), one correctly rounded operation.  A query row's neighbours are the two smallest
// (s, train index) pairs (batchDistance, K = 2: ascending train index, admission iff s < dist[K-1], strict shifts).
//
// L2 is shift invariant: every byte is XORed with 0x80 when a matrix arrives (a' = a - 128 as int8), and
//     D = |q'|^2 + |t'|^2 - 2 <q', t'>,   |<q', t'>| <= 2^21, norms <= 2^21: exact in int32.
//
// k_l2_pack      one workgroup per tile of 32 rows: writes the int8 image of the tile in the operand order of
//                v_mfma_i32_32x32x32_i8 (k-step ks of 32 bytes, lane (r = lane & 31, h = lane >> 5) holds bytes
//                [32 ks + 16 h, +16) of row r: 4 k-steps x 64 lanes x 16 bytes = 4 KiB, the size of the raw rows) and one
//                word per row, tw = |t'|^2 << 9 | row's index inside its 512-row train segment.  Rows past a matrix's
//                end are zero in the image.
// k_l2_score     one workgroup (4 waves) = one item: a chunk of 128 * QT query rows against one train segment of <= 512
//                rows (16 tiles).  Wave w keeps query tiles w * QT + j as B operands for the whole item; a train tile is
//                an A operand read straight from global memory (4 KiB that the 4 waves share through the vector cache),
//                the next tile's fragments in flight while the current one is consumed.  4 MFMAs give a 32 x 32 tile of
//                dot products: lane l holds query column l & 31 and train rows (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
//                Epilogue, per distance: one add (tw + |q'|^2 << 9), one v_mad_i32_i24 (- dot << 10) -> the packed key
//                D << 9 | segment-local train index (23 + 9 bits), then lcm_knn.hip's exact top-2 update
//                (med3, min, min3 per TWO keys): 3.5 VALU instructions per distance, 56 per lane and tile beside 4 MFMAs
//                (128 matrix-pipe cycles) per wave and tile: the VALU work, not the MFMA, bounds the kernel.
//                The two lanes that share a query row merge their lists by one shuffle at the end.
//                THE PADDING TRAP of lcm_knn.hip applies unchanged: a pad row of a segment's last tile has the key
//                tw + |q'|^2 << 9 of a zero row and would become a neighbour; that one tile runs the CHECKED epilogue
//                (wave-uniform branch), which replaces the keys of rows >= nt by L2_NONE.
// k_l2_fold      one thread per query row: merges the segments' lists in ascending segment order with batchDistance's
//                own strict insertion -> (D1, idx1, D2, idx2) with GLOBAL train indices, ordered by (D, index).
//
// NO SQUARE ROOT IN THE HOT LOOP.  The (D, index) order equals the (s, index) order whenever the second neighbour's D is
// below 2^22: sqrtf is injective on integers below 2^22 (2^22 maps to exactly 2048.0), and above that exactly PAIRS of
// adjacent integers share a root (first: 4197200, 4197201), where a lower-index row with D + 1 precedes a higher-index row
// with D.  k_l2_fold flags the rows whose second D is >= 2^22 and
// k_l2_rescan    one wave per flagged row redoes the row over the raw bytes with 64-bit keys class(D) << 39 | index << 23
//                | D, where class(D) = D below 2^22 and 2^23 + m(D) above, m(D) = the 24-bit significand of the correctly
//                rounded sqrtf(D), found in INTEGER arithmetic (m^2 - m < D * 2^24 <= m^2 + m): two D share a class iff
//                they share a float root, with no dependence on the device's sqrt.  A fixed grid walks the flag list, so
//                the host never reads the count.  Real SIFT neighbours sit far below 2^22 (uniform random bytes give D
//                between 0.8 M and 2.1 M): a correctness path, not a hot one.
// The host turns D into s with sqrtf (lcm_l2.cpp) and runs Lowe's ratio test in double.
//
// Budget (tests/test_kernel_metadata_l2.py): no scratch, no spills, no LDS beyond the pack kernel's 1 KiB, at most 128
// VGPRs (4 waves per SIMD) for every kernel but k_l2_score<2>, whose two query tiles per wave get 168 (3 waves per SIMD).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lcm_kernels.h"
#include "lcm_l2_device.h"

namespace lcm {

// ---- raw rows -> operand image + per-row word ------------------------------------------------------------------------
__device__ __forceinline__ int l2_sq4(uint32_t w) {           // sum of squares of the four int8 of w
    int s = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) { const int v = (int)(int8_t)(w >> (8 * b)); s += v * v; }
    return s;
}

__global__ __launch_bounds__(256) void k_l2_pack(L2PackArgs a) {
    __shared__ int part[8][32];
    const uint32_t T = blockIdx.x;
    const uint32_t ks = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const uint32_t meta = a.tile_meta[T], valid = meta & 0xFFu, tile_in_frame = meta >> 8;
    uint4 v = make_uint4(0, 0, 0, 0);
    int s2 = 0;
    if (r < valid) {
        v = *reinterpret_cast<const uint4*>(a.raw + ((size_t)T * L2_TILE_ROWS + r) * L2_ROW_BYTES + ks * 32 + h * 16);
        v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
        s2 = l2_sq4(v.x) + l2_sq4(v.y) + l2_sq4(v.z) + l2_sq4(v.w);
    }
    reinterpret_cast<uint4*>(a.img)[(size_t)T * 256 + ks * 64 + lane] = v;
    part[ks * 2 + h][r] = s2;
    __syncthreads();
    if (threadIdx.x < 32) {
        int n2 = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) n2 += part[k][threadIdx.x];
        a.tw[(size_t)T * L2_TILE_ROWS + threadIdx.x] = ((uint32_t)n2 << L2_KEY_SHIFT) | ((tile_in_frame & 15u) << 5) | threadIdx.x;
    }
}

hipError_t launch_l2_pack(const L2PackArgs& a, hipStream_t st) {
    if (a.n_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_l2_pack, dim3(a.n_tiles), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---- the score kernel ------------------------------------------------------------------------------------------------
// the exact top-2 update and the key epilogue: lcm_l2_device.h (shared with lcm_l2_count.hip)
template <int QT>
__global__ __launch_bounds__(256, QT == 1 ? 4 : 3) void k_l2_score(L2ScoreArgs a) {
    const L2Item it = a.items[blockIdx.x];
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
        const bool partial = (t + 1) * L2_TILE_ROWS > nt;       // wave-uniform: only a segment's last tile
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

    // lanes l and l + 32 hold the same query rows over different train rows: their keys never compare equal
#pragma unroll
    for (int j = 0; j < QT; ++j) {
        const uint32_t o1 = (uint32_t)__shfl_xor((int)b1[j], 32, 64), o2 = (uint32_t)__shfl_xor((int)b2[j], 32, 64);
        l2_top2_insert(b1[j], b2[j], o1);
        l2_top2_insert(b1[j], b2[j], o2);
        const uint32_t row = (qt0 + j) * L2_TILE_ROWS + r;
        if (h == 0 && row < it.q_rows) a.seg_keys[(size_t)blockIdx.x * a.chunk_rows + row] = make_uint2(b1[j], b2[j]);
    }
}

hipError_t launch_l2_score(const L2ScoreArgs& a, uint32_t n_items, hipStream_t st) {
    if (n_items == 0) return hipSuccess;
    if (a.chunk_rows == 128) hipLaunchKernelGGL(k_l2_score<1>, dim3(n_items), dim3(256), 0, st, a);
    else if (a.chunk_rows == 256) hipLaunchKernelGGL(k_l2_score<2>, dim3(n_items), dim3(256), 0, st, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---- fold over segments ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_l2_fold(L2FoldArgs a) {
    const uint32_t job = a.job_base + blockIdx.y;
    const L2Job jb = a.jobs[job];
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= jb.nq) return;
    const uint32_t c = r / a.chunk_rows, lr = r % a.chunk_rows;
    const uint2* src = a.seg_keys + ((size_t)jb.first_item + (size_t)c * jb.n_seg) * a.chunk_rows + lr;
    uint32_t d1 = L2_NONE, i1 = L2_NONE, d2 = L2_NONE, i2 = L2_NONE;
    for (uint32_t g = 0; g < jb.n_seg; ++g) {                  // ascending train index: batchDistance's insertion
        const uint2 k = src[(size_t)g * a.chunk_rows];
        const uint32_t ks[2] = {k.x, k.y};
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            if (ks[n] == L2_NONE) continue;
            const uint32_t d = ks[n] >> L2_KEY_SHIFT, i = (ks[n] & ((1u << L2_KEY_SHIFT) - 1u)) + g * (uint32_t)L2_SEG_ROWS;
            if (d < d2) {
                if (d < d1) { d2 = d1; i2 = i1; d1 = d; i1 = i; }
                else { d2 = d; i2 = i; }
            }
        }
    }
    a.final_keys[(size_t)jb.out_row0 + r] = make_uint4(d1, i1, d2, i2);
    if (d2 != L2_NONE && d2 >= L2_RESCAN_MIN) {
        const uint32_t slot = atomicAdd(a.counter, 1u);
        if (slot < a.flag_cap) a.flagged[slot] = make_uint2(job, r);
    }
}

hipError_t launch_l2_fold(const L2FoldArgs& a, uint32_t n_jobs, uint32_t max_nq, hipStream_t st) {
    if (n_jobs == 0 || max_nq == 0) return hipSuccess;
    return launch_y_sliced(k_l2_fold, a, &L2FoldArgs::job_base, n_jobs, (max_nq + 255) / 256, 256, st);
}

// ---- rescan of the rows whose second neighbour may share a float root with its rival ----------------------------------
// class(D): equal for two D iff sqrtf gives them the same float, monotone in D
__device__ __forceinline__ uint32_t l2_sqrt_class(uint32_t D) {
    if (D < L2_RESCAN_MIN) return D;                            // injective there
    const uint64_t X = (uint64_t)D << 24;                       // sqrt(D) in [2048, 4096): ulp 2^-12, m = round(sqrt(X))
    uint64_t m = (uint64_t)sqrt((double)X);
    while (m * m > X) --m;
    while ((m + 1) * (m + 1) <= X) ++m;                         // m = floor(sqrt(X)), whatever the estimate was
    if (X > m * m + m) ++m;                                     // (m + 1/2)^2 < X: round up (a tie is impossible)
    return (1u << 23) + (uint32_t)m;                            // m in [2^23, 2^24)
}

__device__ __forceinline__ uint32_t l2_sqdiff4(uint32_t x, uint32_t y) {
    uint32_t s = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int d = (int)((x >> (8 * b)) & 0xFFu) - (int)((y >> (8 * b)) & 0xFFu);
        s += (uint32_t)(d * d);
    }
    return s;
}

__device__ __forceinline__ void l2_top2_insert64(uint64_t& b1, uint64_t& b2, uint64_t k) {
    b2 = min(b2, max(b1, k));
    b1 = min(b1, k);
}

__device__ __forceinline__ uint64_t l2_shfl_xor64(uint64_t v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(256) void k_l2_rescan(L2FoldArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n_waves = gridDim.x * 4u;
    const uint32_t n = min(*a.counter, a.flag_cap);
    for (uint32_t e = blockIdx.x * 4u + (threadIdx.x >> 6); e < n; e += n_waves) {
        const uint2 f = a.flagged[e];
        const L2Job jb = a.jobs[f.x];
        const uint4* q = reinterpret_cast<const uint4*>(a.raw + ((size_t)jb.q_tile * L2_TILE_ROWS + f.y) * L2_ROW_BYTES);
        uint64_t b1 = ~0ull, b2 = ~0ull;
        for (uint32_t t = lane; t < jb.nt; t += 64) {
            const uint4* tr = reinterpret_cast<const uint4*>(a.raw + ((size_t)jb.t_tile * L2_TILE_ROWS + t) * L2_ROW_BYTES);
            uint32_t D = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint4 x = q[k], y = tr[k];
                D += l2_sqdiff4(x.x, y.x) + l2_sqdiff4(x.y, y.y) + l2_sqdiff4(x.z, y.z) + l2_sqdiff4(x.w, y.w);
            }
            l2_top2_insert64(b1, b2, ((uint64_t)l2_sqrt_class(D) << 39) | ((uint64_t)t << 23) | D);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const uint64_t o1 = l2_shfl_xor64(b1, o), o2 = l2_shfl_xor64(b2, o);
            l2_top2_insert64(b1, b2, o1);
            l2_top2_insert64(b1, b2, o2);
        }
        if (lane == 0)
            a.final_keys[(size_t)jb.out_row0 + f.y] = make_uint4((uint32_t)b1 & 0x7FFFFFu, (uint32_t)(b1 >> 23) & 0xFFFFu,
                                                                (uint32_t)b2 & 0x7FFFFFu, (uint32_t)(b2 >> 23) & 0xFFFFu);
    }
}

hipError_t launch_l2_rescan(const L2FoldArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_l2_rescan, dim3(256), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace lcm
