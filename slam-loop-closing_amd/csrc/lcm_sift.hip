// lcm_sift.hip — the SIFT keypoint detector's scale space, extrema and refinement on the device (include/lcm.h, lcm_sift_*), with
// every step's arithmetic defined in lcm_sift_device.h.  The path is bound by memory traffic: a blur reads one layer and writes
// two.  No floating-point atomic and no atomic cursor anywhere: the lists are ordered compactions (block counts, k_block_scan of
// lcm_kernels.hip, a ballot rank), so the same call gives the same bytes.  Every load index of a blur goes through sift_fold,
// those of the lanes beyond the image included; the extrema and the refinement read only inside the border (>= 1).  Every grid is
// one-dimensional (the tile or block in x), so none meets the y limit and nothing here is launched in slices.
//
// k_sift_base        one lane per pixel of the base image: uint8 -> float, with upsample the 2x bilinear enlargement.
// k_sift_blur        one workgroup of 256 threads per 32 x 32 output tile, both passes over LDS: the source tile with a halo of
//                    the radius on every side ((32 + 2 r)^2 floats, a wave a row, loaded through the reflect map), the row pass into (32 + 2 r)
//                    x 32 floats, the column pass into registers.  It stores G[i] and, the centre of G[i - 1] being in the tile
//                    already, D[i - 1] = G[i] - G[i - 1] in the same pass.  The LDS is dynamic, sized from the blur's radius
//                    (sift_blur_lds_bytes, lcm_sift_host.h): 20.4 KiB at radius 13, 80 KiB at the largest radius, 48.
// k_sift_half        layer 0 of the next octave: the pixels (2 x, 2 y) of layer n_octave_layers.
// k_sift_extrema     256 pixels per workgroup in the search's linear order (octave, layer, row, col), so that a block's candidates
//                    are consecutive in the list: a pixel inside the border reads its own value and, only when |v| > T, its 26
//                    neighbours in the three DoG layers (from the caches: the neighbours of a row segment are its lanes' own).
//                    emit == 0 counts the block's candidates; emit == 1 ranks them (the block's prefix, the waves before, the
//                    ballot's lower lanes) and writes {octave, layer, row, col}.
// k_sift_refine      one lane per candidate: sift_refine; the 32-byte record, a flag, the block's survivors.
// k_sift_compact     the survivors' records moved to their rank, in candidate order.
//
// Budget (tests/test_kernel_metadata_sift.py): no scratch, no spills.  k_sift_refine at most 80 VGPRs and 256 bytes of LDS (the
// block's count); k_sift_blur at most 48 VGPRs and no static LDS (its dynamic LDS is sift_blur_lds_bytes of the radius: at most
// 80 KiB of a CU's 160); k_sift_extrema and k_sift_compact at most 32 VGPRs and 16 bytes of LDS; k_sift_base and k_sift_half at
// most 32 VGPRs and no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcm_sift_device.h"

namespace lcm {

struct SiftBaseArgs { const uint8_t* img; float* dst; int32_t w, h, upsample; };       // img: w x h packed bytes
struct SiftBlurArgs { const float* src; float* dst; float* dog; const float* taps; int32_t w, h, r, tiles_x; };
struct SiftHalfArgs { const float* src; float* dst; int32_t src_w, w, h; };
struct SiftExtremaArgs {
    const float* space; const SiftLevel* levels; uint32_t* blocks; SiftCandidate* out;
    int32_t n_octaves, n_layers, border; float T; uint32_t cap, emit;
};
struct SiftRefineArgs {
    const float* space; const SiftLevel* levels; const SiftCandidate* cand; SiftKeypoint* rec; uint8_t* kept; uint32_t* blocks;
    SiftRefine k; uint32_t n;
};
struct SiftCompactArgs { const SiftKeypoint* rec; const uint8_t* kept; const uint32_t* blocks; SiftKeypoint* out; uint32_t n; };

__global__ __launch_bounds__(256) void k_sift_base(SiftBaseArgs a) {
    const int bw = a.upsample ? 2 * a.w : a.w, bh = a.upsample ? 2 * a.h : a.h;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)bw * (uint32_t)bh) return;
    const int y = (int)(i / (uint32_t)bw), x = (int)(i - (uint32_t)y * (uint32_t)bw);
    a.dst[i] = a.upsample ? sift_upsampled(a.img, (size_t)a.w, a.w, a.h, x, y) : (float)a.img[(size_t)y * (size_t)a.w + (size_t)x];
}

__global__ __launch_bounds__(256) void k_sift_blur(SiftBlurArgs a) {
#pragma clang fp contract(off)
    extern __shared__ float lds[];
    const int r = a.r, S = SIFT_TILE + 2 * r, n_taps = 2 * r + 1;
    float* s_src = lds;                     // S rows of S
    float* s_tmp = lds + S * S;             // S rows of SIFT_TILE
    const int tx0 = (int)(blockIdx.x % (uint32_t)a.tiles_x) * SIFT_TILE, ty0 = (int)(blockIdx.x / (uint32_t)a.tiles_x) * SIFT_TILE;
    for (int ly = (int)(threadIdx.x >> 6); ly < S; ly += 4) {                   // a wave a row: the row's fold once, no division
        const float* row = a.src + (size_t)sift_fold(ty0 + ly - r, a.h) * (size_t)a.w;
        for (int lx = (int)(threadIdx.x & 63); lx < S; lx += 64) s_src[ly * S + lx] = row[sift_fold(tx0 + lx - r, a.w)];
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < S * SIFT_TILE; i += 256) {
        const float* p = s_src + (i / SIFT_TILE) * S + (i % SIFT_TILE);
        float acc = a.taps[0] * p[0];
        for (int j = 1; j < n_taps; ++j) acc = acc + a.taps[j] * p[j];
        s_tmp[i] = acc;
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < SIFT_TILE * SIFT_TILE; i += 256) {
        const int ly = i / SIFT_TILE, lx = i % SIFT_TILE, x = tx0 + lx, y = ty0 + ly;
        const float* p = s_tmp + ly * SIFT_TILE + lx;
        float acc = a.taps[0] * p[0];
        for (int j = 1; j < n_taps; ++j) acc = acc + a.taps[j] * p[j * SIFT_TILE];
        if (x < a.w && y < a.h) {
            const size_t at = (size_t)y * (size_t)a.w + (size_t)x;
            a.dst[at] = acc;
            if (a.dog) a.dog[at] = acc - s_src[(ly + r) * S + lx + r];
        }
    }
}

__global__ __launch_bounds__(256) void k_sift_half(SiftHalfArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)a.w * (uint32_t)a.h) return;
    const uint32_t y = i / (uint32_t)a.w, x = i - y * (uint32_t)a.w;
    a.dst[i] = a.src[(size_t)(2u * y) * (size_t)a.src_w + (size_t)(2u * x)];
}

// the lane's pixel in the search's linear order: is it a candidate, and which?
__device__ __forceinline__ bool sift_candidate_at(const SiftExtremaArgs& a, SiftCandidate& c) {
    int o = 0;
    while (o + 1 < a.n_octaves && a.levels[o + 1].block0 <= blockIdx.x) ++o;      // uniform over the workgroup
    const SiftLevel lv = a.levels[o];
    const uint32_t plane = (uint32_t)lv.w * (uint32_t)lv.h, i = (blockIdx.x - lv.block0) * 256u + threadIdx.x;
    if (i >= plane * (uint32_t)a.n_layers) return false;
    const uint32_t l = i / plane, rem = i - l * plane, row = rem / (uint32_t)lv.w, col = rem - row * (uint32_t)lv.w;
    if ((int)col < a.border || (int)col >= lv.w - a.border || (int)row < a.border || (int)row >= lv.h - a.border) return false;
    c = SiftCandidate{o, (int32_t)l + 1, (int32_t)row, (int32_t)col};
    return sift_is_extremum(a.space + lv.dog_off + (size_t)(l + 1u) * (size_t)plane + (size_t)rem, (size_t)plane, lv.w, a.T);
}

__global__ __launch_bounds__(256) void k_sift_extrema(SiftExtremaArgs a) {
    __shared__ uint32_t wave_n[4];
    SiftCandidate c;
    const bool is = sift_candidate_at(a, c);
    const uint64_t m = __ballot(is);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!a.emit) {
        if (threadIdx.x == 0) a.blocks[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        return;
    }
    if (!is) return;
    uint32_t k = a.blocks[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; ++w) k += wave_n[w];
    if (k < a.cap) a.out[k] = c;
}

__global__ __launch_bounds__(256) void k_sift_refine(SiftRefineArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool kept = false;
    if (i < a.n) {
        const SiftCandidate c = a.cand[i];
        const SiftLevel lv = a.levels[c.octave];
        SiftKeypoint kp = SiftKeypoint{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, 0, 0, 0};
        kept = sift_refine(a.space + lv.dog_off, lv.w, lv.h, c.octave, c.layer, c.row, c.col, a.k, kp) == SIFT_KEPT;
        a.rec[i] = kp;
        a.kept[i] = kept ? 1 : 0;
    }
    const int n = __syncthreads_count(kept ? 1 : 0);
    if (threadIdx.x == 0) a.blocks[blockIdx.x] = (uint32_t)n;
}

__global__ __launch_bounds__(256) void k_sift_compact(SiftCompactArgs a) {
    __shared__ uint32_t wave_n[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool kept = i < a.n && a.kept[i] != 0;
    const uint64_t m = __ballot(kept);
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!kept) return;
    uint32_t k = a.blocks[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; ++w) k += wave_n[w];
    a.out[k] = a.rec[i];
}

hipError_t launch_sift_base(const uint8_t* img, float* dst, int w, int h, int upsample, hipStream_t st) {
    const uint32_t px = (uint32_t)(upsample ? 4 : 1) * (uint32_t)w * (uint32_t)h;
    hipLaunchKernelGGL(k_sift_base, dim3((px + 255u) / 256u), dim3(256), 0, st, SiftBaseArgs{img, dst, w, h, upsample});
    return hipGetLastError();
}

// dog may be NULL (the first blur).  lds_bytes = sift_blur_lds_bytes(r); above 64 KiB the kernel's limit is raised first.
hipError_t launch_sift_blur(const float* src, float* dst, float* dog, const float* taps, int w, int h, int r, size_t lds_bytes, hipStream_t st) {
    if (lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_sift_blur), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    const int tiles_x = (w + SIFT_TILE - 1) / SIFT_TILE, tiles_y = (h + SIFT_TILE - 1) / SIFT_TILE;
    hipLaunchKernelGGL(k_sift_blur, dim3((uint32_t)tiles_x * (uint32_t)tiles_y), dim3(256), lds_bytes, st, SiftBlurArgs{src, dst, dog, taps, w, h, r, tiles_x});
    return hipGetLastError();
}

hipError_t launch_sift_half(const float* src, int src_w, float* dst, int w, int h, hipStream_t st) {
    hipLaunchKernelGGL(k_sift_half, dim3(((uint32_t)w * (uint32_t)h + 255u) / 256u), dim3(256), 0, st, SiftHalfArgs{src, dst, src_w, w, h});
    return hipGetLastError();
}

// emit == false: the candidates of every block -> blocks[0 .. n_blocks); emit == true: blocks holds their exclusive prefixes
hipError_t launch_sift_extrema(const float* space, const SiftLevel* levels, int n_octaves, int n_layers, int border, float T, uint32_t* blocks,
                               uint32_t n_blocks, SiftCandidate* out, uint32_t cap, bool emit, hipStream_t st) {
    if (n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sift_extrema, dim3(n_blocks), dim3(256), 0, st,
                       SiftExtremaArgs{space, levels, blocks, out, n_octaves, n_layers, border, T, cap, emit ? 1u : 0u});
    return hipGetLastError();
}

hipError_t launch_sift_refine(const float* space, const SiftLevel* levels, const SiftCandidate* cand, uint32_t n, const SiftRefine& k,
                              SiftKeypoint* rec, uint8_t* kept, uint32_t* blocks, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sift_refine, dim3((n + 255u) / 256u), dim3(256), 0, st, SiftRefineArgs{space, levels, cand, rec, kept, blocks, k, n});
    return hipGetLastError();
}

hipError_t launch_sift_compact(const SiftKeypoint* rec, const uint8_t* kept, const uint32_t* blocks, uint32_t n, SiftKeypoint* out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sift_compact, dim3((n + 255u) / 256u), dim3(256), 0, st, SiftCompactArgs{rec, kept, blocks, out, n});
    return hipGetLastError();
}

}  // namespace lcm
