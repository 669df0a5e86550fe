// lcm_l2_count_device.h — the body of the ratio-test count on SIFT rows, shared by the two kernels that run it:
// k_l2_count (lcm_l2_count.hip: the item comes from a host-built table) and k_l2_count_store (lcm_l2_store.hip: the
// workgroup derives its item from the store's tables).  The verdict, the roots and the top-2 walk exist here, once.
// lcm_l2_emit.hip (the survivors' lists) takes the verdict and the root from here too.  Included by those three files only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcm_kernels.h"
#include "lcm_l2_device.h"

namespace lcm {

// OpenCV's distance of a squared distance D <= L2_MAX_DSQ: sqrtf((float)D), bit for bit (lcm_l2_count.hip's header)
__device__ __forceinline__ float l2_root(uint32_t D) { return (float)sqrt((double)D); }

// Lowe's ratio test on the two smallest squared distances of a query row (src/main.cpp:524-531), as lcm_l2.cpp's host
// list runs it: strict, in IEEE double.
__device__ __forceinline__ bool l2_ratio_pass(uint32_t D1, uint32_t D2, double ratio) {
#pragma clang fp contract(off)
    const double s1 = (double)l2_root(D1), s2 = (double)l2_root(D2);
    const double lim = ratio * s2;
    return s1 < lim;
}

// One workgroup (4 waves) = one item: q_rows <= 128 * QT query rows starting at tile q_tile against ALL t_rows train rows
// starting at tile t_tile; each wave adds its survivors to rec[0] and takes the minimum of its rows' D1 into rec[1].
// Every argument is workgroup-uniform.
template <int QT>
__device__ __forceinline__ void l2_count_item(const uint8_t* img_bytes, const uint32_t* tw_all, uint32_t q_tile, uint32_t q_rows,
                                              uint32_t t_tile, uint32_t t_rows, uint32_t* rec, double ratio) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const uint32_t qt0 = wave * QT;
    if (qt0 * L2_TILE_ROWS >= q_rows) return;                  // whole wave, no barrier in this kernel
    const uint4* img = reinterpret_cast<const uint4*>(img_bytes);

    // B operands: this wave's query tiles x 4 k-steps, resident for the whole item (tiles past the chunk: zeros, unused)
    l2_v4i b[QT][4];
    uint32_t qterm[QT], b1[QT], b2[QT];
#pragma unroll
    for (int j = 0; j < QT; ++j) {
        const bool have = (qt0 + j) * L2_TILE_ROWS < q_rows;
        const size_t tile = (size_t)q_tile + qt0 + j;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            uint4 x = make_uint4(0, 0, 0, 0);
            if (have) x = img[tile * 256 + ks * 64 + lane];
            b[j][ks] = l2_v4i{(int)x.x, (int)x.y, (int)x.z, (int)x.w};
        }
        qterm[j] = have ? (tw_all[tile * L2_TILE_ROWS + r] & ~((1u << L2_KEY_SHIFT) - 1u)) : 0u;
        b1[j] = b2[j] = L2_NONE;
    }

    // every train tile of the matrix, the next one's fragments in flight; the running keys live across all of them
    const uint32_t nt = t_rows, nt_tiles = (nt + L2_TILE_ROWS - 1) / L2_TILE_ROWS;
    const uint4* timg = img + (size_t)t_tile * 256 + lane;
    const uint4* ttw = reinterpret_cast<const uint4*>(tw_all + (size_t)t_tile * L2_TILE_ROWS) + h;
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
    const bool live = (QT == 2 || h == 0) && row < q_rows;
    const uint32_t D1 = k1 >> L2_KEY_SHIFT, D2 = k2 >> L2_KEY_SHIFT;
    const bool pass = live && k2 != L2_NONE && l2_ratio_pass(D1, D2, ratio);       // fewer than 2 neighbours: not counted
    const uint32_t good = (uint32_t)__popcll(__ballot(pass));
    uint32_t dmin = live && k1 != L2_NONE ? D1 : L2_NONE;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) dmin = min(dmin, (uint32_t)__shfl_xor((int)dmin, o, 64));
    if (lane == 0) {
        if (good) atomicAdd(rec, good);
        if (dmin != L2_NONE) atomicMin(rec + 1, dmin);
    }
}

}  // namespace lcm
