// lcm_l2_device.h — __device__ helpers shared by the SIFT / L2 kernels: lcm_l2.hip (pair mode: per-segment keys, fold,
// rescan) and lcm_l2_count.hip (ratio-test counts per pair).  Included by those two files only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcm_kernels.h"

namespace lcm {

typedef int l2_v4i __attribute__((ext_vector_type(4)));
typedef int l2_v16i __attribute__((ext_vector_type(16)));

constexpr uint32_t L2_NONE = 0xFFFFFFFFu;      // "no neighbour": above every real key (at most 8323200 << 9 | 511)

// (b1, b2) <- the two smallest of {b1, b2, k0, k1}, b1 <= b2: lcm_knn.hip's update.  The keys are a MULTISET: a key equal
// to b1 becomes b2 (the median of {b1, k0, k1} is the second smallest of the three, counted with multiplicity).
__device__ __forceinline__ void l2_top2_pair(uint32_t& b1, uint32_t& b2, uint32_t k0, uint32_t k1) {
    uint32_t m;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(m) : "v"(b1), "v"(k0), "v"(k1));
    b2 = min(b2, m);
    b1 = min(min(b1, k0), k1);
}

__device__ __forceinline__ void l2_top2_insert(uint32_t& b1, uint32_t& b2, uint32_t k) {
    b2 = min(b2, max(b1, k));
    b1 = min(b1, k);
}

// 16 accumulators of one lane -> 16 keys -> the lane's running top-2.  tw[reg] = the train row's word, qterm = the query
// row's |q'|^2 << 9; |dot| <= 2^21 fits the 24-bit multiply.  CHECK: rows >= nt of the tile (row0 = first row of this
// lane's half: 32 t + 4 h) get L2_NONE.
template <bool CHECK>
__device__ __forceinline__ void l2_epilogue(const l2_v16i& acc, const uint32_t (&tw)[16], uint32_t qterm, uint32_t& b1, uint32_t& b2,
                                            uint32_t row0, uint32_t nt) {
    uint32_t key[16];
    int m1024;
    asm("s_movk_i32 %0, 0xfc00" : "=s"(m1024));                  // -1024
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        // key = (tw + qterm) - (dot << 10) as one v_mad_i32_i24: m1024 is opaque to the compiler, which would otherwise
        // shift and subtract.  The accumulators are read by compiler-visible code only (never by inline asm): the wait
        // states between an MFMA and the VALU that reads its result are inserted by the compiler.
        key[reg] = (uint32_t)(__mul24(acc[reg], m1024) + (int)(tw[reg] + qterm));
        if (CHECK) {
            const uint32_t row = row0 + (uint32_t)((reg & 3) + 8 * (reg >> 2));
            key[reg] = row < nt ? key[reg] : L2_NONE;
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i += 2) l2_top2_pair(b1, b2, key[i], key[i + 1]);
}

}  // namespace lcm
