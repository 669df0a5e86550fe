// lcm_sift_device.h — the arithmetic of the SIFT keypoint detector (include/lcm.h, lcm_sift_*) that the kernels of lcm_sift.hip run
// per pixel and per candidate, stated once:
//   sift_fold          the reflect-101 index of a line of n pixels, folded with period 2 (n - 1) until it is inside; 0 for n == 1
//   sift_upsampled     one pixel of the 2x bilinear enlargement of a uint8 image (weights 0.25 / 0.75, indices clamped)
//   sift_is_extremum   |v| > T and v >= (v > 0) or v <= (v < 0) all 26 neighbours in the three DoG layers
//   sift_solve3        3 x 3 Gaussian elimination with partial pivoting (largest |.|, first of equals); false: a pivot is zero
//   sift_pow2          2^e of the keypoint's size: k = rint(e), the Taylor polynomial of exp((e - k) ln 2) by Horner, times 2^k
//   sift_refine        the sub-pixel refinement of one candidate with its contrast and edge tests; 0 and the record, or the reason
// In float, every product and sum rounded on its own, sums in the stated order.  The fp contract pragma is lexical, an inlined
// callee does not take it from its caller: every function states its own.  Everything is __host__ __device__: the host compiles
// the same text (tests/cpp/sift_host_check.cpp runs it under a sanitizer against tests/siftref.py, bit for bit).  Only + - x /,
// comparisons, fabsf, rintf and ldexpf by a small integer are used, so that numpy can restate it exactly.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace lcm {

constexpr int SIFT_MAX_OCTAVES = 16;      // = LCM_SIFT_MAX_OCTAVES
constexpr int SIFT_MAX_LAYERS = 8;        // n_octave_layers; 11 Gaussian and 10 DoG layers per octave at most
constexpr int SIFT_MAX_RADIUS = 48;       // = LCM_SIFT_MAX_RADIUS: a blur of at most 97 taps
constexpr int SIFT_TILE = 32;             // the blur kernel's output tile is SIFT_TILE x SIFT_TILE
constexpr int SIFT_THREADS = 256;

// why the refinement dropped a candidate (tests/siftref.py has the same numbers)
enum SiftReason { SIFT_KEPT = 0, SIFT_ZERO_PIVOT = 1, SIFT_TOO_FAR = 2, SIFT_LEFT = 3, SIFT_NOT_CONVERGED = 4, SIFT_LOW_CONTRAST = 5, SIFT_EDGE = 6 };

// = lcm_sift_keypoint, lcm_sift_candidate (include/lcm.h; lcm_sift.cpp asserts the layouts)
struct SiftKeypoint { float x, y, size, response, xi; int16_t octave, layer; int32_t col, row; };
struct SiftCandidate { int32_t octave, layer, row, col; };
// one octave as the kernels see it: its size, where its DoG layers start in the space (in floats), its first block in the
// extrema search's linear order
struct SiftLevel { int32_t w, h; uint32_t block0, pad; uint64_t dog_off; };
// the refinement's constants, rounded to float once, on the host
struct SiftRefine {
    float img_scale, deriv_scale, cross_scale;     // 1/255, 0.5/255, 0.25/255: the quotient rounded, then the product
    float contrast, edge, sigma, layers_f;         // (float) of the parameters; n_octave_layers as a float
    int32_t n_layers, border, max_steps, upsample;
};

constexpr float SIFT_X_LIMIT = 715827882.0f;       // INT_MAX / 3, rounded to float
constexpr float SIFT_LN2 = 0.693147182f;

// The line is mirrored about 0, so -i folds as i does; an index below the period (every halo of an image wider than the radius)
// needs no division.
__host__ __device__ __forceinline__ int sift_fold(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    if (i < 0) i = -i;
    if (i >= p) i %= p;
    return i < n ? i : p - i;
}

// pixel (dx, dy) of the enlarged image: the source coordinate is (d + 0.5) / 2 - 0.5, so an even d = 2 k takes 0.25 of pixel k - 1
// and 0.75 of pixel k, an odd d = 2 k + 1 takes 0.75 of k and 0.25 of k + 1, indices clamped to the image; rows first, then the
// column.  Every value is a multiple of 1/16 below 256: exact in float.
__host__ __device__ __forceinline__ float sift_upsampled(const uint8_t* __restrict__ img, size_t stride, int w, int h, int dx, int dy) {
#pragma clang fp contract(off)
    const int kx = dx >> 1, ky = dy >> 1;
    const bool ex = (dx & 1) == 0, ey = (dy & 1) == 0;
    const int x0 = ex ? (kx > 0 ? kx - 1 : 0) : kx, x1 = ex ? kx : (kx + 1 < w ? kx + 1 : w - 1);
    const int y0 = ey ? (ky > 0 ? ky - 1 : 0) : ky, y1 = ey ? ky : (ky + 1 < h ? ky + 1 : h - 1);
    const float wx0 = ex ? 0.25f : 0.75f, wx1 = ex ? 0.75f : 0.25f, wy0 = ey ? 0.25f : 0.75f, wy1 = ey ? 0.75f : 0.25f;
    const float top = wx0 * (float)img[(size_t)y0 * stride + x0] + wx1 * (float)img[(size_t)y0 * stride + x1];
    const float bot = wx0 * (float)img[(size_t)y1 * stride + x0] + wx1 * (float)img[(size_t)y1 * stride + x1];
    return wy0 * top + wy1 * bot;
}

// cur: the pixel in its DoG layer, a row being w floats and a layer `plane` floats; the caller keeps it one pixel inside
__host__ __device__ __forceinline__ bool sift_is_extremum(const float* __restrict__ cur, size_t plane, int w, float T) {
    const float v = *cur;
    if (!(fabsf(v) > T)) return false;
    if (!(v > 0.0f) && !(v < 0.0f)) return false;
    const bool up = v > 0.0f;
#pragma clang loop unroll(disable)
    for (int dl = -1; dl <= 1; ++dl) {                       // one layer at a time: its nine loads together, then one decision
        const float* layer = cur + (ptrdiff_t)plane * dl;
        bool all = true;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const float n = layer[(ptrdiff_t)w * dy + dx];
                all = all && (up ? v >= n : v <= n);
            }
        if (!all) return false;
    }
    return true;
}

// A x = b.  Column by column: the row with the largest |entry| at or below the diagonal (the first of equals) comes up, a zero
// pivot ends it; row i takes f = a_ik / a_kk and a_ij - f a_kj, b_i - f b_k; then x2 = b2 / a22, x1 = (b1 - a12 x2) / a11,
// x0 = ((b0 - a01 x1) - a02 x2) / a00.  Scalars only: no array is indexed by a pivot.
__host__ __device__ __forceinline__ bool sift_solve3(float a00, float a01, float a02, float a10, float a11, float a12, float a20, float a21,
                                                     float a22, float b0, float b1, float b2, float& x0, float& x1, float& x2) {
#pragma clang fp contract(off)
    float t;
#define LCM_SIFT_SWAP(p, q) do { t = p; p = q; q = t; } while (0)
    int p = 0;
    float m = fabsf(a00);
    if (fabsf(a10) > m) { p = 1; m = fabsf(a10); }
    if (fabsf(a20) > m) p = 2;
    if (p == 1) { LCM_SIFT_SWAP(a00, a10); LCM_SIFT_SWAP(a01, a11); LCM_SIFT_SWAP(a02, a12); LCM_SIFT_SWAP(b0, b1); }
    if (p == 2) { LCM_SIFT_SWAP(a00, a20); LCM_SIFT_SWAP(a01, a21); LCM_SIFT_SWAP(a02, a22); LCM_SIFT_SWAP(b0, b2); }
    if (a00 == 0.0f) return false;
    float f = a10 / a00;
    a11 = a11 - f * a01; a12 = a12 - f * a02; b1 = b1 - f * b0;
    f = a20 / a00;
    a21 = a21 - f * a01; a22 = a22 - f * a02; b2 = b2 - f * b0;
    if (fabsf(a21) > fabsf(a11)) { LCM_SIFT_SWAP(a11, a21); LCM_SIFT_SWAP(a12, a22); LCM_SIFT_SWAP(b1, b2); }
#undef LCM_SIFT_SWAP
    if (a11 == 0.0f) return false;
    f = a21 / a11;
    a22 = a22 - f * a12; b2 = b2 - f * b1;
    if (a22 == 0.0f) return false;
    x2 = b2 / a22;
    x1 = (b1 - a12 * x2) / a11;
    x0 = ((b0 - a01 * x1) - a02 * x2) / a00;
    return true;
}

__host__ __device__ __forceinline__ float sift_pow2(float e) {
#pragma clang fp contract(off)
    const float k = rintf(e);
    const float x = (e - k) * SIFT_LN2;
    float acc = (float)(1.0 / 40320.0);
    acc = (float)(1.0 / 5040.0) + x * acc;
    acc = (float)(1.0 / 720.0) + x * acc;
    acc = (float)(1.0 / 120.0) + x * acc;
    acc = (float)(1.0 / 24.0) + x * acc;
    acc = (float)(1.0 / 6.0) + x * acc;
    acc = 0.5f + x * acc;
    acc = 1.0f + x * acc;
    acc = 1.0f + x * acc;
    return acc * ldexpf(1.0f, (int)k);
}

// dog: the octave's DoG layers, w x h each, layer after layer.  At most max_steps steps: the derivatives at (layer, row, col) with
// OpenCV's scales, X = -(H^-1 dD); all |X_i| < 0.5 ends the walk; an |X_i| above INT_MAX / 3 (or a NaN) drops the candidate;
// else the position moves by rint(X) (half to even) and must stay in layers 1 .. n and inside the border.  Then the contrast
// v (1/255) + 0.5 (dD . X) and the edge test on the last position's dxx, dyy, dxy.
__host__ __device__ __forceinline__ int sift_refine(const float* __restrict__ dog, int w, int h, int octave, int layer, int row, int col,
                                                    const SiftRefine& k, SiftKeypoint& out) {
#pragma clang fp contract(off)
    const size_t plane = (size_t)w * (size_t)h;
    float xc = 0.0f, xr = 0.0f, xi = 0.0f, g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, dxx = 0.0f, dyy = 0.0f, dxy = 0.0f, v = 0.0f;
    bool converged = false;
    for (int step = 0; step < k.max_steps; ++step) {
        const float* img = dog + plane * (size_t)layer + (size_t)row * (size_t)w + (size_t)col;
        const float* prev = img - plane;
        const float* next = img + plane;
        v = img[0];
        g0 = (img[1] - img[-1]) * k.deriv_scale;
        g1 = (img[w] - img[-w]) * k.deriv_scale;
        g2 = (next[0] - prev[0]) * k.deriv_scale;
        const float v2 = v * 2.0f;
        dxx = ((img[1] + img[-1]) - v2) * k.img_scale;
        dyy = ((img[w] + img[-w]) - v2) * k.img_scale;
        const float dss = ((next[0] + prev[0]) - v2) * k.img_scale;
        dxy = (((img[w + 1] - img[w - 1]) - img[-w + 1]) + img[-w - 1]) * k.cross_scale;
        const float dxs = (((next[1] - next[-1]) - prev[1]) + prev[-1]) * k.cross_scale;
        const float dys = (((next[w] - next[-w]) - prev[w]) + prev[-w]) * k.cross_scale;
        float s0, s1, s2;
        if (!sift_solve3(dxx, dxy, dxs, dxy, dyy, dys, dxs, dys, dss, g0, g1, g2, s0, s1, s2)) return SIFT_ZERO_PIVOT;
        xc = -s0; xr = -s1; xi = -s2;
        if (fabsf(xc) < 0.5f && fabsf(xr) < 0.5f && fabsf(xi) < 0.5f) { converged = true; break; }
        if (!(fabsf(xc) <= SIFT_X_LIMIT && fabsf(xr) <= SIFT_X_LIMIT && fabsf(xi) <= SIFT_X_LIMIT)) return SIFT_TOO_FAR;
        col += (int)rintf(xc); row += (int)rintf(xr); layer += (int)rintf(xi);
        if (layer < 1 || layer > k.n_layers || col < k.border || col >= w - k.border || row < k.border || row >= h - k.border) return SIFT_LEFT;
    }
    if (!converged) return SIFT_NOT_CONVERGED;
    const float t = (g0 * xc + g1 * xr) + g2 * xi;
    const float contr = v * k.img_scale + t * 0.5f;
    if (fabsf(contr) * k.layers_f < k.contrast) return SIFT_LOW_CONTRAST;
    const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
    if (det <= 0.0f || (tr * tr) * k.edge >= ((k.edge + 1.0f) * (k.edge + 1.0f)) * det) return SIFT_EDGE;
    const float scale = ldexpf(1.0f, octave) * (k.upsample ? 0.5f : 1.0f);
    out.x = ((float)col + xc) * scale;
    out.y = ((float)row + xr) * scale;
    out.size = (k.sigma * sift_pow2(((float)layer + xi) / k.layers_f)) * (scale * 2.0f);
    out.response = fabsf(contr);
    out.xi = xi;
    out.octave = (int16_t)octave; out.layer = (int16_t)layer; out.col = col; out.row = row;
    return SIFT_KEPT;
}

// ---- the launchers of lcm_sift.hip (every grid is one-dimensional)
hipError_t launch_sift_base(const uint8_t* img, float* dst, int w, int h, int upsample, hipStream_t st);            // k_sift_base
hipError_t launch_sift_blur(const float* src, float* dst, float* dog, const float* taps, int w, int h, int r, size_t lds_bytes,
                            hipStream_t st);                                                                         // k_sift_blur
hipError_t launch_sift_half(const float* src, int src_w, float* dst, int w, int h, hipStream_t st);                 // k_sift_half
hipError_t launch_sift_extrema(const float* space, const SiftLevel* levels, int n_octaves, int n_layers, int border, float T, uint32_t* blocks,
                               uint32_t n_blocks, SiftCandidate* out, uint32_t cap, bool emit, hipStream_t st);     // k_sift_extrema
hipError_t launch_sift_refine(const float* space, const SiftLevel* levels, const SiftCandidate* cand, uint32_t n, const SiftRefine& k,
                              SiftKeypoint* rec, uint8_t* kept, uint32_t* blocks, hipStream_t st);                   // k_sift_refine
hipError_t launch_sift_compact(const SiftKeypoint* rec, const uint8_t* kept, const uint32_t* blocks, uint32_t n, SiftKeypoint* out,
                               hipStream_t st);                                                                      // k_sift_compact

}  // namespace lcm
