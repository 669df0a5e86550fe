// lcm_sift_host.h — the pure host side of the SIFT keypoint detector (lcm_sift.cpp): the parameters' defaults and checks, the plan
// of a scale space (octaves, sizes, sigmas, radii and taps, in double), where every layer lies in a space, the extrema search's
// blocks, the refinement's constants and the blur kernel's LDS bytes.  No HIP call and no handle: tests/cpp/sift_host_check.cpp
// compiles this text into a stand-alone program that runs under a sanitizer.  A check returns {0, NULL} or the status and what is wrong.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/lcm.h"
#include "lcm_sift_device.h"

namespace lcm {

struct SiftProblem { int code; const char* what; };      // code: LCM_OK, LCM_ERR_INVALID_ARG or LCM_ERR_CAPACITY
constexpr SiftProblem SIFT_FINE{LCM_OK, nullptr};
constexpr size_t SIFT_LDS_BYTES = 160 * 1024;            // of a CU

inline void sift_params_default(lcm_sift_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->contrast_threshold = 0.04; p->edge_threshold = 10.0; p->sigma = 1.6; p->init_sigma = 0.5;
    p->n_octave_layers = 3; p->upsample = 1; p->n_octaves = 0; p->border = 5; p->max_steps = 5;
}

inline const char* sift_params_problem(const lcm_sift_params& p) {
    const double v[4] = {p.contrast_threshold, p.edge_threshold, p.sigma, p.init_sigma};
    for (double x : v)
        if (!std::isfinite(x) || !(x > 0.0)) return "contrast_threshold, edge_threshold, sigma and init_sigma must be finite and > 0";
    if (p.n_octave_layers < 1 || p.n_octave_layers > SIFT_MAX_LAYERS) return "n_octave_layers must be 1 .. 8";
    if (p.border < 1) return "border must be >= 1";
    if (p.max_steps < 1) return "max_steps must be >= 1";
    if (p.n_octaves < 0 || p.n_octaves > SIFT_MAX_OCTAVES) return "n_octaves must be 0 (derived) .. 16";
    if (p.upsample != 0 && p.upsample != 1) return "upsample must be 0 or 1";
    return nullptr;
}

inline int sift_cv_round(double x) { return (int)std::nearbyint(x); }      // half to even (the default rounding mode)
inline int sift_radius(double sig) { return (sift_cv_round(8.0 * sig + 1.0) | 1) / 2; }

// 2 r + 1 taps of sig: exp(-(j - r)^2 / (2 sig^2)) in double, divided by their sum (ascending j), rounded to float
inline void sift_taps(double sig, std::vector<float>& out) {
#pragma clang fp contract(off)
    const int r = sift_radius(sig);
    std::vector<double> t((size_t)(2 * r + 1));
    double s = 0.0;
    for (int j = 0; j <= 2 * r; ++j) {
        const double x = (double)(j - r);
        t[(size_t)j] = std::exp(-(x * x) / (2.0 * sig * sig));
        s += t[(size_t)j];
    }
    out.resize(t.size());
    for (size_t j = 0; j < t.size(); ++j) out[j] = (float)(t[j] / s);
}

// *out zeroed first; every field set on SIFT_FINE
inline SiftProblem sift_plan(int w, int h, const lcm_sift_params& p, lcm_sift_plan_info* out) {
#pragma clang fp contract(off)
    std::memset(out, 0, sizeof(*out));
    if (const char* what = sift_params_problem(p)) return {LCM_ERR_INVALID_ARG, what};
    if (w < 1 || h < 1) return {LCM_ERR_INVALID_ARG, "the image must have at least one pixel a side"};
    if (w > LCM_SIFT_MAX_SIDE || h > LCM_SIFT_MAX_SIDE) return {LCM_ERR_CAPACITY, "the image is larger than LCM_SIFT_MAX_SIDE a side"};
    const int bw = p.upsample ? 2 * w : w, bh = p.upsample ? 2 * h : h, side = bw < bh ? bw : bh;
    const int n_oct = p.n_octaves > 0 ? p.n_octaves : sift_cv_round(std::log2((double)side) - 2.0) + (p.upsample ? 1 : 0);
    if (n_oct < 1) return {LCM_ERR_INVALID_ARG, "the image is too small for one octave"};
    if (n_oct > SIFT_MAX_OCTAVES) return {LCM_ERR_CAPACITY, "more octaves than LCM_SIFT_MAX_OCTAVES"};
    if ((side >> (n_oct - 1)) < 1) return {LCM_ERR_INVALID_ARG, "the last octave would have no pixel"};
    const int n = p.n_octave_layers;
    out->n_octaves = n_oct; out->n_gauss = n + 3; out->n_dog = n + 2; out->base_w = bw; out->base_h = bh;
    const double k = std::pow(2.0, 1.0 / (double)n);
    out->sig[0] = p.sigma;
    for (int i = 1; i < n + 3; ++i) {
        const double prev = p.sigma * std::pow(k, (double)(i - 1)), total = prev * k;
        out->sig[i] = std::sqrt(total * total - prev * prev);
        out->radius[i] = sift_radius(out->sig[i]);
        if (out->radius[i] > out->max_radius) out->max_radius = out->radius[i];
    }
    const double a = p.upsample ? 2.0 * p.init_sigma : p.init_sigma, d = p.sigma * p.sigma - a * a;
    out->first_sigma = std::sqrt(d > 0.01 ? d : 0.01);
    out->first_radius = sift_radius(out->first_sigma);
    if (out->first_radius > out->max_radius) out->max_radius = out->first_radius;
    if (out->max_radius > SIFT_MAX_RADIUS) return {LCM_ERR_CAPACITY, "a blur's radius is above LCM_SIFT_MAX_RADIUS"};
    uint64_t floats = (uint64_t)bw * (uint64_t)bh;
    for (int o = 0; o < n_oct; ++o) {
        out->width[o] = bw >> o; out->height[o] = bh >> o;
        floats += (uint64_t)(2 * n + 5) * (uint64_t)out->width[o] * (uint64_t)out->height[o];
    }
    out->space_floats = floats;
    return SIFT_FINE;
}

// Where the layers of a plan lie in a space, in floats: the base image at 0, then per octave its Gaussian layers and its DoG layers
inline uint64_t sift_gauss_offset(const lcm_sift_plan_info& pl, int octave, int layer) {
    uint64_t at = (uint64_t)pl.base_w * (uint64_t)pl.base_h;
    for (int o = 0; o < octave; ++o) at += (uint64_t)(pl.n_gauss + pl.n_dog) * (uint64_t)pl.width[o] * (uint64_t)pl.height[o];
    return at + (uint64_t)layer * (uint64_t)pl.width[octave] * (uint64_t)pl.height[octave];
}
inline uint64_t sift_dog_offset(const lcm_sift_plan_info& pl, int octave, int layer) {
    return sift_gauss_offset(pl, octave, pl.n_gauss) + (uint64_t)layer * (uint64_t)pl.width[octave] * (uint64_t)pl.height[octave];
}

// The extrema search's linear order: octave o's pixels of layers 1 .. n, row after row, in blocks of SIFT_THREADS; levels[o] set,
// *n_blocks = all blocks.  The pixels that may be candidates (inside the border) counted into *n_inside.
inline void sift_levels(const lcm_sift_plan_info& pl, const lcm_sift_params& p, SiftLevel* levels, uint32_t* n_blocks, uint64_t* n_inside) {
    uint32_t b = 0;
    uint64_t inside = 0;
    for (int o = 0; o < pl.n_octaves; ++o) {
        const uint64_t px = (uint64_t)p.n_octave_layers * (uint64_t)pl.width[o] * (uint64_t)pl.height[o];
        levels[o] = SiftLevel{pl.width[o], pl.height[o], b, 0u, sift_dog_offset(pl, o, 0)};
        b += (uint32_t)((px + SIFT_THREADS - 1) / SIFT_THREADS);
        const int64_t iw = (int64_t)pl.width[o] - 2 * (int64_t)p.border, ih = (int64_t)pl.height[o] - 2 * (int64_t)p.border;
        if (iw > 0 && ih > 0) inside += (uint64_t)p.n_octave_layers * (uint64_t)iw * (uint64_t)ih;
    }
    *n_blocks = b; *n_inside = inside;
}

inline float sift_threshold(const lcm_sift_params& p) {
#pragma clang fp contract(off)
    return (float)std::floor(0.5 * p.contrast_threshold / (double)p.n_octave_layers * 255.0);
}

inline SiftRefine sift_refine_consts(const lcm_sift_params& p) {
#pragma clang fp contract(off)
    const float s = 1.0f / 255.0f;
    return SiftRefine{s, s * 0.5f, s * 0.25f, (float)p.contrast_threshold, (float)p.edge_threshold, (float)p.sigma, (float)p.n_octave_layers,
                      p.n_octave_layers, p.border, p.max_steps, p.upsample};
}

// The blur kernel's dynamic LDS for radius r: the source tile with its halo, (T + 2 r)^2 floats, and the row pass's output,
// (T + 2 r) x T floats.  20.4 KiB at the defaults' largest radius (13: seven workgroups a CU), 80 KiB at SIFT_MAX_RADIUS (one).
constexpr size_t sift_blur_lds_bytes(int r) {
    return ((size_t)(SIFT_TILE + 2 * r) * (size_t)(SIFT_TILE + 2 * r) + (size_t)(SIFT_TILE + 2 * r) * (size_t)SIFT_TILE) * sizeof(float);
}
static_assert(sift_blur_lds_bytes(SIFT_MAX_RADIUS) <= SIFT_LDS_BYTES / 2, "the largest tile leaves room for two workgroups' worth of LDS");

}  // namespace lcm
