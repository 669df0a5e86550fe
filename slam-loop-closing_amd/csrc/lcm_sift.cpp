// lcm_sift.cpp — the host side of the SIFT keypoint detector (include/lcm.h, lcm_sift_*): the first half of detectAndDescribeSIFT
// (src/main.cpp:497-504).  The kernels are lcm_sift.hip's, the arithmetic lcm_sift_device.h's, the checks, the plan and the layout
// lcm_sift_host.h's.  Here: a space's memory (allocated once, at creation), the launches of a build, the layer reads and writes, the
// two ordered compactions (candidates, survivors) with only their counts read back in between, and the one-call form on a space
// cached in the handle.  Part of liblcm_hip.so's host side; shared state and helpers: lcm_internal.h.
#include "lcm_internal.h"

#include "lcm_sift_host.h"

static_assert(sizeof(lcm_sift_params) == 64 && sizeof(lcm_sift_plan_info) == 320 && sizeof(lcm_sift_keypoint) == 32 &&
              sizeof(lcm::SiftKeypoint) == 32 && sizeof(lcm_sift_candidate) == 16 && sizeof(lcm::SiftCandidate) == 16 && sizeof(lcm::SiftLevel) == 24,
              "record sizes");
static_assert(offsetof(lcm_sift_keypoint, octave) == 20 && offsetof(lcm::SiftKeypoint, octave) == 20 && offsetof(lcm_sift_keypoint, col) == 24 &&
              offsetof(lcm::SiftKeypoint, col) == 24 && offsetof(lcm_sift_params, n_octave_layers) == 32 && offsetof(lcm_sift_plan_info, width) == 32 &&
              offsetof(lcm_sift_plan_info, radius) == 160 && offsetof(lcm_sift_plan_info, first_sigma) == 208 &&
              offsetof(lcm_sift_plan_info, space_floats) == 312, "record layouts");
static_assert(LCM_SIFT_MAX_OCTAVES == lcm::SIFT_MAX_OCTAVES && LCM_SIFT_MAX_RADIUS == lcm::SIFT_MAX_RADIUS, "limits");

struct lcm_sift_space {
    lcm_handle* h = nullptr;
    lcm_sift_params params{};
    int max_w = 0, max_h = 0, w = 0, h_img = 0;               // w == 0: nothing built yet
    lcm_sift_plan_info plan{};                                // the last build's
    lcm::SiftLevel levels[lcm::SIFT_MAX_OCTAVES]{};           // ... and its octaves, as uploaded (read by the copy until the build's wait)
    uint32_t n_blocks = 0;                                    // ... and its extrema blocks
    std::vector<uint32_t> tap0;                               // taps of layer i at d_taps + tap0[i]; the first blur's at tap0[0]
    float* d_space = nullptr;     size_t space_floats = 0;
    uint8_t* d_img = nullptr;
    float* d_taps = nullptr;
    lcm::SiftLevel* d_levels = nullptr;
    uint32_t* d_blocks = nullptr; size_t blocks_cap = 0;      // extrema: per block, then the total
    uint32_t* d_rblocks = nullptr;                            // refinement: per block of candidates, then the total
    lcm::SiftCandidate* d_cand = nullptr; size_t cand_cap = 0;
    lcm::SiftKeypoint* d_rec = nullptr;                       // one record per candidate
    lcm::SiftKeypoint* d_kp = nullptr;                        // the survivors, compacted
    uint8_t* d_kept = nullptr;
    size_t device_bytes = 0;
};

namespace {
using lcm::SiftProblem;

int sift_problem(const SiftProblem& p) { return p.what ? fail(p.code, "%s", p.what) : LCM_OK; }

int sift_no_device() {
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e == hipSuccess && ndev > 0) return LCM_OK;
    (void)hipGetLastError();
    return fail(LCM_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback", e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
}

void sift_set_info(lcm_handle* h, uint32_t launches, size_t workgroups, size_t records, size_t bytes) {
    h->info_pending = true;
    h->info.launches = launches; h->info.workgroups = (uint32_t)workgroups; h->info.route = LCM_ROUTE_PLAIN;
    h->info.pairs = records; h->info.distances = 0; h->info.algo_bytes = bytes;
}

// the DoG layers of a plan, in bytes: what an extrema search reads once
size_t sift_dog_bytes(const lcm_sift_plan_info& pl) {
    size_t px = 0;
    for (int o = 0; o < pl.n_octaves; ++o) px += (size_t)pl.width[o] * (size_t)pl.height[o];
    return px * (size_t)pl.n_dog * sizeof(float);
}

template <typename T>
int sift_alloc(lcm_sift_space* s, T*& p, size_t n) {
    HIP_TRY(hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)));
    s->device_bytes += std::max<size_t>(n, 1) * sizeof(T);
    return LCM_OK;
}

void sift_free(lcm_sift_space* s) {
    if (!s) return;
    if (s->h) { (void)hipSetDevice(s->h->device); if (s->h->stream) (void)hipStreamSynchronize(s->h->stream); }
    (void)hipFree(s->d_space); (void)hipFree(s->d_img); (void)hipFree(s->d_taps); (void)hipFree(s->d_levels); (void)hipFree(s->d_blocks);
    (void)hipFree(s->d_rblocks); (void)hipFree(s->d_cand); (void)hipFree(s->d_rec); (void)hipFree(s->d_kp); (void)hipFree(s->d_kept);
    delete s;
}

int sift_space_create_impl(lcm_handle* h, int max_w, int max_h, const lcm_sift_params* sp, lcm_sift_space** out) {
    if (!out) return fail(LCM_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    lcm_sift_params p;
    if (sp) p = *sp; else lcm::sift_params_default(&p);
    lcm_sift_plan_info big;
    int rc = sift_problem(lcm::sift_plan(max_w, max_h, p, &big)); if (rc) return rc;
    if (!h) return fail(LCM_ERR_INVALID_ARG, "NULL handle");
    rc = sift_no_device(); if (rc) return rc;
    rc = set_device(h); if (rc) return rc;
    lcm_sift_space* s = new lcm_sift_space();
    s->h = h; s->params = p; s->max_w = max_w; s->max_h = max_h;
    auto bail = [&](int code) { sift_free(s); return code; };
    // the taps of every layer, and the first blur's at the head
    std::vector<float> all, t;
    lcm::sift_taps(big.first_sigma, t);
    s->tap0.assign((size_t)big.n_gauss, 0u);
    all.insert(all.end(), t.begin(), t.end());
    for (int i = 1; i < big.n_gauss; ++i) {
        lcm::sift_taps(big.sig[i], t);
        s->tap0[(size_t)i] = (uint32_t)all.size();
        all.insert(all.end(), t.begin(), t.end());
    }
    lcm::SiftLevel levels[lcm::SIFT_MAX_OCTAVES];
    uint32_t n_blocks = 0;
    uint64_t inside = 0;
    lcm::sift_levels(big, p, levels, &n_blocks, &inside);
    s->space_floats = (size_t)big.space_floats;
    s->blocks_cap = (size_t)n_blocks + 1;
    s->cand_cap = (size_t)std::min<uint64_t>(std::max<uint64_t>(inside, 1), LCM_SIFT_MAX_CANDIDATES);
    if ((rc = sift_alloc(s, s->d_space, s->space_floats))) return bail(rc);
    if ((rc = sift_alloc(s, s->d_img, (size_t)max_w * (size_t)max_h))) return bail(rc);
    if ((rc = sift_alloc(s, s->d_taps, all.size()))) return bail(rc);
    if ((rc = sift_alloc(s, s->d_levels, (size_t)lcm::SIFT_MAX_OCTAVES))) return bail(rc);
    if ((rc = sift_alloc(s, s->d_blocks, s->blocks_cap))) return bail(rc);
    if ((rc = sift_alloc(s, s->d_rblocks, (s->cand_cap + lcm::SIFT_THREADS - 1) / lcm::SIFT_THREADS + 1))) return bail(rc);
    if ((rc = sift_alloc(s, s->d_cand, s->cand_cap))) return bail(rc);
    if ((rc = sift_alloc(s, s->d_rec, s->cand_cap))) return bail(rc);
    if ((rc = sift_alloc(s, s->d_kp, s->cand_cap))) return bail(rc);
    if ((rc = sift_alloc(s, s->d_kept, s->cand_cap))) return bail(rc);
    if (hipMemcpyAsync(s->d_taps, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
        return bail(fail(LCM_ERR_HIP, "the taps' upload failed: %s", hipGetErrorString(hipGetLastError())));
    *out = s;
    return LCM_OK;
}

int sift_build_impl(lcm_sift_space* s, const uint8_t* img, int w, int height, size_t stride) {
    if (!s) return fail(LCM_ERR_INVALID_ARG, "NULL space");
    if (!img) return fail(LCM_ERR_INVALID_ARG, "NULL image");
    if (w < 1 || height < 1 || stride < (size_t)w) return fail(LCM_ERR_INVALID_ARG, "bad image size or stride");
    if (w > s->max_w || height > s->max_h) return fail(LCM_ERR_CAPACITY, "a %d x %d image in a space made for %d x %d", w, height, s->max_w, s->max_h);
    lcm_sift_plan_info pl;
    int rc = sift_problem(lcm::sift_plan(w, height, s->params, &pl)); if (rc) return rc;
    if (pl.space_floats > s->space_floats) return fail(LCM_ERR_CAPACITY, "the image's pyramid does not fit the space");
    lcm_handle* h = s->h;
    rc = set_device(h); if (rc) return rc;
    uint64_t inside = 0;
    s->w = 0;                                                 // nothing valid until the build is through
    lcm::sift_levels(pl, s->params, s->levels, &s->n_blocks, &inside);
    if ((size_t)s->n_blocks + 1 > s->blocks_cap) return fail(LCM_ERR_CAPACITY, "the image's extrema blocks do not fit the space");
    hipStream_t st = h->stream;
    HIP_TRY(hipMemcpy2DAsync(s->d_img, (size_t)w, img, stride, (size_t)w, (size_t)height, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->d_levels, s->levels, sizeof(lcm::SiftLevel) * (size_t)pl.n_octaves, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(h->ev_start, st));
    const int n = s->params.n_octave_layers;
    uint32_t launches = 0;
    size_t groups = 0, bytes = (size_t)w * (size_t)height;
    auto layer = [&](int o, int i) { return s->d_space + lcm::sift_gauss_offset(pl, o, i); };
    auto tiles = [](int ww, int hh) { return (size_t)((ww + lcm::SIFT_TILE - 1) / lcm::SIFT_TILE) * (size_t)((hh + lcm::SIFT_TILE - 1) / lcm::SIFT_TILE); };
    hipError_t e = lcm::launch_sift_base(s->d_img, s->d_space, w, height, s->params.upsample, st);
    if (e == hipSuccess)
        e = lcm::launch_sift_blur(s->d_space, layer(0, 0), nullptr, s->d_taps + s->tap0[0], pl.base_w, pl.base_h, pl.first_radius,
                                  lcm::sift_blur_lds_bytes(pl.first_radius), st);
    launches += 2; groups += tiles(pl.base_w, pl.base_h);
    bytes += 3 * sizeof(float) * (size_t)pl.base_w * (size_t)pl.base_h;
    for (int o = 0; o < pl.n_octaves && e == hipSuccess; ++o) {
        const int ow = pl.width[o], oh = pl.height[o];
        const size_t px = (size_t)ow * (size_t)oh;
        if (o > 0) { e = lcm::launch_sift_half(layer(o - 1, n), pl.width[o - 1], layer(o, 0), ow, oh, st); ++launches; bytes += 2 * sizeof(float) * px; }
        for (int i = 1; i < pl.n_gauss && e == hipSuccess; ++i) {
            e = lcm::launch_sift_blur(layer(o, i - 1), layer(o, i), s->d_space + lcm::sift_dog_offset(pl, o, i - 1), s->d_taps + s->tap0[(size_t)i], ow, oh,
                                      pl.radius[i], lcm::sift_blur_lds_bytes(pl.radius[i]), st);
            ++launches; groups += tiles(ow, oh); bytes += 3 * sizeof(float) * px;
        }
    }
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "scale-space kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(h->ev_stop, st));
    sift_set_info(h, launches, groups, (size_t)pl.space_floats, bytes);
    HIP_TRY(hipStreamSynchronize(st));                        // the image and the levels (pageable) have been consumed
    s->plan = pl; s->w = w; s->h_img = height;
    return LCM_OK;
}

// the layer's place and size, or what is wrong with the request
int sift_layer_at(const lcm_sift_space* s, int kind, int octave, int layer, const void* buf, float** at, size_t* floats) {
    if (!s) return fail(LCM_ERR_INVALID_ARG, "NULL space");
    if (!buf) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    if (s->w == 0) return fail(LCM_ERR_INVALID_ARG, "the space holds no image yet");
    if (kind != LCM_SIFT_GAUSSIAN && kind != LCM_SIFT_DOG) return fail(LCM_ERR_INVALID_ARG, "kind must be LCM_SIFT_GAUSSIAN or LCM_SIFT_DOG");
    const int layers = kind == LCM_SIFT_GAUSSIAN ? s->plan.n_gauss : s->plan.n_dog;
    if (octave < 0 || octave >= s->plan.n_octaves || layer < 0 || layer >= layers) return fail(LCM_ERR_INVALID_ARG, "no such octave or layer");
    *at = s->d_space + (kind == LCM_SIFT_GAUSSIAN ? lcm::sift_gauss_offset(s->plan, octave, layer) : lcm::sift_dog_offset(s->plan, octave, layer));
    *floats = (size_t)s->plan.width[octave] * (size_t)s->plan.height[octave];
    return LCM_OK;
}

// The candidates of the built space into s->d_cand, in order; *n_cand read back (the one wait).  More than the space's room:
// LCM_ERR_CAPACITY before the emit.
int sift_extrema_run(lcm_sift_space* s, uint32_t* n_cand, uint32_t* launches) {
    lcm_handle* h = s->h;
    const lcm_sift_params& p = s->params;
    const float T = lcm::sift_threshold(p);
    *n_cand = 0; *launches = 0;
    if (s->n_blocks == 0) return LCM_OK;
    hipError_t e = lcm::launch_sift_extrema(s->d_space, s->d_levels, s->plan.n_octaves, p.n_octave_layers, p.border, T, s->d_blocks, s->n_blocks,
                                            s->d_cand, 0, false, h->stream);
    if (e == hipSuccess) e = lcm::launch_block_scan(s->d_blocks, s->n_blocks, s->d_blocks + s->n_blocks, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "extrema count kernels: launch failed: %s", hipGetErrorString(e));
    *launches = 2;
    HIP_TRY(hipMemcpyAsync(n_cand, s->d_blocks + s->n_blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (*n_cand > s->cand_cap) return fail(LCM_ERR_CAPACITY, "%u candidates but the space has room for %zu", *n_cand, s->cand_cap);
    if (*n_cand == 0) return LCM_OK;
    e = lcm::launch_sift_extrema(s->d_space, s->d_levels, s->plan.n_octaves, p.n_octave_layers, p.border, T, s->d_blocks, s->n_blocks, s->d_cand,
                                 (uint32_t)s->cand_cap, true, h->stream);
    if (e != hipSuccess) return fail(LCM_ERR_HIP, "extrema kernel launch failed: %s", hipGetErrorString(e));
    *launches = 3;
    return LCM_OK;
}

int sift_extrema_impl(lcm_sift_space* s, lcm_sift_candidate* cand, size_t cap, size_t* n) {
    if (!s || !n) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (cap > 0 && !cand) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    if (s->w == 0) return fail(LCM_ERR_INVALID_ARG, "the space holds no image yet");
    lcm_handle* h = s->h;
    int rc = set_device(h); if (rc) return rc;
    uint32_t found = 0, launches = 0;
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    rc = sift_extrema_run(s, &found, &launches);
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    sift_set_info(h, launches, s->n_blocks, found, sift_dog_bytes(s->plan) + (size_t)found * sizeof(lcm_sift_candidate));
    *n = found;
    if (rc) return rc;
    if (found > cap) return fail(LCM_ERR_CAPACITY, "%u candidates but room for %zu", found, cap);
    if (found) HIP_TRY(hipMemcpyAsync(cand, s->d_cand, (size_t)found * sizeof(lcm_sift_candidate), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return LCM_OK;
}

int sift_detect_impl(lcm_sift_space* s, lcm_sift_keypoint* kp, size_t cap, size_t* n, size_t* n_candidates) {
    if (!s || !n) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (cap > 0 && !kp) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    if (s->w == 0) return fail(LCM_ERR_INVALID_ARG, "the space holds no image yet");
    lcm_handle* h = s->h;
    int rc = set_device(h); if (rc) return rc;
    uint32_t found = 0, kept = 0, launches = 0;
    *n = 0;
    if (n_candidates) *n_candidates = 0;
    HIP_TRY(hipEventRecord(h->ev_start, h->stream));
    rc = sift_extrema_run(s, &found, &launches);
    if (n_candidates) *n_candidates = found;
    const uint32_t r_blocks = (found + lcm::SIFT_THREADS - 1) / lcm::SIFT_THREADS;
    if (rc == LCM_OK && found) {
        hipError_t e = lcm::launch_sift_refine(s->d_space, s->d_levels, s->d_cand, found, lcm::sift_refine_consts(s->params), s->d_rec, s->d_kept,
                                               s->d_rblocks, h->stream);
        if (e == hipSuccess) e = lcm::launch_block_scan(s->d_rblocks, r_blocks, s->d_rblocks + r_blocks, h->stream);
        if (e != hipSuccess) return fail(LCM_ERR_HIP, "refinement kernels: launch failed: %s", hipGetErrorString(e));
        launches += 2;
        HIP_TRY(hipMemcpyAsync(&kept, s->d_rblocks + r_blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (kept > found) return fail(LCM_ERR_HIP, "%u survivors of %u candidates", kept, found);
        *n = kept;
        if (kept > cap) rc = fail(LCM_ERR_CAPACITY, "%u keypoints but room for %zu", kept, cap);
        else if (kept) {
            e = lcm::launch_sift_compact(s->d_rec, s->d_kept, s->d_rblocks, found, s->d_kp, h->stream);
            if (e != hipSuccess) return fail(LCM_ERR_HIP, "compaction kernel launch failed: %s", hipGetErrorString(e));
            ++launches;
        }
    }
    HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
    sift_set_info(h, launches, (size_t)s->n_blocks + r_blocks, found, sift_dog_bytes(s->plan) + (size_t)found * (2 * 16 + 32 + 2 + 32) + (size_t)kept * 32);
    if (rc) return rc;
    if (kept) HIP_TRY(hipMemcpyAsync(kp, s->d_kp, (size_t)kept * sizeof(lcm_sift_keypoint), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return LCM_OK;
}

int sift_detect_image_impl(lcm_handle* h, const uint8_t* img, int w, int height, size_t stride, const lcm_sift_params* sp, lcm_sift_keypoint* kp,
                           size_t cap, size_t* n) {
    if (!n) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    if (!img || (cap > 0 && !kp)) return fail(LCM_ERR_INVALID_ARG, "NULL buffer");
    if (stride < (size_t)(w > 0 ? w : 0)) return fail(LCM_ERR_INVALID_ARG, "bad image size or stride");
    lcm_sift_params p;
    if (sp) p = *sp; else lcm::sift_params_default(&p);
    lcm_sift_plan_info pl;
    int rc = sift_problem(lcm::sift_plan(w, height, p, &pl)); if (rc) return rc;
    if (!h) return fail(LCM_ERR_INVALID_ARG, "NULL handle");
    rc = sift_no_device(); if (rc) return rc;
    lcm_sift_space* s = h->sift_cached;
    if (!s || std::memcmp(&s->params, &p, sizeof(p)) != 0 || w > s->max_w || height > s->max_h) {
        const bool grow = s && std::memcmp(&s->params, &p, sizeof(p)) == 0;       // the same detector, a larger image: room for both
        const int mw = grow ? std::max(w, s->max_w) : w, mh = grow ? std::max(height, s->max_h) : height;
        h->sift_cached = nullptr;
        sift_free(s);
        s = nullptr;
        rc = sift_space_create_impl(h, mw, mh, &p, &s); if (rc) return rc;
        h->sift_cached = s;
    }
    rc = sift_build_impl(s, img, w, height, stride); if (rc) return rc;
    return sift_detect_impl(s, kp, cap, n, nullptr);
}

}  // namespace

extern "C" {

void lcm_sift_params_default(lcm_sift_params* p) { if (p) lcm::sift_params_default(p); }
int lcm_sift_plan(int w, int h, const lcm_sift_params* sp, lcm_sift_plan_info* out) {
    return guarded([&] {
        if (!out) return fail(LCM_ERR_INVALID_ARG, "out is NULL");
        lcm_sift_params p;
        if (sp) p = *sp; else lcm::sift_params_default(&p);
        lcm_sift_plan_info pl;
        const int rc = sift_problem(lcm::sift_plan(w, h, p, &pl)); if (rc) return rc;
        *out = pl;
        return (int)LCM_OK;
    });
}
int lcm_sift_plan_read(int w, int h, const lcm_sift_params* sp, int layer, float* taps, int cap, int* n_taps) {
    return guarded([&] {
        if (!n_taps || cap < 0 || (cap > 0 && !taps)) return fail(LCM_ERR_INVALID_ARG, "bad argument");
        lcm_sift_params p;
        if (sp) p = *sp; else lcm::sift_params_default(&p);
        lcm_sift_plan_info pl;
        const int rc = sift_problem(lcm::sift_plan(w, h, p, &pl)); if (rc) return rc;
        if (layer != -1 && (layer < 1 || layer >= pl.n_gauss)) return fail(LCM_ERR_INVALID_ARG, "no such layer");
        std::vector<float> t;
        lcm::sift_taps(layer == -1 ? pl.first_sigma : pl.sig[layer], t);
        *n_taps = (int)t.size();
        if ((int)t.size() > cap) return fail(LCM_ERR_CAPACITY, "%zu taps but room for %d", t.size(), cap);
        std::memcpy(taps, t.data(), t.size() * sizeof(float));
        return (int)LCM_OK;
    });
}
int lcm_sift_space_create(lcm_handle* h, int max_w, int max_h, const lcm_sift_params* sp, lcm_sift_space** out) {
    return guarded([&] { return sift_space_create_impl(h, max_w, max_h, sp, out); });
}
void lcm_sift_space_destroy(lcm_sift_space* s) { sift_free(s); }
int lcm_sift_space_build(lcm_sift_space* s, const uint8_t* img, int w, int h, size_t stride) {
    return guarded([&] { return sift_build_impl(s, img, w, h, stride); });
}
int lcm_sift_space_info(const lcm_sift_space* s, lcm_sift_space_info_t* out) {
    if (!s || !out) return fail(LCM_ERR_INVALID_ARG, "bad argument");
    std::memset(out, 0, sizeof(*out));
    out->max_w = s->max_w; out->max_h = s->max_h; out->w = s->w; out->h = s->w ? s->h_img : 0;
    out->device_bytes = s->device_bytes; out->candidate_capacity = s->cand_cap;
    if (s->w) out->plan = s->plan;
    return LCM_OK;
}
int lcm_sift_space_read(lcm_sift_space* s, int kind, int octave, int layer, float* out) {
    return guarded([&] {
        float* at = nullptr;
        size_t floats = 0;
        int rc = sift_layer_at(s, kind, octave, layer, out, &at, &floats); if (rc) return rc;
        rc = set_device(s->h); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(out, at, floats * sizeof(float), hipMemcpyDeviceToHost, s->h->stream));
        HIP_TRY(hipStreamSynchronize(s->h->stream));
        return (int)LCM_OK;
    });
}
int lcm_sift_space_write(lcm_sift_space* s, int kind, int octave, int layer, const float* in) {
    return guarded([&] {
        float* at = nullptr;
        size_t floats = 0;
        int rc = sift_layer_at(s, kind, octave, layer, in, &at, &floats); if (rc) return rc;
        rc = set_device(s->h); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(at, in, floats * sizeof(float), hipMemcpyHostToDevice, s->h->stream));
        HIP_TRY(hipStreamSynchronize(s->h->stream));
        return (int)LCM_OK;
    });
}
int lcm_sift_extrema(lcm_sift_space* s, lcm_sift_candidate* cand, size_t cap, size_t* n) {
    return guarded([&] { return sift_extrema_impl(s, cand, cap, n); });
}
int lcm_sift_detect(lcm_sift_space* s, lcm_sift_keypoint* kp, size_t cap, size_t* n, size_t* n_candidates) {
    return guarded([&] { return sift_detect_impl(s, kp, cap, n, n_candidates); });
}
int lcm_sift_detect_image(lcm_handle* h, const uint8_t* img, int w, int height, size_t stride, const lcm_sift_params* sp, lcm_sift_keypoint* kp,
                          size_t cap, size_t* n) {
    return guarded([&] { return sift_detect_image_impl(h, img, w, height, stride, sp, kp, cap, n); });
}

}  // extern "C"

namespace lcm {
void sift_cached_destroy(lcm_handle* h) { sift_free(h->sift_cached); h->sift_cached = nullptr; }
}  // namespace lcm
