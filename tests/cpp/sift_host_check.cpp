// sift_host_check.cpp — csrc/lcm_sift_host.h and csrc/lcm_sift_device.h as a stand-alone program (plain C++, no HIP runtime linked),
// built with ASan + UBSan by tests/test_sift_host.py.  It replays the file that test wrote from tests/siftcases.py: per case a
// planted DoG stack, the candidates and what tests/siftref.py makes of them; the search and the refinement compiled here from the
// device's own text must give the same candidates, the same reasons and the same 32-byte records, bit for bit.  Then an image and
// its 2x enlargement, the fold against a mirror walk, the plan's layout and the blur's LDS bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lcm_sift_host.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

template <typename T>
static bool take(FILE* f, T* out, size_t n) { return std::fread(out, sizeof(T), n, f) == n; }

// the index a walk over the mirrored line reaches: step by step, turning at both ends without repeating them
static int mirror_walk(int i, int n) {
    if (n == 1) return 0;
    int at = 0, dir = 1;
    for (int k = 0; k < (i < 0 ? -i : i); ++k) {
        if (at + dir < 0 || at + dir >= n) dir = -dir;
        at += dir;
    }
    return at;                                   // the line is symmetric about 0: -i reaches what i does
}

static void replay_case(FILE* f, int index) {
    lcm_sift_params p;
    int32_t dims[4];
    CHECK(take(f, &p, 1) && take(f, dims, 4));
    const int w = dims[0], h = dims[1], octave = dims[2], n_cand = dims[3], n = p.n_octave_layers;
    CHECK(lcm::sift_params_problem(p) == nullptr);
    std::vector<float> d((size_t)(n + 2) * (size_t)w * (size_t)h);
    std::vector<lcm::SiftCandidate> cand((size_t)n_cand);
    std::vector<int32_t> reasons((size_t)n_cand);
    int32_t n_kept = 0;
    CHECK(take(f, d.data(), d.size()) && take(f, cand.data(), cand.size()) && take(f, reasons.data(), reasons.size()) && take(f, &n_kept, 1));
    std::vector<lcm::SiftKeypoint> want((size_t)n_kept);
    CHECK(take(f, want.data(), want.size()));
    // the search, in the linear order
    const float T = lcm::sift_threshold(p);
    const size_t plane = (size_t)w * (size_t)h;
    size_t found = 0;
    for (int l = 1; l <= n; ++l)
        for (int r = p.border; r < h - p.border; ++r)
            for (int c = p.border; c < w - p.border; ++c)
                if (lcm::sift_is_extremum(d.data() + plane * (size_t)l + (size_t)r * (size_t)w + (size_t)c, plane, w, T)) {
                    if (found < cand.size()) CHECK(cand[found].octave == octave && cand[found].layer == l && cand[found].row == r && cand[found].col == c);
                    ++found;
                }
    CHECK(found == cand.size());
    // the refinement
    const lcm::SiftRefine k = lcm::sift_refine_consts(p);
    size_t kept = 0;
    for (size_t i = 0; i < cand.size(); ++i) {
        lcm::SiftKeypoint kp;
        std::memset(&kp, 0, sizeof(kp));
        const int why = lcm::sift_refine(d.data(), w, h, octave, cand[i].layer, cand[i].row, cand[i].col, k, kp);
        CHECK(why == reasons[i]);
        if (why == lcm::SIFT_KEPT) {
            if (kept < want.size()) CHECK(std::memcmp(&kp, &want[kept], sizeof(kp)) == 0);
            ++kept;
        }
    }
    CHECK(kept == want.size());
    std::printf("case %d: %d x %d, %d layers, %d candidates, %zu kept\n", index, w, h, n, n_cand, kept);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: sift_host_check <replay file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    int32_t head[2];
    CHECK(take(f, head, 2) && head[0] == 0x53494654);
    for (int i = 0; i < head[1] && failures == 0; ++i) replay_case(f, i);
    // an image and its enlargement
    int32_t iw = 0, ih = 0, stride = 0;
    CHECK(take(f, &iw, 1) && take(f, &ih, 1) && take(f, &stride, 1));
    std::vector<uint8_t> img((size_t)ih * (size_t)stride);
    std::vector<float> big((size_t)4 * (size_t)iw * (size_t)ih);
    CHECK(take(f, img.data(), img.size()) && take(f, big.data(), big.size()));
    for (int y = 0; y < 2 * ih; ++y)
        for (int x = 0; x < 2 * iw; ++x) {
            const float v = lcm::sift_upsampled(img.data(), (size_t)stride, iw, ih, x, y);
            if (std::memcmp(&v, &big[(size_t)y * (size_t)(2 * iw) + (size_t)x], 4) != 0) { CHECK(!"enlarged pixel"); y = 2 * ih; break; }
        }
    std::fclose(f);
    // the fold against the mirror walk
    for (int n = 1; n <= 8; ++n)
        for (int i = -40; i <= 40 + n; ++i) CHECK(lcm::sift_fold(i, n) == mirror_walk(i, n));
    // the solve: a diagonal system, a permuted one (the pivot comes up from the last row), a zero pivot
    float x0, x1, x2;
    CHECK(lcm::sift_solve3(2, 0, 0, 0, 4, 0, 0, 0, 8, 2, 4, 8, x0, x1, x2) && x0 == 1.0f && x1 == 1.0f && x2 == 1.0f);
    CHECK(lcm::sift_solve3(0, 0, 1, 0, 1, 0, 1, 0, 0, 3, 2, 1, x0, x1, x2) && x0 == 1.0f && x1 == 2.0f && x2 == 3.0f);
    CHECK(!lcm::sift_solve3(1, 2, 3, 2, 4, 6, 1, 1, 1, 1, 1, 1, x0, x1, x2));
    CHECK(!lcm::sift_solve3(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, x0, x1, x2));
    CHECK(lcm::sift_pow2(0.0f) == 1.0f && lcm::sift_pow2(1.0f) == 2.0f && lcm::sift_pow2(2.0f) == 4.0f);
    // the plan: the defaults at 640 x 480, by hand; the layout has no gaps; the refusals
    lcm_sift_params p;
    lcm::sift_params_default(&p);
    lcm_sift_plan_info pl;
    CHECK(lcm::sift_plan(640, 480, p, &pl).what == nullptr && pl.n_octaves == 9 && pl.n_gauss == 6 && pl.n_dog == 5 && pl.base_w == 1280 &&
          pl.base_h == 960 && pl.width[8] == 5 && pl.height[8] == 3 && pl.max_radius == 13 && pl.first_radius == 5 && pl.radius[1] == 5);
    uint64_t at = (uint64_t)pl.base_w * pl.base_h;
    for (int o = 0; o < pl.n_octaves; ++o) {
        for (int i = 0; i < pl.n_gauss; ++i) { CHECK(lcm::sift_gauss_offset(pl, o, i) == at); at += (uint64_t)pl.width[o] * pl.height[o]; }
        for (int i = 0; i < pl.n_dog; ++i) { CHECK(lcm::sift_dog_offset(pl, o, i) == at); at += (uint64_t)pl.width[o] * pl.height[o]; }
    }
    CHECK(at == pl.space_floats);
    lcm::SiftLevel levels[lcm::SIFT_MAX_OCTAVES];
    uint32_t n_blocks = 0;
    uint64_t inside = 0;
    lcm::sift_levels(pl, p, levels, &n_blocks, &inside);
    CHECK(levels[0].block0 == 0 && levels[1].block0 == (3u * 1280u * 960u + 255u) / 256u && levels[8].w == 5 && inside > 0 && n_blocks > levels[8].block0);
    CHECK(lcm::sift_plan(4, 4, p, &pl).code == LCM_OK && lcm::sift_plan(4097, 8, p, &pl).code == LCM_ERR_CAPACITY);
    p.upsample = 0;
    CHECK(lcm::sift_plan(5, 5, p, &pl).code == LCM_ERR_INVALID_ARG);          // no octave
    p.n_octave_layers = 1; p.sigma = 2.0;
    CHECK(lcm::sift_plan(64, 64, p, &pl).code == LCM_ERR_CAPACITY);           // a radius above 48
    lcm::sift_params_default(&p);
    p.sigma = -1.0;
    CHECK(lcm::sift_plan(64, 64, p, &pl).code == LCM_ERR_INVALID_ARG);
    std::vector<float> t;
    lcm::sift_taps(1.6, t);
    CHECK(t.size() == 15);
    for (size_t j = 0; j < t.size(); ++j) CHECK(t[j] == t[t.size() - 1 - j] && t[j] > 0.0f);
    CHECK(lcm::sift_threshold(p) == 1.0f);
    CHECK(lcm::sift_blur_lds_bytes(13) == (58u * 58u + 58u * 32u) * 4u && lcm::sift_blur_lds_bytes(lcm::SIFT_MAX_RADIUS) == 81920u);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all held\n");
    return 0;
}
