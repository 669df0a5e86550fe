// The pure host side of the essential-matrix RANSAC (csrc/lcm_epi_host.h: parameter checks, the loop verdict, the walk over
// a call's offsets, the records of an empty call) as a stand-alone program: tests/test_epi_abi_host.py builds it with
// -fsanitize=address,undefined and runs it on the CPU.  No HIP, no device.  Exit status 0 = every check held.
#include <cstdio>
#include <limits>
#include <vector>

#include "lcm_epi_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    lcm_epi_params ep;
    std::memset(&ep, 0xAB, sizeof(ep));
    lcm::epi_params_default(&ep);
    CHECK(ep.fx == 0.0 && ep.fy == 0.0 && ep.cx == 0.0 && ep.cy == 0.0 && ep.threshold == 1.0 && ep.min_ratio == 0.6);
    CHECK(ep.iters == 1024 && ep.min_inliers == 200 && ep.seed == 0 && ep.reserved == 0);
    CHECK(lcm::epi_params_problem(nullptr) != nullptr);
    CHECK(lcm::epi_params_problem(&ep) != nullptr);                       // K left zero
    ep.fx = ep.fy = 700.0; ep.cx = 320.0; ep.cy = 240.0;
    CHECK(lcm::epi_params_problem(&ep) == nullptr);
    CHECK(lcm::epi_t2(ep) == (1.0 / 700.0) * (1.0 / 700.0));
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (double bad : {0.0, -1.0, nan, inf}) {
        lcm_epi_params q = ep; q.fx = bad; CHECK(lcm::epi_params_problem(&q) != nullptr);
        q = ep; q.fy = bad; CHECK(lcm::epi_params_problem(&q) != nullptr);
    }
    for (double bad : {nan, inf, -inf}) {
        lcm_epi_params q = ep; q.cx = bad; CHECK(lcm::epi_params_problem(&q) != nullptr);
        q = ep; q.threshold = bad; CHECK(lcm::epi_params_problem(&q) != nullptr);
    }
    { lcm_epi_params q = ep; q.threshold = -0.5; CHECK(lcm::epi_params_problem(&q) != nullptr); }
    { lcm_epi_params q = ep; q.min_ratio = nan; CHECK(lcm::epi_params_problem(&q) != nullptr); }
    for (int bad : {0, -64, 63, 65, 100, 65536 + 64, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()}) {
        lcm_epi_params q = ep; q.iters = bad; CHECK(lcm::epi_params_problem(&q) != nullptr);
    }
    for (int good : {64, 128, 1024, 65536}) { lcm_epi_params q = ep; q.iters = good; CHECK(lcm::epi_params_problem(&q) == nullptr); }

    // the verdict: both comparisons strict (src/main.cpp:1403)
    lcm_epi_result r;
    std::memset(&r, 0, sizeof(r));
    r.n_points = 300; r.n_inliers = 200; CHECK(lcm::epi_loop_test(&r, &ep) == 0);
    r.n_inliers = 201; CHECK(lcm::epi_loop_test(&r, &ep) == 1);
    ep.min_inliers = 100;
    r.n_points = 200; r.n_inliers = 120; CHECK(lcm::epi_loop_test(&r, &ep) == 0);          // exactly 0.6
    r.n_inliers = 121; CHECK(lcm::epi_loop_test(&r, &ep) == 1);
    r.n_points = 0; r.n_inliers = 0; CHECK(lcm::epi_loop_test(&r, &ep) == 0);
    r.n_points = std::numeric_limits<int32_t>::max(); r.n_inliers = r.n_points; CHECK(lcm::epi_loop_test(&r, &ep) == 1);
    CHECK(lcm::epi_loop_test(nullptr, &ep) == 0 && lcm::epi_loop_test(&r, nullptr) == 0);

    // the offsets walk
    size_t total = 99;
    uint32_t max_n = 99;
    bool cap = true;
    CHECK(lcm::epi_offsets_problem(nullptr, 1, 65535, &total, &max_n, &cap) != nullptr && total == 0 && max_n == 0 && !cap);
    std::vector<size_t> offs{0};
    CHECK(lcm::epi_offsets_problem(offs.data(), 0, 65535, &total, &max_n, &cap) == nullptr && total == 0 && max_n == 0);
    CHECK(lcm::epi_offsets_problem(offs.data(), -1, 65535, &total, &max_n, &cap) != nullptr);
    offs = {0, 400, 400, 407, 65942};
    CHECK(lcm::epi_offsets_problem(offs.data(), 4, 65535, &total, &max_n, &cap) == nullptr && total == 65942 && max_n == 65535 && !cap);
    offs.back() += 1;
    CHECK(lcm::epi_offsets_problem(offs.data(), 4, 65535, &total, &max_n, &cap) != nullptr && cap);
    offs = {0, 10, 9};
    CHECK(lcm::epi_offsets_problem(offs.data(), 2, 65535, &total, &max_n, &cap) != nullptr && !cap);
    offs = {1, 10};
    CHECK(lcm::epi_offsets_problem(offs.data(), 1, 65535, &total, &max_n, &cap) != nullptr);
    offs = {0, std::numeric_limits<size_t>::max()};
    CHECK(lcm::epi_offsets_problem(offs.data(), 1, 65535, &total, &max_n, &cap) != nullptr && cap);

    // the records of a call that launches nothing
    std::vector<lcm_epi_result> res(5);
    std::memset(res.data(), 0xCD, res.size() * sizeof(lcm_epi_result));
    lcm::epi_empty_results(res.data(), 4);
    for (int p = 0; p < 4; ++p) {
        for (double e : res[(size_t)p].E) CHECK(e == 0.0);
        CHECK(res[(size_t)p].n_points == 0 && res[(size_t)p].n_inliers == 0 && res[(size_t)p].best_iter == 0 && res[(size_t)p].status == LCM_EPI_TOO_FEW);
    }
    CHECK(reinterpret_cast<const unsigned char*>(&res[4])[0] == 0xCD);    // not one record more
    lcm::epi_empty_results(nullptr, 0);

    std::printf(failures ? "%d check(s) failed\n" : "epi host checks: all held\n", failures);
    return failures ? 1 : 0;
}
