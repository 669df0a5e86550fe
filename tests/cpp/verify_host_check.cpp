// The pure host side of the loop verification's plan (csrc/lcm_verify_host.h: what a call with a plan must be given, the
// records of a call that launches nothing) as a stand-alone program: tests/test_verify_host.py builds it with
// -fsanitize=address,undefined and runs it on the CPU.  No HIP runtime, no device.  Exit status 0 = every check held.
#include <cstdio>
#include <cstring>
#include <vector>

#include "lcm_verify_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static const char* const PTS_RESULTS = "the verification needs pts and results";
static const char* const POSE_RESULTS = "the pose recovery needs pose_results";
static const char* const INFO = "the optimisation needs info";

static bool is(const char* got, const char* want) { return want ? (got && std::strcmp(got, want) == 0) : got == nullptr; }

int main() {
    lcm_epi_params ep;
    lcm::epi_params_default(&ep);
    ep.fx = ep.fy = 700.0; ep.cx = 320.0; ep.cy = 240.0;
    std::vector<lcm_epi_result> res(3);
    std::vector<lcm_lo_info> info(3);
    std::vector<lcm_pose_result> pres(3);
    std::vector<lcm_point_pair> pts(4);
    std::vector<uint8_t> mask(4), pmask(4);

    struct Stages { bool lo, pose; };
    for (const Stages st : {Stages{false, false}, Stages{false, true}, Stages{true, true}}) {
        const lcm::VerifyPlan full{&ep, st.lo, st.pose, res.data(), mask.data(), st.lo ? info.data() : nullptr,
                                   st.pose ? pres.data() : nullptr, st.pose ? pmask.data() : nullptr};
        for (const size_t n : {(size_t)1, (size_t)3}) {
            CHECK(is(lcm::verify_plan_problem(full, pts.data(), n), nullptr));
            // the masks are optional
            lcm::VerifyPlan p = full;
            p.mask = nullptr; p.pose_mask = nullptr;
            CHECK(is(lcm::verify_plan_problem(p, pts.data(), n), nullptr));
            // one output missing at a time: a stage that is off needs nothing
            p = full; p.results = nullptr;
            CHECK(is(lcm::verify_plan_problem(p, pts.data(), n), PTS_RESULTS));
            p = full; p.pose_results = nullptr;
            CHECK(is(lcm::verify_plan_problem(p, pts.data(), n), st.pose ? POSE_RESULTS : nullptr));
            p = full; p.info = nullptr;
            CHECK(is(lcm::verify_plan_problem(p, pts.data(), n), st.lo ? INFO : nullptr));
            CHECK(is(lcm::verify_plan_problem(full, nullptr, n), PTS_RESULTS));
            // the precedence: pts / results, then pose_results, then info
            p = full; p.results = nullptr; p.pose_results = nullptr; p.info = nullptr;
            CHECK(is(lcm::verify_plan_problem(p, pts.data(), n), PTS_RESULTS));
            CHECK(is(lcm::verify_plan_problem(p, nullptr, n), PTS_RESULTS));
            p.results = res.data();
            CHECK(is(lcm::verify_plan_problem(p, nullptr, n), PTS_RESULTS));
            CHECK(is(lcm::verify_plan_problem(p, pts.data(), n), st.pose ? POSE_RESULTS : nullptr));
            p.pose_results = pres.data();
            CHECK(is(lcm::verify_plan_problem(p, pts.data(), n), st.lo ? INFO : nullptr));
            // the RANSAC's parameters come before every buffer
            p.ep = nullptr;
            CHECK(is(lcm::verify_plan_problem(p, nullptr, n), lcm::epi_params_problem(nullptr)));
            lcm_epi_params bad = ep;
            bad.iters = 65;
            p.ep = &bad; p.results = nullptr;
            CHECK(is(lcm::verify_plan_problem(p, pts.data(), n), lcm::epi_params_problem(&bad)) && lcm::epi_params_problem(&bad) != nullptr);
        }
        // no outputs: nothing but pts is required
        lcm::VerifyPlan none{&ep, st.lo, st.pose, nullptr, nullptr};
        CHECK(is(lcm::verify_plan_problem(none, pts.data(), 0), nullptr));
        CHECK(is(lcm::verify_plan_problem(none, nullptr, 0), PTS_RESULTS));
        CHECK(is(lcm::verify_plan_problem(full, nullptr, 0), PTS_RESULTS));
        none.ep = nullptr;
        CHECK(is(lcm::verify_plan_problem(none, pts.data(), 0), lcm::epi_params_problem(nullptr)));

        // the records of a call that launches nothing: the stages present, and only their buffers
        std::memset(res.data(), 0xA7, res.size() * sizeof(lcm_epi_result));
        std::memset(info.data(), 0xA7, info.size() * sizeof(lcm_lo_info));
        std::memset(pres.data(), 0xA7, pres.size() * sizeof(lcm_pose_result));
        lcm::VerifyPlan p = full;
        if (!st.lo) p.info = nullptr;                       // a stage that is off is not written, whatever its pointer
        if (!st.pose) p.pose_results = nullptr;
        lcm::verify_empty(p, 2);
        std::vector<lcm_epi_result> er(2);
        std::vector<lcm_lo_info> ei(2);
        std::vector<lcm_pose_result> epr(2);
        lcm::epi_empty_results(er.data(), 2);
        lcm::lo_empty_info(ei.data(), 2);
        lcm::pose_empty_results(epr.data(), 2);
        const std::vector<uint8_t> fill(128, 0xA7);
        CHECK(std::memcmp(res.data(), er.data(), 2 * sizeof(lcm_epi_result)) == 0 && std::memcmp(&res[2], fill.data(), sizeof(lcm_epi_result)) == 0);
        CHECK(std::memcmp(info.data(), st.lo ? (const void*)ei.data() : fill.data(), 2 * sizeof(lcm_lo_info)) == 0);
        CHECK(std::memcmp(&info[2], fill.data(), sizeof(lcm_lo_info)) == 0);
        CHECK(std::memcmp(pres.data(), st.pose ? (const void*)epr.data() : fill.data(), sizeof(lcm_pose_result)) == 0);
        CHECK(std::memcmp(&pres[1], st.pose ? (const void*)&epr[1] : fill.data(), sizeof(lcm_pose_result)) == 0);
        CHECK(std::memcmp(&pres[2], fill.data(), sizeof(lcm_pose_result)) == 0);
        lcm::verify_empty(none, 0);                         // nothing to write: NULL buffers are fine
    }
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all held\n");
    return 0;
}
