// The pure host side of the relative-pose recovery (csrc/lcm_pose_host.h: parameter checks, the pose verdict, the choice of
// the best loop, the records of an empty call) and the arithmetic of csrc/lcm_pose_device.h compiled for the host, as a
// stand-alone program: tests/test_pose_abi_host.py builds it with -fsanitize=address,undefined and runs it on the CPU.  No
// device.  With a file name it also replays the cases tests/poseref.py has written there and compares bit for bit:
//   int64 n_pairs, total, has_mask | double fx, fy, cx, cy, max_depth | uint64 offsets[n_pairs + 1] | float pts[total][4] |
//   double E[n_pairs][9] | uint8 mask_in[total] | lcm_pose_result want[n_pairs] | uint8 want_mask[total] |
//   double want_R4[n_pairs][36] | double want_t4[n_pairs][12]
// Exit status 0 = every check held.
#include <cstdio>
#include <limits>
#include <vector>

#include "lcm_pose_device.h"
#include "lcm_pose_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static_assert(sizeof(lcm::PoseResult) == sizeof(lcm_pose_result) && sizeof(lcm_pose_result) == 128 && sizeof(lcm_pose_params) == 32, "sizes");

// k_pose_recover's two passes over one pair, serially
static void recover(const float* pts, size_t n, const double* E9, const uint8_t* mask_in, const double* K, double max_depth,
                    lcm_pose_result* res, uint8_t* mask_out, double* R4, double* t4) {
    double e[9], ra[9], rb[9], t[3];
    for (int k = 0; k < 9; ++k) e[k] = E9[k];
    const bool ok = lcm::pose_decompose(e, ra, rb, t);
    for (int k = 0; k < 4; ++k) {
        double r[9], tk[3];
        lcm::pose_candidate(k, ra, rb, t, r, tk);
        for (int i = 0; i < 9; ++i) R4[9 * k + i] = r[i];
        for (int i = 0; i < 3; ++i) t4[3 * k + i] = ok ? tk[i] : 0.0;
    }
    std::memset(res, 0, sizeof(*res));
    if (!ok) {
        for (size_t i = 0; i < n; ++i) mask_out[i] = 0;
        res->choice = -1; res->status = LCM_POSE_NO_MODEL;
        return;
    }
    uint32_t c[4] = {0, 0, 0, 0}, used = 0;
    std::vector<double> x(4 * n);
    for (size_t i = 0; i < n; ++i) {
        x[4 * i + 0] = lcm::epi_norm(pts[4 * i + 0], K[2], K[0]); x[4 * i + 1] = lcm::epi_norm(pts[4 * i + 1], K[3], K[1]);
        x[4 * i + 2] = lcm::epi_norm(pts[4 * i + 2], K[2], K[0]); x[4 * i + 3] = lcm::epi_norm(pts[4 * i + 3], K[3], K[1]);
        if (mask_in && mask_in[i] == 0) continue;
        c[0] += lcm::pose_in_front(ra, t[0], t[1], t[2], x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3], max_depth);
        c[1] += lcm::pose_in_front(rb, t[0], t[1], t[2], x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3], max_depth);
        c[2] += lcm::pose_in_front(ra, -t[0], -t[1], -t[2], x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3], max_depth);
        c[3] += lcm::pose_in_front(rb, -t[0], -t[1], -t[2], x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3], max_depth);
        ++used;
    }
    const int choice = lcm::pose_choose(c[0], c[1], c[2], c[3]);
    double rk[9], tk[3];
    lcm::pose_candidate(choice, ra, rb, t, rk, tk);
    for (size_t i = 0; i < n; ++i)
        mask_out[i] = (!mask_in || mask_in[i] != 0) &&
                      lcm::pose_in_front(rk, tk[0], tk[1], tk[2], x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3], max_depth);
    for (int i = 0; i < 9; ++i) res->R[i] = rk[i];
    for (int i = 0; i < 3; ++i) res->t[i] = tk[i];
    for (int k = 0; k < 4; ++k) res->counts[k] = (int32_t)c[k];
    res->n_used = (int32_t)used; res->n_good = (int32_t)c[choice]; res->choice = choice; res->status = LCM_POSE_OK;
}

template <typename T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

static void replay(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    CHECK(f != nullptr);
    if (!f) return;
    std::vector<int64_t> head;
    std::vector<double> cam, E, wR4, wt4;
    std::vector<uint64_t> offs;
    std::vector<float> pts;
    std::vector<uint8_t> mask_in, want_mask;
    std::vector<lcm_pose_result> want;
    bool ok = read_n(f, head, 3) && head[0] >= 0 && head[1] >= 0 && read_n(f, cam, 5);
    const size_t P = ok ? (size_t)head[0] : 0, total = ok ? (size_t)head[1] : 0;
    ok = ok && read_n(f, offs, P + 1) && read_n(f, pts, total * 4) && read_n(f, E, P * 9) && read_n(f, mask_in, total) &&
         read_n(f, want, P) && read_n(f, want_mask, total) && read_n(f, wR4, P * 36) && read_n(f, wt4, P * 12);
    std::fclose(f);
    CHECK(ok);
    if (!ok) return;
    CHECK(offs[0] == 0 && offs[P] == total);
    std::vector<uint8_t> got_mask(total + 1, 0xA7);
    size_t bad_res = 0, bad_mask = 0, bad_cand = 0;
    for (size_t p = 0; p < P; ++p) {
        const size_t lo = (size_t)offs[p], n = (size_t)(offs[p + 1] - offs[p]);
        CHECK(offs[p + 1] >= offs[p] && offs[p + 1] <= total);
        if (offs[p + 1] < offs[p] || offs[p + 1] > total) return;
        lcm_pose_result r;
        double R4[36], t4[12];
        recover(pts.data() + 4 * lo, n, E.data() + 9 * p, head[2] ? mask_in.data() + lo : nullptr, cam.data(), cam[4], &r, got_mask.data() + lo, R4, t4);
        bad_res += std::memcmp(&r, &want[p], sizeof(r)) != 0;
        bad_cand += std::memcmp(R4, wR4.data() + 36 * p, sizeof(R4)) != 0 || std::memcmp(t4, wt4.data() + 12 * p, sizeof(t4)) != 0;
    }
    bad_mask = total ? std::memcmp(got_mask.data(), want_mask.data(), total) != 0 : 0;
    CHECK(bad_res == 0); CHECK(bad_mask == 0); CHECK(bad_cand == 0); CHECK(got_mask[total] == 0xA7);
    std::printf("replayed %zu pairs, %zu records: %zu results, %zu candidate sets differ\n", P, total, bad_res, bad_cand);
}

int main(int argc, char** argv) {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    lcm_pose_params pp;
    std::memset(&pp, 0xAB, sizeof(pp));
    lcm::pose_params_default(&pp);
    CHECK(pp.max_depth == 50.0 && pp.min_pose_inliers == 100);
    for (int r : pp.reserved) CHECK(r == 0);
    CHECK(lcm::pose_params_problem(nullptr) == nullptr && lcm::pose_params_problem(&pp) == nullptr);
    for (double bad : {0.0, -1.0, nan, -inf}) { lcm_pose_params q = pp; q.max_depth = bad; CHECK(lcm::pose_params_problem(&q) != nullptr); }
    { lcm_pose_params q = pp; q.max_depth = inf; CHECK(lcm::pose_params_problem(&q) == nullptr); }      // no far limit
    lcm_epi_params ep;
    lcm::epi_params_default(&ep);
    CHECK(lcm::pose_camera_problem(nullptr) != nullptr && lcm::pose_camera_problem(&ep) != nullptr);
    ep.fx = ep.fy = 700.0; ep.cx = 320.0; ep.cy = 240.0;
    ep.iters = 0;                                                          // K only: the RANSAC's settings are not looked at
    CHECK(lcm::pose_camera_problem(&ep) == nullptr);
    for (double bad : {0.0, -1.0, nan, inf}) { lcm_epi_params q = ep; q.fy = bad; CHECK(lcm::pose_camera_problem(&q) != nullptr); }
    { lcm_epi_params q = ep; q.cx = nan; CHECK(lcm::pose_camera_problem(&q) != nullptr); }

    // the verdict: strict at 100 (src/main.cpp:1409), and the RANSAC's two clauses first
    lcm_epi_result er;
    lcm_pose_result pr;
    std::memset(&er, 0, sizeof(er)); std::memset(&pr, 0, sizeof(pr));
    er.n_points = 300; er.n_inliers = 250;
    pr.n_good = 100; CHECK(lcm::pose_loop_test(&er, &pr, &ep, &pp) == 0);
    pr.n_good = 101; CHECK(lcm::pose_loop_test(&er, &pr, &ep, &pp) == 1 && lcm::pose_loop_test(&er, &pr, &ep, nullptr) == 1);
    pr.status = LCM_POSE_NO_MODEL; CHECK(lcm::pose_loop_test(&er, &pr, &ep, &pp) == 0);
    pr.status = LCM_POSE_OK;
    er.n_inliers = 200; CHECK(lcm::pose_loop_test(&er, &pr, &ep, &pp) == 0);
    er.n_inliers = 250;
    CHECK(lcm::pose_loop_test(nullptr, &pr, &ep, &pp) == 0 && lcm::pose_loop_test(&er, nullptr, &ep, &pp) == 0 && lcm::pose_loop_test(&er, &pr, nullptr, &pp) == 0);
    pp.min_pose_inliers = 101; CHECK(lcm::pose_loop_test(&er, &pr, &ep, &pp) == 0);
    pp.min_pose_inliers = 100;

    // the best loop: first of equals, a failing candidate with more inliers is ignored, the floor is strict
    std::vector<lcm_epi_result> ers(5, er);
    std::vector<lcm_pose_result> prs(5, pr);
    const int inl[5] = {210, 260, 290, 260, 150};
    for (int c = 0; c < 5; ++c) { ers[(size_t)c].n_inliers = inl[c]; prs[(size_t)c].n_good = 150; }
    prs[2].n_good = 100;                                                   // the most inliers, fails the pose test
    CHECK(lcm::pose_best(ers.data(), prs.data(), 5, &ep, &pp, -1) == 1);
    CHECK(lcm::pose_best(ers.data(), prs.data(), 5, &ep, &pp, 259) == 1 && lcm::pose_best(ers.data(), prs.data(), 5, &ep, &pp, 260) == -1);
    CHECK(lcm::pose_best(ers.data(), prs.data(), 1, &ep, &pp, -1) == 0 && lcm::pose_best(ers.data(), prs.data(), 0, &ep, &pp, -1) == -1);
    CHECK(lcm::pose_best(nullptr, nullptr, 0, &ep, &pp, -1) == -1);
    CHECK(lcm::pose_best(ers.data() + 4, prs.data() + 4, 1, &ep, &pp, -1) == -1);       // 150 inliers of 300: not a loop
    CHECK(lcm::pose_best(ers.data(), prs.data(), 5, &ep, &pp, std::numeric_limits<int>::max()) == -1);
    CHECK(lcm::pose_best(ers.data(), prs.data(), 5, &ep, &pp, std::numeric_limits<int>::min()) == 1);

    // the records of a call that launches nothing
    std::vector<lcm_pose_result> res(3);
    std::memset(res.data(), 0xCD, res.size() * sizeof(lcm_pose_result));
    lcm::pose_empty_results(res.data(), 2);
    for (size_t p = 0; p < 2; ++p) {
        for (double v : res[p].R) CHECK(v == 0.0);
        for (double v : res[p].t) CHECK(v == 0.0);
        for (int32_t v : res[p].counts) CHECK(v == 0);
        CHECK(res[p].n_used == 0 && res[p].n_good == 0 && res[p].choice == -1 && res[p].status == LCM_POSE_NO_MODEL);
    }
    CHECK(reinterpret_cast<const unsigned char*>(&res[2])[0] == 0xCD);
    lcm::pose_empty_results(nullptr, 0);

    // the arithmetic on the host: E = [e_z]x, R = I: Ra = I, Rb = diag(-1, -1, 1), t = e_z, all exact
    {
        const double E[9] = {0, -1, 0, 1, 0, 0, 0, 0, 0};
        double ra[9], rb[9], t[3];
        CHECK(lcm::pose_decompose(E, ra, rb, t));
        const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, flip[9] = {-1, 0, 0, 0, -1, 0, 0, 0, 1};
        for (int k = 0; k < 9; ++k) CHECK(ra[k] == eye[k] && rb[k] == flip[k]);
        CHECK(t[0] == 0.0 && t[1] == 0.0 && t[2] == 1.0);
        // X1 = (0.5, 0, 4): X2 = (0.5, 0, 5) -> in front under (I, e_z) only; identical rays: never
        CHECK(lcm::pose_in_front(ra, 0, 0, 1, 0.125, 0.0, 0.1, 0.0, 50.0));
        CHECK(!lcm::pose_in_front(ra, 0, 0, -1, 0.125, 0.0, 0.1, 0.0, 50.0) && !lcm::pose_in_front(rb, 0, 0, 1, 0.125, 0.0, 0.1, 0.0, 50.0));
        CHECK(!lcm::pose_in_front(ra, 0, 0, 1, 0.125, 0.0, 0.1, 0.0, 4.5));                 // 5 baselines deep
        CHECK(!lcm::pose_in_front(ra, 0, 0, 1, 0.0, 0.0, 0.0, 0.0, 50.0) && !lcm::pose_in_front(rb, 0, 0, -1, 0.0, 0.0, 0.0, 0.0, 50.0));
        const double zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bad[9] = {nan, 0, 0, 0, 1, 0, 0, 0, 0}, huge[9] = {1e200, 0, 0, 0, 1e200, 0, 0, 0, 0};
        const double rank1[9] = {1, 0, 0, 0, 0, 0, 0, 0, 0};
        for (const double (*m)[9] : {&zero, &bad, &huge, &rank1}) {
            CHECK(!lcm::pose_decompose(*m, ra, rb, t));
            for (int k = 0; k < 9; ++k) CHECK(ra[k] == 0.0 && rb[k] == 0.0);
            CHECK(t[0] == 0.0 && t[1] == 0.0 && t[2] == 0.0);
        }
        CHECK(lcm::pose_choose(3, 3, 3, 3) == 0 && lcm::pose_choose(1, 5, 5, 2) == 1 && lcm::pose_choose(0, 0, 0, 1) == 3 && lcm::pose_choose(0, 2, 7, 7) == 2);
    }
    if (argc > 1) replay(argv[1]);

    std::printf(failures ? "%d check(s) failed\n" : "pose host checks: all held\n", failures);
    return failures ? 1 : 0;
}
