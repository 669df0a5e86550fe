// The pure host side of the RANSAC's local optimisation (csrc/lcm_lo_host.h: the parameters' defaults and checks, the check
// of a caller's counts, the records of an empty call) and its arithmetic (csrc/lcm_lo_device.h, compiled as plain C++: one
// refit round over a noise-free two-view scene, the eigen step on matrices with known answers, the degenerate case, the
// acceptance rule) as a stand-alone program: tests/test_lo_abi_host.py builds it with -fsanitize=address,undefined and runs
// it on the CPU.  No HIP runtime, no device.  Exit status 0 = every check held.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "lcm_lo_device.h"
#include "lcm_lo_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static_assert(sizeof(lcm::LoInfo) == sizeof(lcm_lo_info) && sizeof(lcm_lo_info) == 16 && sizeof(lcm_lo_params) == 96, "sizes");

struct Rec { double a, b, c, d; };

// One round of lcm_lo_device.h on the host, as k_lo_refine's lane runs it: status, e = E' when LO_OK
static int32_t refit(const std::vector<Rec>& recs, double (&e)[9], double t, double mult, uint32_t* n_sel) {
    const double t2m = lcm::lo_threshold2(t, mult);
    uint32_t cnt = 0;
    double sa = 0, sb = 0, sc = 0, sd = 0;
    for (const Rec& r : recs)
        if (lcm::epi_inlier(e, r.a, r.b, r.c, r.d, t2m)) { ++cnt; sa += r.a; sb += r.b; sc += r.c; sd += r.d; }
    *n_sel = cnt;
    if (cnt < 8) return lcm::LO_TOO_FEW;
    const double nn = (double)cnt, m1x = sa / nn, m1y = sb / nn, m2x = sc / nn, m2y = sd / nn;
    double v1 = 0, v2 = 0;
    for (const Rec& r : recs)
        if (lcm::epi_inlier(e, r.a, r.b, r.c, r.d, t2m)) { v1 += lcm::lo_sqdist(r.a, r.b, m1x, m1y); v2 += lcm::lo_sqdist(r.c, r.d, m2x, m2y); }
    double s1, s2;
    const bool ok1 = lcm::lo_hartley_scale(v1, nn, &s1), ok2 = lcm::lo_hartley_scale(v2, nn, &s2);
    if (!(ok1 && ok2)) return lcm::LO_DEGENERATE;
    double m[lcm::LO_MOMENTS] = {};
    for (const Rec& r : recs)
        if (lcm::epi_inlier(e, r.a, r.b, r.c, r.d, t2m))
            lcm::lo_add_moments(m, lcm::lo_centre(r.a, m1x, s1), lcm::lo_centre(r.b, m1y, s1), lcm::lo_centre(r.c, m2x, s2), lcm::lo_centre(r.d, m2y, s2));
    std::vector<double> W(lcm::LO_WORK);
    for (int k = 0; k < lcm::LO_MOMENTS; ++k) W[(size_t)k] = m[k];
    double f[9];
    lcm::lo_eig9<1>(W.data(), f);
    lcm::lo_denormalise(f, m1x, m1y, s1, m2x, m2y, s2);
    if (!lcm::epi_project(f)) return lcm::LO_NO_MODEL;
    for (int k = 0; k < 9; ++k) e[k] = f[k];
    return lcm::LO_OK;
}

static double distance_up_to_sign(const double (&x)[9], const double (&y)[9]) {
    double nx = 0, ny = 0;
    for (int k = 0; k < 9; ++k) { nx += x[k] * x[k]; ny += y[k] * y[k]; }
    double dm = 0, dp = 0;
    for (int k = 0; k < 9; ++k) {
        const double u = x[k] / std::sqrt(nx), v = y[k] / std::sqrt(ny);
        dm += (u - v) * (u - v); dp += (u + v) * (u + v);
    }
    return std::sqrt(dm < dp ? dm : dp);
}

int main() {
    // ---- parameters
    lcm_lo_params lp;
    std::memset(&lp, 0xAB, sizeof(lp));
    lcm::lo_params_default(&lp);
    CHECK(lp.rounds == 4 && lp.seeds == 64 && lp.mult[0] == 3.0 && lp.mult[1] == 2.0 && lp.mult[2] == 1.5 && lp.mult[3] == 1.0);
    for (int r = 4; r < 8; ++r) CHECK(lp.mult[r] == 0.0);
    for (uint32_t w : lp.reserved) CHECK(w == 0);
    CHECK(lcm::lo_params_problem(nullptr) == nullptr);                    // NULL = the defaults
    CHECK(lcm::lo_params_problem(&lp) == nullptr);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (int bad : {0, -1, 9, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()}) {
        lcm_lo_params q = lp; q.rounds = bad; CHECK(lcm::lo_params_problem(&q) != nullptr);
    }
    for (int bad : {0, 32, 63, 65, 128, -64}) { lcm_lo_params q = lp; q.seeds = bad; CHECK(lcm::lo_params_problem(&q) != nullptr); }
    for (double bad : {0.0, 0.999, -3.0, nan, inf, -inf}) {
        lcm_lo_params q = lp; q.mult[2] = bad; CHECK(lcm::lo_params_problem(&q) != nullptr);
        q = lp; q.mult[5] = bad; CHECK(lcm::lo_params_problem(&q) == nullptr);       // beyond `rounds`: not read
        CHECK(lcm::lo_mult_problem(bad) != nullptr);
    }
    { lcm_lo_params q = lp; q.rounds = 1; q.mult[1] = nan; CHECK(lcm::lo_params_problem(&q) == nullptr); }
    { lcm_lo_params q = lp; q.rounds = 8; CHECK(lcm::lo_params_problem(&q) != nullptr); for (int r = 4; r < 8; ++r) q.mult[r] = 1.0; CHECK(lcm::lo_params_problem(&q) == nullptr); }
    CHECK(lcm::lo_mult_problem(1.0) == nullptr && lcm::lo_mult_problem(3.0) == nullptr);

    // ---- a caller's counts
    std::vector<int32_t> counts(128, 5);
    CHECK(lcm::lo_counts_problem(counts.data(), 128) == nullptr && lcm::lo_counts_problem(counts.data(), 64) == nullptr);
    CHECK(lcm::lo_counts_problem(nullptr, 64) != nullptr);
    for (int bad : {0, -64, 63, 100, 65536 + 64}) CHECK(lcm::lo_counts_problem(counts.data(), bad) != nullptr);      // before any read
    counts[127] = 65535; CHECK(lcm::lo_counts_problem(counts.data(), 128) == nullptr);
    counts[127] = 65536; CHECK(lcm::lo_counts_problem(counts.data(), 128) != nullptr && lcm::lo_counts_problem(counts.data(), 64) == nullptr);
    counts[127] = -1; CHECK(lcm::lo_counts_problem(counts.data(), 128) != nullptr);

    // ---- the records of a call that launches nothing
    std::vector<lcm_lo_info> info(4);
    std::memset(info.data(), 0xCD, info.size() * sizeof(lcm_lo_info));
    lcm::lo_empty_info(info.data(), 3);
    for (int p = 0; p < 3; ++p)
        CHECK(info[(size_t)p].seed_iter == 0 && info[(size_t)p].round == -1 && info[(size_t)p].n_inliers_ransac == 0 && info[(size_t)p].status == LCM_LO_TOO_FEW);
    CHECK(reinterpret_cast<const unsigned char*>(&info[3])[0] == 0xCD);   // not one record more
    lcm::lo_empty_info(nullptr, 0);

    // ---- the rules
    CHECK(lcm::lo_threshold2(1.0 / 700.0, 1.0) == (1.0 / 700.0) * (1.0 / 700.0));
    CHECK(lcm::lo_threshold2(0.5, 3.0) == 2.25);
    CHECK(lcm::lo_accepts(11, 10) && !lcm::lo_accepts(10, 10) && !lcm::lo_accepts(9, 10));
    CHECK(lcm::lo_lane_key(10, 0) > lcm::lo_lane_key(10, 1) && lcm::lo_lane_key(11, 63) > lcm::lo_lane_key(10, 0));
    CHECK((lcm::lo_lane_key(65535, 63) >> 6) == 65535 && (lcm::lo_lane_key(65535, 17) & 63u) == 63u - 17u);
    double s = -1.0;
    CHECK(lcm::lo_hartley_scale(8.0, 4.0, &s) && s == 1.0);
    CHECK(!lcm::lo_hartley_scale(0.0, 4.0, &s) && s == 0.0);
    CHECK(!lcm::lo_hartley_scale(4e-32, 40.0, &s) && !lcm::lo_hartley_scale(nan, 4.0, &s) && !lcm::lo_hartley_scale(inf, 4.0, &s));
    CHECK(!lcm::lo_hartley_scale(0.0, 0.0, &s));                          // no record selected: 0 / 0
    int seen[lcm::LO_MOMENTS] = {};
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) { CHECK(lcm::sym_index<9>(i, j) == lcm::sym_index<9>(j, i)); if (i <= j) ++seen[lcm::sym_index<9>(i, j)]; }
    for (int k : seen) CHECK(k == 1);                                     // a bijection onto 0 .. 44

    // ---- the eigen step: a diagonal matrix names its smallest entry's axis; a rank-8 projector its null vector
    {
        std::vector<double> W(lcm::LO_WORK, 0.0);
        for (int k = 0; k < 9; ++k) W[(size_t)lcm::sym_index<9>(k, k)] = k == 6 ? 0.25 : 1.0 + k;
        double f[9];
        lcm::lo_eig9<1>(W.data(), f);
        for (int k = 0; k < 9; ++k) CHECK(f[k] == (k == 6 ? 1.0 : 0.0));
        double u[9], nu = 0;
        for (int k = 0; k < 9; ++k) { u[k] = 1.0 + 0.37 * k * (k % 2 ? -1 : 1); nu += u[k] * u[k]; }
        for (int i = 0; i < 9; ++i)
            for (int j = i; j < 9; ++j) W[(size_t)lcm::sym_index<9>(i, j)] = 3.0 * ((i == j ? 1.0 : 0.0) - u[i] * u[j] / nu);
        lcm::lo_eig9<1>(W.data(), f);
        double dot = 0, nf = 0;
        for (int k = 0; k < 9; ++k) { dot += f[k] * u[k] / std::sqrt(nu); nf += f[k] * f[k]; }
        CHECK(std::fabs(std::fabs(dot) - 1.0) < 1e-14 && std::fabs(nf - 1.0) < 1e-14);
    }

    // ---- one round over a noise-free scene: X2 = R X1 + t, E = [t]x R; from a perturbed model the refit returns E
    {
        const double cy = std::cos(0.1), sy = std::sin(0.1);
        const double R[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy}, T[3] = {0.6, -0.15, 0.2};
        const double Tx[9] = {0, -T[2], T[1], T[2], 0, -T[0], -T[1], T[0], 0};
        double E[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) E[3 * i + j] = Tx[3 * i] * R[j] + Tx[3 * i + 1] * R[3 + j] + Tx[3 * i + 2] * R[6 + j];
        std::vector<Rec> recs;
        uint32_t h = 12345;
        auto next = [&h]() { h = lcm::epi_fmix32(h + 0x9E3779B9u); return (double)h / 4294967296.0; };
        for (int i = 0; i < 200; ++i) {
            const double X[3] = {4.0 * next() - 2.0, 3.0 * next() - 1.5, 4.0 + 6.0 * next()};
            double Y[3];
            for (int k = 0; k < 3; ++k) Y[k] = R[3 * k] * X[0] + R[3 * k + 1] * X[1] + R[3 * k + 2] * X[2] + T[k];
            recs.push_back(Rec{X[0] / X[2], X[1] / X[2], Y[0] / Y[2], Y[1] / Y[2]});
        }
        for (int i = 0; i < 60; ++i) recs.push_back(Rec{next() - 0.5, next() - 0.5, next() - 0.5, next() - 0.5});       // outliers
        double e[9];
        for (int k = 0; k < 9; ++k) e[k] = E[k] * (1.0 + 0.004 * (k % 3 - 1));                       // a model that is off
        uint32_t n_sel = 0;
        const double t = 1.0 / 700.0;
        CHECK(refit(recs, e, t, 3.0, &n_sel) == lcm::LO_OK && n_sel >= 8);
        CHECK(refit(recs, e, t, 1.0, &n_sel) == lcm::LO_OK && n_sel >= 200);
        CHECK(distance_up_to_sign(e, E) < 1e-9);
        uint32_t in = 0;
        for (const Rec& r : recs) in += lcm::epi_inlier(e, r.a, r.b, r.c, r.d, lcm::lo_threshold2(t, 1.0)) ? 1u : 0u;
        CHECK(in >= 200 && in == n_sel);
        double sv[9];
        for (int k = 0; k < 9; ++k) sv[k] = e[k];
        CHECK(lcm::epi_project(sv) && distance_up_to_sign(sv, e) < 1e-14);                           // already on the manifold

        // identical records: selected by a model they satisfy, no spread; too few: a zero model selects nothing
        std::vector<Rec> same(40, recs[0]);
        double e2[9];
        for (int k = 0; k < 9; ++k) e2[k] = E[k];
        CHECK(refit(same, e2, t, 1.0, &n_sel) == lcm::LO_DEGENERATE && n_sel == 40);
        for (int k = 0; k < 9; ++k) CHECK(e2[k] == E[k]);                                            // untouched
        double zero[9] = {};
        CHECK(refit(recs, zero, t, 3.0, &n_sel) == lcm::LO_TOO_FEW && n_sel == 0);
        std::vector<Rec> seven(recs.begin(), recs.begin() + 7);
        CHECK(refit(seven, e2, t, 1.0, &n_sel) == lcm::LO_TOO_FEW && n_sel == 7);
    }

    std::printf(failures ? "%d check(s) failed\n" : "lo host checks: all held\n", failures);
    return failures ? 1 : 0;
}
