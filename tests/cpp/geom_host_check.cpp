// The shared records and arithmetic of the geometry stages (csrc/lcm_geom_device.h) compiled for the host, as a stand-alone
// program: tests/test_geom_host.py builds it with -fsanitize=address,undefined and runs it on the CPU.  No device.  The checks of
// exp, log and the Cholesky are the ones the pose graph's and the bundle adjustment's programs held before the functions moved
// here, with their cases and tolerances; the properties of the templates are exact (compared bit for bit).
// Exit status 0 = every check held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "lcm_geom_device.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static_assert(sizeof(lcm::Pose) == 96 && sizeof(lcm::Point3) == 24 && sizeof(lcm::Observation) == 24 && sizeof(lcm::Camera) == 32, "records");
static_assert(lcm::tri_index(0, 0) == 0 && lcm::tri_index(2, 1) == 4 && lcm::tri_index(5, 5) == 20, "packed lower triangle");
static_assert(lcm::sym_index<4>(0, 0) == 0 && lcm::sym_index<4>(3, 3) == 9 && lcm::sym_index<9>(8, 8) == 44, "packed upper triangle");

static const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

template <int N>
static bool same_bits(const double (&a)[N], const double (&b)[N]) { return std::memcmp(a, b, sizeof(a)) == 0; }

// max |R R^T - I| <= 1e-6 and a positive determinant: lcm_pgo_host.h's rule for an accepted rotation
static bool is_rotation(const double (&R)[9]) {
    double P[9];
    lcm::mat3_mul_nt(R, R, P);
    for (int k = 0; k < 9; ++k)
        if (!(std::fabs(P[k] - I3[k]) <= 1e-6)) return false;
    return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]) > 0.0;
}

template <int N>
static void check_sym_index() {
    int seen[N * (N + 1) / 2] = {0};
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            const int k = lcm::sym_index<N>(i, j);
            CHECK(k == lcm::sym_index<N>(j, i) && k >= 0 && k < N * (N + 1) / 2);
            if (i <= j) ++seen[k];
        }
    for (int k = 0; k < N * (N + 1) / 2; ++k) CHECK(seen[k] == 1);
}

static void check_exp_log() {
    const double r[3] = {0.3, -0.2, 0.5};
    double R[9], back[3];
    lcm::so3_exp(r, R);
    CHECK(is_rotation(R) && lcm::so3_log(R, back));
    for (int k = 0; k < 3; ++k) CHECK(std::fabs(back[k] - r[k]) < 1e-15);
    const double tiny[3] = {1e-17, 0, 0}, small[3] = {3e-6, -2e-6, 1e-6};
    lcm::so3_exp(tiny, R);
    CHECK(std::memcmp(R, I3, sizeof(I3)) == 0);
    lcm::so3_exp(small, R);
    CHECK(lcm::so3_log(R, back) && back[0] != 0.0 && std::fabs(back[0] - 3e-6) < 1e-16);      // first order, not a zero vector
    const double half[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1};
    CHECK(!lcm::so3_log(half, back));
    const double rv[3] = {0.1, -0.2, 0.3};                              // the round trip as the camera phase uses it
    lcm::so3_exp(rv, R);
    CHECK(lcm::so3_log(R, back) && std::fabs(back[0] - 0.1) < 1e-15 && std::fabs(back[1] + 0.2) < 1e-15 && std::fabs(back[2] - 0.3) < 1e-15);
}

static void check_products() {
    // small integers: every product and sum is exact, so the four products must agree with one another bit for bit
    const double A[9] = {1, 2, 3, -4, 5, 6, 7, -8, 9}, B[9] = {2, 0, -1, 3, 1, 4, -2, 5, 6};
    double At[9], Bt[9], C[9], D[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { At[3 * i + j] = A[3 * j + i]; Bt[3 * i + j] = B[3 * j + i]; }
    lcm::mat3_mul(A, B, C);
    CHECK(C[0] == 2 && C[1] == 17 && C[2] == 25 && C[3] == -5 && C[4] == 35 && C[5] == 60 && C[6] == -28 && C[7] == 37 && C[8] == 15);
    lcm::mat3_mul_tn(At, B, D);
    CHECK(same_bits(C, D));
    lcm::mat3_mul_nt(A, Bt, D);
    CHECK(same_bits(C, D));
    const double x[3] = {B[0], B[3], B[6]};
    double y[3];
    lcm::mat3_apply(A, x, y);
    CHECK(y[0] == C[0] && y[1] == C[3] && y[2] == C[6]);
    // Xc = (R X) + t on exact numbers: R = I, t = (1, 2, 3), X = (1, 0, 1)
    const double t[3] = {1, 2, 3}, X[3] = {1, 0, 1};
    double R[9], Xc[3];
    std::memcpy(R, I3, sizeof(I3));
    lcm::rigid_apply(R, t, X, Xc);
    CHECK(Xc[0] == 2 && Xc[1] == 2 && Xc[2] == 4);
    // rigid_apply is mat3_apply followed by + t, bit for bit, on numbers that round
    const double rv[3] = {0.3, -0.2, 0.5}, tt[3] = {0.1, -7.3, 1e-3}, XX[3] = {1.0 / 3, -2.0 / 7, 5.1};
    double want[3];
    lcm::so3_exp(rv, R);
    lcm::mat3_apply(R, XX, y);
    for (int k = 0; k < 3; ++k) want[k] = y[k] + tt[k];
    lcm::rigid_apply(R, tt, XX, Xc);
    CHECK(same_bits(Xc, want));
    // the pixel: u = ((fx x) / z) + cx
    const lcm::Camera K{1000.0, 1000.0, 640.0, 360.0};
    const double P[3] = {2, 2, 4};
    double u, v;
    lcm::pinhole_project(K, P, u, v);
    CHECK(u == 1140.0 && v == 860.0);
    const double zero[3] = {2, 2, 0};
    lcm::pinhole_project(K, zero, u, v);
    CHECK(std::isinf(u) && std::isinf(v));                              // no test on z
}

static void check_cholesky() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // the 6 x 6 factor and its solves against the full matrix
    double a[21] = {4, 2, 5, 0, 1, 6, 0, 0, 1, 7, 0, 0, 0, 1, 8, 0, 0, 0, 0, 1, 9}, x[6] = {4, 7, 8, 9, 10, 10};
    CHECK(lcm::chol<6>(a) && a[0] == 2.0 && a[1] == 1.0 && a[2] == 2.0);
    lcm::lower_solve<6>(a, x);
    lcm::upper_solve<6>(a, x);
    const double full[6][6] = {{4, 2, 0, 0, 0, 0}, {2, 5, 1, 0, 0, 0}, {0, 1, 6, 1, 0, 0}, {0, 0, 1, 7, 1, 0}, {0, 0, 0, 1, 8, 1}, {0, 0, 0, 0, 1, 9}};
    const double rhs[6] = {4, 7, 8, 9, 10, 10};
    for (int i = 0; i < 6; ++i) {
        double s = 0.0;
        for (int j = 0; j < 6; ++j) s += full[i][j] * x[j];
        CHECK(std::fabs(s - rhs[i]) < 1e-13);
    }
    double bad6[21] = {1, 2, 1};                                        // not positive definite
    CHECK(!lcm::chol<6>(bad6));
    // the 3 x 3 factor: A = L L^T with L = [[2,0,0],[1,3,0],[-1,2,4]]
    double b[6] = {4, 2, 10, -2, 5, 21};
    CHECK(lcm::chol<3>(b) && b[0] == 2 && b[1] == 1 && b[2] == 3 && b[3] == -1 && b[4] == 2 && b[5] == 4);
    double y[3] = {2, 7, 11};                                           // L y = x: y = (1, 2, 2);  L^T z = y
    lcm::lower_solve<3>(b, y);
    CHECK(y[0] == 1 && y[1] == 2 && y[2] == 2);
    lcm::upper_solve<3>(b, y);
    CHECK(y[2] == 0.5 && y[1] == (2 - 2 * 0.5) / 3 && std::fabs(y[0] - (1.5 - 1.0 / 3) / 2) < 1e-15);
    double bad3[6] = {1, 2, 1, 0, 0, 1};                                // not positive definite
    CHECK(!lcm::chol<3>(bad3));
    double nan3[6] = {nan, 0, 1, 0, 0, 1};
    CHECK(!lcm::chol<3>(nan3));
    // one text at two sizes: the leading 3 x 3 block of a dense 6 x 6 matrix (M M^T + 6 I, M of small integers and thirds, so the
    // factor's entries round) gives the first six packed entries and the first three solved entries, bit for bit
    double M[6][6], S[21], S3[6];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) M[i][j] = ((7 * i + 3 * j) % 5 - 2) / 3.0;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = i == j ? 6.0 : 0.0;
            for (int k = 0; k < 6; ++k) s += M[i][k] * M[j][k];
            S[lcm::tri_index(i, j)] = s;
        }
    std::memcpy(S3, S, sizeof(S3));
    CHECK(lcm::chol<6>(S) && lcm::chol<3>(S3) && std::memcmp(S, S3, sizeof(S3)) == 0);
    double v6[6] = {0.7, -1.3, 2.9, 0.1, -0.4, 1.0}, v3[3] = {0.7, -1.3, 2.9};
    lcm::lower_solve<6>(S, v6);
    lcm::lower_solve<3>(S3, v3);
    CHECK(std::memcmp(v6, v3, sizeof(v3)) == 0 && v3[1] != -1.3);
}

static void check_damped_solves() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // H = diag, damping added absolutely: + 1 gives 4, 9, 16
    double H3[6] = {3, 0, 8, 0, 0, 15}, g3[3] = {-8, -18, -32}, dp3[3];
    CHECK(lcm::solve_damped<3>(H3, g3, 1.0, dp3) && dp3[0] == 2 && dp3[1] == 2 && dp3[2] == 2 && H3[0] == 3);
    double H6[21] = {0}, g6[6], dp6[6];
    for (int k = 0; k < 6; ++k) { H6[lcm::tri_index(k, k)] = (k + 2.0) * (k + 2.0) - 1.0; g6[k] = -(k + 2.0) * (k + 2.0); }
    CHECK(lcm::solve_damped<6>(H6, g6, 1.0, dp6) && dp6[0] == 1 && dp6[5] == 1);
    // false for a pivot that is negative, zero or NaN, at both sizes, wherever it stands
    for (const double pivot : {-2.0, -1.0, nan}) {                      // + 1 of damping: negative, zero, NaN
        for (int k = 0; k < 3; ++k) {
            double H[6] = {3, 0, 8, 0, 0, 15};
            H[lcm::tri_index(k, k)] = pivot;
            CHECK(!lcm::solve_damped<3>(H, g3, 1.0, dp3));
        }
        for (int k = 0; k < 6; ++k) {
            double H[21];
            std::memcpy(H, H6, sizeof(H));
            H[lcm::tri_index(k, k)] = pivot;
            CHECK(!lcm::solve_damped<6>(H, g6, 1.0, dp6));
        }
    }
}

static void check_jacobi_angle() {
    double t = 7, cs = 7, sn = 7;
    CHECK(!lcm::jacobi_angle(1.0, 2.0, 0.0, t, cs, sn) && t == 0.0 && cs == 0.0 && sn == 0.0);       // nothing to annihilate
    CHECK(!lcm::jacobi_angle(1.0, 1.0, 0.5e-18, t, cs, sn));           // below 1e-18 of sqrt(|app aqq|)
    CHECK(lcm::jacobi_angle(1.0, 1.0, 2e-18, t, cs, sn));              // above it
    CHECK(!lcm::jacobi_angle(1.0, 1.0, std::numeric_limits<double>::quiet_NaN(), t, cs, sn));
    CHECK(lcm::jacobi_angle(0.0, 5.0, 1e-100, t, cs, sn));             // a zero diagonal entry: an off-diagonal whose square is not 0 rotates
    // equal diagonal entries: zeta = 0, a quarter turn's half
    CHECK(lcm::jacobi_angle(3.0, 3.0, 0.5, t, cs, sn) && t == 1.0 && cs == 1.0 / std::sqrt(2.0) && sn == cs);
    CHECK(lcm::jacobi_angle(3.0, 3.0, -0.5, t, cs, sn) && t == 1.0);    // zeta = -0.0 counts as >= 0
    // the rotation annihilates (p, q): a'pq = (cs^2 - sn^2) apq + cs sn (app - aqq)
    const double app = 2.0, aqq = -1.0, apq = 0.75;
    CHECK(lcm::jacobi_angle(app, aqq, apq, t, cs, sn) && t < 0.0 && cs > 0.0 && sn < 0.0);
    // every term is below 1 in size and carries a few roundings of t, cs and sn: eight units of the last place of 1
    CHECK(std::fabs((cs * cs - sn * sn) * apq + cs * sn * (app - aqq)) < 8 * std::numeric_limits<double>::epsilon());
}

int main() {
    check_sym_index<4>();
    check_sym_index<9>();
    check_exp_log();
    check_products();
    check_cholesky();
    check_damped_solves();
    check_jacobi_angle();
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all held\n");
    return 0;
}
