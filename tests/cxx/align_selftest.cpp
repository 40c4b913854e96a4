// align_selftest.cpp — x-slam_amd/host/align_host.hpp under the host sanitizers, no GPU: align_seeded_maps against merge_affine (real parts)
// and central differences (imaginary parts), its refusals, align_se3_exp against the group's laws, align_step on systems with a known
// solution and its refusals.  Built and run by tests/test_align_cases_cpu.py with -fsanitize=address,undefined -fno-sanitize-recover=all
// -ffp-contract=off.
#include "align_host.hpp"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

using namespace xs_host;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {   // xorshift64*, [0, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}
static double uniform(double lo, double hi) { return lo + (hi - lo) * uniform(); }

static void rigid(double T[16]) {
    const double d[6] = {uniform(-4, 4), uniform(-4, 4), uniform(-4, 4), uniform(-1.5, 1.5), uniform(-1.5, 1.5), uniform(-1.5, 1.5)};
    align_se3_exp(d, T);
}
static void mul44(const double *A, const double *B, double *C) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            double s = 0;
            for (int k = 0; k < 4; ++k) s += A[4 * r + k] * B[4 * k + c];
            C[4 * r + c] = s;
        }
}
// merge_affine's formula without the final rounding
static void affine64(const double *T, double vd, double vs, double m[12]) {
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) m[3 * a + b] = T[4 * a + b] * vd / vs;
        m[9 + a] = ((T[4 * a] + T[4 * a + 1] + T[4 * a + 2]) * 0.5 * vd + T[4 * a + 3]) / vs - 0.5;
    }
}

static void test_seeded_maps() {
    const double h = (double)(float)GN_H;
    for (int it = 0; it < 200; ++it) {
        double T[16];
        rigid(T);
        const double vd = uniform(0.01, 0.2), vs = uniform(0.01, 0.2);
        float re[12], out[6][24];
        CHECK(merge_affine(T, vd, vs, re));
        CHECK(align_seeded_maps(T, vd, vs, out));
        for (int k = 0; k < 6; ++k) {
            for (int i = 0; i < 12; ++i) CHECK(std::memcmp(&out[k][2 * i], &re[i], sizeof(float)) == 0);
            double G[16] = {0}, P[16], M[16], hi[12], lo[12];
            if (k < 3) G[4 * k + 3] = 1.0;
            else { const int a = k - 3, b = (a + 1) % 3, c = (a + 2) % 3; G[4 * c + b] = 1.0; G[4 * b + c] = -1.0; }
            const double eps = 1e-6;
            for (int s = 0; s < 2; ++s) {
                for (int i = 0; i < 16; ++i) P[i] = (i % 5 == 0 ? 1.0 : 0.0) + (s ? -eps : eps) * G[i];
                mul44(P, T, M);
                affine64(M, vd, vs, s ? lo : hi);
            }
            double scale = 0;
            for (int i = 0; i < 12; ++i) scale = std::fmax(scale, std::fabs(hi[i] - lo[i]) / (2 * eps));
            for (int i = 0; i < 12; ++i) CHECK(std::fabs((double)out[k][2 * i + 1] / h - (hi[i] - lo[i]) / (2 * eps)) <= 1e-6 * scale);
        }
    }
    // a real part of -0 stays -0 in every seed
    double Z[16] = {1, -0.0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    float out[6][24];
    CHECK(align_seeded_maps(Z, 0.1, 0.1, out));
    for (int k = 0; k < 6; ++k) CHECK(std::signbit(out[k][2]) && out[k][2] == 0.f);
    // refusals leave the output alone
    float keep[6][24];
    for (int k = 0; k < 6; ++k)
        for (int i = 0; i < 24; ++i) keep[k][i] = out[k][i] = 5.f + (float)(24 * k + i);
    double B[16];
    std::memcpy(B, Z, sizeof(Z));
    B[6] = std::numeric_limits<double>::quiet_NaN();
    CHECK(!align_seeded_maps(B, 0.1, 0.1, out));
    B[6] = std::numeric_limits<double>::infinity();
    CHECK(!align_seeded_maps(B, 0.1, 0.1, out));
    CHECK(!align_seeded_maps(Z, 0.0, 0.1, out) && !align_seeded_maps(Z, 0.1, -1.0, out) && !align_seeded_maps(nullptr, 0.1, 0.1, out));
    CHECK(!align_seeded_maps(Z, 0.1, 0.1, nullptr));
    B[6] = 1e300;
    CHECK(!align_seeded_maps(B, 1.0, 1e-10, out));
    CHECK(std::memcmp(keep, out, sizeof(out)) == 0);
}

static void test_exp() {
    for (int it = 0; it < 300; ++it) {
        const double scale = std::pow(10.0, uniform(-9, 0.4));
        const double d[6] = {uniform(-1, 1), uniform(-1, 1), uniform(-1, 1), scale * uniform(-1, 1), scale * uniform(-1, 1), scale * uniform(-1, 1)};
        double E[16], Em[16], P[16];
        align_se3_exp(d, E);
        const double m[6] = {-d[0], -d[1], -d[2], -d[3], -d[4], -d[5]};
        align_se3_exp(m, Em);
        mul44(E, Em, P);   // exp(d) exp(-d) = I
        for (int i = 0; i < 16; ++i) CHECK(std::fabs(P[i] - (i % 5 == 0 ? 1.0 : 0.0)) < 1e-12);
        for (int r = 0; r < 3; ++r)   // a rotation
            for (int c = 0; c < 3; ++c) {
                double s = 0;
                for (int k = 0; k < 3; ++k) s += E[4 * r + k] * E[4 * c + k];
                CHECK(std::fabs(s - (r == c ? 1.0 : 0.0)) < 1e-12);
            }
        CHECK(E[12] == 0 && E[13] == 0 && E[14] == 0 && E[15] == 1);
    }
    const double t[6] = {1, 2, 3, 0, 0, 0};   // a pure translation
    double E[16];
    align_se3_exp(t, E);
    CHECK(E[3] == 1 && E[7] == 2 && E[11] == 3 && E[0] == 1 && E[5] == 1 && E[10] == 1 && E[1] == 0);
    // both sides of the small-angle branch agree: the angles differ by 2e-15, the series' next term is below 1e-18
    const double a[6] = {0.3, -0.2, 0.1, 1e-4 - 1e-15, 0, 0}, b[6] = {0.3, -0.2, 0.1, 1e-4 + 1e-15, 0, 0};
    double Ea[16], Eb[16];
    align_se3_exp(a, Ea);
    align_se3_exp(b, Eb);
    for (int i = 0; i < 16; ++i) CHECK(std::fabs(Ea[i] - Eb[i]) < 1e-13);
}

static void test_step() {
    for (int it = 0; it < 200; ++it) {
        // A = J^T J of a random J, g = A x0: the undamped step solves for -x0
        double J[12][6], x0[6], s[29] = {0};
        for (auto &row : J) for (double &v : row) v = uniform(-2, 2);
        for (double &v : x0) v = uniform(-0.2, 0.2);
        int q = 0;
        double A[6][6];
        for (int j = 0; j < 6; ++j)
            for (int k = 0; k < 6; ++k) { A[j][k] = 0; for (auto &row : J) A[j][k] += row[j] * row[k]; }
        for (int j = 0; j < 6; ++j)
            for (int k = j; k < 6; ++k) s[q++] = A[j][k];
        for (int j = 0; j < 6; ++j) for (int k = 0; k < 6; ++k) s[21 + j] += A[j][k] * x0[k];
        s[27] = 1.0; s[28] = 12;
        double T[16], want[16], E[16], keep[16];
        rigid(T);
        std::memcpy(keep, T, sizeof(T));
        const double m[6] = {-x0[0], -x0[1], -x0[2], -x0[3], -x0[4], -x0[5]};
        align_se3_exp(m, E);
        mul44(E, T, want);
        CHECK(align_step(s, 0.0, T));
        for (int i = 0; i < 16; ++i) CHECK(std::fabs(T[i] - want[i]) < 1e-8);
        // refusals: too few voxels, an indefinite system, null pointers: T untouched
        std::memcpy(T, keep, sizeof(T));
        double few[29];
        std::memcpy(few, s, sizeof(s));
        few[28] = 5;
        CHECK(!align_step(few, 1e-3, T));
        double bad[29];
        std::memcpy(bad, s, sizeof(s));
        bad[20] = -1.0;
        CHECK(!align_step(bad, 1e-3, T));
        bad[20] = std::numeric_limits<double>::quiet_NaN();
        CHECK(!align_step(bad, 1e-3, T));
        CHECK(!align_step(nullptr, 1e-3, T) && !align_step(s, 1e-3, nullptr));
        CHECK(std::memcmp(T, keep, sizeof(T)) == 0);
    }
}

int main() {
    test_seeded_maps();
    test_exp();
    test_step();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks held\n");
    return 0;
}
