// align_search_selftest.cpp — x-slam_amd/host/align_search_host.hpp under the host sanitizers, no GPU: the Halton radical inverse on known
// values, align_search_free (rotations, centroid-matched translations inside their box, the cover of SO(3)), align_search_around (entry 0,
// the pivot's image, the angle), align_search_rank against a sort written here, band_centroid against sums formed here, and every refusal.
// Built and run by tests/test_align_score_cpu.py with -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off.
#include "align_search_host.hpp"
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

static bool is_rotation(const double *T, double tol) {
    bool ok = true;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += T[4 * r + k] * T[4 * c + k];
            ok = ok && std::fabs(s - (r == c ? 1.0 : 0.0)) <= tol;
        }
    const double det = T[0] * (T[5] * T[10] - T[6] * T[9]) - T[1] * (T[4] * T[10] - T[6] * T[8]) + T[2] * (T[4] * T[9] - T[5] * T[8]);
    return ok && std::fabs(det - 1.0) <= tol && T[12] == 0 && T[13] == 0 && T[14] == 0 && T[15] == 1;
}
static void apply(const double *T, const double *p, double *q) {
    for (int a = 0; a < 3; ++a) q[a] = T[4 * a] * p[0] + T[4 * a + 1] * p[1] + T[4 * a + 2] * p[2] + T[4 * a + 3];
}
// the angle of Ra Rb^T
static double angle_between(const double *A, const double *B) {
    double tr = 0;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) tr += A[4 * r + k] * B[4 * r + k];
    return std::acos(std::fmax(-1.0, std::fmin(1.0, 0.5 * (tr - 1.0))));
}

static void test_halton() {
    CHECK(align_halton(1, 2) == 0.5 && align_halton(2, 2) == 0.25 && align_halton(3, 2) == 0.75 && align_halton(4, 2) == 0.125);
    CHECK(std::fabs(align_halton(1, 3) - 1.0 / 3) < 1e-16 && std::fabs(align_halton(4, 3) - 4.0 / 9) < 1e-16);
    CHECK(align_halton(0, 2) == 0.0);
    for (unsigned long long i = 1; i < 5000; ++i)
        for (unsigned b : {2u, 3u, 5u, 7u, 11u, 13u}) CHECK(align_halton(i, b) > 0.0 && align_halton(i, b) < 1.0);
}

static void test_free() {
    const int n = 2048;
    std::vector<double> T((size_t)n * 16, -7.0), again((size_t)n * 16);
    const double ct[3] = {2.4, 2.3, 2.9}, co[3] = {2.1, 2.6, 2.2}, box = 0.3;
    CHECK(align_search_free(n, ct, co, box, T.data()));
    CHECK(align_search_free(n, ct, co, box, again.data()) && std::memcmp(T.data(), again.data(), T.size() * sizeof(double)) == 0);
    for (int i = 0; i < n; ++i) {
        const double *M = &T[(size_t)i * 16];
        CHECK(is_rotation(M, 1e-12));
        double q[3];
        apply(M, ct, q);
        for (int a = 0; a < 3; ++a) CHECK(std::fabs(q[a] - co[a]) <= box * (1.0 + 1e-12) + 1e-12);
    }
    // a prefix of the sequence is the shorter call's result
    std::vector<double> few(5 * 16);
    CHECK(align_search_free(5, ct, co, box, few.data()) && std::memcmp(few.data(), T.data(), few.size() * sizeof(double)) == 0);
    // the cover: every one of 200 random rotations has a candidate within 35 degrees (2048 candidates cover SO(3) to about 20)
    for (int it = 0; it < 200; ++it) {
        double R[16] = {0};
        double Q[9];
        align_shoemake(uniform(), uniform(), uniform(), Q);
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[4 * r + c] = Q[3 * r + c];
        double best = 10;
        for (int i = 0; i < n; ++i) best = std::fmin(best, angle_between(R, &T[(size_t)i * 16]));
        CHECK(best < 35.0 * 3.14159265358979 / 180.0);
    }
    // box 0: the centroid lands on the centroid
    CHECK(align_search_free(3, ct, co, 0.0, few.data()));
    for (int i = 0; i < 3; ++i) {
        double q[3];
        apply(&few[(size_t)i * 16], ct, q);
        for (int a = 0; a < 3; ++a) CHECK(std::fabs(q[a] - co[a]) < 1e-12);
    }
    // refusals write nothing
    std::vector<double> keep(few);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double bad[3] = {nan, 0, 0};
    CHECK(!align_search_free(0, ct, co, box, few.data()) && !align_search_free(3, nullptr, co, box, few.data()) && !align_search_free(3, ct, nullptr, box, few.data()));
    CHECK(!align_search_free(3, ct, co, -0.1, few.data()) && !align_search_free(3, ct, co, nan, few.data()) && !align_search_free(3, ct, co, inf, few.data()));
    CHECK(!align_search_free(3, bad, co, box, few.data()) && !align_search_free(3, ct, bad, box, few.data()) && !align_search_free(3, ct, co, box, nullptr));
    CHECK(std::memcmp(keep.data(), few.data(), few.size() * sizeof(double)) == 0);
}

static void test_around() {
    for (int it = 0; it < 50; ++it) {
        double T[16] = {0}, Q[9];
        align_shoemake(uniform(), uniform(), uniform(), Q);
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T[4 * r + c] = Q[3 * r + c]; T[4 * r + 3] = uniform(-3, 3); }
        T[15] = 1.0;
        const double pivot[3] = {uniform(0, 5), uniform(0, 5), uniform(0, 5)}, bt = uniform(0, 0.5), br = uniform(0, 0.5);
        const int n = 256;
        std::vector<double> out((size_t)n * 16, -7.0);
        CHECK(align_search_around(T, pivot, bt, br, n, out.data()));
        CHECK(std::memcmp(out.data(), T, sizeof(T)) == 0);
        double q[3];
        apply(T, pivot, q);
        const double s3 = std::sqrt(3.0);
        for (int i = 1; i < n; ++i) {
            const double *M = &out[(size_t)i * 16];
            CHECK(is_rotation(M, 1e-12));
            double p[3];
            apply(M, pivot, p);
            const double d = std::sqrt((p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]) + (p[2] - q[2]) * (p[2] - q[2]));
            CHECK(d <= bt * s3 + 1e-12);
            for (int a = 0; a < 3; ++a) CHECK(std::fabs(p[a] - q[a]) <= bt + 1e-12);
            CHECK(angle_between(M, T) <= br * s3 + 1e-7);
        }
        // both boxes 0: every entry is T to rounding
        CHECK(align_search_around(T, pivot, 0.0, 0.0, 4, out.data()));
        for (int i = 0; i < 4 * 16; ++i) CHECK(std::fabs(out[(size_t)i] - T[i % 16]) < 1e-12);
    }
    double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, out[32], keep[32];
    for (int i = 0; i < 32; ++i) keep[i] = out[i] = 3.0 + i;
    const double p[3] = {1, 2, 3}, nan = std::numeric_limits<double>::quiet_NaN();
    const double badp[3] = {1, nan, 3};
    double B[16];
    std::memcpy(B, I, sizeof(I));
    B[7] = std::numeric_limits<double>::infinity();
    CHECK(!align_search_around(I, p, 0.1, 0.1, 0, out) && !align_search_around(nullptr, p, 0.1, 0.1, 2, out) && !align_search_around(I, nullptr, 0.1, 0.1, 2, out));
    CHECK(!align_search_around(I, p, -0.1, 0.1, 2, out) && !align_search_around(I, p, 0.1, -0.1, 2, out) && !align_search_around(I, p, nan, 0.1, 2, out));
    CHECK(!align_search_around(I, p, 0.1, nan, 2, out) && !align_search_around(B, p, 0.1, 0.1, 2, out) && !align_search_around(I, badp, 0.1, 0.1, 2, out));
    CHECK(!align_search_around(I, p, 0.1, 0.1, 2, nullptr));
    CHECK(std::memcmp(keep, out, sizeof(out)) == 0);
}

static void test_rank() {
    for (int it = 0; it < 200; ++it) {
        const int P = 1 + (int)(uniform() * 70), keep = 1 + (int)(uniform() * 40);
        std::vector<double> o((size_t)P * 2);
        for (int i = 0; i < P; ++i) { o[2 * (size_t)i + 1] = std::floor(uniform(0, 6)); o[2 * (size_t)i] = 0.25 * std::floor(uniform(0, 4)); }   // many ties
        std::vector<int> idx((size_t)keep + 1, -9);
        const int n = align_search_rank(o.data(), P, keep, idx.data());
        CHECK(n == (keep < P ? keep : P) && idx[(size_t)n] == -9);
        // selection by hand: repeatedly the best remaining, the lower index on ties
        std::vector<char> used((size_t)P, 0);
        for (int k = 0; k < n; ++k) {
            int best = -1;
            for (int i = 0; i < P; ++i) {
                if (used[(size_t)i]) continue;
                if (best < 0 || o[2 * (size_t)i + 1] - o[2 * (size_t)i] > o[2 * (size_t)best + 1] - o[2 * (size_t)best]) best = i;
            }
            used[(size_t)best] = 1;
            CHECK(idx[(size_t)k] == best);
        }
    }
    int one = -9;
    const double o[2] = {0.5, 3};
    CHECK(align_search_rank(o, 0, 3, &one) == 0 && align_search_rank(o, 1, 0, &one) == 0 && align_search_rank(nullptr, 1, 1, &one) == 0 && one == -9);
    CHECK(align_search_rank(o, 1, 1, nullptr) == 0);
}

static void test_centroid() {
    for (int it = 0; it < 50; ++it) {
        const long long n = 1 + (long long)(uniform() * 3000);
        std::vector<unsigned long long> keys((size_t)n);
        unsigned long long s[3] = {0, 0, 0};
        for (auto &k : keys) {
            const unsigned long long x = (unsigned long long)(uniform() * 2097151), y = (unsigned long long)(uniform() * 2097151), z = (unsigned long long)(uniform() * 4194303);
            k = x | (y << 21) | (z << 42);
            s[0] += x; s[1] += y; s[2] += z;
        }
        double c[3];
        CHECK(band_centroid(keys.data(), n, 0.05, c));
        for (int a = 0; a < 3; ++a) CHECK(c[a] == ((double)s[a] / (double)n + 0.5) * 0.05);
    }
    const unsigned long long k1 = 3ull | (5ull << 21) | (7ull << 42);
    double c[3] = {-1, -1, -1};
    CHECK(band_centroid(&k1, 1, 2.0, c) && c[0] == 7.0 && c[1] == 11.0 && c[2] == 15.0);
    CHECK(!band_centroid(&k1, 0, 2.0, c) && !band_centroid(nullptr, 1, 2.0, c) && !band_centroid(&k1, 1, 2.0, nullptr) && c[0] == 7.0);
}

int main() {
    test_halton();
    test_free();
    test_around();
    test_rank();
    test_centroid();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks held\n");
    return 0;
}
