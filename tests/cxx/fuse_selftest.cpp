// fuse_selftest.cpp — x-slam_amd/host/fuse_host.hpp on its own: what the fuse calls refuse (and that their limits are accepted), K in the
// contract's float32 operations, the transformed origin, the float xform12, the accumulator's size and the runs a cloud is cut into.  Built by
// tests/test_fuse_cases_cpu.py with -fsanitize=address,undefined -fno-sanitize-recover and run without a GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "fuse_host.hpp"

using namespace xs_host;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

struct AccArgs {
    long long n = 100;
    const void *points, *acc, *counts;
    const float *xform, *origin;
    const int *res;
    float vs = 0.0625f, tranc = 0.25f, mn = 0.2f, mx = 5.0f;
    bool have_opts = true;
    unsigned bytes = 16, expected = 16;
    int run() const { return fuse_validate_accumulate(n, points, xform, origin, res, vs, tranc, have_opts, bytes, expected, mn, mx, acc, counts); }
};

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    int token = 0;
    const int res[3] = {70, 9, 11};
    const float id[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const float origin[3] = {0.1f, 0.2f, 0.3f};
    AccArgs good;
    good.points = good.acc = good.counts = &token;
    good.xform = id; good.origin = origin; good.res = res;
    CHECK(good.run() == FUSE_ACCEPTED);
    { AccArgs a = good; a.xform = nullptr; CHECK(a.run() == FUSE_ACCEPTED); }
    { AccArgs a = good; a.n = 1; CHECK(a.run() == FUSE_ACCEPTED); a.n = FUSE_MAX_POINTS; CHECK(a.run() == FUSE_ACCEPTED); }
    { AccArgs a = good; a.n = 0; CHECK(a.run() == FUSE_COUNT); a.n = -1; CHECK(a.run() == FUSE_COUNT); a.n = FUSE_MAX_POINTS + 1; CHECK(a.run() == FUSE_COUNT); }
    { AccArgs a = good; a.points = nullptr; CHECK(a.run() == FUSE_NULL); }
    { AccArgs a = good; a.origin = nullptr; CHECK(a.run() == FUSE_NULL); }
    { AccArgs a = good; a.res = nullptr; CHECK(a.run() == FUSE_NULL); }
    { AccArgs a = good; a.have_opts = false; CHECK(a.run() == FUSE_NULL); }
    { AccArgs a = good; a.acc = nullptr; CHECK(a.run() == FUSE_NULL); }
    { AccArgs a = good; a.counts = nullptr; CHECK(a.run() == FUSE_NULL); }
    { AccArgs a = good; a.bytes = 12; CHECK(a.run() == FUSE_STRUCT); }
    { const int r0[3] = {0, 9, 11}, r1[3] = {70, 65535 * 4 + 1, 1}, r2[3] = {4, 65536, 32768}; AccArgs a = good;
      a.res = r0; CHECK(a.run() == FUSE_RES); a.res = r1; CHECK(a.run() == FUSE_RES); a.res = r2; CHECK(a.run() == FUSE_RES); }
    for (float v : {0.f, -0.05f, nan, inf}) {
        AccArgs a = good; a.vs = v; CHECK(a.run() == FUSE_VOXEL);
        AccArgs b = good; b.tranc = v; CHECK(b.run() == FUSE_TRANC);
    }
    // K: the cap itself is accepted, one half step more is not
    CHECK(fuse_half_steps(0.0625f, 0.25f) == 8);
    CHECK(fuse_half_steps(0.0625f, 0.2f) == 7);
    CHECK(fuse_half_steps(0.0625f, 8.0f) == 256);
    CHECK(fuse_half_steps(0.01f, 0.03f) == (int)std::ceil(0.03f / (0.5f * 0.01f)));
    CHECK(fuse_half_steps(1e-30f, 1e30f) == INT_MAX);
    { AccArgs a = good; a.tranc = 8.0f; a.mx = 5.0f; CHECK(a.run() == FUSE_ACCEPTED); a.tranc = 8.01f; CHECK(a.run() == FUSE_HALF_STEPS); a.tranc = 1e30f; CHECK(a.run() == FUSE_HALF_STEPS); }
    for (int i = 0; i < 12; ++i)
        for (float v : {nan, inf, -inf}) {
            float m[12];
            for (int k = 0; k < 12; ++k) m[k] = id[k];
            m[i] = v;
            AccArgs a = good; a.xform = m; CHECK(a.run() == FUSE_NOT_FINITE);
        }
    for (int i = 0; i < 3; ++i) {
        float o[3] = {origin[0], origin[1], origin[2]};
        o[i] = nan;
        AccArgs a = good; a.origin = o; CHECK(a.run() == FUSE_NOT_FINITE);
    }
    { AccArgs a = good; a.mn = nan; CHECK(a.run() == FUSE_NOT_FINITE); a.mn = 0.2f; a.mx = inf; CHECK(a.run() == FUSE_NOT_FINITE); }
    { AccArgs a = good; a.mn = 0.f; CHECK(a.run() == FUSE_MIN_RANGE); a.mn = -1.f; CHECK(a.run() == FUSE_MIN_RANGE); }
    { AccArgs a = good; a.mx = 0.1f; CHECK(a.run() == FUSE_MAX_RANGE); a.mx = a.mn; CHECK(a.run() == FUSE_ACCEPTED); }
    { AccArgs a = good; a.mx = 32768.f; CHECK(a.run() == FUSE_ACCEPTED); a.mx = 32769.f; CHECK(a.run() == FUSE_RAY_STEPS); }   // 2^20 half steps of 1 / 32 m

    // the fold
    CHECK(fuse_validate_fold(true, 280, res, 0, 11, &token, 1, 100) == FUSE_ACCEPTED);
    CHECK(fuse_validate_fold(true, 4096, res, 3, 4, &token, 100, 100) == FUSE_ACCEPTED);
    CHECK(fuse_validate_fold(true, 280, res, 0, 11, &token, 1, 1 << 24) == FUSE_ACCEPTED);
    CHECK(fuse_validate_fold(false, 280, res, 0, 11, &token, 1, 100) == FUSE_NULL);
    CHECK(fuse_validate_fold(true, 280, nullptr, 0, 11, &token, 1, 100) == FUSE_NULL);
    CHECK(fuse_validate_fold(true, 280, res, 0, 11, nullptr, 1, 100) == FUSE_NULL);
    CHECK(fuse_validate_fold(true, 276, res, 0, 11, &token, 1, 100) == FUSE_PITCH);
    CHECK(fuse_validate_fold(true, 282, res, 0, 11, &token, 1, 100) == FUSE_PITCH);
    CHECK(fuse_validate_fold(true, 280, res, -1, 11, &token, 1, 100) == FUSE_PLANES);
    CHECK(fuse_validate_fold(true, 280, res, 0, 12, &token, 1, 100) == FUSE_PLANES);
    CHECK(fuse_validate_fold(true, 280, res, 5, 5, &token, 1, 100) == FUSE_PLANES);
    CHECK(fuse_validate_fold(true, 280, res, 6, 5, &token, 1, 100) == FUSE_PLANES);
    CHECK(fuse_validate_fold(true, 280, res, 0, 11, &token, 1, 0) == FUSE_MAX_WEIGHT_RANGE);
    CHECK(fuse_validate_fold(true, 280, res, 0, 11, &token, 1, (1 << 24) + 1) == FUSE_MAX_WEIGHT_RANGE);
    CHECK(fuse_validate_fold(true, 280, res, 0, 11, &token, 0, 100) == FUSE_OBS_WEIGHT);
    CHECK(fuse_validate_fold(true, 280, res, 0, 11, &token, 101, 100) == FUSE_OBS_WEIGHT);
    for (int r = 0; r <= FUSE_OBS_WEIGHT + 1; ++r) CHECK(fuse_refusal_str(r) != nullptr && fuse_refusal_str(r)[0] != 0);

    // the accumulator: 8 bytes per voxel, in 64 bits
    CHECK(fuse_accumulator_bytes(res) == (size_t)70 * 9 * 11 * 8);
    { const int big[3] = {2048, 2048, 1024}; CHECK(fuse_accumulator_bytes(big) == ((size_t)1 << 35)); }
    { const int bad[3] = {0, 1, 1}; CHECK(fuse_accumulator_bytes(bad) == 0); }

    // the origin: the sample formula in float32, in the order written; the bits as they are without a transform
    {
        const float m[12] = {0.36f, 0.48f, -0.8f, -0.8f, 0.6f, 0.0f, 0.48f, 0.64f, 0.6f, 0.1f, -0.2f, 0.3f};
        float out[3];
        fuse_origin(m, origin, out);
        for (int c = 0; c < 3; ++c) {
            volatile float a = m[3 * c] * origin[0], b = m[3 * c + 1] * origin[1], cc = m[3 * c + 2] * origin[2];
            volatile float s = a + b;
            s = s + cc;
            s = s + m[9 + c];
            CHECK(out[c] == s);
        }
        const float neg0[3] = {-0.0f, 1.0f, 2.0f};
        fuse_origin(nullptr, neg0, out);
        CHECK(std::signbit(out[0]) && out[1] == 1.0f && out[2] == 2.0f);
    }

    // xform12: the registration's rule
    {
        double T[16] = {1, 0, 0, 0.1, 0, 1, 0, 0.2, 0, 0, 1, 0.3, 0, 0, 0, 1};
        float a[12], b[12];
        CHECK(fuse_xform12(T, a) && register_xform12(T, b));
        for (int i = 0; i < 12; ++i) CHECK(a[i] == b[i]);
        CHECK(a[9] == (float)0.1 && a[11] == (float)0.3);
        T[3] = std::numeric_limits<double>::infinity();
        a[0] = 7.f;
        CHECK(!fuse_xform12(T, a) && a[0] == 7.f);
        T[3] = 1e300;
        CHECK(!fuse_xform12(T, a));
        CHECK(!fuse_xform12(nullptr, a));
    }

    // the runs: they cover 0 .. n in order, none is empty, none is longer than the limit
    for (long long n : {1ll, 2ll, FUSE_MAX_POINTS - 1, FUSE_MAX_POINTS, FUSE_MAX_POINTS + 1, 2 * FUSE_MAX_POINTS, 2 * FUSE_MAX_POINTS + 1, 100000000ll, 1ll << 40}) {
        const long long runs = fuse_run_count(n);
        CHECK(runs == (n + FUSE_MAX_POINTS - 1) / FUSE_MAX_POINTS);
        long long at = 0, first = -1, count = -1;
        const long long probe[4] = {0, 1, runs / 2, runs - 1};
        for (long long i : probe) {
            if (i < 0 || i >= runs) continue;
            CHECK(fuse_run(n, i, &first, &count));
            CHECK(first == i * FUSE_MAX_POINTS && count >= 1 && count <= FUSE_MAX_POINTS && first + count <= n);
            if (i == runs - 1) CHECK(first + count == n);
            else CHECK(count == FUSE_MAX_POINTS);
        }
        if (runs <= 8)
            for (long long i = 0; fuse_run(n, i, &first, &count); ++i) { CHECK(first == at); at += count; }
        if (runs <= 8) CHECK(at == n);
        CHECK(!fuse_run(n, runs, &first, &count) && !fuse_run(n, -1, &first, &count));
    }
    CHECK(fuse_run_count(0) == 0 && fuse_run_count(-5) == 0);

    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks held\n");
    return 0;
}
