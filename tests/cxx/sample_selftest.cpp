// sample_selftest.cpp — x-slam_amd/host/sample_host.hpp (what xs_tsdf_sample_points and xs_tsdf_sample_depth refuse, the float xform12 of a double
// T16, the composition of two transforms; no GPU) built with -fsanitize=address,undefined and run.
#include "sample_host.hpp"
#include <cstdio>
#include <cstring>
#include <limits>

using namespace xs_host;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

namespace {
struct Call {
    long long n = 100;
    int rows = 48, cols = 64;
    size_t depth_step = 64 * 2;
    float input[4] = {0.f, 0.f, 0.f, 0.f};           // stands for the points or the depth image: only its address matters
    float xform[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.1f, 0.2f, 0.3f};
    float intr[4] = {60.f, -55.f, 31.5f, 23.5f}, R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, t[3] = {0.1f, 0.2f, 0.3f};
    int res[3] = {33, 17, 20};
    size_t step = 33 * 4;
    float vs = 0.05f;
    unsigned struct_bytes = 8, expected = 8;
    unsigned char status = 0;
    float value = 0.f, dvalue = 0.f, gradient[3] = {0.f, 0.f, 0.f};
    unsigned long long counts[4] = {0, 0, 0, 0};
    SampleOutputPtrs out{&status, &value, nullptr, gradient, counts};
    bool volume = true, grad = false, null_input = false, null_xform = false, null_res = false, null_intr = false, null_R = false, null_t = false;
    int points() {
        return sample_validate_points(n, null_input ? nullptr : input, null_xform ? nullptr : xform, out, volume, grad, step, null_res ? nullptr : res, vs, struct_bytes,
                                      expected);
    }
    int depth() {
        return sample_validate_depth(null_input ? nullptr : input, depth_step, rows, cols, null_intr ? nullptr : intr, null_R ? nullptr : R, null_t ? nullptr : t, out,
                                     volume, grad, step, null_res ? nullptr : res, vs, struct_bytes, expected);
    }
};
}  // namespace

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the accepted calls and the limits themselves
    {
        Call c;
        CHECK(c.points() == SAMPLE_ACCEPTED && c.depth() == SAMPLE_ACCEPTED);
        c.n = 1; CHECK(c.points() == SAMPLE_ACCEPTED);
        c.n = SAMPLE_MAX_POINTS; CHECK(c.points() == SAMPLE_ACCEPTED);
        c.null_xform = true; CHECK(c.points() == SAMPLE_ACCEPTED);
        c.rows = 1; c.cols = 4096; c.depth_step = 8192; CHECK(c.depth() == SAMPLE_ACCEPTED);
        c.rows = 4096; c.cols = 1; c.depth_step = 2; CHECK(c.depth() == SAMPLE_ACCEPTED);
        c.depth_step = 10; CHECK(c.depth() == SAMPLE_ACCEPTED);
        c.out = SampleOutputPtrs{nullptr, nullptr, nullptr, nullptr, c.counts}; CHECK(c.points() == SAMPLE_ACCEPTED);     // one output is enough
        c.out = SampleOutputPtrs{nullptr, nullptr, &c.dvalue, nullptr, nullptr}; c.grad = true; CHECK(c.points() == SAMPLE_ACCEPTED && c.depth() == SAMPLE_ACCEPTED);
        c.step = 33 * 4 + 12; CHECK(c.points() == SAMPLE_ACCEPTED);
    }
    // the refusals, one at a time
#define REFUSED(call, change, why) do { Call c; change; CHECK(c.call() == why); } while (0)
#define REFUSED_BOTH(change, why) do { REFUSED(points, change, why); REFUSED(depth, change, why); } while (0)
    REFUSED(points, c.n = 0, SAMPLE_COUNT);
    REFUSED(points, c.n = -1, SAMPLE_COUNT);
    REFUSED(points, c.n = SAMPLE_MAX_POINTS + 1, SAMPLE_COUNT);
    REFUSED(depth, c.rows = 0, SAMPLE_IMAGE);
    REFUSED(depth, c.cols = 0, SAMPLE_IMAGE);
    REFUSED(depth, c.rows = 4097, SAMPLE_IMAGE);
    REFUSED(depth, (c.cols = 4097, c.depth_step = 2 * 4097), SAMPLE_IMAGE);
    REFUSED_BOTH(c.null_input = true, SAMPLE_NULL);
    REFUSED_BOTH(c.null_res = true, SAMPLE_NULL);
    REFUSED_BOTH(c.volume = false, SAMPLE_NULL);
    REFUSED(depth, c.null_intr = true, SAMPLE_NULL);
    REFUSED(depth, c.null_R = true, SAMPLE_NULL);
    REFUSED(depth, c.null_t = true, SAMPLE_NULL);
    REFUSED_BOTH(c.out = SampleOutputPtrs{}, SAMPLE_NO_OUTPUT);
    REFUSED_BOTH(c.out.dvalue = &c.dvalue, SAMPLE_NO_GRAD);
    REFUSED_BOTH(c.out.status = c.input, SAMPLE_ALIAS);
    REFUSED_BOTH(c.out.value = c.input, SAMPLE_ALIAS);
    REFUSED_BOTH((c.grad = true, c.out.dvalue = c.input), SAMPLE_ALIAS);
    REFUSED_BOTH(c.out.gradient = c.input, SAMPLE_ALIAS);
    REFUSED_BOTH(c.out.counts = c.input, SAMPLE_ALIAS);
    REFUSED_BOTH(c.struct_bytes = 4, SAMPLE_STRUCT);
    REFUSED_BOTH(c.struct_bytes = 0, SAMPLE_STRUCT);
    REFUSED_BOTH(c.res[0] = 0, SAMPLE_RES);
    REFUSED_BOTH(c.res[2] = -3, SAMPLE_RES);
    REFUSED_BOTH(c.res[1] = 65535 * 4 + 1, SAMPLE_RES);
    REFUSED_BOTH((c.res[1] = 65536, c.res[2] = 32768), SAMPLE_RES);     // rows that do not fit an int
    REFUSED_BOTH(c.step = 33 * 4 - 4, SAMPLE_PITCH);
    REFUSED_BOTH(c.step = 33 * 4 + 2, SAMPLE_PITCH);
    REFUSED_BOTH(c.vs = 0.f, SAMPLE_VOXEL);
    REFUSED_BOTH(c.vs = -0.05f, SAMPLE_VOXEL);
    REFUSED_BOTH(c.vs = nan, SAMPLE_VOXEL);
    REFUSED_BOTH(c.vs = inf, SAMPLE_VOXEL);
    REFUSED(points, c.xform[0] = nan, SAMPLE_NOT_FINITE);
    REFUSED(points, c.xform[11] = -inf, SAMPLE_NOT_FINITE);
    REFUSED(depth, c.depth_step = 64 * 2 - 2, SAMPLE_DEPTH_PITCH);
    REFUSED(depth, c.depth_step = 64 * 2 + 1, SAMPLE_DEPTH_PITCH);
    REFUSED(depth, c.R[4] = nan, SAMPLE_NOT_FINITE);
    REFUSED(depth, c.t[2] = inf, SAMPLE_NOT_FINITE);
    REFUSED(depth, c.intr[3] = nan, SAMPLE_NOT_FINITE);
    REFUSED(depth, c.intr[0] = inf, SAMPLE_NOT_FINITE);
    REFUSED(depth, c.intr[0] = 0.f, SAMPLE_FOCAL);
    REFUSED(depth, c.intr[1] = -0.f, SAMPLE_FOCAL);
    {   // the order of the checks: the first one decides
        Call c;
        c.n = 0; c.null_input = true; c.vs = 0.f;
        CHECK(c.points() == SAMPLE_COUNT);
        c.n = 5;
        CHECK(c.points() == SAMPLE_NULL);
        c.null_input = false;
        CHECK(c.points() == SAMPLE_VOXEL);
    }
    for (int r = 0; r <= SAMPLE_VOXEL; ++r) CHECK(sample_refusal_str(r)[0] != '?');
    CHECK(sample_refusal_str(-1)[0] == '?' && sample_refusal_str(SAMPLE_VOXEL + 1)[0] == '?');
    // xform12 from a double T16: row-major R, then t, one rounding each
    {
        double T[16];
        for (int i = 0; i < 16; ++i) T[i] = 0.1 * (double)(i + 1);
        float m[12];
        for (int i = 0; i < 12; ++i) m[i] = -7.f;
        CHECK(sample_xform12(T, m));
        const int Ri[9] = {0, 1, 2, 4, 5, 6, 8, 9, 10}, ti[3] = {3, 7, 11};
        for (int i = 0; i < 9; ++i) CHECK(m[i] == (float)T[Ri[i]]);
        for (int i = 0; i < 3; ++i) CHECK(m[9 + i] == (float)T[ti[i]]);
        T[15] = std::numeric_limits<double>::quiet_NaN();      // the last row is not read
        CHECK(sample_xform12(T, m));
        float keep[12];
        std::memcpy(keep, m, sizeof(m));
        T[6] = std::numeric_limits<double>::infinity();
        CHECK(!sample_xform12(T, m) && !std::memcmp(keep, m, sizeof(m)));
        T[6] = 1e300;                                           // finite in double, not in float
        CHECK(!sample_xform12(T, m) && !std::memcmp(keep, m, sizeof(m)));
        T[6] = 0.7;
        CHECK(!sample_xform12(nullptr, m) && !sample_xform12(T, nullptr) && sample_xform12(T, m));
    }
    // the composition: a quarter turn about z with a shift, after a shift
    {
        const double A[16] = {0, -1, 0, 1, 1, 0, 0, 2, 0, 0, 1, 3, 9, 9, 9, 9}, B[16] = {1, 0, 0, 0.5, 0, 1, 0, 0, 0, 0, 1, -1, 0, 0, 0, 1};
        double T[16];
        sample_compose(A, B, T);
        const double want[16] = {0, -1, 0, 1, 1, 0, 0, 2.5, 0, 0, 1, 2, 0, 0, 0, 1};
        for (int i = 0; i < 16; ++i) CHECK(T[i] == want[i]);
        // a point through the composition is the point through both: p = (1, 2, 3)
        const double p[3] = {1, 2, 3};
        double q[3], r[3], s[3];
        for (int a = 0; a < 3; ++a) q[a] = B[4 * a] * p[0] + B[4 * a + 1] * p[1] + B[4 * a + 2] * p[2] + B[4 * a + 3];
        for (int a = 0; a < 3; ++a) r[a] = A[4 * a] * q[0] + A[4 * a + 1] * q[1] + A[4 * a + 2] * q[2] + A[4 * a + 3];
        for (int a = 0; a < 3; ++a) s[a] = T[4 * a] * p[0] + T[4 * a + 1] * p[1] + T[4 * a + 2] * p[2] + T[4 * a + 3];
        for (int a = 0; a < 3; ++a) CHECK(r[a] == s[a]);
        const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        sample_compose(I, A, T);
        for (int i = 0; i < 12; ++i) CHECK(T[i] == A[i]);
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks held\n");
    return 0;
}
