// register_selftest.cpp — x-slam_amd/host/register_host.hpp (what xs_tsdf_register_terms refuses, the float xform12 of a double T16, the damped
// step on the kernel's sums; no GPU) built with -fsanitize=address,undefined and run.
#include "register_host.hpp"
#include <cstdio>
#include <cstring>
#include <limits>

using namespace xs_host;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

namespace {
struct Call {
    int transforms = 3;
    long long n = 100;
    float points[3] = {0.f, 0.f, 0.f};               // stands for the device array: only its address matters
    float xforms[32 * 12];
    int res[3] = {33, 17, 20};
    size_t step = 33 * 4;
    float vs = 0.05f, max_residual = 0.9f;
    int min_weight = 1;
    double ws[4] = {0, 0, 0, 0}, out[29] = {};
    bool volume = true, null_points = false, null_xforms = false, null_res = false, null_ws = false, null_out = false;
    Call() {
        for (int m = 0; m < 32; ++m) {
            const float I[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.1f, 0.2f, 0.3f};
            std::memcpy(xforms + 12 * m, I, sizeof(I));
        }
    }
    int run() {
        return register_validate(transforms, n, null_points ? nullptr : points, null_xforms ? nullptr : xforms, volume, step, null_res ? nullptr : res, vs, min_weight,
                                 max_residual, null_ws ? nullptr : ws, null_out ? nullptr : out);
    }
};

// the sums of a synthetic problem r_i = J_i . d + e_i with J = (g, P x g): what the kernel would add, in double
void sums_of(int n, const double d[6], double s[29]) {
    for (int i = 0; i < 29; ++i) s[i] = 0.0;
    unsigned long long state = 12345;
    auto rnd = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (double)(state >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
    for (int i = 0; i < n; ++i) {
        const double g[3] = {rnd(), rnd(), rnd()}, P[3] = {rnd() + 1.0, rnd() - 0.5, rnd() * 2.0};
        const double J[6] = {g[0], g[1], g[2], P[1] * g[2] - P[2] * g[1], P[2] * g[0] - P[0] * g[2], P[0] * g[1] - P[1] * g[0]};
        double r = 0.0;
        for (int k = 0; k < 6; ++k) r -= J[k] * d[k];   // the step that zeroes r is +d
        int q = 0;
        for (int j = 0; j < 6; ++j)
            for (int k = j; k < 6; ++k) s[q++] += J[j] * J[k];
        for (int k = 0; k < 6; ++k) s[21 + k] += J[k] * r;
        s[27] += r * r;
        s[28] += 1.0;
    }
}
}  // namespace

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the accepted calls and the limits themselves
    {
        Call c;
        CHECK(c.run() == REGISTER_ACCEPTED);
        c.transforms = 1; CHECK(c.run() == REGISTER_ACCEPTED);
        c.transforms = REGISTER_MAX_TRANSFORMS; CHECK(c.run() == REGISTER_ACCEPTED);
        c.n = 1; CHECK(c.run() == REGISTER_ACCEPTED);
        c.n = SAMPLE_MAX_POINTS; CHECK(c.run() == REGISTER_ACCEPTED);
        c.step = 33 * 4 + 12; CHECK(c.run() == REGISTER_ACCEPTED);
        c.min_weight = 1 << 30; CHECK(c.run() == REGISTER_ACCEPTED);
        c.max_residual = std::numeric_limits<float>::max(); CHECK(c.run() == REGISTER_ACCEPTED);
        c.max_residual = std::numeric_limits<float>::denorm_min(); CHECK(c.run() == REGISTER_ACCEPTED);
        c.res[0] = c.res[1] = c.res[2] = 1; c.step = 4; CHECK(c.run() == REGISTER_ACCEPTED);
        // an entry past the launch's transforms is not read
        c.transforms = 2; c.xforms[24] = nan; CHECK(c.run() == REGISTER_ACCEPTED);
    }
#define REFUSED(change, why) do { Call c; change; CHECK(c.run() == why); } while (0)
    REFUSED(c.transforms = 0, REGISTER_TRANSFORMS);
    REFUSED(c.transforms = -1, REGISTER_TRANSFORMS);
    REFUSED(c.transforms = REGISTER_MAX_TRANSFORMS + 1, REGISTER_TRANSFORMS);
    REFUSED(c.n = 0, REGISTER_COUNT);
    REFUSED(c.n = -1, REGISTER_COUNT);
    REFUSED(c.n = SAMPLE_MAX_POINTS + 1, REGISTER_COUNT);
    REFUSED(c.null_points = true, REGISTER_NULL);
    REFUSED(c.null_xforms = true, REGISTER_NULL);
    REFUSED(c.volume = false, REGISTER_NULL);
    REFUSED(c.null_res = true, REGISTER_NULL);
    REFUSED(c.null_ws = true, REGISTER_NULL);
    REFUSED(c.null_out = true, REGISTER_NULL);
    REFUSED(c.res[0] = 0, REGISTER_RES);
    REFUSED(c.res[2] = -3, REGISTER_RES);
    REFUSED(c.res[1] = 65535 * 4 + 1, REGISTER_RES);
    REFUSED((c.res[1] = 65536, c.res[2] = 32768), REGISTER_RES);     // rows that do not fit an int
    REFUSED(c.step = 33 * 4 - 4, REGISTER_PITCH);
    REFUSED(c.step = 33 * 4 + 2, REGISTER_PITCH);
    REFUSED(c.vs = 0.f, REGISTER_VOXEL);
    REFUSED(c.vs = -0.05f, REGISTER_VOXEL);
    REFUSED(c.vs = nan, REGISTER_VOXEL);
    REFUSED(c.vs = inf, REGISTER_VOXEL);
    REFUSED(c.min_weight = 0, REGISTER_MIN_WEIGHT);
    REFUSED(c.min_weight = -5, REGISTER_MIN_WEIGHT);
    REFUSED(c.max_residual = 0.f, REGISTER_MAX_RESIDUAL);
    REFUSED(c.max_residual = -0.5f, REGISTER_MAX_RESIDUAL);
    REFUSED(c.max_residual = nan, REGISTER_MAX_RESIDUAL);
    REFUSED(c.max_residual = inf, REGISTER_MAX_RESIDUAL);
    REFUSED(c.xforms[0] = nan, REGISTER_NOT_FINITE);
    REFUSED(c.xforms[12 + 11] = -inf, REGISTER_NOT_FINITE);
    REFUSED(c.xforms[35] = inf, REGISTER_NOT_FINITE);                  // the last entry of the last transform
    {   // the order of the checks: the first one decides
        Call c;
        c.transforms = 0; c.n = 0; c.null_points = true; c.vs = 0.f; c.min_weight = 0;
        CHECK(c.run() == REGISTER_TRANSFORMS);
        c.transforms = 2; CHECK(c.run() == REGISTER_COUNT);
        c.n = 5; CHECK(c.run() == REGISTER_NULL);
        c.null_points = false; CHECK(c.run() == REGISTER_VOXEL);
        c.vs = 0.1f; CHECK(c.run() == REGISTER_MIN_WEIGHT);
    }
    for (int r = 0; r <= REGISTER_NOT_FINITE; ++r) CHECK(register_refusal_str(r)[0] != '?');
    CHECK(register_refusal_str(-1)[0] == '?' && register_refusal_str(REGISTER_NOT_FINITE + 1)[0] == '?');
    // xform12 from a double T16: sample_xform12's rule
    {
        double T[16];
        for (int i = 0; i < 16; ++i) T[i] = 0.1 * (double)(i + 1);
        float m[12], want[12];
        for (int i = 0; i < 12; ++i) m[i] = -7.f;
        CHECK(register_xform12(T, m) && sample_xform12(T, want) && !std::memcmp(m, want, sizeof(m)));
        CHECK(m[0] == (float)T[0] && m[5] == (float)T[6] && m[9] == (float)T[3] && m[11] == (float)T[11]);
        float keep[12];
        std::memcpy(keep, m, sizeof(m));
        T[6] = 1e300;                                           // finite in double, not in float
        CHECK(!register_xform12(T, m) && !std::memcmp(keep, m, sizeof(m)));
        T[6] = std::numeric_limits<double>::quiet_NaN();
        CHECK(!register_xform12(T, m) && !register_xform12(nullptr, m));
    }
    // the step: on the sums of an exactly linear problem with no damping it recovers the twist; T <- exp(delta) T
    {
        const double d[6] = {0.01, -0.02, 0.015, 0.003, -0.002, 0.004};
        double s[29];
        sums_of(200, d, s);
        double T[16] = {1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 2, 0, 0, 0, 1}, E[16], want[16];
        const double T0[16] = {1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 2, 0, 0, 0, 1};
        CHECK(register_step(s, 0.0, T));
        align_se3_exp(d, E);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) want[4 * i + j] = E[4 * i] * T0[j] + E[4 * i + 1] * T0[4 + j] + E[4 * i + 2] * T0[8 + j] + (j == 3 ? E[4 * i + 3] : 0.0);
        for (int i = 0; i < 12; ++i) CHECK(std::fabs(T[i] - want[i]) < 1e-9);
        CHECK(T[12] == 0 && T[13] == 0 && T[14] == 0 && T[15] == 1);
        // the same call is align_step's, bit for bit
        double Ta[16], Tb[16];
        std::memcpy(Ta, T0, sizeof(Ta)); std::memcpy(Tb, T0, sizeof(Tb));
        CHECK(register_step(s, 1e-3, Ta) && align_step(s, 1e-3, Tb) && !std::memcmp(Ta, Tb, sizeof(Ta)));
        // fewer than six points, an indefinite system and null pointers refuse and leave T alone
        double few[29];
        std::memcpy(few, s, sizeof(few));
        few[28] = 5;
        std::memcpy(Ta, T0, sizeof(Ta));
        CHECK(!register_step(few, 1e-3, Ta) && !std::memcmp(Ta, T0, sizeof(Ta)));
        double bad[29];
        std::memcpy(bad, s, sizeof(bad));
        bad[0] = -1.0;
        CHECK(!register_step(bad, 1e-3, Ta) && !std::memcmp(Ta, T0, sizeof(Ta)));
        double zero[29] = {};
        CHECK(!register_step(zero, 1e-3, Ta) && !register_step(nullptr, 1e-3, Ta) && !register_step(s, 1e-3, nullptr));
    }
    {   // the cleared report
        double rep[7] = {1, 2, 3, 4, 5, 6, 7};
        register_report_clear(rep);
        CHECK(rep[0] == -1.0);
        for (int i = 1; i < 7; ++i) CHECK(rep[i] == 0.0);
        register_report_clear(nullptr);
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks held\n");
    return 0;
}
