// register_search_selftest.cpp — x-slam_amd/host/register_search_host.hpp and the scoring call's refusal table of register_host.hpp under the
// host sanitizers, no GPU: points_centroid against sums formed here (strides, a ragged tail, refusals that write nothing), the options' defaults
// and every refusal of register_search_validate in the order of its checks, register_score_validate's table, and a search round on candidates
// built with the cloud as "this": the centroid lands in its box and a kept transform is entry 0 of its own group.
// Built and run by tests/test_register_score_cpu.py with -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off.
#include "register_search_host.hpp"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

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

static void test_centroid() {
    for (int it = 0; it < 60; ++it) {
        const long long n = 1 + (long long)(uniform() * 700);
        const int stride = 1 + (int)(uniform() * 9);
        std::vector<float> p((size_t)n * 3);   // exactly n points: a read past the last scored one is the sanitizer's to find
        for (auto &v : p) v = (float)(uniform() * 10.0 - 5.0);
        double s[3] = {0, 0, 0};
        long long scored = 0;
        for (long long i = 0; i < n; i += stride, ++scored)
            for (int a = 0; a < 3; ++a) s[a] += (double)p[(size_t)(3 * i + a)];
        CHECK(scored == register_scored_points(n, stride));
        double c[3];
        CHECK(points_centroid(p.data(), n, stride, c));
        for (int a = 0; a < 3; ++a) CHECK(c[a] == s[a] / (double)scored);
        // a strided copy of the scored points at stride 1 gives the same bits (what the orchestrator does for a device cloud)
        std::vector<float> q((size_t)scored * 3);
        for (long long i = 0; i < scored; ++i) std::memcpy(&q[(size_t)(3 * i)], &p[(size_t)(3 * i * stride)], 3 * sizeof(float));
        double c2[3];
        CHECK(points_centroid(q.data(), scored, 1, c2) && std::memcmp(c, c2, sizeof(c)) == 0);
    }
    const float one[3] = {1.5f, -2.25f, 3.0f};
    double c[3] = {-7, -7, -7};
    CHECK(points_centroid(one, 1, 5, c) && c[0] == 1.5 && c[1] == -2.25 && c[2] == 3.0);
    double keep[3] = {c[0], c[1], c[2]};
    CHECK(!points_centroid(nullptr, 1, 1, c) && !points_centroid(one, 0, 1, c) && !points_centroid(one, -3, 1, c) && !points_centroid(one, 1, 0, c));
    CHECK(!points_centroid(one, 1, 1, nullptr) && std::memcmp(keep, c, sizeof(c)) == 0);
}

static void test_options() {
    xs_register_search_opts o;
    std::memset(&o, 0x5a, sizeof(o));
    register_search_defaults(0.3, &o);
    CHECK(o.struct_bytes == sizeof(o) && o.candidates == 2048 && o.keep == 8 && o.rounds == 2 && o.stride == 4 && o.iterations == 10 && o.min_weight == 1);
    CHECK(o.user_n == 0 && o.user_T16xN == nullptr && o.box_t == 0.3 && o.refine_t == 0.3 && o.refine_r == 0.25 && o.damping == 1e-3 && o.max_residual == 0.9);
    register_search_defaults(0.3, nullptr);
    const long long n = 1000;
    CHECK(register_search_validate(o, n) == RSEARCH_ACCEPTED);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto with = [&](auto change) { xs_register_search_opts b = o; change(b); return register_search_validate(b, n); };
    CHECK(with([](auto &b) { b.struct_bytes -= 8; }) == RSEARCH_STRUCT && with([](auto &b) { b.struct_bytes = 0; }) == RSEARCH_STRUCT);
    CHECK(with([](auto &b) { b.candidates = 0; }) == RSEARCH_COUNTS && with([](auto &b) { b.keep = 0; }) == RSEARCH_COUNTS && with([](auto &b) { b.keep = 33; }) == RSEARCH_COUNTS);
    CHECK(with([](auto &b) { b.rounds = -1; }) == RSEARCH_COUNTS && with([](auto &b) { b.stride = 0; }) == RSEARCH_COUNTS && with([](auto &b) { b.iterations = -1; }) == RSEARCH_COUNTS);
    CHECK(with([](auto &b) { b.min_weight = 0; }) == RSEARCH_COUNTS);
    CHECK(with([&](auto &b) { b.box_t = -0.1; }) == RSEARCH_BOX && with([&](auto &b) { b.refine_t = nan; }) == RSEARCH_BOX && with([&](auto &b) { b.refine_r = inf; }) == RSEARCH_BOX);
    CHECK(with([&](auto &b) { b.damping = -1e-9; }) == RSEARCH_DAMPING && with([&](auto &b) { b.damping = nan; }) == RSEARCH_DAMPING);
    CHECK(with([&](auto &b) { b.max_residual = 0.0; }) == RSEARCH_MAX_RESIDUAL && with([&](auto &b) { b.max_residual = nan; }) == RSEARCH_MAX_RESIDUAL);
    CHECK(with([&](auto &b) { b.max_residual = inf; }) == RSEARCH_MAX_RESIDUAL && with([&](auto &b) { b.max_residual = 1e-60; }) == RSEARCH_MAX_RESIDUAL);
    CHECK(with([](auto &b) { b.user_n = -1; }) == RSEARCH_USER && with([](auto &b) { b.user_n = 2; }) == RSEARCH_USER);
    const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    CHECK(with([&](auto &b) { b.user_n = 1; b.user_T16xN = I; }) == RSEARCH_ACCEPTED);
    // the limits themselves, and the first of two errors wins
    CHECK(with([](auto &b) { b.keep = 32; b.rounds = 0; b.iterations = 0; b.box_t = 0; b.refine_t = 0; b.refine_r = 0; b.damping = 0; }) == RSEARCH_ACCEPTED);
    CHECK(with([&](auto &b) { b.keep = 0; b.damping = nan; }) == RSEARCH_COUNTS);
    // the cloud: n, and the scored count
    CHECK(register_search_validate(o, 0) == RSEARCH_POINTS && register_search_validate(o, (1ll << 30) + 1) == RSEARCH_POINTS);
    CHECK(register_search_validate(o, 1ll << 26) == RSEARCH_ACCEPTED && register_search_validate(o, (1ll << 26) + 1) == RSEARCH_SCORED);   // stride 4
    CHECK(with([](auto &b) { b.stride = 1; }) == RSEARCH_ACCEPTED);
    xs_register_search_opts s1 = o;
    s1.stride = 1;
    CHECK(register_search_validate(s1, 1ll << 24) == RSEARCH_ACCEPTED && register_search_validate(s1, (1ll << 24) + 1) == RSEARCH_SCORED);
    s1.stride = 64;
    CHECK(register_search_validate(s1, 1ll << 30) == RSEARCH_ACCEPTED);
    for (int r = 0; r <= RSEARCH_SCORED; ++r) CHECK(std::strlen(register_search_refusal_str(r)) > 1);
    CHECK(std::strcmp(register_search_refusal_str(99), "?") == 0);
}

static void test_score_table() {
    const float x[24] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5f, 0.5f, 0.5f};
    const int res[3] = {33, 17, 20};
    int dummy = 0;
    const void *p = &dummy;
    auto v = [&](int transforms, long long n, int stride, const void *points, const float *xf, bool vol, size_t step, const int *r, float vs, int mw, float mr,
                 const void *ws, const void *out) { return register_score_validate(transforms, n, stride, points, xf, vol, step, r, vs, mw, mr, ws, out); };
    CHECK(v(2, 10, 1, p, x, true, 132, res, 0.05f, 1, 0.9f, p, p) == REGISTER_ACCEPTED);
    CHECK(v(0, 10, 1, p, x, true, 132, res, 0.05f, 1, 0.9f, p, p) == REGISTER_TRANSFORMS && v(4097, 10, 1, p, x, true, 132, res, 0.05f, 1, 0.9f, p, p) == REGISTER_TRANSFORMS);
    CHECK(v(2, 10, 0, p, x, true, 132, res, 0.05f, 1, 0.9f, p, p) == REGISTER_STRIDE && v(2, 10, -2, p, x, true, 132, res, 0.05f, 1, 0.9f, p, p) == REGISTER_STRIDE);
    CHECK(v(2, 0, 1, p, x, true, 132, res, 0.05f, 1, 0.9f, p, p) == REGISTER_COUNT && v(2, (1ll << 30) + 1, 1, p, x, true, 132, res, 0.05f, 1, 0.9f, p, p) == REGISTER_COUNT);
    CHECK(v(2, 10, 1, nullptr, x, true, 132, res, 0.05f, 1, 0.9f, p, p) == REGISTER_NULL && v(2, 10, 1, p, nullptr, true, 132, res, 0.05f, 1, 0.9f, p, p) == REGISTER_NULL);
    CHECK(v(2, 10, 1, p, x, false, 132, res, 0.05f, 1, 0.9f, p, p) == REGISTER_NULL && v(2, 10, 1, p, x, true, 132, nullptr, 0.05f, 1, 0.9f, p, p) == REGISTER_NULL);
    CHECK(v(2, 10, 1, p, x, true, 132, res, 0.05f, 1, 0.9f, nullptr, p) == REGISTER_NULL && v(2, 10, 1, p, x, true, 132, res, 0.05f, 1, 0.9f, p, nullptr) == REGISTER_NULL);
    const int bad_res[3] = {0, 17, 20};
    CHECK(v(2, 10, 1, p, x, true, 132, bad_res, 0.05f, 1, 0.9f, p, p) == REGISTER_RES);
    CHECK(v(2, 10, 1, p, x, true, 128, res, 0.05f, 1, 0.9f, p, p) == REGISTER_PITCH && v(2, 10, 1, p, x, true, 134, res, 0.05f, 1, 0.9f, p, p) == REGISTER_PITCH);
    CHECK(v(2, 10, 1, p, x, true, 132, res, 0.f, 1, 0.9f, p, p) == REGISTER_VOXEL && v(2, 10, 1, p, x, true, 132, res, 0.05f, 0, 0.9f, p, p) == REGISTER_MIN_WEIGHT);
    CHECK(v(2, 10, 1, p, x, true, 132, res, 0.05f, 1, 0.f, p, p) == REGISTER_MAX_RESIDUAL);
    float bad[24];
    std::memcpy(bad, x, sizeof(x));
    bad[23] = std::numeric_limits<float>::infinity();
    CHECK(v(2, 10, 1, p, bad, true, 132, res, 0.05f, 1, 0.9f, p, p) == REGISTER_NOT_FINITE && v(1, 10, 1, p, bad, true, 132, res, 0.05f, 1, 0.9f, p, p) == REGISTER_ACCEPTED);
    // xs_tsdf_register_terms keeps its own bound
    CHECK(register_validate(33, 10, p, x, true, 132, res, 0.05f, 1, 0.9f, p, p) == REGISTER_TRANSFORMS);
    CHECK(std::strcmp(register_score_refusal_str(REGISTER_STRIDE), "stride below 1") == 0 && std::strcmp(register_score_refusal_str(REGISTER_STRIDE + 1), "?") == 0);
    CHECK(std::strstr(register_score_refusal_str(REGISTER_TRANSFORMS), "XS_REGISTER_SCORE_MAX_TRANSFORMS") && std::strcmp(register_score_refusal_str(REGISTER_NULL), "null pointer") == 0);
}

// the search's rounds on the cloud: candidates take the cloud's centroid into the box about the map's, and a kept transform leads its own group
static void test_rounds() {
    const double c_cloud[3] = {7.1, -3.2, 0.4}, c_map[3] = {2.4, 2.3, 2.9}, box = 0.3;
    const int n = 64;
    std::vector<double> T((size_t)n * 16);
    CHECK(align_search_free(n, c_cloud, c_map, box, T.data()));
    for (int i = 0; i < n; ++i) {
        const double *M = &T[(size_t)i * 16];
        for (int a = 0; a < 3; ++a) {
            const double q = M[4 * a] * c_cloud[0] + M[4 * a + 1] * c_cloud[1] + M[4 * a + 2] * c_cloud[2] + M[4 * a + 3];
            CHECK(std::fabs(q - c_map[a]) <= box + 1e-12);
        }
    }
    std::vector<double> out2((size_t)n * 2);
    for (int i = 0; i < n; ++i) { out2[2 * (size_t)i] = 0.25 * (double)(i % 5); out2[2 * (size_t)i + 1] = (double)((i * 37) % 11); }
    int idx[8];
    CHECK(align_search_rank(out2.data(), n, 8, idx) == 8);
    for (int k = 0; k + 1 < 8; ++k) CHECK(score_S(&out2[2 * (size_t)idx[k]]) >= score_S(&out2[2 * (size_t)idx[k + 1]]));
    std::vector<double> group(8 * 16);
    CHECK(align_search_around(&T[(size_t)idx[0] * 16], c_cloud, 0.15, 0.125, 8, group.data()));
    CHECK(std::memcmp(group.data(), &T[(size_t)idx[0] * 16], 16 * sizeof(double)) == 0);
}

int main() {
    test_centroid();
    test_options();
    test_score_table();
    test_rounds();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks held\n");
    return 0;
}
