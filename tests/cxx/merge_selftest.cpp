// merge_selftest.cpp — x-slam_amd/host/merge_host.hpp under the host sanitizers, no GPU: merge_affine against the closed forms, map_transform's
// round trip, second_map_ok's table, and merge_tile_box (the text the merge kernel compiles for the device) against the per-voxel indices of whole tiles.
// Built and run by tests/test_merge_cases_cpu.py with -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off.
#include "merge_host.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
static double uniform(double lo, double hi) { return lo + (hi - lo) * uniform(); }

static void rotation(const double axis[3], double angle, double R[9]) {
    const double n = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    const double a[3] = {axis[0] / n, axis[1] / n, axis[2] / n}, c = std::cos(angle), s = std::sin(angle);
    const double K[9] = {0, -a[2], a[1], a[2], 0, -a[0], -a[1], a[0], 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (i == j ? c : 0.0) + s * K[3 * i + j] + (1 - c) * a[i] * a[j];
}
static void rigid(double T[16]) {
    const double axis[3] = {uniform(-1, 1), uniform(-1, 1), uniform(0.1, 1)};
    double R[9];
    rotation(axis, uniform(-3, 3), R);
    std::memset(T, 0, 16 * sizeof(double));
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * i + j];
        T[4 * i + 3] = uniform(-4, 4);
    }
    T[15] = 1.0;
}

static void test_affine() {
    const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    float m[12];
    CHECK(merge_affine(I, 0.1, 0.1, m));
    for (int i = 0; i < 9; ++i) CHECK(m[i] == (i % 4 == 0 ? 1.f : 0.f));
    for (int a = 0; a < 3; ++a) CHECK(m[9 + a] == 0.f);
    // a shift by whole voxels: t = k vs gives the offset k up to the rounding of the quotient
    double S[16];
    std::memcpy(S, I, sizeof(I));
    S[3] = 3 * 0.125; S[7] = -2 * 0.125; S[11] = 5 * 0.125;
    CHECK(merge_affine(S, 0.125, 0.125, m));
    CHECK(m[9] == 3.f && m[10] == -2.f && m[11] == 5.f);
    // ratios: a destination voxel twice the size covers two source voxels and its centre sits between two of them
    CHECK(merge_affine(I, 0.25, 0.125, m));
    CHECK(m[0] == 2.f && m[4] == 2.f && m[8] == 2.f && m[9] == 0.5f);
    CHECK(merge_affine(I, 0.125, 0.25, m));
    CHECK(m[0] == 0.5f && m[9] == -0.25f);
    // refusals leave the output alone
    float keep[12];
    for (int i = 0; i < 12; ++i) keep[i] = m[i] = 77.f + (float)i;
    double B[16];
    std::memcpy(B, I, sizeof(I));
    B[6] = std::numeric_limits<double>::quiet_NaN();
    CHECK(!merge_affine(B, 0.1, 0.1, m));
    B[6] = std::numeric_limits<double>::infinity();
    CHECK(!merge_affine(B, 0.1, 0.1, m));
    CHECK(!merge_affine(I, 0.0, 0.1, m) && !merge_affine(I, 0.1, -1.0, m) && !merge_affine(I, std::numeric_limits<double>::infinity(), 0.1, m));
    CHECK(!merge_affine(nullptr, 0.1, 0.1, m) && !merge_affine(I, 0.1, 0.1, nullptr));
    B[6] = 1e300;   // finite in float64, not in float32
    CHECK(!merge_affine(B, 1.0, 1e-10, m));
    CHECK(std::memcmp(keep, m, sizeof(m)) == 0);
    // the definition, on random rigid transforms: the centre of destination voxel d lands on the continuous source index m d + o
    for (int it = 0; it < 200; ++it) {
        double T[16];
        rigid(T);
        const double vd = uniform(0.01, 0.2), vs = uniform(0.01, 0.2);
        CHECK(merge_affine(T, vd, vs, m));
        const int d[3] = {(int)uniform(0, 500), (int)uniform(0, 500), (int)uniform(0, 500)};
        for (int a = 0; a < 3; ++a) {
            double p = T[4 * a + 3];
            for (int c = 0; c < 3; ++c) p += T[4 * a + c] * (d[c] + 0.5) * vd;
            const double want = p / vs - 0.5;
            const double got = (double)m[3 * a] * d[0] + (double)m[3 * a + 1] * d[1] + (double)m[3 * a + 2] * d[2] + (double)m[9 + a];
            CHECK(std::fabs(got - want) <= 1e-6 * (1500.0 * vd / vs + std::fabs(want) + 1.0));
        }
    }
}

static void test_transform() {
    for (int it = 0; it < 200; ++it) {
        double A[16], B[16], T[16], back[16];
        rigid(A);
        rigid(B);
        map_transform(A, B, T);
        // T takes this map's frame to the other's: T A = B
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) {
                double s = 0;
                for (int k = 0; k < 4; ++k) s += T[4 * r + k] * A[4 * k + c];
                CHECK(std::fabs(s - B[4 * r + c]) < 1e-12);
            }
        map_transform(A, A, T);
        for (int i = 0; i < 16; ++i) CHECK(std::fabs(T[i] - (i % 5 == 0 ? 1.0 : 0.0)) < 1e-12);
        map_transform(A, B, T);
        map_transform(B, A, back);   // the inverse
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) {
                double s = 0;
                for (int k = 0; k < 4; ++k) s += T[4 * r + k] * back[4 * k + c];
                CHECK(std::fabs(s - (r == c ? 1.0 : 0.0)) < 1e-12);
            }
    }
}

// every voxel of the tile that passes the contract's step 2 reads corners inside the box; a tile reported as a miss has no such voxel
static void check_tile(const float m[12], const int lo[3], const int hi[3], const int S[3]) {
    int box[6] = {-7, -7, -7, -7, -7, -7};
    const bool hit = merge_tile_box(m, lo, hi, S, box);
    if (hit)
        for (int a = 0; a < 3; ++a) CHECK(0 <= box[a] && box[a] <= box[3 + a] && box[3 + a] <= S[a] - 1);
    for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y)
            for (int x = lo[0]; x <= hi[0]; ++x) {
                float g[3];
                bool inside = true;
                for (int a = 0; a < 3; ++a) {
                    g[a] = merge_index(m, a, x, y, z);
                    inside = inside && g[a] >= 0.f && g[a] <= (float)(S[a] - 1);
                }
                if (!inside) continue;
                CHECK(hit);
                if (!hit) return;
                for (int a = 0; a < 3; ++a) {
                    const int b = (int)std::floor(g[a]);
                    const int top = g[a] - (float)b > 0.f ? b + 1 : b;
                    CHECK(box[a] <= b && top <= box[3 + a]);
                }
            }
}

static void test_tile_box() {
    for (int it = 0; it < 3000; ++it) {
        const int S[3] = {1 + (int)uniform(0, 70), 1 + (int)uniform(0, 70), 1 + (int)uniform(0, 70)};
        float m[12];
        const int kind = it % 5;
        if (kind == 0) {   // a rotation with a scale, the image near the source
            const double axis[3] = {uniform(-1, 1), uniform(-1, 1), uniform(0.1, 1)};
            double R[9];
            rotation(axis, uniform(-3, 3), R);
            const double s = uniform(0.3, 2.5);
            for (int i = 0; i < 9; ++i) m[i] = (float)(s * R[i]);
            for (int a = 0; a < 3; ++a) m[9 + a] = (float)uniform(-40, 80);
        } else if (kind == 1) {   // integer shifts and half shifts: indices exactly on faces
            for (int i = 0; i < 9; ++i) m[i] = i % 4 == 0 ? 1.f : 0.f;
            for (int a = 0; a < 3; ++a) m[9 + a] = (float)((int)uniform(-20, 20)) * 0.5f;
        } else if (kind == 2) {   // anything
            for (int i = 0; i < 12; ++i) m[i] = (float)uniform(-3, 3);
        } else if (kind == 3) {   // huge entries: overflow to infinities and NaNs inside the tile
            for (int i = 0; i < 12; ++i) m[i] = (float)uniform(-1, 1) * 3e38f;
        } else {                  // tiny entries and negative zeros
            for (int i = 0; i < 12; ++i) m[i] = (it & 8) ? -0.f : (float)uniform(-1e-30, 1e-30);
            m[9] = (float)uniform(-1, 3);
        }
        int lo[3], hi[3];
        const int ext[3] = {64, 4, 4};
        for (int a = 0; a < 3; ++a) {
            lo[a] = ext[a] * (int)uniform(0, 6);
            hi[a] = lo[a] + (int)uniform(0, ext[a]);   // whole tiles and the clipped ones at a volume's far faces
        }
        check_tile(m, lo, hi, S);
    }
    // the far face: the last voxel exactly on S - 1
    const float id[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const int S[3] = {64, 4, 4}, lo[3] = {0, 0, 0}, hi[3] = {63, 3, 3};
    int box[6];
    CHECK(merge_tile_box(id, lo, hi, S, box));
    CHECK(box[0] == 0 && box[3] == 63 && box[4] == 3 && box[5] == 3);
    const float off[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 64, 0, 0};
    CHECK(!merge_tile_box(off, lo, hi, S, box));
    const float neg[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, -3.5f, 0};
    CHECK(!merge_tile_box(neg, lo, hi, S, box));
}

// second_map_ok: one case per rule and per parameter combination.  The accepted map first; every other row changes one thing about it.
static void test_second_map() {
    static float this_value[4], this_grad[4], value[4], grad[4];
    static int this_weight[4], weight[4];
    const float td = 0.03f;
    const SecondMap good{value, weight, grad, 40, {10, 3, 2}, 0.01f, td};   // a pitch of exactly 4 X
    auto ok = [&](const SecondMap &m, int min_axis, bool need_grad) { return second_map_ok(m, min_axis, need_grad, td, this_value, this_weight, this_grad); };
    auto with = [&](void (*change)(SecondMap &)) { SecondMap m = good; change(m); return m; };
    struct Row { SecondMap m; int min_axis; bool need_grad, want; const char *what; };
    const Row rows[] = {
        {good, 1, true, true, "the map, for a merge"},
        {good, 2, false, true, "the map, for an alignment"},
        {with([](SecondMap &m) { m.value = nullptr; }), 1, false, false, "no value array"},
        {with([](SecondMap &m) { m.weight = nullptr; }), 1, false, false, "no weight array"},
        {with([](SecondMap &m) { m.grad = nullptr; }), 1, true, false, "no grad array where it is needed"},
        {with([](SecondMap &m) { m.grad = nullptr; }), 1, false, true, "no grad array where it is not"},
        {with([](SecondMap &m) { m.res[0] = 0; m.step = 4; }), 1, false, false, "an axis of 0 (x)"},
        {with([](SecondMap &m) { m.res[1] = 0; }), 1, false, false, "an axis of 0 (y)"},
        {with([](SecondMap &m) { m.res[2] = 0; }), 1, false, false, "an axis of 0 (z)"},
        {with([](SecondMap &m) { m.res[2] = -3; }), 1, false, false, "a negative axis"},
        {with([](SecondMap &m) { m.res[2] = 1; }), 1, false, true, "an axis of 1, minimum 1"},
        {with([](SecondMap &m) { m.res[2] = 1; }), 2, false, false, "an axis of 1, minimum 2"},
        {with([](SecondMap &m) { m.res[0] = 1; m.step = 4; }), 2, false, false, "an x axis of 1, minimum 2"},
        {with([](SecondMap &m) { m.res[0] = 1; m.step = 4; }), 1, true, true, "a volume of one column"},
        {with([](SecondMap &m) { m.voxel_size = 0.f; }), 1, false, false, "a voxel size of 0"},
        {with([](SecondMap &m) { m.voxel_size = -0.01f; }), 1, false, false, "a negative voxel size"},
        {with([](SecondMap &m) { m.voxel_size = std::numeric_limits<float>::quiet_NaN(); }), 1, false, false, "a voxel size that is NaN"},
        {with([](SecondMap &m) { m.voxel_size = std::numeric_limits<float>::infinity(); }), 1, false, false, "an infinite voxel size"},
        {with([](SecondMap &m) { m.voxel_size = 7.f; }), 2, true, true, "another voxel size"},
        {with([](SecondMap &m) { m.tranc_dist = std::nextafter(m.tranc_dist, 1.f); }), 1, false, false, "a truncation distance one ulp above"},
        {with([](SecondMap &m) { m.tranc_dist = std::nextafter(m.tranc_dist, 0.f); }), 2, false, false, "a truncation distance one ulp below"},
        {with([](SecondMap &m) { m.value = this_value; }), 1, false, false, "this map's value array"},
        {with([](SecondMap &m) { m.weight = this_weight; }), 2, false, false, "this map's weight array"},
        {with([](SecondMap &m) { m.grad = this_grad; }), 1, true, false, "this map's grad array, for a merge"},
        {with([](SecondMap &m) { m.grad = this_grad; }), 1, false, true, "this map's grad array where grad is not read"},
        {with([](SecondMap &m) { m.step = 36; }), 1, false, false, "a pitch below 4 X"},
        {with([](SecondMap &m) { m.step = 0; }), 1, false, false, "no pitch"},
        {with([](SecondMap &m) { m.step = 42; }), 1, false, false, "a pitch that is no multiple of 4"},
        {with([](SecondMap &m) { m.step = 256; }), 2, true, true, "a padded pitch"},
    };
    for (const Row &r : rows) {
        const bool got = ok(r.m, r.min_axis, r.need_grad);
        if (got != r.want) { std::printf("FAILED second_map_ok: %s\n", r.what); ++failures; }
    }
    CHECK(!second_map_ok(SecondMap{}, 1, false, 0.f, this_value, this_weight, this_grad));   // the empty descriptor
}

int main() {
    test_second_map();
    test_affine();
    test_transform();
    test_tile_box();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks held\n");
    return 0;
}
