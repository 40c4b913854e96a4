// newton_selftest.cpp — x-slam_amd/host/newton_host.hpp (the host's side of a Newton pass, no GPU) built with
// -fsanitize=address,undefined and run: the 21 seeded poses of a rigid camera2volume and the step on definite, indefinite and empty sums.
#include "newton_host.hpp"
#include <cstdio>
#include <cstring>

using namespace xs_host;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

int main() {
    hostComplex xi[6] = {{0.3f, 0.f}, {-0.2f, 0.f}, {1.1f, 0.f}, {0.2f, 0.f}, {-0.4f, 0.f}, {0.1f, 0.f}};
    Matrix4cf c2v = se3Exp(xi);
    float R[21][36], t[21][12];
    newton_seeded_poses(c2v, R, t);
    for (int p = 1; p < 21; ++p)
        for (int e = 0; e < 9; ++e) CHECK(std::memcmp(&R[p][4 * e], &R[0][4 * e], sizeof(float)) == 0);
    for (int p = 0; p < 21; ++p) {
        float seed = 0.f;
        for (int e = 0; e < 9; ++e) seed += std::fabs(R[p][4 * e + 1]) + std::fabs(R[p][4 * e + 2]);
        for (int e = 0; e < 3; ++e) seed += std::fabs(t[p][4 * e + 1]) + std::fabs(t[p][4 * e + 2]);
        CHECK(seed > 0.f && seed < 1e-4f);
    }
    double s[29] = {};
    int q = 0;
    for (int j = 0; j < 6; ++j) for (int k = j; k < 6; ++k, ++q) s[q] = j == k ? 100.0 + j : 1.0;
    for (int k = 0; k < 6; ++k) s[21 + k] = 0.5 * (k - 2);
    s[27] = 3.0; s[28] = 1000.0;
    Matrix4cf m = c2v;
    CHECK(newton_step(s, 1e-3, m));
    CHECK(std::memcmp(&m, &c2v, sizeof(m)) != 0);
    Matrix4cf keep = m;
    s[0] = -100.0;                                   // indefinite
    CHECK(!newton_step(s, 1e-3, m) && std::memcmp(&m, &keep, sizeof(m)) == 0);
    s[0] = 100.0; s[28] = 5.0;                       // nothing to align to
    CHECK(!newton_step(s, 1e-3, m) && std::memcmp(&m, &keep, sizeof(m)) == 0);
    double raw[29], scaled[29];
    for (int i = 0; i < 29; ++i) raw[i] = 1e-12;
    newton_scale_sums(raw, scaled);
    CHECK(std::fabs(scaled[0] - 1.0) < 1e-9 && std::fabs(scaled[21] - 1e-6) < 1e-15 && scaled[27] == 1e-12 && scaled[28] == 1e-12);
    if (!failures) std::printf("all checks held\n");
    return failures ? 1 : 0;
}
