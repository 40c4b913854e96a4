// reach_selftest.cpp — the reachability side of x-slam_amd/host/view_host.hpp (no GPU) built with -fsanitize=address,undefined and run:
// next_reachable_view (the next-best-view rule restricted to reachable candidates) and reach_radius (a radius in metres as r2 and R).
#include "view_host.hpp"
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

using namespace xs_host;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

int main() {
    // {unknown, free, hits, frontier}: the table of view_selftest.cpp
    const std::vector<unsigned> a = {100, 5, 10, 1, 900, 0, 0, 7, 300, 9, 10, 2, 300, 1, 50, 3, 50, 2, 400, 0, 300, 4, 9, 4};
    const std::vector<unsigned char> all(6, 1), none(6, 0);
    for (unsigned h : {0u, 1u, 9u, 10u, 11u, 51u, 401u})                        // everybody reachable: the unrestricted rule
        CHECK(next_reachable_view(a.data(), all.data(), 6, h) == next_best_view(a.data(), 6, h));
    CHECK(next_reachable_view(a.data(), none.data(), 6, 0) == -1);             // nobody reachable
    CHECK(next_reachable_view(a.data(), nullptr, 6, 0) == -1);
    const std::vector<unsigned char> r1 = {1, 0, 0, 1, 1, 1};                   // 2 (the unrestricted winner at 10) is out of reach
    CHECK(next_best_view(a.data(), 6, 10) == 2 && next_reachable_view(a.data(), r1.data(), 6, 10) == 3);
    CHECK(next_reachable_view(a.data(), r1.data(), 6, 9) == 3);                // 3 and 5 tie: the lower index
    CHECK(next_reachable_view(a.data(), r1.data(), 6, 0) == 3);                // 1 sees the most but cannot be reached
    CHECK(next_reachable_view(a.data(), r1.data(), 6, 51) == 4 && next_reachable_view(a.data(), r1.data(), 6, 401) == -1);
    const std::vector<unsigned char> r2v = {1, 0, 0, 0, 0, 1};                  // any non-zero byte counts
    CHECK(next_reachable_view(a.data(), r2v.data(), 6, 10) == 0 && next_reachable_view(a.data(), r2v.data(), 6, 9) == 5);
    const std::vector<unsigned char> r3 = {0, 0, 0, 0, 0, 200};
    CHECK(next_reachable_view(a.data(), r3.data(), 6, 9) == 5 && next_reachable_view(a.data(), r3.data(), 6, 10) == -1);
    CHECK(next_reachable_view(a.data(), all.data(), 0, 0) == -1 && next_reachable_view(nullptr, nullptr, 0, 0) == -1 && next_reachable_view(a.data(), all.data(), -2, 0) == -1);
    CHECK(next_reachable_view(a.data() + 20, all.data(), 1, 9) == 0 && next_reachable_view(a.data() + 20, none.data(), 1, 9) == -1);
    // a long list: the first reachable qualifying index among ties
    std::vector<unsigned> many(4 * 1000, 0u);
    std::vector<unsigned char> flags(1000, 0);
    for (int i = 0; i < 1000; ++i) { many[4 * (size_t)i] = 77; many[4 * (size_t)i + 2] = i % 7 == 3 ? 20u : 5u; flags[(size_t)i] = i >= 501; }
    CHECK(next_reachable_view(many.data(), flags.data(), 1000, 20) == 507 && next_reachable_view(many.data(), flags.data(), 1000, 5) == 501);

    // reach_radius: on and beside integer multiples of the voxel size
    int q = -7, R = -7;
    CHECK(reach_radius(0.f, 0.05f, q, R) && q == 1 && R == 1);                  // a point: r2 is at least 1
    CHECK(reach_radius(0.05f, 0.05f, q, R) && q == 1 && R == 1);
    CHECK(reach_radius(0.1f, 0.05f, q, R) && q == 4 && R == 2);
    CHECK(reach_radius(0.5f, 0.25f, q, R) && q == 4 && R == 2);                 // exact in binary
    CHECK(reach_radius(std::nextafter(0.5f, 1.f), 0.25f, q, R) && q == 5 && R == 3);
    CHECK(reach_radius(std::nextafter(0.5f, 0.f), 0.25f, q, R) && q == 4 && R == 2);
    CHECK(reach_radius(0.75f, 0.25f, q, R) && q == 9 && R == 3);
    CHECK(reach_radius(0.8f, 0.25f, q, R) && q == 11 && R == 4);                // 3.2^2 = 10.24
    CHECK(reach_radius(63.75f, 0.25f, q, R) && q == 65025 && R == 255);         // the largest radius
    q = R = -7;
    CHECK(!reach_radius(std::nextafter(63.75f, 100.f), 0.25f, q, R) && q == -7 && R == -7);
    CHECK(!reach_radius(64.f, 0.25f, q, R) && !reach_radius(1e30f, 0.25f, q, R) && !reach_radius(-0.1f, 0.25f, q, R) && !reach_radius(0.1f, 0.f, q, R));
    CHECK(!reach_radius(0.1f, -1.f, q, R) && !reach_radius(std::numeric_limits<float>::quiet_NaN(), 0.25f, q, R));
    CHECK(!reach_radius(std::numeric_limits<float>::infinity(), 0.25f, q, R) && !reach_radius(0.1f, std::numeric_limits<float>::infinity(), q, R));
    CHECK(!reach_radius(0.1f, std::numeric_limits<float>::quiet_NaN(), q, R) && q == -7 && R == -7);
    for (int k = 1; k <= 255; ++k) {                                            // every integer multiple of a binary voxel size
        CHECK(reach_radius(0.125f * (float)k, 0.125f, q, R) && q == k * k && R == k);
    }
    if (!failures) std::printf("all checks held\n");
    return failures ? 1 : 0;
}
