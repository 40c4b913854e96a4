// travel_selftest.cpp — the travel side of x-slam_amd/host/view_host.hpp (no GPU) built with -fsanitize=address,undefined and run:
// travel_limit and travel_bias (metres as the field's units) and next_view_by_travel (what a view sees against how far away it is).
#include "view_host.hpp"
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

using namespace xs_host;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // travel_limit: on and beside integer multiples of a binary voxel size
    CHECK(travel_limit(0.f, 0.125f) == 65534 && travel_limit(-1.f, 0.125f) == 65534 && travel_limit(inf, 0.125f) == 65534 && travel_limit(nan, 0.125f) == 65534);
    CHECK(travel_limit(1.f, 0.125f) == 24 && travel_limit(std::nextafter(1.f, 0.f), 0.125f) == 23 && travel_limit(std::nextafter(1.f, 2.f), 0.125f) == 24);
    CHECK(travel_limit(0.125f, 0.125f) == 3 && travel_limit(0.04f, 0.125f) == 0 && travel_limit(0.05f, 0.125f) == 1);
    CHECK(travel_limit(2730.f, 0.125f) == 65520 && travel_limit(2730.6f, 0.125f) == 65534 && travel_limit(1e30f, 0.125f) == 65534 && travel_limit(3e38f, 0.125f) == 65534);
    CHECK(travel_limit(1.f, 0.f) == 65534);                                     // a divide by zero: the cap
    for (int k = 1; k <= 21844; k += 7) CHECK(travel_limit(0.25f * (float)k, 0.25f) == 3 * k);
    // travel_bias
    CHECK(travel_bias(0.f, 0.125f) == 1 && travel_bias(0.01f, 0.125f) == 1 && travel_bias(0.125f, 0.125f) == 3 && travel_bias(0.5f, 0.125f) == 12);
    CHECK(travel_bias(std::nextafter(0.5f, 1.f), 0.125f) == 13 && travel_bias(std::nextafter(0.5f, 0.f), 0.125f) == 12 && travel_bias(-3.f, 0.125f) == 1);
    CHECK(travel_bias(1e30f, 0.125f) == (1 << 30) && travel_bias(inf, 0.125f) == (1 << 30) && travel_bias(nan, 0.125f) == (1 << 30));
    // next_view_by_travel over {unknown, free, hits, frontier}
    const std::vector<unsigned> a = {100, 5, 10, 1, 900, 0, 0, 7, 300, 9, 10, 2, 300, 1, 50, 3, 50, 2, 400, 0, 300, 4, 9, 4};
    const std::vector<unsigned short> near0 = {0, 0, 0, 0, 0, 0}, none(6, 65535);
    for (unsigned h : {0u, 9u, 10u, 11u, 51u, 401u})                            // everybody at distance 0: the unweighted rule
        CHECK(next_view_by_travel(a.data(), near0.data(), 6, h, 3) == next_best_view(a.data(), 6, h));
    CHECK(next_view_by_travel(a.data(), none.data(), 6, 0, 3) == -1 && next_view_by_travel(a.data(), nullptr, 6, 0, 3) == -1);
    CHECK(next_view_by_travel(a.data(), near0.data(), 0, 0, 3) == -1 && next_view_by_travel(nullptr, nullptr, 0, 0, 3) == -1 && next_view_by_travel(a.data(), near0.data(), -2, 0, 3) == -1);
    const std::vector<unsigned short> t1 = {3, 65535, 30, 12, 0, 27};           // 100/6, -, 300/33, 300/15 = 20, 50/3, 300/30 = 10
    CHECK(next_view_by_travel(a.data(), t1.data(), 6, 0, 3) == 3 && next_view_by_travel(a.data(), t1.data(), 6, 51, 3) == 4);
    CHECK(next_view_by_travel(a.data(), t1.data(), 6, 0, 300) == 3);            // a large fixed cost: the counts decide, 300/312 is the nearest of the 300s
    CHECK(next_view_by_travel(a.data(), t1.data(), 6, 0, 1) == 4);              // a small one: 50/1 at distance 0 beats 300/13
    CHECK(next_view_by_travel(a.data(), t1.data(), 6, 401, 3) == -1);
    const std::vector<unsigned short> t2 = {0, 0, 10, 10, 0, 10};               // 2, 3 and 5 tie at 300/13: the lowest index
    CHECK(next_view_by_travel(a.data(), t2.data(), 6, 9, 3) == 0);              // 100/3 beats 300/13
    CHECK(next_view_by_travel(a.data() + 8, t2.data() + 2, 4, 9, 3) == 0 && next_view_by_travel(a.data() + 12, t2.data() + 3, 3, 9, 3) == 0);
    CHECK(next_view_by_travel(a.data(), t2.data(), 6, 9, 0) == next_view_by_travel(a.data(), t2.data(), 6, 9, 1));   // a bias below 1 counts as 1
    // a pair float32 would order wrongly: 4000000000 / 2 against 2000000001 / 1
    const std::vector<unsigned> big = {4000000000u, 0, 1, 0, 2000000001u, 0, 1, 0};
    const std::vector<unsigned short> tb = {1, 0};
    CHECK(next_view_by_travel(big.data(), tb.data(), 2, 1, 1) == 1);
    CHECK(4000000000.f / 2.f == 2000000001.f / 1.f);
    // the largest operands: no overflow
    const std::vector<unsigned> top = {4294967295u, 0, 1, 0, 4294967294u, 0, 1, 0};
    const std::vector<unsigned short> tt = {65534, 65534};
    CHECK(next_view_by_travel(top.data(), tt.data(), 2, 1, 1 << 30) == 0);
    const std::vector<unsigned short> tu = {65534, 65533};
    CHECK(next_view_by_travel(top.data(), tu.data(), 2, 1, 1) == 1);            // 4294967295 / 65535 < 4294967294 / 65534
    if (!failures) std::printf("all checks held\n");
    return failures ? 1 : 0;
}
