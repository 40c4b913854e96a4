// view_selftest.cpp — x-slam_amd/host/view_host.hpp (the next-best-view selection rule, no GPU) built with -fsanitize=address,undefined
// and run: the rule, ties, nobody qualifies, P = 1, min_hits = 0.
#include "view_host.hpp"
#include <cstdio>
#include <vector>

using namespace xs_host;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

int main() {
    // {unknown, free, hits, frontier}
    const std::vector<unsigned> a = {100, 5, 10, 1,   /* 0 */
                                     900, 0, 0, 7,    /* 1: the most unknown space, no surface in view */
                                     300, 9, 10, 2,   /* 2 */
                                     300, 1, 50, 3,   /* 3: ties with 2 */
                                     50, 2, 400, 0,   /* 4 */
                                     300, 4, 9, 4};   /* 5: ties with 2 and 3, one hit short of 10 */
    CHECK(next_best_view(a.data(), 6, 10) == 2);      // 1 has no hits; 2 and 3 tie: the lower index; 5 does not qualify
    CHECK(next_best_view(a.data(), 6, 11) == 3);
    CHECK(next_best_view(a.data(), 6, 51) == 4);
    CHECK(next_best_view(a.data(), 6, 401) == -1);    // nobody qualifies
    CHECK(next_best_view(a.data(), 6, 0) == 1);       // min_hits 0: everybody does
    CHECK(next_best_view(a.data(), 6, 1) == 2);
    CHECK(next_best_view(a.data(), 6, 9) == 2);       // 5 qualifies now and ties: still the lower index
    CHECK(next_best_view(a.data() + 8, 4, 9) == 0);   // (2, 3, 4, 5 alone)
    CHECK(next_best_view(a.data() + 20, 1, 9) == 0);  // P = 1
    CHECK(next_best_view(a.data() + 20, 1, 10) == -1);
    CHECK(next_best_view(a.data() + 4, 1, 0) == 0 && next_best_view(a.data() + 4, 1, 1) == -1);
    CHECK(next_best_view(a.data(), 0, 0) == -1 && next_best_view(nullptr, 0, 0) == -1 && next_best_view(a.data(), -3, 0) == -1);
    // nothing seen by anybody
    const std::vector<unsigned> z(4 * 5, 0u);
    CHECK(next_best_view(z.data(), 5, 0) == 0 && next_best_view(z.data(), 5, 1) == -1);
    // counts near the top of the range compare as unsigned
    const std::vector<unsigned> big = {0x7fffffffu, 0, 0xffffffffu, 0, 0xfffffffeu, 0, 0x80000000u, 0, 0xffffffffu, 0, 0x80000000u, 0};
    CHECK(next_best_view(big.data(), 3, 0x80000000u) == 2);
    CHECK(next_best_view(big.data(), 2, 0x80000000u) == 1);
    CHECK(next_best_view(big.data(), 3, 0xffffffffu) == 0);
    // a long list of ties: the first qualifying index
    std::vector<unsigned> many(4 * 1000, 0u);
    for (int i = 0; i < 1000; ++i) { many[4 * (size_t)i] = 77; many[4 * (size_t)i + 2] = i % 7 == 3 ? 20u : 5u; }
    CHECK(next_best_view(many.data(), 1000, 20) == 3 && next_best_view(many.data(), 1000, 5) == 0 && next_best_view(many.data(), 1000, 21) == -1);
    if (!failures) std::printf("all checks held\n");
    return failures ? 1 : 0;
}
