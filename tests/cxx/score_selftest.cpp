// score_selftest.cpp — x-slam_amd/host/score_host.hpp (the ranking of global relocalisation, no GPU) built with
// -fsanitize=address,undefined and run: the score, the stable top-K with ties, K > P, all-zero scores, and the winner rule.
#include "score_host.hpp"
#include <cstdio>

using namespace xs_host;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static bool is(const std::vector<int> &v, std::initializer_list<int> want) { return v == std::vector<int>(want); }

int main() {
    // {sum loss, count}: S = count - sum loss
    const double a[] = {10.0, 100.0,  /* 90 */   1.0, 3.0,    /* 2: a small mean loss on three voxels does not win */
                        50.0, 140.0,  /* 90: ties with 0 */  0.0, 0.0,  /* 0 */   5.0, 200.0,  /* 195 */   30.0, 120.0 /* 90: ties with 0 and 2 */};
    CHECK(score_S(a) == 90.0 && score_S(a + 2) == 2.0 && score_S(a + 6) == 0.0);
    CHECK(is(score_top_k(a, 6, 1), {4}));
    CHECK(is(score_top_k(a, 6, 2), {4, 0}));                   // the tie goes to the lower index
    CHECK(is(score_top_k(a, 6, 3), {4, 0, 2}));
    CHECK(is(score_top_k(a, 6, 4), {4, 0, 2, 5}));
    CHECK(is(score_top_k(a, 6, 6), {4, 0, 2, 5, 1, 3}));
    CHECK(is(score_top_k(a, 6, 60), {4, 0, 2, 5, 1, 3}));      // K > P: all of them
    CHECK(score_top_k(a, 6, 0).empty() && score_top_k(a, 0, 4).empty() && score_top_k(a, 6, -1).empty());
    CHECK(is(score_top_k(a, 1, 8), {0}));
    // nothing seen by anybody: index order
    const double z[10] = {};
    CHECK(is(score_top_k(z, 5, 3), {0, 1, 2}));
    CHECK(is(score_top_k(z, 5, 9), {0, 1, 2, 3, 4}));
    // many ties in a long list: the K lowest indices of the best score, in order
    std::vector<double> many(2 * 1000, 0.0);
    for (int i = 0; i < 1000; ++i) { many[2 * (size_t)i] = 1.0; many[2 * (size_t)i + 1] = i % 7 == 3 ? 51.0 : 11.0 + (i % 5); }
    const std::vector<int> top = score_top_k(many.data(), 1000, 20);
    CHECK(top.size() == 20);
    for (size_t k = 0; k < top.size(); ++k) CHECK(top[k] == 3 + 7 * (int)k);
    // the winner: highest S among the loops that ended ok
    int ok[6] = {1, 1, 1, 1, 1, 1};
    CHECK(score_winner(a, ok, 6) == 4);
    ok[4] = 0;
    CHECK(score_winner(a, ok, 6) == 0);                        // 0, 2 and 5 tie: the lowest index
    ok[0] = 0;
    CHECK(score_winner(a, ok, 6) == 2);
    ok[2] = 0; ok[5] = 0;
    CHECK(score_winner(a, ok, 6) == 1);
    ok[1] = 0;
    CHECK(score_winner(a, ok, 6) == 3);                        // an ok loop with nothing in view still ended ok
    ok[3] = 0;
    CHECK(score_winner(a, ok, 6) == -1);                       // nothing ended ok
    CHECK(score_winner(a, ok, 0) == -1);
    const int all[5] = {1, 1, 1, 1, 1};
    CHECK(score_winner(z, all, 5) == 0);
    if (!failures) std::printf("all checks held\n");
    return failures ? 1 : 0;
}
