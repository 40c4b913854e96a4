// score_host.hpp — the host's side of global relocalisation: how the {sum loss, count} pairs of
// xs_tsdf_score_poses_band rank pose hypotheses, which of them go on to the Gauss-Newton refinement and which refined pose wins.  Pure
// host code, no device call and no HIP header: the orchestrator uses it between launches and tests/cxx/score_selftest.cpp runs it under
// the sanitizers without a GPU.
#pragma once
#include <algorithm>
#include <vector>

namespace xs_host {

// The truncated-quadratic inlier score of a pose: a kept voxel counts 1 - r^2 (r^2 <= 1: the kernel's last gate), a dropped one 0 — as
// if its residual were 1.  S = count - sum loss, higher is better.  The mean loss alone would let a pose that sees three voxels well beat
// one that sees the whole room.
inline double score_S(const double *out2) { return out2[1] - out2[0]; }

// The indices of the min(K, P) best of P candidates (out2xP: {sum loss, count} per candidate), best first; equal scores in index order.
inline std::vector<int> score_top_k(const double *out2xP, int P, int K) {
    std::vector<int> order;
    if (P <= 0 || K <= 0) return order;
    order.resize((size_t)P);
    for (int i = 0; i < P; ++i) order[(size_t)i] = i;
    const size_t keep = (size_t)std::min(K, P);
    auto better = [&](int a, int b) {
        const double sa = score_S(out2xP + 2 * (size_t)a), sb = score_S(out2xP + 2 * (size_t)b);
        return sa > sb || (sa == sb && a < b);   // a strict total order: no stable sort needed
    };
    std::partial_sort(order.begin(), order.begin() + (std::ptrdiff_t)keep, order.end(), better);
    order.resize(keep);
    return order;
}

// Of K refined candidates (out2xK: their scores after refinement; ok[k]: candidate k's loop ended ok) the one with the highest S among
// those that ended ok, the lower index on equal scores; -1 when none did.
inline int score_winner(const double *out2xK, const int *ok, int K) {
    int best = -1;
    for (int k = 0; k < K; ++k) {
        if (!ok[k]) continue;
        if (best < 0 || score_S(out2xK + 2 * (size_t)k) > score_S(out2xK + 2 * (size_t)best)) best = k;
    }
    return best;
}

}  // namespace xs_host
