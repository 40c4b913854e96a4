// view_host.hpp — the host's side of next-best-view selection: which of the candidate views that xs_score_views
// has counted {unknown, free, hits, frontier} for the camera should go to next.  Pure host code, no device call and no HIP header: the
// orchestrator uses it behind the launch and tests/cxx/view_selftest.cpp runs it under the sanitizers without a GPU.
#pragma once
#include <cstddef>

namespace xs_host {

// The pose that sees the most unknown space (out4xP[4 p]) among those that still see min_hits rays end on a known surface
// (out4xP[4 p + 2] >= min_hits): a view with no known surface in it cannot be tracked by the ICP, so it cannot win however much unknown
// space it looks at.  Equal counts: the lower index.  -1 when no pose qualifies (or P <= 0).
inline int next_best_view(const unsigned *out4xP, int P, unsigned min_hits) {
    int best = -1;
    for (int p = 0; p < P; ++p) {
        const unsigned *o = out4xP + 4 * (size_t)p;
        if (o[2] < min_hits) continue;
        if (best < 0 || o[0] > out4xP[4 * (size_t)best]) best = p;
    }
    return best;
}

}  // namespace xs_host
