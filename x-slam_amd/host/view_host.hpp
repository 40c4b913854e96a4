// view_host.hpp — the host's side of next-best-view selection (DESIGN.md sections 4.18, 4.19 and 4.20): which of the candidate views that xs_score_views
// has counted {unknown, free, hits, frontier} for the camera should go to next.  Pure host code, no device call and no HIP header: the
// orchestrator uses it behind the launch and tests/cxx/view_selftest.cpp runs it under the sanitizers without a GPU.
#pragma once
#include <cmath>
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

// The same rule restricted to the candidates a body can get to: reachable[p] != 0 says the centre voxel of pose p
// was reached by the flood from the camera.  -1 when no reachable pose qualifies (or P <= 0, or reachable is null).
inline int next_reachable_view(const unsigned *out4xP, const unsigned char *reachable, int P, unsigned min_hits) {
    int best = -1;
    if (!reachable) return best;
    for (int p = 0; p < P; ++p) {
        const unsigned *o = out4xP + 4 * (size_t)p;
        if (!reachable[p] || o[2] < min_hits) continue;
        if (best < 0 || o[0] > out4xP[4 * (size_t)best]) best = p;
    }
    return best;
}

// A body's radius in metres as the clearance field's integers: rv = radius_m / voxel_size (one float32 divide), r2 = max(1, (int)ceilf(rv * rv))
// (a voxel is passable where field >= r2), R the smallest integer with R * R >= r2 (the field's cap).  False, with nothing written, for
// a radius or a voxel size that is negative, zero (the voxel size), not finite, or that needs R above 255.
inline bool reach_radius(float radius_m, float voxel_size, int &r2, int &R) {
    if (!(voxel_size > 0.f) || !(radius_m >= 0.f) || !std::isfinite(radius_m) || !std::isfinite(voxel_size)) return false;
    const float rv = radius_m / voxel_size;
    const float sq = std::ceil(rv * rv);
    if (!(sq <= 65025.f)) return false;
    const int q = (int)sq < 1 ? 1 : (int)sq;
    int r = 1;
    while (r * r < q) ++r;
    if (r > 255) return false;
    r2 = q; R = r;
    return true;
}

// Travel costs are in units of a third of a voxel edge, uint16, 65535 = not reached or beyond the limit.
enum : int { TRAVEL_NONE = 65535, TRAVEL_MAX = 65534 };

// The farthest travel in metres as the field's limit: 65534 for max_travel_m <= 0 or not finite (no limit but the number format's),
// otherwise min(65534, (int)floorf(3 * max_travel_m / voxel_size)) in float32.
inline int travel_limit(float max_travel_m, float voxel_size) {
    if (!(max_travel_m > 0.f) || !std::isfinite(max_travel_m)) return TRAVEL_MAX;
    const float units = std::floor(3.f * max_travel_m / voxel_size);
    return units < (float)TRAVEL_MAX ? (int)units : (int)TRAVEL_MAX;   // (a NaN or an infinity from the divide: the cap)
}

// The fixed cost of taking any view at all, in the field's units: max(1, (int)ceilf(3 * bias_m / voxel_size)); what does not fit an int
// (or is no number) saturates at 2^30.
inline int travel_bias(float bias_m, float voxel_size) {
    const float units = std::ceil(3.f * bias_m / voxel_size);
    if (!(units < 1073741824.f)) return 1 << 30;
    return units < 1.f ? 1 : (int)units;
}

// Weighs what a view sees against how far away it is: among the poses with travel[p] != TRAVEL_NONE and hits (out4xP[4 p + 2]) >= min_hits
// the one with the largest unknown[p] / (travel[p] + bias3), compared by cross-multiplication in 64-bit integers (unknown < 2^32 and
// travel + bias3 <= 2^16 + 2^30: no overflow, no rounding).  Equal ratios: the lower index.  -1 when no pose qualifies (or P <= 0, or
// travel is null).  bias3 >= 1 keeps a candidate at distance 0 from winning by division alone.
inline int next_view_by_travel(const unsigned *out4xP, const unsigned short *travel, int P, unsigned min_hits, int bias3) {
    int best = -1;
    if (!travel) return best;
    const unsigned long long bias = (unsigned long long)(bias3 < 1 ? 1 : bias3);
    for (int p = 0; p < P; ++p) {
        const unsigned *o = out4xP + 4 * (size_t)p;
        if (travel[p] == TRAVEL_NONE || o[2] < min_hits) continue;
        if (best < 0) { best = p; continue; }
        const unsigned long long lhs = (unsigned long long)o[0] * ((unsigned long long)travel[best] + bias);
        const unsigned long long rhs = (unsigned long long)out4xP[4 * (size_t)best] * ((unsigned long long)travel[p] + bias);
        if (lhs > rhs) best = p;
    }
    return best;
}

}  // namespace xs_host
