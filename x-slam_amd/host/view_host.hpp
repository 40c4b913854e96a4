// view_host.hpp — the host's side of next-best-view selection (DESIGN.md sections 4.18 to 4.21): which of the candidate views that xs_score_views
// has counted {unknown, free, hits, frontier} for the camera should go to next, and the algebra that turns frontier clusters into candidate views.  Pure host code, no device call and no HIP header: the
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

// ---- frontier clusters as candidate views ----
// A cluster record of xs_frontier_clusters: {label, count, sum x, sum y, sum z, packed min, packed max, 0}.
enum : int { FRONTIER_RECORD_WORDS = 8 };

// The centre of voxel v along one axis, in metres: (float(v) + 0.5f) * voxel_size.  floorf(centre / voxel_size) gives v back for every
// index a volume can have (v <= 65535: v + 0.5 is exact, the product and the quotient are each within 2^-24 relative of the true values,
// so the quotient stays within (v + 0.5) * 2^-23 < 0.5 of v + 0.5; tests/cxx/frontier_selftest.cpp walks the whole range).
inline float voxel_centre(int v, float voxel_size) { return ((float)v + 0.5f) * voxel_size; }

// The centroid of a record in metres: per axis q = float(double(sum) / double(count)) (one float64 divide, rounded once to float32), then
// (q + 0.5f) * voxel_size.  False, with nothing written, for a record with count 0.
inline bool frontier_centroid(const unsigned long long *rec, float voxel_size, float c[3]) {
    if (rec[1] == 0ull) return false;
    for (int a = 0; a < 3; ++a) c[a] = ((float)((double)rec[2 + a] / (double)rec[1]) + 0.5f) * voxel_size;
    return true;
}

// Element `index` (>= 1) of the van der Corput sequence in `base`: exact in float64 for base 2, a few roundings for base 3.
inline double halton(unsigned index, unsigned base) {
    double f = 1.0, r = 0.0;
    while (index > 0u) {
        f /= (double)base;
        r += f * (double)(index % base);
        index /= base;
    }
    return r;
}

// Direction j of a cluster's standpoints: the unit vector of the Halton pair (u, v) = (halton(j + 1, 2), halton(j + 1, 3)) with
// z = 1 - 2 u and phi = 2 pi v, computed in float64 and rounded to float32 at the end.
inline void frontier_direction(int j, float d[3]) {
    const double u = halton((unsigned)j + 1u, 2u), v = halton((unsigned)j + 1u, 3u);
    const double z = 1.0 - 2.0 * u, r = std::sqrt(z * z < 1.0 ? 1.0 - z * z : 0.0), phi = 6.283185307179586476925286766559 * v;
    d[0] = (float)(r * std::cos(phi)); d[1] = (float)(r * std::sin(phi)); d[2] = (float)z;
}

// Standpoint j of a cluster with centroid c: p = c + standoff * d_j, one float32 multiply and one add per axis.
inline void frontier_standpoint(const float c[3], float standoff_m, int j, float p[3]) {
    float d[3];
    frontier_direction(j, d);
    for (int a = 0; a < 3; ++a) p[a] = c[a] + standoff_m * d[a];
}

// The hint is not used when it is within acos(LOOK_AT_HINT_COS) = 8.1 degrees of the view direction (either way round).
constexpr double LOOK_AT_HINT_COS = 0.99;

// A camera-to-volume rotation R (row-major, columns = the camera's x, y and z axes in volume coordinates) for a camera at `pos` whose
// optical axis (the third column) points at `target`.  The image-down axis (the second column) is as close to hint_down as orthogonality
// allows: x = normalise(hint x z), y = z x x.  Where hint_down is within 8.1 degrees of +-z, hint_side takes its place.  Computed in
// float64, rounded to float32 at the end.  False, with nothing written, when target == pos, when an input is not finite, or when neither
// hint has a usable component across z.
inline bool look_at(const float pos[3], const float target[3], const float hint_down[3], const float hint_side[3], float R9[9]) {
    double z[3], n2 = 0.0;
    for (int a = 0; a < 3; ++a) { z[a] = (double)target[a] - (double)pos[a]; n2 += z[a] * z[a]; }
    if (!(n2 > 0.0) || !std::isfinite(n2)) return false;
    const double n = std::sqrt(n2);
    for (int a = 0; a < 3; ++a) z[a] /= n;
    const float *hints[2] = {hint_down, hint_side};
    for (int k = 0; k < 2; ++k) {
        double h[3], hn2 = 0.0;
        for (int a = 0; a < 3; ++a) { h[a] = (double)hints[k][a]; hn2 += h[a] * h[a]; }
        if (!(hn2 > 0.0) || !std::isfinite(hn2)) continue;
        const double hn = std::sqrt(hn2), dot = (h[0] * z[0] + h[1] * z[1] + h[2] * z[2]) / hn;
        if (std::fabs(dot) > LOOK_AT_HINT_COS) continue;
        double x[3] = {h[1] * z[2] - h[2] * z[1], h[2] * z[0] - h[0] * z[2], h[0] * z[1] - h[1] * z[0]};
        const double xn = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
        for (int a = 0; a < 3; ++a) x[a] /= xn;
        const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
        for (int a = 0; a < 3; ++a) { R9[3 * a] = (float)x[a]; R9[3 * a + 1] = (float)y[a]; R9[3 * a + 2] = (float)z[a]; }
        return true;
    }
    return false;
}

// The indices of the records (n of them, 8 words each) with at least min_size voxels, in order, into out (room for n); their number.
inline int frontier_select(const unsigned long long *records, int n, unsigned long long min_size, int *out) {
    int m = 0;
    for (int i = 0; i < n; ++i)
        if (records[(size_t)i * FRONTIER_RECORD_WORDS + 1] >= min_size) out[m++] = i;
    return m;
}

// The cells of the labelling: 0 (one cell, the whole volume) or a multiple of 8 in 8 .. 65528.
inline bool frontier_cell_valid(int cell) { return cell == 0 || (cell >= 8 && cell <= 65528 && cell % 8 == 0); }

}  // namespace xs_host
