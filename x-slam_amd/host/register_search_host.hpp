// register_search_host.hpp — the host's side of registering a point cloud to a map with no starting guess: the
// centroid of the scored points, and the defaults and refusals of the search's options.  The candidates, their boxes and their ranking are the
// map-to-map search's (align_search_host.hpp: align_search_free, align_search_around, align_search_rank) with "this" read as the cloud (its
// centroid is centroid_this and the pivot) and "other" as the map (its band centroid); the loop behind the search is gn_multistart through
// RegisterVolume.  No device call and no HIP header, float64 and deterministic: the orchestrator uses it between launches and
// tests/cxx/register_search_selftest.cpp runs all of it under the sanitizers without a GPU.
#pragma once
#include <cmath>
#include <cstring>
#include "align_search_host.hpp"
#include "register_host.hpp"
#include "../../include/xslam_amd_pipeline.h"   // xs_register_search_opts

namespace xs_host {

// The mean of the scored points (points stride i, i = 0 .. ceil(n / stride) - 1) of a host array of n x 3 floats: each axis added in double in
// index order, then divided by the scored count.  False, nothing written: n < 1, stride < 1, a null pointer.
inline bool points_centroid(const float *points, long long n, int stride, double *out3) {
    if (!points || !out3 || n < 1 || stride < 1) return false;
    double s[3] = {0.0, 0.0, 0.0};
    const long long scored = register_scored_points(n, stride);
    for (long long i = 0; i < scored; ++i) {
        const float *p = points + 3 * (size_t)(i * stride);
        s[0] += (double)p[0]; s[1] += (double)p[1]; s[2] += (double)p[2];
    }
    for (int a = 0; a < 3; ++a) out3[a] = s[a] / (double)scored;
    return true;
}

// xs_kf_register_search_defaults: tranc_dist is the map's truncation distance in metres (0 without a volume)
inline void register_search_defaults(double tranc_dist, xs_register_search_opts *o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->struct_bytes = sizeof(*o);
    o->candidates = 2048; o->keep = 8; o->rounds = 2; o->stride = 4; o->iterations = 10; o->min_weight = 1;
    o->box_t = o->refine_t = tranc_dist;
    o->refine_r = 0.25; o->damping = 1e-3; o->max_residual = 0.9;
}

// why the search refuses its options or its cloud (0: it does not); the order is the order of the checks
enum RegisterSearchRefusal : int { RSEARCH_ACCEPTED = 0, RSEARCH_STRUCT, RSEARCH_COUNTS, RSEARCH_BOX, RSEARCH_DAMPING, RSEARCH_MAX_RESIDUAL, RSEARCH_USER,
                                   RSEARCH_POINTS, RSEARCH_SCORED };
inline const char *register_search_refusal_str(int r) {
    static const char *const s[] = {"ok", "struct_bytes is not sizeof(xs_register_search_opts)",
                                    "candidates < 1, keep outside 1 .. 32, rounds < 0, stride < 1, iterations < 0 or min_weight < 1",
                                    "a box is negative or not finite", "damping is negative or not finite", "max_residual is not finite (in float32) and positive",
                                    "user_n < 0, or user_n > 0 without user_T16xN", "n outside 1 .. 2^30", "more than 2^24 scored points: raise the stride"};
    return r >= 0 && r <= RSEARCH_SCORED ? s[r] : "?";
}
// What xs_kf_register_points_global itself refuses (the scoring call and RegisterVolume refuse the rest): the options, then the cloud's size.
inline int register_search_validate(const xs_register_search_opts &o, long long n) {
    if (o.struct_bytes != sizeof(xs_register_search_opts)) return RSEARCH_STRUCT;
    if (o.candidates < 1 || o.keep < 1 || o.keep > 32 || o.rounds < 0 || o.stride < 1 || o.iterations < 0 || o.min_weight < 1) return RSEARCH_COUNTS;
    for (double b : {o.box_t, o.refine_t, o.refine_r})
        if (!(b >= 0.0) || !std::isfinite(b)) return RSEARCH_BOX;
    if (!(o.damping >= 0.0) || !std::isfinite(o.damping)) return RSEARCH_DAMPING;
    if (!(o.max_residual > 0.0) || !std::isfinite((double)(float)o.max_residual) || !((float)o.max_residual > 0.f)) return RSEARCH_MAX_RESIDUAL;
    if (o.user_n < 0 || (o.user_n > 0 && !o.user_T16xN)) return RSEARCH_USER;
    if (n < 1 || n > SAMPLE_MAX_POINTS) return RSEARCH_POINTS;
    if (register_scored_points(n, o.stride) > REGISTER_SEARCH_MAX_SCORED) return RSEARCH_SCORED;
    return RSEARCH_ACCEPTED;
}

}  // namespace xs_host
