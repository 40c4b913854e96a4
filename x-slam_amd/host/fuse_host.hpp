// fuse_host.hpp — the host's side of fusing a point cloud into the map (xs_tsdf_fuse_points_accumulate and
// xs_tsdf_fuse_points_fold in include/xslam_amd.h: the contract): what the two calls refuse, K (the half steps behind the point), the transformed
// origin, the float xform12 of a double T16, and the runs a cloud is cut into so that no accumulator field can overflow between two folds.  Pure
// host code, no device call and no HIP header: csrc/xs_fuse.hip validates with it in front of its launches, the orchestrator chunks with it, and
// tests/cxx/fuse_selftest.cpp runs it under the sanitizers without a GPU.
#pragma once
#include <climits>
#include "register_host.hpp"   // register_xform12, render_res_ok: the transform is the registration's result, the volume rules the merge's

namespace xs_host {

constexpr long long FUSE_MAX_POINTS = (1ll << 24) - 1;   // between two folds: count < 2^24, sum q <= (2^24 - 1) 2^16 < 2^40
constexpr int FUSE_MAX_HALF_STEPS = 256;
constexpr float FUSE_MAX_RAY_STEPS = 1048576.f;          // 2^20: max_range / step above it is refused, so k_far fits an int with room to spare
constexpr int FUSE_MAX_WEIGHT = 1 << 24;                 // the merge's limit on max_weight

// why a call is refused (0: it is not); the order is the order of the checks
enum FuseRefusal : int { FUSE_ACCEPTED = 0, FUSE_COUNT, FUSE_NULL, FUSE_STRUCT, FUSE_RES, FUSE_PITCH, FUSE_VOXEL, FUSE_TRANC, FUSE_HALF_STEPS, FUSE_NOT_FINITE,
                         FUSE_MIN_RANGE, FUSE_MAX_RANGE, FUSE_RAY_STEPS, FUSE_PLANES, FUSE_MAX_WEIGHT_RANGE, FUSE_OBS_WEIGHT };
inline const char *fuse_refusal_str(int r) {
    static const char *const s[] = {"ok", "n outside 1 .. 2^24 - 1", "null pointer", "opts->struct_bytes is not sizeof(xs_fuse_opts)", "bad resolution", "bad pitch",
                                    "voxel_size is not positive and finite", "tranc_dist is not positive and finite", "K above XS_FUSE_MAX_HALF_STEPS",
                                    "a transform, origin or range entry is not finite", "min_range is not positive", "max_range below min_range",
                                    "max_range / step above 2^20", "empty or reversed plane range", "max_weight outside [1, 1 << 24]",
                                    "obs_weight outside [1, max_weight]"};
    return r >= 0 && r <= FUSE_OBS_WEIGHT ? s[r] : "?";
}

// K = (int)ceilf(tranc_dist / step), step = 0.5f * voxel_size: the contract's float32 operations.  INT_MAX where the quotient is not a number
// an int holds (the callers refuse it with every K above the cap).
inline int fuse_half_steps(float voxel_size, float tranc_dist) {
    const float step = 0.5f * voxel_size;
    const float k = std::ceil(tranc_dist / step);
    return (k >= 0.f && k < 2147483648.f) ? (int)k : INT_MAX;
}

// O = T o by xs_tsdf_sample_points' formula (float32, in the order written); without a transform the origin's bits as they are
inline void fuse_origin(const float *xform12, const float *origin3, float out3[3]) {
    for (int c = 0; c < 3; ++c)
        out3[c] = xform12 ? ((xform12[3 * c] * origin3[0] + xform12[3 * c + 1] * origin3[1]) + xform12[3 * c + 2] * origin3[2]) + xform12[9 + c] : origin3[c];
}

// Everything xs_tsdf_fuse_points_accumulate refuses.  xform12: null for "the points as they are".
inline int fuse_validate_accumulate(long long n, const void *points, const float *xform12, const float *origin3, const int *res, float voxel_size, float tranc_dist,
                                    bool have_opts, unsigned struct_bytes, unsigned expected_bytes, float min_range, float max_range, const void *accumulator,
                                    const void *counts) {
    if (n < 1 || n > FUSE_MAX_POINTS) return FUSE_COUNT;
    if (!points || !origin3 || !res || !have_opts || !accumulator || !counts) return FUSE_NULL;
    if (struct_bytes != expected_bytes) return FUSE_STRUCT;
    if (!render_res_ok(res)) return FUSE_RES;
    if (!(voxel_size > 0.f) || !std::isfinite(voxel_size)) return FUSE_VOXEL;
    if (!(tranc_dist > 0.f) || !std::isfinite(tranc_dist)) return FUSE_TRANC;
    if (fuse_half_steps(voxel_size, tranc_dist) > FUSE_MAX_HALF_STEPS) return FUSE_HALF_STEPS;
    if (xform12)
        for (int i = 0; i < 12; ++i)
            if (!std::isfinite(xform12[i])) return FUSE_NOT_FINITE;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(origin3[i])) return FUSE_NOT_FINITE;
    if (!std::isfinite(min_range) || !std::isfinite(max_range)) return FUSE_NOT_FINITE;
    if (!(min_range > 0.f)) return FUSE_MIN_RANGE;
    if (max_range < min_range) return FUSE_MAX_RANGE;
    if (!(max_range / (0.5f * voxel_size) <= FUSE_MAX_RAY_STEPS)) return FUSE_RAY_STEPS;
    return FUSE_ACCEPTED;
}

// Everything xs_tsdf_fuse_points_fold refuses.
inline int fuse_validate_fold(bool have_volume, size_t step, const int *res, int z0, int z1, const void *accumulator, int obs_weight, int max_weight) {
    if (!have_volume || !res || !accumulator) return FUSE_NULL;
    if (!render_res_ok(res)) return FUSE_RES;
    if (step % 4 != 0 || step < (size_t)res[0] * 4) return FUSE_PITCH;
    if (z0 < 0 || z1 > res[2] || z1 <= z0) return FUSE_PLANES;
    if (max_weight < 1 || max_weight > FUSE_MAX_WEIGHT) return FUSE_MAX_WEIGHT_RANGE;
    if (obs_weight < 1 || obs_weight > max_weight) return FUSE_OBS_WEIGHT;
    return FUSE_ACCEPTED;
}

// the accumulator of a volume: one 64-bit word per voxel; 0 for an unusable resolution
inline size_t fuse_accumulator_bytes(const int *res) {
    return render_res_ok(res) ? (size_t)res[0] * (size_t)res[1] * (size_t)res[2] * sizeof(unsigned long long) : 0;
}

// xform12 from T16 (a real 4 x 4, row-major, the cloud's frame to the volume frame): the registration's rule, so that the transform
// register_points returns is fused at the bits it was scored at
inline bool fuse_xform12(const double *T16, float *out12) { return register_xform12(T16, out12); }

// A cloud of n points is fused in runs of at most FUSE_MAX_POINTS points, a fold after each: the runs are as long as the limit allows and the
// last one takes the rest.  fuse_run_count: how many (0 for n < 1); fuse_run: run i's first point and length, false past the last run.
inline long long fuse_run_count(long long n) { return n < 1 ? 0 : (n + FUSE_MAX_POINTS - 1) / FUSE_MAX_POINTS; }
inline bool fuse_run(long long n, long long i, long long *first, long long *count) {
    if (i < 0 || i >= fuse_run_count(n)) return false;
    *first = i * FUSE_MAX_POINTS;
    *count = n - *first < FUSE_MAX_POINTS ? n - *first : FUSE_MAX_POINTS;
    return true;
}

}  // namespace xs_host
