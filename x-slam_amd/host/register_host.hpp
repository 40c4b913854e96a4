// register_host.hpp — the host's side of registering a point cloud to a map (xs_tsdf_register_terms in
// include/xslam_amd.h: the contract): what the call refuses, the float xform12 of a double T16, and the damped step on the 29 sums.  Pure host
// code, no device call and no HIP header: csrc/xs_register.hip validates with it in front of the launch, the orchestrator converts and steps its
// transforms with it between launches, and tests/cxx/register_selftest.cpp runs it under the sanitizers without a GPU.
#pragma once
#include "align_host.hpp"    // align_step: the damped step is the map-to-map alignment's, unchanged
#include "sample_host.hpp"   // sample_xform12, SAMPLE_MAX_POINTS, render_res_ok: the points and the volume are sample_points'

namespace xs_host {

constexpr int REGISTER_MAX_TRANSFORMS = 32;

// why a call is refused (0: it is not); the order is the order of the checks
enum RegisterRefusal : int { REGISTER_ACCEPTED = 0, REGISTER_TRANSFORMS, REGISTER_COUNT, REGISTER_NULL, REGISTER_RES, REGISTER_PITCH, REGISTER_VOXEL,
                             REGISTER_MIN_WEIGHT, REGISTER_MAX_RESIDUAL, REGISTER_NOT_FINITE, REGISTER_STRIDE };
inline const char *register_refusal_str(int r) {
    static const char *const s[] = {"ok", "transforms outside 1 .. XS_REGISTER_MAX_TRANSFORMS", "n outside 1 .. 2^30", "null pointer", "bad resolution", "bad pitch",
                                    "voxel_size is not positive and finite", "min_weight below 1", "max_residual is not finite and positive",
                                    "a transform entry is not finite"};
    return r >= 0 && r <= REGISTER_NOT_FINITE ? s[r] : "?";
}
// the same for xs_tsdf_score_points, which has its own bound on the transforms and refuses a stride as well (REGISTER_STRIDE: that call alone)
inline const char *register_score_refusal_str(int r) {
    return r == REGISTER_TRANSFORMS ? "transforms outside 1 .. XS_REGISTER_SCORE_MAX_TRANSFORMS" : r == REGISTER_STRIDE ? "stride below 1" : register_refusal_str(r);
}

// Everything xs_tsdf_register_terms refuses.  xform12xN: host array, transform m's twelve floats at + 12 m.  max_transforms: the call's bound
// (xs_tsdf_score_points validates with the same table and its own).
inline int register_validate(int transforms, long long n, const void *points, const float *xform12xN, bool have_volume, size_t vol_step, const int *res,
                             float voxel_size, int min_weight, float max_residual, const void *workspace, const void *out,
                             int max_transforms = REGISTER_MAX_TRANSFORMS) {
    if (transforms < 1 || transforms > max_transforms) return REGISTER_TRANSFORMS;
    if (n < 1 || n > SAMPLE_MAX_POINTS) return REGISTER_COUNT;
    if (!points || !xform12xN || !have_volume || !res || !workspace || !out) return REGISTER_NULL;
    if (!render_res_ok(res)) return REGISTER_RES;
    if (vol_step % 4 != 0 || vol_step < (size_t)res[0] * 4) return REGISTER_PITCH;
    if (!(voxel_size > 0.f) || !std::isfinite(voxel_size)) return REGISTER_VOXEL;
    if (min_weight < 1) return REGISTER_MIN_WEIGHT;
    if (!(max_residual > 0.f) || !std::isfinite(max_residual)) return REGISTER_MAX_RESIDUAL;
    for (int i = 0; i < 12 * transforms; ++i)
        if (!std::isfinite(xform12xN[i])) return REGISTER_NOT_FINITE;
    return REGISTER_ACCEPTED;
}

// Everything xs_tsdf_score_points refuses: the table above with its own bound on the transforms, and a stride below 1.
constexpr int REGISTER_SCORE_MAX_TRANSFORMS = 4096;
constexpr long long REGISTER_SEARCH_MAX_SCORED = 1ll << 24;   // the search's bound on ceil(n / stride): "raise the stride"
inline int register_score_validate(int transforms, long long n, int stride, const void *points, const float *xform12xP, bool have_volume, size_t vol_step,
                                   const int *res, float voxel_size, int min_weight, float max_residual, const void *workspace, const void *out) {
    if (transforms < 1 || transforms > REGISTER_SCORE_MAX_TRANSFORMS) return REGISTER_TRANSFORMS;
    if (stride < 1) return REGISTER_STRIDE;
    return register_validate(transforms, n, points, xform12xP, have_volume, vol_step, res, voxel_size, min_weight, max_residual, workspace, out,
                             REGISTER_SCORE_MAX_TRANSFORMS);
}
// the scored points of xs_tsdf_score_points: points 0, stride, 2 stride, ...
inline long long register_scored_points(long long n, int stride) { return (n + stride - 1) / stride; }

// xform12 of xs_tsdf_register_terms from T16 (a real 4 x 4, row-major, taking a point of the cloud's frame to the volume frame): sample_xform12's
// rule, one rounding to float32 per entry; false, nothing written, for an entry that is not finite in double or after the rounding.
inline bool register_xform12(const double *T16, float *out12) { return sample_xform12(T16, out12); }

// One damped step on the sums s = {J^T J upper triangle (21), J^T r (6), sum r^2, count} of xs_tsdf_register_terms, which are the normal
// equations as they stand (no seed: gn_scale_sums is not applied).  J is the derivative of F(exp(delta) T p) at delta = 0 with delta =
// (translation, rotation): exactly the parametrisation align_step solves and applies, (A + damping diag A) delta = -g by Cholesky and
// T <- exp(delta) T in float64.  false, T untouched: fewer than six points, a system that is not positive definite, a step that is not finite.
inline bool register_step(const double s[29], double damping, double T16[16]) { return align_step(s, damping, T16); }

// the report of a registration call that has no result (yet): zeros, and -1 where the winner's index goes
inline void register_report_clear(double *report7) { align_report_clear(report7, 7); }

}  // namespace xs_host
