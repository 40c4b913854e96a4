// sample_host.hpp — the host's side of sampling a map at the caller's points (xs_tsdf_sample_points and
// xs_tsdf_sample_depth in include/xslam_amd.h: the contract): what the two calls refuse, the float xform12 of a double T16, and the composition
// "the points are in frame A, T maps A to the volume".  Pure host code, no device call and no HIP header: csrc/xs_sample.hip validates with it
// in front of the launch, the orchestrator converts its transforms with it, and tests/cxx/sample_selftest.cpp runs it under the sanitizers
// without a GPU.
#pragma once
#include <cmath>
#include <cstddef>
#include "render_host.hpp"   // render_res_ok, RENDER_MAX_IMAGE: the volume and image rules are render's

namespace xs_host {

constexpr long long SAMPLE_MAX_POINTS = 1ll << 30;
enum : int { SAMPLE_OUTSIDE = 0, SAMPLE_UNSEEN = 1, SAMPLE_OK = 2, SAMPLE_NO_DEPTH = 3 };   // the status byte, and the index into counts4
enum : int { SAMPLE_DEPTH_MIN = 200, SAMPLE_DEPTH_MAX = 5000 };                              // xs_scale_depth's rule, millimetres

// why a call is refused (0: it is not); the order is the order of the checks
enum SampleRefusal : int { SAMPLE_ACCEPTED = 0, SAMPLE_COUNT, SAMPLE_IMAGE, SAMPLE_NULL, SAMPLE_NO_OUTPUT, SAMPLE_NO_GRAD, SAMPLE_ALIAS, SAMPLE_STRUCT, SAMPLE_RES,
                           SAMPLE_PITCH, SAMPLE_DEPTH_PITCH, SAMPLE_NOT_FINITE, SAMPLE_FOCAL, SAMPLE_VOXEL };
inline const char *sample_refusal_str(int r) {
    static const char *const s[] = {"ok", "n outside 1 .. 2^30", "rows or cols outside 1 .. 4096", "null pointer", "every output is null",
                                    "dvalue wanted without a grad array", "an output is the input array", "opts->struct_bytes is not sizeof(xs_sample_opts)",
                                    "bad resolution", "bad pitch", "a depth pitch shorter than a row or odd", "a transform, pose or intrinsic entry is not finite",
                                    "fx or fy is 0", "voxel_size is not positive and finite"};
    return r >= 0 && r <= SAMPLE_VOXEL ? s[r] : "?";
}

// the outputs of a call as the validation sees them
struct SampleOutputPtrs { const void *status, *value, *dvalue, *gradient, *counts; };

// what both calls share, after the checks of their own input: the outputs, the options' size, the volume, the voxel size
inline int sample_validate_volume(const void *input, const SampleOutputPtrs &o, bool have_volume, bool have_grad, size_t vol_step, const int *res, float voxel_size,
                                  unsigned struct_bytes, unsigned expected_bytes) {
    if (!input || !res || !have_volume) return SAMPLE_NULL;
    if (!o.status && !o.value && !o.dvalue && !o.gradient && !o.counts) return SAMPLE_NO_OUTPUT;
    if (o.dvalue && !have_grad) return SAMPLE_NO_GRAD;
    if (o.status == input || o.value == input || o.dvalue == input || o.gradient == input || o.counts == input) return SAMPLE_ALIAS;
    if (struct_bytes != expected_bytes) return SAMPLE_STRUCT;
    if (!render_res_ok(res)) return SAMPLE_RES;
    if (vol_step % 4 != 0 || vol_step < (size_t)res[0] * 4) return SAMPLE_PITCH;
    if (!(voxel_size > 0.f) || !std::isfinite(voxel_size)) return SAMPLE_VOXEL;
    return SAMPLE_ACCEPTED;
}

// Everything xs_tsdf_sample_points refuses.  xform12: null for "the points as they are".
inline int sample_validate_points(long long n, const void *points, const float *xform12, const SampleOutputPtrs &o, bool have_volume, bool have_grad, size_t vol_step,
                                  const int *res, float voxel_size, unsigned struct_bytes, unsigned expected_bytes) {
    if (n < 1 || n > SAMPLE_MAX_POINTS) return SAMPLE_COUNT;
    const int why = sample_validate_volume(points, o, have_volume, have_grad, vol_step, res, voxel_size, struct_bytes, expected_bytes);
    if (why != SAMPLE_ACCEPTED) return why;
    if (xform12)
        for (int i = 0; i < 12; ++i)
            if (!std::isfinite(xform12[i])) return SAMPLE_NOT_FINITE;
    return SAMPLE_ACCEPTED;
}

// Everything xs_tsdf_sample_depth refuses.
inline int sample_validate_depth(const void *depth, size_t depth_step, int rows, int cols, const float *intr4, const float *Rc2v9, const float *tc2v3,
                                 const SampleOutputPtrs &o, bool have_volume, bool have_grad, size_t vol_step, const int *res, float voxel_size, unsigned struct_bytes,
                                 unsigned expected_bytes) {
    if (rows < 1 || rows > RENDER_MAX_IMAGE || cols < 1 || cols > RENDER_MAX_IMAGE) return SAMPLE_IMAGE;
    if (!intr4 || !Rc2v9 || !tc2v3) return SAMPLE_NULL;
    const int why = sample_validate_volume(depth, o, have_volume, have_grad, vol_step, res, voxel_size, struct_bytes, expected_bytes);
    if (why != SAMPLE_ACCEPTED) return why;
    if (depth_step % 2 != 0 || depth_step < (size_t)cols * 2) return SAMPLE_DEPTH_PITCH;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(Rc2v9[i])) return SAMPLE_NOT_FINITE;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(tc2v3[i])) return SAMPLE_NOT_FINITE;
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(intr4[i])) return SAMPLE_NOT_FINITE;
    if (intr4[0] == 0.f || intr4[1] == 0.f) return SAMPLE_FOCAL;
    return SAMPLE_ACCEPTED;
}

// xform12 of xs_tsdf_sample_points (row-major R, then t) from T16: a real 4 x 4, row-major, taking a point of the frame the points are given in
// to the volume frame, both in metres.  One rounding to float32 per entry.  False, with nothing written, for an entry of rows 0 .. 2 that is
// not finite, in double or after the rounding.
inline bool sample_xform12(const double *T16, float *out12) {
    if (!T16 || !out12) return false;
    float m[12];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) m[3 * r + c] = (float)T16[4 * r + c];
        m[9 + r] = (float)T16[4 * r + 3];
    }
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(T16[i]) || !std::isfinite(m[i])) return false;
    for (int i = 0; i < 12; ++i) out12[i] = m[i];
    return true;
}

// The points are in a frame P that T_p2a takes to frame A, and T_a2v takes A to the volume: T16 = T_a2v T_p2a, the one transform the call wants
// (a scan in its sensor's frame with the sensor's pose in the world, and the world's pose in the map).  Affine: the last rows are taken as
// (0, 0, 0, 1) whatever they hold.  Float64, in the order written.
inline void sample_compose(const double *T_a2v16, const double *T_p2a16, double *T16) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)
            T16[4 * r + c] = (T_a2v16[4 * r] * T_p2a16[c] + T_a2v16[4 * r + 1] * T_p2a16[4 + c]) + T_a2v16[4 * r + 2] * T_p2a16[8 + c];
        T16[4 * r + 3] = ((T_a2v16[4 * r] * T_p2a16[3] + T_a2v16[4 * r + 1] * T_p2a16[7]) + T_a2v16[4 * r + 2] * T_p2a16[11]) + T_a2v16[4 * r + 3];
    }
    T16[12] = 0.0; T16[13] = 0.0; T16[14] = 0.0; T16[15] = 1.0;
}

}  // namespace xs_host
