// render_host.hpp — the host's side of rendering views of a map (xs_render_views in include/xslam_amd.h: the contract): what
// the call refuses, the number of samples per ray exactly as the kernel counts them, the brick mask's sizes and the workspace's layout, and
// the real pose of a view from a camera2volume matrix.  Pure host code, no device call and no HIP header: csrc/xs_render.hip validates with it
// in front of the launch, the orchestrator sizes its buffers with it, and tests/cxx/render_selftest.cpp runs it under the sanitizers
// without a GPU.
#pragma once
#include <cmath>
#include <cstddef>

namespace xs_host {

enum : int { RENDER_MAX_VIEWS = 64, RENDER_MAX_SAMPLES = 4096, RENDER_MAX_IMAGE = 4096, RENDER_POSE_FLOATS = 12, RENDER_BRICK = 8,
             RENDER_HEADER_BYTES = 256,                                          // the workspace's first bytes: RenderHeader
             RENDER_STAGING_BYTES = RENDER_MAX_VIEWS * RENDER_POSE_FLOATS * 4 }; // behind it: one launch's poses, then the mask words
constexpr unsigned RENDER_MAGIC = 0x52444e52u;   // "RNDR"

// what xs_render_mask_build leaves at the start of the workspace and xs_render_views with the cull reads back
struct RenderHeader { unsigned magic; int res[3]; int min_weight; };

// why a call is refused (0: it is not); the order is the order of the checks
enum RenderRefusal : int { RENDER_OK = 0, RENDER_VIEWS, RENDER_IMAGE, RENDER_NULL, RENDER_NO_OUTPUT, RENDER_STRUCT, RENDER_RES, RENDER_PITCH, RENDER_NOT_FINITE,
                           RENDER_FOCAL, RENDER_VOXEL, RENDER_STEP, RENDER_RANGE, RENDER_SAMPLES, RENDER_SHADE_MODE, RENDER_MASK };
inline const char *render_refusal_str(int r) {
    static const char *const s[] = {"ok", "views outside 1 .. XS_RENDER_MAX_VIEWS", "rows or cols outside 1 .. 4096", "null pointer", "every output is null",
                                    "opts->struct_bytes is not sizeof(xs_render_opts)", "bad resolution", "bad pitch", "a pose or intrinsic entry is not finite",
                                    "fx or fy is 0", "voxel_size is not positive and finite", "step is negative or not finite", "t_far <= t_near, or not finite",
                                    "more than 4096 samples per ray", "unknown shade_mode", "the cull needs a mask built in this workspace for this resolution"};
    return r >= 0 && r <= RENDER_MASK ? s[r] : "?";
}

// the resolutions the launches can index: xs_tsdf_merge's rule (an axis in 1 .. 65535 x 4, rows that fit an int)
inline bool render_res_ok(const int *r) {
    if (!r) return false;
    for (int k = 0; k < 3; ++k)
        if (r[k] < 1 || r[k] > 65535 * 4) return false;
    return (long long)r[1] * (long long)r[2] < (1ll << 31);
}

// The brick mask: bricks of 8 x 8 x 8 voxels, BX x BY x BZ of them, a row of BX bits padded to WX whole words
struct RenderMaskDims { int BX, BY, BZ, WX; size_t words; };
inline bool render_mask_dims(const int *res, RenderMaskDims &m) {
    if (!render_res_ok(res)) return false;
    m.BX = (res[0] + RENDER_BRICK - 1) / RENDER_BRICK; m.BY = (res[1] + RENDER_BRICK - 1) / RENDER_BRICK; m.BZ = (res[2] + RENDER_BRICK - 1) / RENDER_BRICK;
    m.WX = (m.BX + 31) / 32;
    m.words = (size_t)m.WX * (size_t)m.BY * (size_t)m.BZ;
    return true;
}
inline size_t render_mask_offset() { return (size_t)RENDER_HEADER_BYTES + (size_t)RENDER_STAGING_BYTES; }
inline size_t render_workspace_bytes(const int *res) {
    RenderMaskDims m;
    if (!render_mask_dims(res, m)) return 0;
    return render_mask_offset() + (m.words * sizeof(unsigned) + 255) / 256 * 256;
}

// The samples of a ray: the number of k = 0, 1, ... with t_near + float(k) * step < t_far, the kernel's own expression (monotone in k), counted
// up to RENDER_MAX_SAMPLES + 1 (which means "too many").  step > 0.
inline int render_samples(float t_near, float t_far, float step) {
    int n = 0;
    while (n <= RENDER_MAX_SAMPLES && t_near + (float)n * step < t_far) ++n;
    return n;
}

// the options with their defaults applied, as the kernel takes them
struct RenderPlan { float t_near, t_far, step; int min_weight, samples; };

// Everything xs_render_views refuses except the mask's header (which lives on the device).  struct_bytes: opts->struct_bytes, or expected_bytes
// for null opts; the option values are the caller's, 0 where opts is null.  any_output: at least one output pointer is not null.
inline int render_validate(int views, const float *Rc2v9xP, const float *tc2v3xP, const float *intr4, int rows, int cols, bool have_volume, size_t vol_step,
                           const int *res, float voxel_size, unsigned struct_bytes, unsigned expected_bytes, float t_near, float t_far, float step,
                           int min_weight, int shade_mode, bool have_workspace, bool any_output, RenderPlan &plan) {
    if (views < 1 || views > RENDER_MAX_VIEWS) return RENDER_VIEWS;
    if (rows < 1 || rows > RENDER_MAX_IMAGE || cols < 1 || cols > RENDER_MAX_IMAGE) return RENDER_IMAGE;
    if (!Rc2v9xP || !tc2v3xP || !intr4 || !res || !have_volume || !have_workspace) return RENDER_NULL;
    if (!any_output) return RENDER_NO_OUTPUT;
    if (struct_bytes != expected_bytes) return RENDER_STRUCT;
    if (!render_res_ok(res)) return RENDER_RES;
    if (vol_step % 4 != 0 || vol_step < (size_t)res[0] * 4) return RENDER_PITCH;
    for (int i = 0; i < 9 * views; ++i)
        if (!std::isfinite(Rc2v9xP[i])) return RENDER_NOT_FINITE;
    for (int i = 0; i < 3 * views; ++i)
        if (!std::isfinite(tc2v3xP[i])) return RENDER_NOT_FINITE;
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(intr4[i])) return RENDER_NOT_FINITE;
    if (intr4[0] == 0.f || intr4[1] == 0.f) return RENDER_FOCAL;
    if (!(voxel_size > 0.f) || !std::isfinite(voxel_size)) return RENDER_VOXEL;
    if (!(step >= 0.f) || !std::isfinite(step)) return RENDER_STEP;
    plan.t_near = t_near; plan.t_far = t_far;
    if (t_near == 0.f && t_far == 0.f) { plan.t_near = 0.2f; plan.t_far = 5.0f; }
    plan.step = step == 0.f ? voxel_size : step;
    plan.min_weight = min_weight < 1 ? 1 : min_weight;
    if (!std::isfinite(plan.t_near) || !std::isfinite(plan.t_far) || !(plan.t_far > plan.t_near)) return RENDER_RANGE;
    plan.samples = render_samples(plan.t_near, plan.t_far, plan.step);
    if (plan.samples > RENDER_MAX_SAMPLES) return RENDER_SAMPLES;
    if (shade_mode != 0) return RENDER_SHADE_MODE;
    return RENDER_OK;
}

// whether a header read back from the workspace allows the cull for (res, min_weight): built for this res with a min_weight not above the call's
// (a brick with no negative voxel of weight >= m has none of weight >= m' >= m either)
inline bool render_mask_usable(const RenderHeader &h, const int *res, int min_weight) {
    return h.magic == RENDER_MAGIC && h.res[0] == res[0] && h.res[1] == res[1] && h.res[2] == res[2] && h.min_weight >= 1 && h.min_weight <= min_weight;
}

// The real pose of a view from a camera2volume matrix: 4 x 4 row-major with `stride` floats per entry (1: real, 2: (re, im) pairs, of which only
// the real part is used) into a row-major rotation and a translation.
inline void render_pose(const float *c2v, int stride, float R9[9], float t3[3]) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) R9[3 * r + c] = c2v[(size_t)(4 * r + c) * stride];
        t3[r] = c2v[(size_t)(4 * r + 3) * stride];
    }
}

}  // namespace xs_host
