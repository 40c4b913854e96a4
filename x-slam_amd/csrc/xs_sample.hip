// xs_sample.hip — the map sampled at points the caller supplies, and at the points of a depth frame's pixels, for gfx950 (DESIGN.md section
// 4.29).  No counterpart in the reference.
//
// The contract is in include/xslam_amd.h (xs_tsdf_sample_points, xs_tsdf_sample_depth), operation by operation; what the calls refuse is
// ../host/sample_host.hpp's, shared with the orchestrator and the host selftest.  F(P) is xs_trilinear.h's, shared with xs_render.hip.
//   sample_at             the per-point device function, in xs_sample_at.h (xs_register.hip shares it): the centre sample (with the grad array
//                         beside it where dvalue is wanted), then, where a gradient is wanted and the centre is OK, the six samples at +- half a
//                         voxel.  Seven evaluations of up to eight corners each, all gathers; nothing is kept between them.
//   k_sample_points       lane = point, wave = workgroup = 64 consecutive points: the three coordinates are 12-byte strided loads, the outputs
//                         coalesced stores.  The transform arrives in the kernel arguments (scalar registers).
//   k_sample_depth        lane = pixel, wave = workgroup = 64 consecutive pixels of one image row (blockIdx.y).
// Both count the four statuses per wave by ballot and popcount, one integer atomic per counter and workgroup: no LDS, no floating-point atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "xs_sample_at.h"
#include "../../include/xslam_amd.h"
#include "../host/sample_host.hpp"

using namespace xs;
using namespace xs_host;

static_assert(TRI_OUTSIDE == SAMPLE_OUTSIDE && TRI_UNSEEN == SAMPLE_UNSEEN && TRI_OK == SAMPLE_OK, "F's refusals are the status bytes");

struct SampleOut {
    unsigned char *status; float *value; float *dvalue; float *gradient; unsigned long long *counts;
};

__device__ __forceinline__ void sample_dispatch(const TrilinearVolume &vol, bool want_dvalue, bool want_gradient, float p0, float p1, float p2, SampleResult &r) {
    if (want_dvalue) sample_at<true>(vol, want_gradient, p0, p1, p2, r);     // (uniform over the launch)
    else sample_at<false>(vol, want_gradient, p0, p1, p2, r);
}

// the four counts of a wave: `status` is -1 in a lane without a point
__device__ __forceinline__ void sample_count(unsigned long long *counts, int status) {
    if (!counts) return;
    unsigned c[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) c[s] = (unsigned)__popcll(__ballot(status == s));
    if (threadIdx.x == 0) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (c[s]) atomicAdd(counts + s, (unsigned long long)c[s]);
    }
}

struct SamplePointsArgs {
    TrilinearVolume vol;
    const float *points; long long n;
    int has_xform; float m[12];          // row-major R, then t
    SampleOut out;
};

__global__ void __launch_bounds__(64) k_sample_points(const SamplePointsArgs a) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    int status = -1;
    if (i < a.n) {
        const float *p = a.points + 3 * (size_t)i;
        float p0 = p[0], p1 = p[1], p2 = p[2];
        if (a.has_xform) {
            const float q0 = ((a.m[0] * p0 + a.m[1] * p1) + a.m[2] * p2) + a.m[9];
            const float q1 = ((a.m[3] * p0 + a.m[4] * p1) + a.m[5] * p2) + a.m[10];
            const float q2 = ((a.m[6] * p0 + a.m[7] * p1) + a.m[8] * p2) + a.m[11];
            p0 = q0; p1 = q1; p2 = q2;
        }
        SampleResult r;
        sample_dispatch(a.vol, a.out.dvalue != nullptr, a.out.gradient != nullptr, p0, p1, p2, r);
        status = r.status;
        if (a.out.status) a.out.status[i] = (unsigned char)r.status;
        if (a.out.value) a.out.value[i] = r.value;
        if (a.out.dvalue) a.out.dvalue[i] = r.dvalue;
        if (a.out.gradient) {
            float *g = a.out.gradient + 3 * (size_t)i;
            g[0] = r.grad[0]; g[1] = r.grad[1]; g[2] = r.grad[2];
        }
    }
    sample_count(a.out.counts, status);
}

struct SampleDepthArgs {
    TrilinearVolume vol;
    const unsigned short *depth; size_t depth_step;
    int rows, cols;
    float fx, fy, cx, cy;
    float R[9], t[3];                    // camera to volume
    SampleOut out;
};

__global__ void __launch_bounds__(64) k_sample_depth(const SampleDepthArgs a) {
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x, y = (int)blockIdx.y;
    int status = -1;
    if (x < a.cols) {
        const unsigned D = row_ptr(a.depth, a.depth_step, y)[x];
        SampleResult r;
        r.status = SAMPLE_NO_DEPTH; r.value = qnan_f(); r.dvalue = qnan_f(); r.grad[0] = r.grad[1] = r.grad[2] = qnan_f();
        if (!(D < (unsigned)SAMPLE_DEPTH_MIN || D > (unsigned)SAMPLE_DEPTH_MAX)) {
            const float z = (float)D / 1000.f;
            const float dx = ((float)x - a.cx) / a.fx, dy = ((float)y - a.cy) / a.fy;
            const float d0 = (a.R[0] * dx + a.R[1] * dy) + a.R[2], d1 = (a.R[3] * dx + a.R[4] * dy) + a.R[5], d2 = (a.R[6] * dx + a.R[7] * dy) + a.R[8];
            sample_dispatch(a.vol, a.out.dvalue != nullptr, a.out.gradient != nullptr, a.t[0] + z * d0, a.t[1] + z * d1, a.t[2] + z * d2, r);
        }
        status = r.status;
        const size_t plane = (size_t)a.rows * (size_t)a.cols, pix = (size_t)y * (size_t)a.cols + (size_t)x;
        if (a.out.status) a.out.status[pix] = (unsigned char)r.status;
        if (a.out.value) a.out.value[pix] = r.value;
        if (a.out.dvalue) a.out.dvalue[pix] = r.dvalue;
        if (a.out.gradient) {
            float *g = a.out.gradient + pix;
            g[0] = r.grad[0]; g[plane] = r.grad[1]; g[2 * plane] = r.grad[2];
        }
    }
    sample_count(a.out.counts, status);
}

static int sample_refuse(const char *call, int why) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", call, sample_refusal_str(why));
    return xs_set_error(hipErrorInvalidValue, msg);
}
static unsigned sample_struct_bytes(const xs_sample_opts *opts) { return opts ? opts->struct_bytes : (unsigned)sizeof(xs_sample_opts); }
static TrilinearVolume sample_volume_of(const float *value, const int *weight, const float *grad, size_t vol_step, const int *res, float voxel_size,
                                        const xs_sample_opts *opts) {
    const int mw = opts ? opts->min_weight : 1;
    return TrilinearVolume{value, weight, grad, vol_step, res[0], res[1], res[2], voxel_size, mw < 1 ? 1 : mw};
}

/* see include/xslam_amd.h */
extern "C" int xs_tsdf_sample_points(long long n, const float *points3xN_dev, const float *xform12, const float *value, const int *weight, const float *grad,
                                     size_t vol_step, const int *res, float voxel_size, const xs_sample_opts *opts, unsigned char *status, float *value_out,
                                     float *dvalue, float *gradient3xN, unsigned long long *counts4, void *stream) {
    const SampleOutputPtrs o = {status, value_out, dvalue, gradient3xN, counts4};
    const int why = sample_validate_points(n, points3xN_dev, xform12, o, value && weight, grad != nullptr, vol_step, res, voxel_size, sample_struct_bytes(opts),
                                           (unsigned)sizeof(xs_sample_opts));
    if (why != SAMPLE_ACCEPTED) return sample_refuse("xs_tsdf_sample_points", why);
    SamplePointsArgs a;
    memset(&a, 0, sizeof(a));
    a.vol = sample_volume_of(value, weight, grad, vol_step, res, voxel_size, opts);
    a.points = points3xN_dev; a.n = n;
    a.has_xform = xform12 ? 1 : 0;
    if (xform12) memcpy(a.m, xform12, sizeof(a.m));
    a.out = SampleOut{status, value_out, dvalue, gradient3xN, counts4};
    hipStream_t st = (hipStream_t)stream;
    if (counts4) XS_CHECK(hipMemsetAsync(counts4, 0, 4 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_sample_points, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a);
    XS_CHECK(hipGetLastError());
    return 0;
}

/* see include/xslam_amd.h */
extern "C" int xs_tsdf_sample_depth(const uint16_t *depth_dev, size_t depth_step, int rows, int cols, const float *intr4, const float *Rc2v9, const float *tc2v3,
                                    const float *value, const int *weight, const float *grad, size_t vol_step, const int *res, float voxel_size,
                                    const xs_sample_opts *opts, unsigned char *status, float *value_out, float *dvalue, float *gradient3, unsigned long long *counts4,
                                    void *stream) {
    const SampleOutputPtrs o = {status, value_out, dvalue, gradient3, counts4};
    const int why = sample_validate_depth(depth_dev, depth_step, rows, cols, intr4, Rc2v9, tc2v3, o, value && weight, grad != nullptr, vol_step, res, voxel_size,
                                          sample_struct_bytes(opts), (unsigned)sizeof(xs_sample_opts));
    if (why != SAMPLE_ACCEPTED) return sample_refuse("xs_tsdf_sample_depth", why);
    SampleDepthArgs a;
    memset(&a, 0, sizeof(a));
    a.vol = sample_volume_of(value, weight, grad, vol_step, res, voxel_size, opts);
    a.depth = depth_dev; a.depth_step = depth_step;
    a.rows = rows; a.cols = cols;
    a.fx = intr4[0]; a.fy = intr4[1]; a.cx = intr4[2]; a.cy = intr4[3];
    memcpy(a.R, Rc2v9, sizeof(a.R));
    memcpy(a.t, tc2v3, sizeof(a.t));
    a.out = SampleOut{status, value_out, dvalue, gradient3, counts4};
    hipStream_t st = (hipStream_t)stream;
    if (counts4) XS_CHECK(hipMemsetAsync(counts4, 0, 4 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_sample_depth, dim3((unsigned)((cols + 63) / 64), (unsigned)rows), dim3(64), 0, st, a);
    XS_CHECK(hipGetLastError());
    return 0;
}
