// xs_register.hip — the Gauss-Newton terms of registering a point cloud to a map, for up to 32 transforms in one launch, for gfx950 (DESIGN.md
// section 4.30).  No counterpart in the reference: its registrations all start from a depth image.
//
// The contract is in include/xslam_amd.h (xs_tsdf_register_terms), operation by operation; what the call refuses is ../host/register_host.hpp's,
// shared with the orchestrator and the host selftest.  The residual of point p under transform m is the map's value at P = R p + t, its
// Jacobian the map's gradient there and P x gradient: sample_at (xs_sample_at.h), the per-point function of xs_tsdf_sample_points, gives both,
// so a point's float32 numbers are the bytes that call would write.
//
// One lane per point, dealt out as k_align_terms deals its band entries: chunks of 64 consecutive points, wave w of workgroup (b, m) takes
// chunks 4 b + w, + 4 nblocks, ..., and the fold is block_fold_and_finish_of<29> with one ticket per transform.  The 29 double accumulators
// stay in registers across the chunk loop.  The transforms arrive in the kernel arguments: blockIdx.y picks one, so the twelve floats are read
// at an address that is uniform over the workgroup.  That needs no staging copy of the host array into the workspace (which the caller could
// not reuse before the copy ran), no LDS and no barrier in front of the loop; 32 x 12 floats are 1536 bytes of the 4 KiB a launch may carry
// (the compiler's summary shows no scratch: the indexed argument is not copied to private memory).  Nothing but the 29 N doubles (and the
// workspace's records and tickets) is written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "xs_gn_band.h"
#include "xs_sample_at.h"
#include "../../include/xslam_amd.h"
#include "../host/register_host.hpp"

static_assert(XS_REGISTER_MAX_TRANSFORMS == xs_host::REGISTER_MAX_TRANSFORMS, "the header's bound");
static_assert(XS_REGISTER_MAX_TRANSFORMS * sizeof(unsigned) <= 256, "one ticket per transform in the first 256 bytes");
static_assert(TRI_OK == xs_host::SAMPLE_OK, "F's refusals are the status bytes");
enum { REGISTER_RECORDS_OFFSET = 256, REGISTER_RECORD_DOUBLES = 32 };

struct RegisterArgs {
    TrilinearVolume vol;
    const float *points; long long n;
    float max_residual;
    double *records;                             // [N][nblocks][32]
    unsigned *tickets;                           // [N], zero between launches
    double *out;                                 // [N][29]
    float m[XS_REGISTER_MAX_TRANSFORMS][12];     // row-major R, then t
};

__global__ void __launch_bounds__(256) k_register_terms(const RegisterArgs a) {
    const int m = blockIdx.y, lane = threadIdx.x, wave = threadIdx.y;
    const float *M = a.m[m];
    double acc[29];
#pragma unroll
    for (int k = 0; k < 29; ++k) acc[k] = 0.0;
    const long long nchunks = (a.n + 63) / 64;
    for (long long c = (long long)blockIdx.x * 4 + wave; c < nchunks; c += 4ll * gridDim.x) {
        const long long i = c * 64 + lane;
        if (i >= a.n) continue;                  // (the last chunk's tail)
        const float *p = a.points + 3 * (size_t)i;
        const float p0 = p[0], p1 = p[1], p2 = p[2];
        const float P0 = ((M[0] * p0 + M[1] * p1) + M[2] * p2) + M[9];
        const float P1 = ((M[3] * p0 + M[4] * p1) + M[5] * p2) + M[10];
        const float P2 = ((M[6] * p0 + M[7] * p1) + M[8] * p2) + M[11];
        SampleResult s;
        sample_at<false>(a.vol, true, P0, P1, P2, s);
        if (s.status != TRI_OK) continue;
        // a refused gradient is the NaN 0x7fffffff in all three words: the bytes xs_tsdf_sample_points writes for it
        if (__float_as_uint(s.grad[0]) == 0x7fffffffu && __float_as_uint(s.grad[1]) == 0x7fffffffu && __float_as_uint(s.grad[2]) == 0x7fffffffu) continue;
        if (fabsf(s.value) > a.max_residual) continue;
        float J[6];
        J[0] = s.grad[0]; J[1] = s.grad[1]; J[2] = s.grad[2];
        J[3] = P1 * s.grad[2] - P2 * s.grad[1];
        J[4] = P2 * s.grad[0] - P0 * s.grad[2];
        J[5] = P0 * s.grad[1] - P1 * s.grad[0];
        const double r = (double)s.value;
        int q = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int k = j; k < 6; ++k) acc[q++] += (double)J[j] * (double)J[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[21 + k] += (double)J[k] * r;
        acc[27] += r * r;
        acc[28] += 1.0;
    }
    block_fold_and_finish_of<29>(acc, a.records + (size_t)m * gridDim.x * REGISTER_RECORD_DOUBLES, a.tickets + m, a.out + 29 * m, nullptr, 0, false,
                                 gridDim.x, blockIdx.x);
}

extern "C" size_t xs_tsdf_register_workspace_bytes(int transforms) {
    if (transforms < 1 || transforms > XS_REGISTER_MAX_TRANSFORMS) return 0;
    return REGISTER_RECORDS_OFFSET + (size_t)transforms * XS_TSDF_REDUCE_MAX_BLOCKS_C * REGISTER_RECORD_DOUBLES * sizeof(double);
}

/* see include/xslam_amd.h */
extern "C" int xs_tsdf_register_terms(int transforms, long long n, const float *points3xN_dev, const float *xform12xN, const float *value, const int *weight,
                                      size_t vol_step, const int *res, float voxel_size, int min_weight, float max_residual, void *workspace,
                                      double *out29xN_dev, void *stream) {
    const int why = xs_host::register_validate(transforms, n, points3xN_dev, xform12xN, value && weight, vol_step, res, voxel_size, min_weight, max_residual,
                                               workspace, out29xN_dev);
    if (why != xs_host::REGISTER_ACCEPTED) {
        char msg[160];
        snprintf(msg, sizeof(msg), "xs_tsdf_register_terms: %s", xs_host::register_refusal_str(why));
        return xs_set_error(hipErrorInvalidValue, msg);
    }
    RegisterArgs a;
    memset(&a, 0, sizeof(a));
    a.vol = TrilinearVolume{value, weight, nullptr, vol_step, res[0], res[1], res[2], voxel_size, min_weight};
    a.points = points3xN_dev; a.n = n;
    a.max_residual = max_residual;
    memcpy(a.m, xform12xN, (size_t)transforms * 12 * sizeof(float));
    // as many workgroups as give every wave a chunk, at most the record workspace's 4096: a function of n alone
    const long long nchunks = (n + 63) / 64, want = (nchunks + 3) / 4;
    const unsigned nblocks = (unsigned)(want < 1 ? 1 : (want > XS_TSDF_REDUCE_MAX_BLOCKS_C ? XS_TSDF_REDUCE_MAX_BLOCKS_C : want));
    char *ws = static_cast<char *>(workspace);
    a.tickets = reinterpret_cast<unsigned *>(ws);
    a.records = reinterpret_cast<double *>(ws + REGISTER_RECORDS_OFFSET);
    a.out = out29xN_dev;
    hipLaunchKernelGGL(k_register_terms, dim3(nblocks, (unsigned)transforms), dim3(64, 4), 0, (hipStream_t)stream, a);
    XS_CHECK(hipGetLastError());
    return 0;
}
