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
//
// k_register_score, after it: the same residual without its Jacobian, for up to 4096 transforms in one pass over every stride-th point
// (DESIGN.md section 4.32), which finds the transform the Gauss-Newton pass above starts from when nobody supplies one.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "xs_gn_band.h"
#include "xs_sample_at.h"
#include "xs_score_fold.h"
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

// ---- many transforms, no derivative: the loss of every hypothesis in one pass over the points ------------------------
// k_align_score's scheme (xs_align.hip) with the CLOUD as what is dealt out: the scored points (every stride-th of the cloud) are cut into
// chunks of 64; wave w of workgroup (b, tile) takes chunks 4 b + w, + 4 nblocks, ...; lane l loads scored point l of the chunk once and then
// meets the tile's transforms 64 tile .. 64 tile + 63 one after the other.  The transform index is wave-uniform (a loop counter through
// readfirstlane): the twelve floats arrive by scalar loads from the workspace copy and stay in scalar registers.  Per (chunk, transform): r * r
// where the contract of include/xslam_amd.h keeps the point, 0 where it drops it (and in the tail of the last chunk), folded across the wave by
// wave_tree_sum_f32, the count by ballot + popcount; lane (p mod 64) adds both to the double and the unsigned it keeps for transform p.  The
// value is trilinear_sample<false> of xs_trilinear.h, the function xs_tsdf_sample_points calls: its range test returns before any load and its
// weight test before any value load, so a wave none of whose lanes passes one of them branches over the loads behind it; and a wave that kept
// nothing skips the tree: what it leaves out is the addition of +0.0 to a sum that is never -0.0, and of 0 to a count.  The end is
// score_tile_fold_and_finish (xs_score_fold.h), shared with k_align_score.
static_assert(XS_REGISTER_SCORE_MAX_TRANSFORMS == xs_host::REGISTER_SCORE_MAX_TRANSFORMS, "the header's bound");
static_assert(XS_REGISTER_SCORE_MAX_TRANSFORMS / SCORE_TILE * sizeof(unsigned) == 256, "one ticket per tile in the first 256 bytes");
enum { RSCORE_XFORMS_OFFSET = 256 };
struct RegisterXform { float m[12]; };
static size_t rscore_records_offset() { return RSCORE_XFORMS_OFFSET + (size_t)XS_REGISTER_SCORE_MAX_TRANSFORMS * sizeof(RegisterXform); }

struct RegisterScoreArgs {
    TrilinearVolume vol;
    const float *points;
    long long scored;                            // ceil(n / stride): scored point i is point stride * i
    long long stride;
    int transforms;
    const RegisterXform *xforms;                 // [transforms], in the workspace
    float max_residual;
    char *records;                               // [tiles][nblocks]{64 doubles, 64 unsigned}
    unsigned *tickets;                           // [tiles], zero between launches
    double *out;                                 // [transforms][2]
};

__global__ void __launch_bounds__(256) k_register_score(const RegisterScoreArgs a) {
    const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const unsigned nblocks = gridDim.x, bid = blockIdx.x, tile = blockIdx.y;
    const int p0 = (int)tile * SCORE_TILE, np = min((int)SCORE_TILE, a.transforms - p0);   // (the last tile may be partial: its other lanes keep zeros)
    const RegisterXform *__restrict__ xforms = a.xforms + p0;
    double acc = 0.0;
    unsigned cnt = 0;
    const long long nchunks = (a.scored + 63) / 64;
    for (long long c = (long long)bid * 4 + wave; c < nchunks; c += 4ll * nblocks) {
        const long long i = c * 64 + lane;
        const bool valid = i < a.scored;         // (the last chunk's tail: masked, and it adds zeros)
        float q0 = 0.f, q1 = 0.f, q2 = 0.f;
        if (valid) {
            const float *q = a.points + 3 * (size_t)(i * a.stride);
            q0 = q[0]; q1 = q[1]; q2 = q[2];
        }
#pragma unroll 1
        for (int j = 0; j < np; ++j) {
            const RegisterXform M = xforms[__builtin_amdgcn_readfirstlane(j)];
            const float *m = M.m;
            const float P0 = ((m[0] * q0 + m[1] * q1) + m[2] * q2) + m[9];
            const float P1 = ((m[3] * q0 + m[4] * q1) + m[5] * q2) + m[10];
            const float P2 = ((m[6] * q0 + m[7] * q1) + m[8] * q2) + m[11];
            float rr = 0.f;
            bool kept = false;
            if (valid) {
                float r = 0.f, unused;
                if (trilinear_sample<false>(a.vol, P0, P1, P2, r, unused) == TRI_OK) {
                    kept = fabsf(r) <= a.max_residual;           // (a NaN drops)
                    rr = kept ? r * r : 0.f;
                }
            }
            const unsigned long long keptmask = __ballot(kept);
            if (keptmask == 0) continue;                         // the wave kept nothing: the zeros it would add change no bit
            const float s = wave_tree_sum_f32(rr);
            const unsigned n = (unsigned)__popcll(keptmask);
            if (lane == j) { acc += (double)s; cnt += n; }
        }
    }
    score_tile_fold_and_finish(acc, cnt, a.records, a.tickets, a.out, p0, np);
}

extern "C" size_t xs_tsdf_score_points_workspace_bytes(int transforms) {
    if (transforms < 1 || transforms > XS_REGISTER_SCORE_MAX_TRANSFORMS) return 0;
    const size_t tiles = ((size_t)transforms + SCORE_TILE - 1) / SCORE_TILE;
    return rscore_records_offset() + tiles * SCORE_MAX_BLOCKS * SCORE_RECORD_BYTES;
}

/* see include/xslam_amd.h */
extern "C" int xs_tsdf_score_points(int transforms, long long n, int stride, const float *points3xN_dev, const float *xform12xP, const float *value,
                                    const int *weight, size_t vol_step, const int *res, float voxel_size, int min_weight, float max_residual,
                                    void *workspace, double *out2xP_dev, void *stream) {
    const int why = xs_host::register_score_validate(transforms, n, stride, points3xN_dev, xform12xP, value && weight, vol_step, res, voxel_size, min_weight,
                                                     max_residual, workspace, out2xP_dev);
    if (why != xs_host::REGISTER_ACCEPTED) {
        char msg[160];
        snprintf(msg, sizeof(msg), "xs_tsdf_score_points: %s", xs_host::register_score_refusal_str(why));
        return xs_set_error(hipErrorInvalidValue, msg);
    }
    RegisterScoreArgs a;
    memset(&a, 0, sizeof(a));
    a.vol = TrilinearVolume{value, weight, nullptr, vol_step, res[0], res[1], res[2], voxel_size, min_weight};
    a.points = points3xN_dev;
    a.stride = stride; a.scored = xs_host::register_scored_points(n, stride);
    a.transforms = transforms; a.max_residual = max_residual;
    // as many workgroups per tile as give every wave a chunk, at most the record workspace's 1024: a function of the scored count alone
    const long long nchunks = (a.scored + 63) / 64, want = (nchunks + 3) / 4;
    const unsigned nblocks = (unsigned)(want < 1 ? 1 : (want > SCORE_MAX_BLOCKS ? SCORE_MAX_BLOCKS : want));
    const unsigned tiles = ((unsigned)transforms + SCORE_TILE - 1) / SCORE_TILE;
    char *ws = static_cast<char *>(workspace);
    a.tickets = reinterpret_cast<unsigned *>(ws);
    a.xforms = reinterpret_cast<const RegisterXform *>(ws + RSCORE_XFORMS_OFFSET);
    a.records = ws + rscore_records_offset();
    a.out = out2xP_dev;
    hipStream_t st = (hipStream_t)stream;
    XS_CHECK(hipMemcpyAsync(ws + RSCORE_XFORMS_OFFSET, xform12xP, (size_t)transforms * sizeof(RegisterXform), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_register_score, dim3(nblocks, tiles), dim3(64, 4), 0, st, a);
    XS_CHECK(hipGetLastError());
    return 0;
}
