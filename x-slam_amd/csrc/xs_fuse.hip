// xs_fuse.hip — a registered point cloud fused into the volume, for gfx950.  No counterpart in the reference: its volume
// is only ever written by integrateTsdfVolume (TsdfFusion.cu), one pinhole depth image at a time.
//
// The contract is in include/xslam_amd.h (xs_tsdf_fuse_points_accumulate, xs_tsdf_fuse_points_fold), operation by operation; what the calls
// refuse is ../host/fuse_host.hpp's, shared with the orchestrator and the host selftest.  This is the one place in the library where a kernel
// scatters, so it is also the one place that has to say why its output does not depend on scheduling: what is added is an integer.
//   k_fuse_accumulate     lane = point, wave = workgroup = 64 consecutive points.  A lane walks its ray in half-voxel steps and adds
//                         (1 << 40) | q to the word of every voxel it enters: one 64-bit integer atomic per visit whose result is not used (the
//                         no-return form), scattered 8-byte requests, since neighbouring lanes hold unrelated points.  The lanes of a wave walk
//                         rays of different lengths; the wave runs as long as its longest.  The four counts are summed over the wave by shuffles:
//                         one integer atomic per counter and workgroup.  No LDS, no floating-point atomics.
//   k_fuse_fold           lane = voxel, 64 consecutive lanes along x, the merge's tile (64 x 4 lanes walking FUSE_TZ planes): the accumulator is
//                         read in coalesced 512-byte segments, and only a touched voxel loads and stores the three arrays and clears its word.
// Not built: sorting the points by brick, a touched-brick bitmap for the fold, a wave-level merge of equal voxels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "xs_device.h"
#include "../../include/xslam_amd.h"
#include "../host/fuse_host.hpp"

using namespace xs;
using namespace xs_host;

static_assert(XS_FUSE_MAX_POINTS == FUSE_MAX_POINTS && XS_FUSE_MAX_HALF_STEPS == FUSE_MAX_HALF_STEPS, "the header's limits are the host's");

enum { FUSE_TZ = 16 };   // planes a fold workgroup walks

struct FuseAccumulateArgs {
    const float *points; int n;
    int has_xform; float m[12];          // row-major R, then t
    float O[3];                          // the origin in the volume frame (formed on the host)
    int X, Y, Z;
    float voxel_size, tranc_dist, step;  // step = 0.5f * voxel_size
    int K, carve;
    float min_range, max_range;
    unsigned long long *acc, *counts;
};

__global__ void __launch_bounds__(64) k_fuse_accumulate(const FuseAccumulateArgs a) {
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    unsigned used = 0, dropped = 0, visits = 0, outside = 0;   // of this lane
    if (i < a.n) {
        const float *p = a.points + 3 * (size_t)i;
        float P0 = p[0], P1 = p[1], P2 = p[2];
        if (a.has_xform) {
            const float q0 = ((a.m[0] * P0 + a.m[1] * P1) + a.m[2] * P2) + a.m[9];
            const float q1 = ((a.m[3] * P0 + a.m[4] * P1) + a.m[5] * P2) + a.m[10];
            const float q2 = ((a.m[6] * P0 + a.m[7] * P1) + a.m[8] * P2) + a.m[11];
            P0 = q0; P1 = q1; P2 = q2;
        }
        const float v0 = P0 - a.O[0], v1 = P1 - a.O[1], v2 = P2 - a.O[2];
        const float L = sqrtf((v0 * v0 + v1 * v1) + v2 * v2);
        if (L >= a.min_range && L <= a.max_range) {   // (a NaN fails)
            used = 1;
            const float d0 = v0 / L, d1 = v1 / L, d2 = v2 / L;
            const int k_far = (int)floorf(L / a.step);   // (L <= max_range: at most 2^20)
            const int k_lo = a.carve ? -k_far : -min(a.K, k_far);
            const float fX = (float)a.X, fY = (float)a.Y, fZ = (float)a.Z;
            int px = -1, py = -1, pz = -1;   // the voxel of the previous inside sample
            for (int k = k_lo; k <= a.K; ++k) {
                const float s = (float)k * a.step;
                const float g0 = (P0 + s * d0) / a.voxel_size, g1 = (P1 + s * d1) / a.voxel_size, g2 = (P2 + s * d2) / a.voxel_size;
                if (!(g0 >= 0.f && g0 < fX && g1 >= 0.f && g1 < fY && g2 >= 0.f && g2 < fZ)) { ++outside; continue; }
                const int ix = (int)floorf(g0), iy = (int)floorf(g1), iz = (int)floorf(g2);   // in [0, res): the test above was made in float
                if (ix == px && iy == py && iz == pz) continue;
                px = ix; py = iy; pz = iz;
                const float C0 = ((float)ix + 0.5f) * a.voxel_size, C1 = ((float)iy + 0.5f) * a.voxel_size, C2 = ((float)iz + 0.5f) * a.voxel_size;
                const float sd = ((P0 - C0) * d0 + (P1 - C1) * d1) + (P2 - C2) * d2;
                float u = sd / a.tranc_dist;
                if (u < -1.0f) continue;
                u = fminf(u, 1.0f);
                const unsigned long long q = (unsigned long long)(int)rintf((u + 1.0f) * 32768.0f);
                const size_t word = ((size_t)iz * (size_t)a.Y + (size_t)iy) * (size_t)a.X + (size_t)ix;
                (void)atomicAdd(a.acc + word, (1ull << 40) | q);   // the result is not used: the no-return form (global_atomic_add_x2 without sc0)
                ++visits;
            }
        } else {
            dropped = 1;
        }
    }
    // the four counts of the wave (a lane's visits stay below 2^21: the sums fit 32 bits)
    used = wave_sum_u32(used); dropped = wave_sum_u32(dropped); visits = wave_sum_u32(visits); outside = wave_sum_u32(outside);
    if (threadIdx.x == 0) {
        if (used) atomicAdd(a.counts + 0, (unsigned long long)used);
        if (dropped) atomicAdd(a.counts + 1, (unsigned long long)dropped);
        if (visits) atomicAdd(a.counts + 2, (unsigned long long)visits);
        if (outside) atomicAdd(a.counts + 3, (unsigned long long)outside);
    }
}

struct FuseFoldArgs {
    float *value; int *weight; float *grad; size_t step;
    int X, Y, z0, z1;
    unsigned long long *acc;
    int obs_weight, max_weight;
    unsigned long long *written;
};

namespace {
// the per-voxel contract of include/xslam_amd.h; true when the voxel was written
__device__ __forceinline__ bool fold_voxel(const FuseFoldArgs &a, int x, int y, int z) {
    unsigned long long *word = a.acc + (((size_t)z * (size_t)a.Y + (size_t)y) * (size_t)a.X + (size_t)x);
    const unsigned long long w = *word;
    const unsigned long long count = w >> 40;
    if (count == 0ull) return false;
    const double m = (double)(w & ((1ull << 40) - 1ull)) / (double)count;
    const float o = (float)(m * 0x1p-15 - 1.0);
    int *wrow = row_ptr(a.weight, a.step, a.Y * z + y);
    float *vrow = row_ptr(a.value, a.step, a.Y * z + y), *grow = row_ptr(a.grad, a.step, a.Y * z + y);
    const int wp = wrow[x], ws = a.obs_weight;
    float nv = o, nq = 0.0f;
    if (wp != 0) {
        const float fp = (float)wp, fs = (float)ws, ft = (float)(wp + ws);
        nv = (vrow[x] * fp + o * fs) / ft;
        nq = (grow[x] * fp) / ft;
    }
    vrow[x] = nv;
    grow[x] = nq;
    wrow[x] = min(wp + ws, a.max_weight);
    *word = 0ull;
    return true;
}
}  // namespace

__global__ void __launch_bounds__(256) k_fuse_fold(const FuseFoldArgs a) {
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int x = (int)blockIdx.x * 64 + lane, y = (int)blockIdx.y * 4 + wave;
    const int zt0 = a.z0 + (int)blockIdx.z * FUSE_TZ, zt1 = min(zt0 + FUSE_TZ, a.z1);
    __shared__ unsigned s_count[4];
    const bool inside = x < a.X && y < a.Y;
    unsigned count = 0;   // of the wave
    for (int z = zt0; z < zt1; ++z) {
        const bool wrote = inside && fold_voxel(a, x, y, z);
        count += (unsigned)__popcll(__ballot(wrote));
    }
    if (!a.written) return;
    if (lane == 0) s_count[wave] = count;
    __syncthreads();
    if (wave == 0 && lane == 0) {
        const unsigned total = s_count[0] + s_count[1] + s_count[2] + s_count[3];
        if (total) atomicAdd(a.written, (unsigned long long)total);
    }
}

static int fuse_refuse(const char *call, int why) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", call, fuse_refusal_str(why));
    return xs_set_error(hipErrorInvalidValue, msg);
}

/* see include/xslam_amd.h */
extern "C" size_t xs_tsdf_fuse_accumulator_bytes(const int *res) { return res ? fuse_accumulator_bytes(res) : 0; }

/* see include/xslam_amd.h */
extern "C" int xs_tsdf_fuse_points_accumulate(long long n, const float *points3xN_dev, const float *xform12, const float *origin3, const int *res, float voxel_size,
                                              float tranc_dist, const xs_fuse_opts *opts, unsigned long long *accumulator, unsigned long long *counts4_dev,
                                              void *stream) {
    const int why = fuse_validate_accumulate(n, points3xN_dev, xform12, origin3, res, voxel_size, tranc_dist, opts != nullptr, opts ? opts->struct_bytes : 0u,
                                             (unsigned)sizeof(xs_fuse_opts), opts ? opts->min_range : 0.f, opts ? opts->max_range : 0.f, accumulator, counts4_dev);
    if (why != FUSE_ACCEPTED) return fuse_refuse("xs_tsdf_fuse_points_accumulate", why);
    FuseAccumulateArgs a;
    memset(&a, 0, sizeof(a));
    a.points = points3xN_dev; a.n = (int)n;
    a.has_xform = xform12 ? 1 : 0;
    if (xform12) memcpy(a.m, xform12, sizeof(a.m));
    fuse_origin(xform12, origin3, a.O);
    a.X = res[0]; a.Y = res[1]; a.Z = res[2];
    a.voxel_size = voxel_size; a.tranc_dist = tranc_dist; a.step = 0.5f * voxel_size;
    a.K = fuse_half_steps(voxel_size, tranc_dist); a.carve = opts->carve ? 1 : 0;
    a.min_range = opts->min_range; a.max_range = opts->max_range;
    a.acc = accumulator; a.counts = counts4_dev;
    hipLaunchKernelGGL(k_fuse_accumulate, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    XS_CHECK(hipGetLastError());
    return 0;
}

/* see include/xslam_amd.h */
extern "C" int xs_tsdf_fuse_points_fold(float *value, int *weight, float *grad, size_t step, const int *res, int z0, int z1, unsigned long long *accumulator,
                                        int obs_weight, int max_weight, unsigned long long *written_dev, void *stream) {
    const int why = fuse_validate_fold(value && weight && grad, step, res, z0, z1, accumulator, obs_weight, max_weight);
    if (why != FUSE_ACCEPTED) return fuse_refuse("xs_tsdf_fuse_points_fold", why);
    FuseFoldArgs a;
    a.value = value; a.weight = weight; a.grad = grad; a.step = step;
    a.X = res[0]; a.Y = res[1]; a.z0 = z0; a.z1 = z1;
    a.acc = accumulator;
    a.obs_weight = obs_weight; a.max_weight = max_weight;
    a.written = written_dev;
    hipLaunchKernelGGL(k_fuse_fold, dim3(div_up(a.X, 64), div_up(a.Y, 4), div_up(z1 - z0, FUSE_TZ)), dim3(64, 4), 0, (hipStream_t)stream, a);
    XS_CHECK(hipGetLastError());
    return 0;
}
