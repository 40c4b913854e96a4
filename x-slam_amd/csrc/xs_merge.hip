// xs_merge.hip — merge a second TSDF volume into the volume under an affine map of voxel indices, for gfx950.  No
// counterpart in the reference: its volumes are only ever written by integrateTsdfVolume (TsdfFusion.cu), one depth image at a time.
//
// One lane per destination voxel, 64 consecutive lanes along x: the destination's three arrays are read and written in coalesced 256-byte
// segments, and a voxel that is skipped is not stored.  A workgroup is 64 (x) x 4 (y) lanes and walks MERGE_TZ = 16 planes; workgroups follow
// each other along x, then y, then z, so neighbours in launch order read neighbouring source bricks.  The source is gathered: up to eight
// corners from each of three arrays, the weights first (a voxel whose corners do not all carry min_weight loads no value), and only the
// corners the contract needs (an axis whose fraction is 0 has one).  Under a near-axis-aligned map neighbouring lanes share their corners
// and the caches carry the gather; no LDS staging.
//
// The cull carries the kernel where the maps overlap little: a tile whose source index box (merge_tile_box of host/merge_host.hpp, the same
// text the host's self-test runs) misses the source leaves before any load, and so does a tile whose box touches only bricks of 4 x 4 x 4
// source voxels without a weight >= min_weight (one bit per brick, built by k_merge_bricks into the workspace).  Both tests are conservative
// and change no output bit; XS_MERGE_NO_CULL switches them off.
#include "xs_merge_sample.h"
#include <math.h>

using namespace xs;

struct MergeArgs {
    float *value; int *weight; float *grad; size_t step;
    int X, Y, Z, z0, z1;
    MergeSource src;                 // (xs_merge_sample.h: the sampler, the brick bits and the cull, shared with xs_diff.hip)
    int max_weight;
    unsigned long long *written;
};

// ---- the brick bits of the source -------------------------------------------------------------------------------------------------------
// lane = x voxel, wave = y voxel of a brick row, one workgroup per 16 bricks along x; each lane folds its four planes, a ballot folds the
// four lanes of a brick, LDS the four rows.  Bits of one word come from several workgroups: atomicOr, whose result does not depend on the order.
__global__ void __launch_bounds__(256) k_merge_bricks(const int *sweight, size_t sstep, int SX, int SY, int SZ, int min_weight, int BX, int BY,
                                                      unsigned *bricks) {
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int x = (int)blockIdx.x * 64 + lane, by = (int)blockIdx.y, bz = (int)blockIdx.z;
    const int y = 4 * by + wave;
    __shared__ unsigned long long s_rows[4];
    bool any = false;
    if (x < SX && y < SY) {
        int w[4];   // the four loads in flight together: no test of one decides whether the next is issued
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = row_ptr(sweight, sstep, SY * min(4 * bz + k, SZ - 1) + y)[x];
#pragma unroll
        for (int k = 0; k < 4; ++k) any |= w[k] >= min_weight;
    }
    const unsigned long long m = __ballot(any);
    if (lane == 0) s_rows[wave] = m;
    __syncthreads();
    if (wave == 0 && lane < 16) {
        const unsigned long long all = s_rows[0] | s_rows[1] | s_rows[2] | s_rows[3];
        const int bx = (int)blockIdx.x * 16 + lane;
        if (bx < BX && ((all >> (4 * lane)) & 0xFull) != 0ull) {
            const size_t b = ((size_t)bz * (size_t)BY + (size_t)by) * (size_t)BX + (size_t)bx;
            atomicOr(bricks + (b >> 5), 1u << (b & 31));
        }
    }
}

// ---- the merge --------------------------------------------------------------------------------------------------------------------------
namespace {
// the per-voxel contract of include/xslam_amd.h; true when the voxel was written
__device__ __forceinline__ bool merge_voxel(const MergeArgs &a, int x, int y, int z) {
    int ws;
    float sv, sq;
    if (!merge_sample<true>(a.src, x, y, z, ws, sv, sq)) return false;
    ws = min(ws, a.max_weight);
    int *wrow = row_ptr(a.weight, a.step, a.Y * z + y);
    float *vrow = row_ptr(a.value, a.step, a.Y * z + y), *grow = row_ptr(a.grad, a.step, a.Y * z + y);
    const int wp = wrow[x];
    float nv = sv, nq = sq;
    if (wp != 0) {
        const float fp = (float)wp, fs = (float)ws, ft = (float)(wp + ws);
        nv = (vrow[x] * fp + sv * fs) / ft;
        nq = (grow[x] * fp + sq * fs) / ft;
    }
    vrow[x] = nv;
    grow[x] = nq;
    wrow[x] = min(wp + ws, a.max_weight);
    return true;
}
}  // namespace

__global__ void __launch_bounds__(256) k_merge(const MergeArgs a) {
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int x0 = (int)blockIdx.x * 64, y0 = (int)blockIdx.y * 4;
    const int zt0 = a.z0 + (int)blockIdx.z * MERGE_TZ, zt1 = min(zt0 + MERGE_TZ, a.z1);
    __shared__ unsigned s_count[4];
    if (a.src.cull) {   // (uniform over the workgroup)
        const int lo[3] = {x0, y0, zt0}, hi[3] = {min(x0 + 63, a.X - 1), min(y0 + 3, a.Y - 1), zt1 - 1};
        if (merge_tile_culled(a.src, lo, hi)) return;
    }
    const int x = x0 + lane, y = y0 + wave;
    const bool inside = x < a.X && y < a.Y;
    unsigned count = 0;   // of the wave
    for (int z = zt0; z < zt1; ++z) {
        const bool wrote = inside && merge_voxel(a, x, y, z);
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

// see xs_merge_sample.h
int xs::merge_source_prepare(MergeSource &s, const float *src_value, const int *src_weight, const float *src_grad, size_t src_step, const int *src_res,
                             const float *xform12, int min_weight, bool cull, void *workspace, hipStream_t st) {
    s.value = src_value; s.weight = src_weight; s.grad = src_grad; s.step = src_step;
    for (int k = 0; k < 3; ++k) s.S[k] = src_res[k];
    for (int i = 0; i < 12; ++i) s.m[i] = xform12[i];
    s.min_weight = min_weight; s.cull = cull ? 1u : 0u;
    s.BX = div_up(src_res[0], 4); s.BY = div_up(src_res[1], 4); s.BZ = div_up(src_res[2], 4);
    s.bricks = nullptr;
    if (cull) {
        unsigned *bricks = (unsigned *)((char *)workspace + MERGE_HEADER_BYTES);
        s.bricks = bricks;
        XS_CHECK(hipMemsetAsync(bricks, 0, merge_brick_words(src_res) * sizeof(unsigned), st));
        hipLaunchKernelGGL(k_merge_bricks, dim3(div_up(s.S[0], 64), s.BY, s.BZ), dim3(64, 4), 0, st, src_weight, src_step, s.S[0], s.S[1], s.S[2], min_weight,
                           s.BX, s.BY, bricks);
    }
    return 0;
}

/* the workspace of xs_tsdf_merge: a header and one bit per brick of 4 x 4 x 4 source voxels; 0 for a null or unusable resolution */
extern "C" size_t xs_tsdf_merge_workspace_bytes(const int *dst_res, const int *src_res) {
    if (!dst_res || !src_res || !merge_res_ok(dst_res) || !merge_res_ok(src_res)) return 0;
    return merge_workspace_bytes(src_res);
}

/* see include/xslam_amd.h */
extern "C" int xs_tsdf_merge(float *value, int *weight, float *grad, size_t step, const int *res, int z0, int z1, const float *src_value,
                             const int *src_weight, const float *src_grad, size_t src_step, const int *src_res, const float *xform12, int min_weight,
                             int max_weight, unsigned flags, unsigned long long *written_dev, void *workspace, void *stream) {
    if (!value || !weight || !grad || !src_value || !src_weight || !src_grad || !res || !src_res || !xform12)
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_merge: null pointer");
    const bool cull = !(flags & XS_MERGE_NO_CULL);
    if (cull && !workspace) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_merge: null workspace");
    if (!merge_res_ok(res) || !merge_res_ok(src_res)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_merge: bad resolution");
    if (step % 4 != 0 || src_step % 4 != 0 || step < (size_t)res[0] * 4 || src_step < (size_t)src_res[0] * 4)
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_merge: bad pitch");
    if (min_weight < 1) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_merge: min_weight below 1");
    if (max_weight < 1 || max_weight > (1 << 24)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_merge: max_weight outside [1, 1 << 24]");
    for (int i = 0; i < 12; ++i)
        if (!isfinite(xform12[i])) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_merge: xform12 is not finite");
    if (z0 < 0 || z1 > res[2] || z1 <= z0) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_merge: empty or reversed plane range");
    if (src_value == value || src_weight == weight || src_grad == grad) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_merge: the source aliases the destination");
    MergeArgs a;
    a.value = value; a.weight = weight; a.grad = grad; a.step = step;
    a.X = res[0]; a.Y = res[1]; a.Z = res[2]; a.z0 = z0; a.z1 = z1;
    a.max_weight = max_weight;
    a.written = written_dev;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = merge_source_prepare(a.src, src_value, src_weight, src_grad, src_step, src_res, xform12, min_weight, cull, workspace, st)) return rc;
    hipLaunchKernelGGL(k_merge, dim3(div_up(a.X, 64), div_up(a.Y, 4), div_up(z1 - z0, MERGE_TZ)), dim3(64, 4), 0, st, a);
    XS_CHECK(hipGetLastError());
    return 0;
}
