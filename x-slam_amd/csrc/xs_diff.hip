// xs_diff.hip — what differs between the volume and a second TSDF volume under an affine map of voxel indices, as two per-brick masks, for gfx950
// (DESIGN.md section 4.25).  No counterpart in the reference, which never holds two maps.
//
// The sample of the other map is xs_tsdf_merge's (xs_merge_sample.h: the sampler without the grad channel, the brick bits, the cull); the masks
// are in the MASK layout of xs_grid.h, so xs_frontier_label and xs_frontier_clusters turn them into clusters.  The merge's tile, 64 (x) x 4 (y)
// lanes walking MERGE_TZ = 16 planes, is 16 x 1 x 4 bricks: per plane a wave's ballot of a class is a row of 64 voxels, the 2 x 16 x 4 rows go to
// LDS (1 KiB) with one barrier, and 2 x 64 threads each put one brick word together from its sixteen four-bit fields and store it, 128
// contiguous bytes per brick row and mask.  Every word has exactly one writer: no atomics on the masks, no read-modify-write, and a tile that
// leaves at the cull stores its zero words.  The destination is read in coalesced 256-byte segments, 8 bytes per voxel; a voxel below
// min_weight gathers nothing.
#include "xs_grid.h"
#include "xs_merge_sample.h"
#include <math.h>

using namespace xs;

struct DiffArgs {
    const float *value; const int *weight; size_t step;
    GridDims d;
    MergeSource src;
    float lo, hi;
    unsigned long long *masks[2];    // only_this, only_other
    unsigned long long *counts;      // compared, only_this, only_other
};

__global__ void __launch_bounds__(256) k_diff(const DiffArgs a) {
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int x0 = (int)blockIdx.x * 64, y0 = (int)blockIdx.y * 4, zt0 = (int)blockIdx.z * MERGE_TZ;
    const int zt1 = min(zt0 + MERGE_TZ, a.d.Z);
    __shared__ unsigned long long s_rows[2][MERGE_TZ][4];   // [class][plane of the tile][y of the tile]: bit x of the tile
    __shared__ unsigned s_count[4][3];
    bool culled = false;   // (uniform over the workgroup)
    if (a.src.cull) {
        const int lo[3] = {x0, y0, zt0}, hi[3] = {min(x0 + 63, a.d.X - 1), min(y0 + 3, a.d.Y - 1), zt1 - 1};
        culled = merge_tile_culled(a.src, lo, hi);
    }
    if (!culled) {
        const int x = x0 + lane, y = y0 + wave;
        const bool inside = x < a.d.X && y < a.d.Y;
        unsigned compared = 0, n_this = 0, n_other = 0;   // of the wave
        for (int k = 0; k < MERGE_TZ; ++k) {              // planes beyond the volume give zero rows: overhang bits are clear
            const int z = zt0 + k;
            bool cmp = false, only_this = false, only_other = false;
            if (inside && z < zt1) {
                const int wp = row_ptr(a.weight, a.step, a.d.Y * z + y)[x];
                const float v = row_ptr(a.value, a.step, a.d.Y * z + y)[x];
                int ws;
                float s, unused;
                if (wp >= a.src.min_weight && merge_sample<false>(a.src, x, y, z, ws, s, unused)) {
                    cmp = true;
                    only_this = v < a.lo && s >= a.hi;
                    only_other = s < a.lo && v >= a.hi;
                }
            }
            const unsigned long long row_this = __ballot(only_this), row_other = __ballot(only_other);
            compared += (unsigned)__popcll(__ballot(cmp));
            n_this += (unsigned)__popcll(row_this);
            n_other += (unsigned)__popcll(row_other);
            if (lane == 0) { s_rows[0][k][wave] = row_this; s_rows[1][k][wave] = row_other; }
        }
        if (lane == 0) { s_count[wave][0] = compared; s_count[wave][1] = n_this; s_count[wave][2] = n_other; }
    }
    __syncthreads();
    if (wave >= 2) return;
    // wave 0 assembles only_this, wave 1 only_other: thread t has brick (t & 15, 0, t >> 4) of the tile
    const int bx = (x0 >> 2) + (lane & 15), by = y0 >> 2, bzl = lane >> 4, bz = (zt0 >> 2) + bzl;
    if (bx < a.d.BX && bz < a.d.BZ) {
        unsigned long long word = 0ull;
        if (!culled) {
#pragma unroll
            for (int lz = 0; lz < 4; ++lz)
#pragma unroll
                for (int ly = 0; ly < 4; ++ly)
                    word |= (s_rows[wave][4 * bzl + lz][ly] >> (4 * (lane & 15)) & 0xFull) << (4 * ly + 16 * lz);
        }
        (wave == 0 ? a.masks[0] : a.masks[1])[grid_brick_at(a.d, bx, by, bz)] = word;
    }
    if (!culled && wave == 0 && lane < 3) {   // one add per counter and workgroup
        const unsigned total = s_count[0][lane] + s_count[1][lane] + s_count[2][lane] + s_count[3][lane];
        if (total) atomicAdd(a.counts + lane, (unsigned long long)total);
    }
}

/* the workspace of xs_tsdf_diff: xs_tsdf_merge's for this source; 0 for a null or unusable resolution or a destination with no mask */
extern "C" size_t xs_tsdf_diff_workspace_bytes(const int *res, const int *src_res) {
    if (!res || !src_res || !merge_res_ok(res) || !merge_res_ok(src_res) || xs_frontier_mask_bytes(res) == 0) return 0;
    return merge_workspace_bytes(src_res);
}

/* see include/xslam_amd.h */
extern "C" int xs_tsdf_diff(const float *value, const int *weight, size_t step, const int *res, const float *src_value, const int *src_weight, size_t src_step,
                            const int *src_res, const float *xform12, int min_weight, float lo, float hi, unsigned flags, void *only_this_mask,
                            void *only_other_mask, unsigned long long *counts3_dev, void *workspace, void *stream) {
    if (!value || !weight || !src_value || !src_weight || !res || !src_res || !xform12) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_diff: null pointer");
    if (!only_this_mask || !only_other_mask || !counts3_dev) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_diff: null mask or counts");
    if (only_this_mask == only_other_mask) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_diff: the two masks are one buffer");
    if (((uintptr_t)only_this_mask | (uintptr_t)only_other_mask) % 8 != 0) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_diff: a mask is not 8-byte aligned");
    const bool cull = !(flags & XS_DIFF_NO_CULL);
    if (cull && !workspace) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_diff: null workspace");
    if (!merge_res_ok(res) || !merge_res_ok(src_res)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_diff: bad resolution");
    DiffArgs a;
    if (xs_frontier_mask_bytes(res) == 0 || !grid_dims(res, a.d)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_diff: the destination has no mask (xs_frontier_mask_bytes)");
    if (step % 4 != 0 || src_step % 4 != 0 || step < (size_t)res[0] * 4 || src_step < (size_t)src_res[0] * 4)
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_diff: bad pitch");
    if (min_weight < 1) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_diff: min_weight below 1");
    for (int i = 0; i < 12; ++i)
        if (!isfinite(xform12[i])) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_diff: xform12 is not finite");
    if (!isfinite(lo) || !isfinite(hi) || lo > hi) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_diff: lo and hi must be finite with lo <= hi");
    if (src_value == value || src_weight == weight) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_diff: the source aliases the destination");
    a.value = value; a.weight = weight; a.step = step;
    a.lo = lo; a.hi = hi;
    a.masks[0] = static_cast<unsigned long long *>(only_this_mask); a.masks[1] = static_cast<unsigned long long *>(only_other_mask);
    a.counts = counts3_dev;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = merge_source_prepare(a.src, src_value, src_weight, nullptr, src_step, src_res, xform12, min_weight, cull, workspace, st)) return rc;
    hipLaunchKernelGGL(k_diff, dim3(div_up(a.d.X, 64), div_up(a.d.Y, 4), div_up(a.d.Z, MERGE_TZ)), dim3(64, 4), 0, st, a);
    XS_CHECK(hipGetLastError());
    return 0;
}
