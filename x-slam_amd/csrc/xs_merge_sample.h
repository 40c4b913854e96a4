// xs_merge_sample.h — "the other map under an affine map of voxel indices", stated once for xs_merge.hip (which averages the sample into the volume)
// and xs_diff.hip (which compares it with the volume): steps 1 to 4 of xs_tsdf_merge's per-voxel contract in include/xslam_amd.h, the brick bits of
// the source, and the cull of a destination tile against them (DESIGN.md sections 4.22 and 4.25).
#pragma once
#include "xs_device.h"
#include "../../include/xslam_amd.h"
#include "../host/merge_host.hpp"

namespace xs {

enum { MERGE_TZ = 16,                // planes a workgroup walks: a tile is 64 x 4 x 16 voxels (at 4 planes the tiles that leave at the cull,
                                     // one dependent load and a barrier each, cost more than the voxels that stay: profiles/merge_probe.txt)
       MERGE_BRICK_CAP = 2048,       // a tile whose box holds more bricks than this is not tested against the brick bits
       MERGE_HEADER_BYTES = 256 };   // the workspace's first bytes, kept free for control words

// the source volume of a merge or a diff as a kernel argument (grad: null where the caller samples the value alone)
struct MergeSource {
    const float *value; const int *weight; const float *grad; size_t step;
    int S[3];
    float m[12];
    int min_weight;
    unsigned cull;
    const unsigned *bricks;          // bit b of the brick grid, brick (bx, by, bz) at b = (bz BY + by) BX + bx
    int BX, BY, BZ;
};

// false for a resolution the launches cannot index: an axis outside 1 .. 65535 x 4, rows that do not fit an int
static inline bool merge_res_ok(const int *r) {
    for (int k = 0; k < 3; ++k)
        if (r[k] < 1 || r[k] > 65535 * 4) return false;
    return (long long)r[1] * (long long)r[2] < (1ll << 31);
}
static inline size_t merge_brick_words(const int *r) {
    const size_t bricks = (size_t)div_up(r[0], 4) * (size_t)div_up(r[1], 4) * (size_t)div_up(r[2], 4);
    return (bricks + 31) / 32;
}
// a header and one bit per brick of 4 x 4 x 4 source voxels
static inline size_t merge_workspace_bytes(const int *src_res) { return MERGE_HEADER_BYTES + ((merge_brick_words(src_res) * sizeof(unsigned) + 255) / 256) * 256; }

// Fills `s` from validated arguments and, with the cull, clears and builds the brick bits in `workspace` on `st` (xs_merge.hip: k_merge_bricks).
int merge_source_prepare(MergeSource &s, const float *src_value, const int *src_weight, const float *src_grad, size_t src_step, const int *src_res,
                         const float *xform12, int min_weight, bool cull, void *workspace, hipStream_t st);

// Steps 1 to 4 of the per-voxel contract for destination voxel (x, y, z).  False when the voxel is skipped at step 2 or at step 3's min_weight
// test; otherwise ws is the smallest needed corner weight (unclamped), sv the interpolated value and, with GRAD, sq the interpolated grad.
template <bool GRAD>
__device__ __forceinline__ bool merge_sample(const MergeSource &a, int x, int y, int z, int &ws_out, float &sv, float &sq) {
    int b[3];
    float f[3];
    bool need[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float g = xs_host::merge_index(a.m, k, x, y, z);
        if (!(g >= 0.f && g <= (float)(a.S[k] - 1))) return false;
        b[k] = __float2int_rd(g);
        f[k] = g - (float)b[k];
        need[k] = f[k] > 0.f;            // then g < S - 1 and b + 1 is inside the source
    }
    const int needmask = (need[0] ? 1 : 0) | (need[1] ? 2 : 0) | (need[2] ? 4 : 0);
    // corner d (bit 0: +x, bit 1: +y, bit 2: +z) is read only where every axis it steps along is needed
    int ws = 0x7fffffff;
#pragma unroll
    for (int d = 0; d < 8; ++d)
        if ((d & ~needmask) == 0) ws = min(ws, row_ptr(a.weight, a.step, a.S[1] * (b[2] + (d >> 2)) + b[1] + (d >> 1 & 1))[b[0] + (d & 1)]);
    if (ws < a.min_weight) return false;
    float v[8], q[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        v[d] = 0.f; q[d] = 0.f;
        if ((d & ~needmask) == 0) {
            const int row = a.S[1] * (b[2] + (d >> 2)) + b[1] + (d >> 1 & 1);
            v[d] = row_ptr(a.value, a.step, row)[b[0] + (d & 1)];
            if (GRAD) q[d] = row_ptr(a.grad, a.step, row)[b[0] + (d & 1)];
        }
    }
    // x, then y, then z; an axis with fraction 0 passes its lower operand through untouched (-0 stays -0)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int stride = 1 << k;
        const float fk = f[k], gk = 1.0f - fk;
#pragma unroll
        for (int d = 0; d < 8; d += 2 * stride) {
            v[d] = need[k] ? v[d] * gk + v[d + stride] * fk : v[d];
            if (GRAD) q[d] = need[k] ? q[d] * gk + q[d + stride] * fk : q[d];
        }
    }
    ws_out = ws;
    sv = v[0];
    sq = q[0];
    return true;
}

// The cull of the destination tile lo .. hi (inclusive voxel indices), by all 256 threads of a 64 x 4 workgroup together: true when the tile's
// source index box misses the source, or touches only bricks without a weight >= min_weight.  The answer is uniform over the workgroup.
__device__ __forceinline__ bool merge_tile_culled(const MergeSource &a, const int *lo, const int *hi) {
    int box[6];
    if (!xs_host::merge_tile_box(a.m, lo, hi, a.S, box)) return true;
    const int bx0 = box[0] >> 2, by0 = box[1] >> 2, bz0 = box[2] >> 2;
    const int nx = (box[3] >> 2) - bx0 + 1, ny = (box[4] >> 2) - by0 + 1, nz = (box[5] >> 2) - bz0 + 1;
    const long long n = (long long)nx * ny * nz;
    if (n > MERGE_BRICK_CAP) return false;
    int any = 0;
    for (int i = (int)threadIdx.y * 64 + (int)threadIdx.x; i < (int)n; i += 256) {
        const int ix = i % nx, iy = i / nx % ny, iz = i / (nx * ny);
        const size_t bi = ((size_t)(bz0 + iz) * (size_t)a.BY + (size_t)(by0 + iy)) * (size_t)a.BX + (size_t)(bx0 + ix);
        any |= (int)(a.bricks[bi >> 5] >> (bi & 31) & 1u);
    }
    return !__syncthreads_or(any);
}

}  // namespace xs
