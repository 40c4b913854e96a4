// xs_scale_depth.hip — depth scaling and the frame's tile table for gfx950.  Replaces XKinectFusion/src/TsdfFusion.cu:68-82
// (scaleDepthKernal).
#include "xs_device.h"
#include "xs_depth_tiles.h"
#include "../../include/xslam_amd.h"

using namespace xs;

// scaleDepthKernal (TsdfFusion.cu:68-82) + what the integrate kernel wants to know about the frame: its largest valid depth and the
// smallest and the largest VALID scaled depth per DEPTH_TILE x DEPTH_TILE pixel tile and per 64 x 32 pixel block of tiles ("super tile":
// what one workgroup covers): {lo, hi}, lo NEGATED where the tile holds an invalid pixel (depth 0) — a tile with a hole or a speckle still
// says how near its valid pixels come (round 5: boxes that see such tiles stream their free planes with a validity test instead of walking
// them); a tile without a valid pixel is {-inf, 0}.  A wave takes a strip of 64 pixels x
// DEPTH_TILE rows — every row a coalesced 128-byte read and 256-byte write — lane l carries its column's min / max down the rows, three
// cross-lane steps fold the eight columns of a tile, three more the eight tiles of the strip, and LDS the workgroup's four strips.
template <class Src> __device__ __forceinline__ float scaled_depth_of(Src v);
template <> __device__ __forceinline__ float scaled_depth_of<uint16_t>(uint16_t v) {
    const int Dp = v;
    return (Dp > 5000 || Dp < 200) ? 0.f : float(Dp) / 1000.f;   // metres
}
template <> __device__ __forceinline__ float scaled_depth_of<float>(float v) { return v; }   // already scaled: tiles only
// grid (ceil(cols / 64), ceil(rows / 32)), block 256: wave w of workgroup (bx, by) takes pixels [64 bx, +64) x rows [32 by + 8 w, +8)
template <class Src>
__global__ void __launch_bounds__(256) k_scale_depth(const Src *depth, size_t dstep, int rows, int cols, float *scaled, size_t sstep,
                                                     unsigned *max_bits, DepthTile *tiles, int tiles_x, int tiles_y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lane, ty = blockIdx.y * 4 + wave;
    float lo = __builtin_inff(), hi = 0.f;   // over the valid pixels
    int inv = 0;                             // an invalid pixel seen
#pragma unroll
    for (int r = 0; r < DEPTH_TILE; ++r) {
        const int y = ty * DEPTH_TILE + r;
        if (x < cols && y < rows) {
            const float v = scaled_depth_of<Src>(row_ptr(depth, dstep, y)[x]);
            if (scaled) row_ptr(scaled, sstep, y)[x] = v;
            if (v > 0.f) lo = fminf(lo, v); else inv = 1;
            hi = fmaxf(hi, v);
        }
    }
    __shared__ float s_lo[4], s_hi[4];
    __shared__ int s_inv[4];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64)); hi = fmaxf(hi, __shfl_xor(hi, off, 64)); inv |= __shfl_xor(inv, off, 64);
        if (off == DEPTH_TILE / 2 && tiles && (lane & (DEPTH_TILE - 1)) == 0 && x < cols && ty < tiles_y)
            tiles[ty * tiles_x + (x / DEPTH_TILE)] = DepthTile{depth_tile_encode(lo, inv != 0), hi};
    }
    if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; s_inv[wave] = inv; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3])); hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
        inv = s_inv[0] | s_inv[1] | s_inv[2] | s_inv[3];
        if (tiles) tiles[(size_t)tiles_x * tiles_y + blockIdx.y * gridDim.x + blockIdx.x] = DepthTile{depth_tile_encode(lo, inv != 0), hi};
        const unsigned b = __float_as_uint(hi);  // non-negative floats order like their bit patterns
        if (max_bits && b) atomicMax(max_bits, b);
    }
}
template <class Src>
static void launch_scale_depth(const Src *src, size_t src_step, int rows, int cols, float *scaled, size_t scaled_step, float *max_dev, void *tiles_dev, hipStream_t st) {
    hipLaunchKernelGGL(k_scale_depth<Src>, dim3(div_up(cols, SUPER_W), div_up(rows, SUPER_H)), dim3(256), 0, st, src, src_step, rows, cols, scaled, scaled_step,
                       (unsigned *)max_dev, (DepthTile *)tiles_dev, div_up(cols, DEPTH_TILE), div_up(rows, DEPTH_TILE));
}
void xs::launch_depth_tiles(const float *scaled, size_t scaled_step, int rows, int cols, void *tiles_dev, hipStream_t st) {
    launch_scale_depth(scaled, scaled_step, rows, cols, (float *)nullptr, (size_t)0, (float *)nullptr, tiles_dev, st);
}

/* max_dev: optional device float that receives max(scaled) via atomicMax on its bits; the caller
 * zeroes it before the launch (used by integrate to stop walking behind the farthest surface).
 * tiles_dev: optional table of xs_depth_tiles_bytes(rows, cols) bytes that receives the per-tile depth range
 * (xs_integrate_opts.depth_tiles hands it to the integrate calls). */
extern "C" size_t xs_depth_tiles_bytes(int rows, int cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return depth_tiles_count(rows, cols) * sizeof(DepthTile);
}
extern "C" int xs_scale_depth_tiles(const uint16_t *depth, size_t depth_step, int rows, int cols, float *scaled, size_t scaled_step,
                                    float *max_dev, void *tiles_dev, void *stream) {
    if (!depth || !scaled) return xs_set_error(hipErrorInvalidValue, "xs_scale_depth: null pointer");
    if (rows <= 0 || cols <= 0) return 0;
    launch_scale_depth(depth, depth_step, rows, cols, scaled, scaled_step, max_dev, tiles_dev, (hipStream_t)stream);
    XS_CHECK(hipGetLastError());
    return 0;
}
extern "C" int xs_scale_depth_max(const uint16_t *depth, size_t depth_step, int rows, int cols, float *scaled, size_t scaled_step,
                                  float *max_dev, void *stream) {
    return xs_scale_depth_tiles(depth, depth_step, rows, cols, scaled, scaled_step, max_dev, nullptr, stream);
}
/* the tile table of an image that is already scaled (what xs_integrate_scaled does itself when nobody handed it one) */
extern "C" int xs_depth_tiles(const float *scaled, size_t scaled_step, int rows, int cols, void *tiles_dev, void *stream) {
    if (!scaled || !tiles_dev) return xs_set_error(hipErrorInvalidValue, "xs_depth_tiles: null pointer");
    if (rows <= 0 || cols <= 0) return 0;
    launch_scale_depth(scaled, scaled_step, rows, cols, (float *)nullptr, (size_t)0, (float *)nullptr, tiles_dev, (hipStream_t)stream);
    XS_CHECK(hipGetLastError());
    return 0;
}
extern "C" int xs_scale_depth(const uint16_t *depth, size_t depth_step, int rows, int cols, float *scaled, size_t scaled_step, void *stream) {
    return xs_scale_depth_max(depth, depth_step, rows, cols, scaled, scaled_step, nullptr, stream);
}
