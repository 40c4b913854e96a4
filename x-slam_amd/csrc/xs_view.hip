// xs_view.hip — what a hypothetical camera would see of the map, for many cameras in one launch (next best view).
//
// The weight volume says which voxels have ever been observed, the value's sign on which side of a surface an observed voxel lies.  Both
// are condensed into an OBSERVATION GRID of two bits per voxel:
//   0 UNKNOWN   weight < min_weight          1 FREE   weight >= min_weight, value >= 0          2 OCCUPIED   weight >= min_weight, value < 0
// one 16-byte word per brick of 4 x 4 x 4 voxels, brick (bx, by, bz) at word (bz * BY + by) * BX + bx, voxel (lx, ly, lz) of it at bit
// 2 (lx + 4 ly + 16 lz): dword lz holds the brick's plane lz.  Bricks that overhang the volume are padded with zeros, which no ray reads
// (a sample is tested against the resolution before its brick is fetched).  Behind the bricks the buffer holds the staging area of one
// launch's poses (xs_score_views copies them there), so one launch at a time per grid.  The layout's arithmetic is xs_grid.h's, shared with
// the kernels that read the grid (xs_reach.hip, xs_frontier.hip).
//   k_view_grid_build    thread = brick: 16 rows of four voxels, each a 16-byte load of the values and one of the weights where the
//                        pitch and the base are 16-byte aligned and the brick lies inside X (the exact per-voxel path otherwise), one
//                        16-byte store.  The volume's 8 bytes per voxel are read once.
//   k_view_grid_expand   one byte per voxel from the grid (tests and viewers)
//   k_score_views        wave = an 8 x 8 tile of the ray lattice of ONE pose (blockIdx.y: the twelve pose floats arrive by scalar loads and
//                        stay in scalar registers); a lane marches its ray through the grid in depth steps, keeps the brick word it is in
//                        in registers and fetches a new one only when the brick index changes; four counters per lane, folded across the
//                        wave (integer DPP adds; the hits by ballot + popcount) and added to the pose's four words by one integer atomic
//                        each — integer sums do not depend on the order, so the result is a pure function of the inputs.
#include <hip/hip_runtime.h>
#include <string.h>
#include <type_traits>
#include <vector>
#include "xs_device.h"
#include "xs_grid.h"
#include "../../include/xslam_amd.h"

static_assert(XS_VIEW_MAX_POSES == 4096, "the header's bound");
enum { VIEW_POSE_FLOATS = 12, VIEW_MAX_SAMPLES = 4096 };

extern "C" size_t xs_view_grid_bytes(const int *res) {
    GridDims d;
    if (!grid_dims(res, d)) return 0;
    return grid_bricks(d) * 16 + (size_t)XS_VIEW_MAX_POSES * VIEW_POSE_FLOATS * sizeof(float);
}

__device__ __forceinline__ unsigned view_state(float value, int weight, int min_weight) {
    return weight < min_weight ? (unsigned)GRID_UNKNOWN : (value < 0.f ? (unsigned)GRID_OCCUPIED : (unsigned)GRID_FREE);
}

__global__ void __launch_bounds__(256) k_view_grid_build(const float *__restrict__ value, const int *__restrict__ weight, size_t vol_step, GridDims d,
                                                         int min_weight, int vector_rows, unsigned nbricks, uint4 *__restrict__ grid) {
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nbricks) return;
    int bx, by, bz;
    grid_brick_of(d, b, bx, by, bz);
    const int x0 = 4 * bx;
    const bool whole_row = vector_rows && x0 + 4 <= d.X;   // (the row's first voxel is then 16-byte aligned: base and pitch are)
    unsigned w[4];
#pragma unroll
    for (int lz = 0; lz < 4; ++lz) {
        unsigned bits = 0;
        const int z = 4 * bz + lz;
#pragma unroll
        for (int ly = 0; ly < 4; ++ly) {
            const int y = 4 * by + ly;
            if (z >= d.Z || y >= d.Y) continue;            // padding: zeros
            const size_t row = (size_t)z * (size_t)d.Y + (size_t)y;
            const float *v = reinterpret_cast<const float *>(reinterpret_cast<const char *>(value) + row * vol_step) + x0;
            const int *k = reinterpret_cast<const int *>(reinterpret_cast<const char *>(weight) + row * vol_step) + x0;
            unsigned s0, s1, s2, s3;
            if (whole_row) {
                const float4 vv = *reinterpret_cast<const float4 *>(v);
                const int4 kk = *reinterpret_cast<const int4 *>(k);
                s0 = view_state(vv.x, kk.x, min_weight); s1 = view_state(vv.y, kk.y, min_weight);
                s2 = view_state(vv.z, kk.z, min_weight); s3 = view_state(vv.w, kk.w, min_weight);
            } else {
                s0 = x0 + 0 < d.X ? view_state(v[0], k[0], min_weight) : 0u; s1 = x0 + 1 < d.X ? view_state(v[1], k[1], min_weight) : 0u;
                s2 = x0 + 2 < d.X ? view_state(v[2], k[2], min_weight) : 0u; s3 = x0 + 3 < d.X ? view_state(v[3], k[3], min_weight) : 0u;
            }
            bits |= (s0 | s1 << 2 | s2 << 4 | s3 << 6) << (8 * ly);
        }
        w[lz] = bits;
    }
    grid[b] = make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ void __launch_bounds__(GRID_VOXEL_THREADS) k_view_grid_expand(const uint4 *__restrict__ grid, GridDims d, unsigned char *__restrict__ states) {
    int x, y, z;
    if (!grid_voxel_of_thread(d, x, y, z)) return;
    states[grid_voxel_of(d, x, y, z)] = (unsigned char)grid_state_of(grid[grid_word_of(d, x, y, z)], x, y, z);
}

extern "C" int xs_view_grid_build(const float *value, const int *weight, size_t vol_step, const int *res, int min_weight, void *grid, void *stream) {
    GridDims d;
    if (!value || !weight || !grid) return xs_set_error(hipErrorInvalidValue, "xs_view_grid_build: null pointer");
    if (!grid_dims(res, d)) return xs_set_error(hipErrorInvalidValue, "xs_view_grid_build: bad resolution");
    if (vol_step < (size_t)d.X * sizeof(float) || vol_step % sizeof(float) != 0) return xs_set_error(hipErrorInvalidValue, "xs_view_grid_build: bad pitch");
    if (reinterpret_cast<uintptr_t>(grid) % 16 != 0) return xs_set_error(hipErrorInvalidValue, "xs_view_grid_build: the grid must be 16-byte aligned");
    const int vector_rows = vol_step % 16 == 0 && reinterpret_cast<uintptr_t>(value) % 16 == 0 && reinterpret_cast<uintptr_t>(weight) % 16 == 0;
    const unsigned nbricks = (unsigned)grid_bricks(d);
    hipLaunchKernelGGL(k_view_grid_build, dim3((nbricks + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, value, weight, vol_step, d,
                       min_weight < 1 ? 1 : min_weight, vector_rows, nbricks, static_cast<uint4 *>(grid));
    XS_CHECK(hipGetLastError());
    return 0;
}

extern "C" int xs_view_grid_expand(const void *grid, const int *res, unsigned char *states_dev, void *stream) {
    GridDims d;
    if (!grid || !states_dev) return xs_set_error(hipErrorInvalidValue, "xs_view_grid_expand: null pointer");
    if (!grid_dims_launchable(res, d)) return xs_set_error(hipErrorInvalidValue, "xs_view_grid_expand: bad resolution");
    hipLaunchKernelGGL(k_view_grid_expand, grid_voxel_blocks(d), dim3(GRID_VOXEL_THREADS), 0, (hipStream_t)stream, static_cast<const uint4 *>(grid), d, states_dev);
    XS_CHECK(hipGetLastError());
    return 0;
}

// ---- the scoring kernel ----------------------------------------------------------------------------------------------------------------
// The arithmetic contract (include/xslam_amd.h): every operation below is one IEEE float operation, in this order (the library is built
// -ffp-contract=off), so a float32 model on the host gives the same counts.
struct ViewArgs {
    const uint4 *grid;
    const float *poses;                          // [P][12]: R row-major, then t (camera to volume), in the grid buffer's staging area
    unsigned *out;                               // [P][4]: unknown, free, hits, frontier
    GridDims d;
    int rays_x, rays_y, tiles_x, samples;
    float sx, sy;                                // float(cols) / float(rays_x), float(rows) / float(rays_y)
    float fx, fy, cx, cy;
    float t_near, step, voxel_size;
};

// all 64 lanes: v[l] + v[l ^ 1], ^ 2, 4, 8 by DPP within a row of 16, then the rows; the same sum in every lane (integer adds: any order)
__device__ __forceinline__ unsigned wave_sum_dpp_u32(unsigned v) {
    auto dpp = [](unsigned x, auto ctrl) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, decltype(ctrl)::value, 0xf, 0xf, false); };
    v += dpp(v, std::integral_constant<int, 0xb1>());    // quad_perm [1, 0, 3, 2]
    v += dpp(v, std::integral_constant<int, 0x4e>());    // quad_perm [2, 3, 0, 1]
    v += dpp(v, std::integral_constant<int, 0x141>());   // row_half_mirror
    v += dpp(v, std::integral_constant<int, 0x140>());   // row_mirror
    v += (unsigned)__shfl_xor((int)v, 16, 64);
    v += (unsigned)__shfl_xor((int)v, 32, 64);
    return v;
}

__global__ void __launch_bounds__(64) k_score_views(const ViewArgs a) {
    const int lane = threadIdx.x;
    const int tile = blockIdx.x, ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const unsigned pose = blockIdx.y;
    const float *__restrict__ P = a.poses + (size_t)pose * VIEW_POSE_FLOATS;   // wave-uniform: scalar loads
    const float R00 = P[0], R01 = P[1], R02 = P[2], R10 = P[3], R11 = P[4], R12 = P[5], R20 = P[6], R21 = P[7], R22 = P[8];
    const float t0 = P[9], t1 = P[10], t2 = P[11];
    const int i = tx * 8 + (lane & 7), j = ty * 8 + (lane >> 3);
    unsigned n_unknown = 0, n_free = 0, n_frontier = 0;
    bool hit = false;
    if (i < a.rays_x && j < a.rays_y) {
        const float u = ((float)i + 0.5f) * a.sx, v = ((float)j + 0.5f) * a.sy;
        const float dx = (u - a.cx) / a.fx, dy = (v - a.cy) / a.fy;
        const float d0 = (R00 * dx + R01 * dy) + R02, d1 = (R10 * dx + R11 * dy) + R12, d2 = (R20 * dx + R21 * dy) + R22;
        const uint4 *__restrict__ grid = a.grid;
        uint4 word = make_uint4(0, 0, 0, 0);
        int cur = -1;                            // the brick `word` holds
        bool prev_free = false, was_inside = false;
        for (int k = 0; k < a.samples; ++k) {
            const float t = a.t_near + (float)k * a.step;
            const float p0 = t0 + t * d0, p1 = t1 + t * d1, p2 = t2 + t * d2;
            const int x = __float2int_rd(p0 / a.voxel_size), y = __float2int_rd(p1 / a.voxel_size), z = __float2int_rd(p2 / a.voxel_size);
            if (!grid_inside(a.d, x, y, z)) {
                // outside: the sample counts nothing.  Every coordinate is monotone in k, so a ray that has left the volume stays outside.
                if (was_inside) break;
                continue;
            }
            was_inside = true;
            const int b = grid_word_of<int>(a.d, x, y, z);
            if (b != cur) { word = grid[b]; cur = b; }
            const unsigned s = grid_state_of(word, x, y, z);
            if (s == GRID_OCCUPIED) { hit = true; break; }
            if (s == GRID_FREE) { ++n_free; prev_free = true; }
            else { ++n_unknown; n_frontier += prev_free ? 1u : 0u; prev_free = false; }
        }
    }
    const unsigned hits = (unsigned)__popcll(__ballot(hit));
    const unsigned unknown = wave_sum_dpp_u32(n_unknown), free_ = wave_sum_dpp_u32(n_free), frontier = wave_sum_dpp_u32(n_frontier);
    if (lane == 0) {
        unsigned *o = a.out + 4 * (size_t)pose;
        if (unknown) atomicAdd(o + 0, unknown);
        if (free_) atomicAdd(o + 1, free_);
        if (hits) atomicAdd(o + 2, hits);
        if (frontier) atomicAdd(o + 3, frontier);
    }
}

extern "C" int xs_score_views(int poses, const float *Rc2v9xP, const float *tc2v3xP, const float *intr4, int rows, int cols, const int *res,
                              float voxel_size, const void *grid, const xs_view_opts *opts, unsigned *out4xP_dev, void *stream) {
    if (poses < 1 || poses > XS_VIEW_MAX_POSES) return xs_set_error(hipErrorInvalidValue, "xs_score_views: poses outside 1 .. XS_VIEW_MAX_POSES");
    if (!Rc2v9xP || !tc2v3xP || !intr4 || !grid || !out4xP_dev) return xs_set_error(hipErrorInvalidValue, "xs_score_views: null pointer");
    if (opts && opts->struct_bytes != sizeof(xs_view_opts)) return xs_set_error(hipErrorInvalidValue, "xs_score_views: opts->struct_bytes is not sizeof(xs_view_opts)");
    ViewArgs a;
    memset(&a, 0, sizeof(a));
    if (!grid_dims(res, a.d)) return xs_set_error(hipErrorInvalidValue, "xs_score_views: bad resolution");
    if (!(voxel_size > 0.f) || rows < 1 || cols < 1) return xs_set_error(hipErrorInvalidValue, "xs_score_views: bad voxel size or image size");
    xs_view_opts o;
    memset(&o, 0, sizeof(o));
    if (opts) o = *opts;
    if (o.rays_x == 0 && o.rays_y == 0) { o.rays_x = 80; o.rays_y = 60; }
    if (o.t_near == 0.f && o.t_far == 0.f) { o.t_near = 0.2f; o.t_far = 5.0f; }
    if (o.step == 0.f) o.step = voxel_size;
    if (o.rays_x < 1 || o.rays_y < 1 || o.rays_x > cols || o.rays_y > rows) return xs_set_error(hipErrorInvalidValue, "xs_score_views: ray lattice outside 1 .. cols x 1 .. rows");
    if (!(o.step > 0.f)) return xs_set_error(hipErrorInvalidValue, "xs_score_views: step <= 0");
    if (!(o.t_far > o.t_near)) return xs_set_error(hipErrorInvalidValue, "xs_score_views: t_far <= t_near");
    // the samples of a ray: k = 0, 1, ... while t_near + float(k) * step < t_far, the kernel's own expression (monotone in k)
    int samples = 0;
    while (samples <= VIEW_MAX_SAMPLES && o.t_near + (float)samples * o.step < o.t_far) ++samples;
    if (samples > VIEW_MAX_SAMPLES) return xs_set_error(hipErrorInvalidValue, "xs_score_views: more than 4096 samples per ray");
    if ((unsigned long long)o.rays_x * (unsigned long long)o.rays_y * (unsigned long long)samples >= (1ull << 32))
        return xs_set_error(hipErrorInvalidValue, "xs_score_views: rays x samples does not fit a 32-bit count");
    a.grid = static_cast<const uint4 *>(grid);
    // the staging area behind the bricks (the one part of the grid buffer this call writes)
    float *staging = reinterpret_cast<float *>(static_cast<char *>(const_cast<void *>(grid)) + grid_bricks(a.d) * 16);
    a.poses = staging;
    a.out = out4xP_dev;
    a.rays_x = o.rays_x; a.rays_y = o.rays_y; a.samples = samples;
    a.tiles_x = (o.rays_x + 7) / 8;
    const unsigned tiles = (unsigned)a.tiles_x * (unsigned)((o.rays_y + 7) / 8);
    a.sx = (float)cols / (float)o.rays_x; a.sy = (float)rows / (float)o.rays_y;
    a.fx = intr4[0]; a.fy = intr4[1]; a.cx = intr4[2]; a.cy = intr4[3];
    a.t_near = o.t_near; a.step = o.step; a.voxel_size = voxel_size;
    std::vector<float> P((size_t)poses * VIEW_POSE_FLOATS);
    for (int p = 0; p < poses; ++p) {
        for (int k = 0; k < 9; ++k) P[(size_t)p * VIEW_POSE_FLOATS + k] = Rc2v9xP[9 * (size_t)p + k];
        for (int k = 0; k < 3; ++k) P[(size_t)p * VIEW_POSE_FLOATS + 9 + k] = tc2v3xP[3 * (size_t)p + k];
    }
    hipStream_t st = (hipStream_t)stream;
    XS_CHECK(hipMemcpyAsync(staging, P.data(), P.size() * sizeof(float), hipMemcpyHostToDevice, st));   // (pageable: staged before the call returns)
    XS_CHECK(hipMemsetAsync(out4xP_dev, 0, (size_t)poses * 4 * sizeof(unsigned), st));
    hipLaunchKernelGGL(k_score_views, dim3(tiles, (unsigned)poses), dim3(64), 0, st, a);
    XS_CHECK(hipGetLastError());
    return 0;
}
