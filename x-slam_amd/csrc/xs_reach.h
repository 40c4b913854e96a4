// xs_reach.h — what xs_reach.hip, xs_travel.hip and xs_frontier.hip share: the dimensions of the brick grid and the layout of the reach
// buffer, which the frontier mask's words follow (DESIGN.md sections 4.19 to 4.21).  One 64-bit word per brick of 4 x 4 x 4 voxels, bricks in the observation grid's order ((bz BY + by) BX + bx),
// voxel (lx, ly, lz) at bit lx + 4 ly + 16 lz, overhang bits clear: the reached words first, the passable words behind them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/xslam_amd.h"

struct ReachDims { int X, Y, Z, BX, BY, BZ; };
// false for a resolution the grid cannot index or whose y / z extents do not fit a launch's grid dimensions
static inline bool reach_dims(const int *res, ReachDims &d) {
    if (!res || res[0] < 1 || res[1] < 1 || res[2] < 1) return false;
    d.X = res[0]; d.Y = res[1]; d.Z = res[2];
    d.BX = (d.X + 3) / 4; d.BY = (d.Y + 3) / 4; d.BZ = (d.Z + 3) / 4;
    if (d.Y > 65535 || d.Z > 65535) return false;
    return (unsigned long long)d.BX * (unsigned long long)d.BY * (unsigned long long)d.BZ < (1ull << 31);
}
static inline size_t reach_voxels(const ReachDims &d) { return (size_t)d.X * (size_t)d.Y * (size_t)d.Z; }
static inline size_t reach_bricks(const ReachDims &d) { return (size_t)d.BX * (size_t)d.BY * (size_t)d.BZ; }
__host__ __device__ static inline unsigned long long *reach_passable_of(void *reach, size_t nbricks) { return static_cast<unsigned long long *>(reach) + nbricks; }

// the word of the brick that holds voxel (x, y, z), the voxel's bit in it, and its index in a dense per-voxel array; inside the volume only
__host__ __device__ static inline size_t reach_word_of(const ReachDims &d, int x, int y, int z) {
    return ((size_t)(z >> 2) * (size_t)d.BY + (size_t)(y >> 2)) * (size_t)d.BX + (size_t)(x >> 2);
}
__host__ __device__ static inline int reach_bit_of(int x, int y, int z) { return (x & 3) + 4 * (y & 3) + 16 * (z & 3); }
__host__ __device__ static inline size_t reach_voxel_of(const ReachDims &d, int x, int y, int z) {
    return ((size_t)z * (size_t)d.Y + (size_t)y) * (size_t)d.X + (size_t)x;
}
__host__ __device__ static inline bool reach_inside(const ReachDims &d, int x, int y, int z) {
    return (unsigned)x < (unsigned)d.X && (unsigned)y < (unsigned)d.Y && (unsigned)z < (unsigned)d.Z;
}

// the seeds of a flood or of a travel field as a kernel argument: n of them, (x, y, z) each
struct ReachSeeds { int n; int v[3 * XS_REACH_MAX_SEEDS]; };
