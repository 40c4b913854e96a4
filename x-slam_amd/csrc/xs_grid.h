// xs_grid.h — the one place that knows the brick grid's layout, for xs_view.hip, xs_reach.hip, xs_travel.hip, xs_frontier.hip and xs_diff.hip
// (DESIGN.md sections 4.18 to 4.21 and 4.25).  The volume is cut into bricks of 4 x 4 x 4 voxels, brick (bx, by, bz) at index (bz BY + by) BX + bx.  Two per-brick
// formats follow that order:
//   the OBSERVATION GRID  one 16-byte word per brick, two bits of state per voxel, voxel (lx, ly, lz) at bit 2 (lx + 4 ly) of dword lz (dword lz
//                         holds the brick's plane lz); bricks that overhang the volume are padded with zeros, which are not a state
//   a MASK                one 64-bit word per brick (the reached and the passable words of the reach buffer, the frontier mask, the two masks of a diff), voxel
//                         (lx, ly, lz) at bit lx + 4 ly + 16 lz, overhang bits clear
// and dense per-voxel arrays (the clearance field, the travel field, the labels) are indexed (z Y + y) X + x.  Also here: the launch shapes
// over voxels and over tiles of 8 x 8 x 8, and the host's loop of rounds to a fixpoint.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "xs_device.h"
#include "../../include/xslam_amd.h"

struct GridDims { int X, Y, Z, BX, BY, BZ; };
// false for a resolution the grid cannot index (a non-positive axis, or 2^31 bricks and more): what a call needs whose kernels run over
// bricks or rays
static inline bool grid_dims(const int *res, GridDims &d) {
    if (!res || res[0] < 1 || res[1] < 1 || res[2] < 1) return false;
    d.X = res[0]; d.Y = res[1]; d.Z = res[2];
    d.BX = (d.X + 3) / 4; d.BY = (d.Y + 3) / 4; d.BZ = (d.Z + 3) / 4;
    return (unsigned long long)d.BX * (unsigned long long)d.BY * (unsigned long long)d.BZ < (1ull << 31);
}
// false also where the y / z extents do not fit a launch's grid dimensions: what a call needs whose kernels run over voxels or tiles
static inline bool grid_dims_launchable(const int *res, GridDims &d) { return grid_dims(res, d) && d.Y <= 65535 && d.Z <= 65535; }
static inline size_t grid_voxels(const GridDims &d) { return (size_t)d.X * (size_t)d.Y * (size_t)d.Z; }
static inline size_t grid_bricks(const GridDims &d) { return (size_t)d.BX * (size_t)d.BY * (size_t)d.BZ; }

// ---- indices -----------------------------------------------------------------------------------------------------------------------------
// the coordinates of brick b, and the index of brick (bx, by, bz)
__host__ __device__ static inline void grid_brick_of(const GridDims &d, unsigned b, int &bx, int &by, int &bz) {
    bx = (int)(b % (unsigned)d.BX); by = (int)(b / (unsigned)d.BX % (unsigned)d.BY); bz = (int)(b / ((unsigned)d.BX * (unsigned)d.BY));
}
// (Index: size_t where the index goes straight into an address, so that a loop over x keeps a 64-bit pointer; int where the caller keeps and
// compares the index itself — fewer than 2^31 bricks, so an int holds it — as k_score_views does per sample)
template <typename Index = size_t>
__host__ __device__ static inline Index grid_brick_at(const GridDims &d, int bx, int by, int bz) {
    return ((Index)bz * (Index)d.BY + (Index)by) * (Index)d.BX + (Index)bx;
}
// the word of the brick that holds voxel (x, y, z), the voxel's bit in a mask word, and its index in a dense per-voxel array; inside the volume only
template <typename Index = size_t>
__host__ __device__ static inline Index grid_word_of(const GridDims &d, int x, int y, int z) { return grid_brick_at<Index>(d, x >> 2, y >> 2, z >> 2); }
__host__ __device__ static inline int grid_bit_of(int x, int y, int z) { return (x & 3) + 4 * (y & 3) + 16 * (z & 3); }
// and back: the voxel of bit `bit` (0 .. 63) of brick (bx, by, bz); it may lie in the brick's overhang
__host__ __device__ static inline void grid_voxel_of_bit(int bx, int by, int bz, int bit, int &x, int &y, int &z) {
    x = 4 * bx + (bit & 3); y = 4 * by + (bit >> 2 & 3); z = 4 * bz + (bit >> 4);
}
__host__ __device__ static inline size_t grid_voxel_of(const GridDims &d, int x, int y, int z) {
    return ((size_t)z * (size_t)d.Y + (size_t)y) * (size_t)d.X + (size_t)x;
}
__host__ __device__ static inline bool grid_inside(const GridDims &d, int x, int y, int z) {
    return (unsigned)x < (unsigned)d.X && (unsigned)y < (unsigned)d.Y && (unsigned)z < (unsigned)d.Z;
}
// voxel (x, y, z)'s bit of the mask words; inside the volume only
__device__ __forceinline__ bool grid_mask_bit(const unsigned long long *__restrict__ words, const GridDims &d, int x, int y, int z) {
    return (words[grid_word_of(d, x, y, z)] >> grid_bit_of(x, y, z) & 1ull) != 0ull;
}

// ---- the observation grid's states -------------------------------------------------------------------------------------------------------
enum { GRID_UNKNOWN = 0, GRID_FREE = 1, GRID_OCCUPIED = 2 };
// the state of voxel (x, y, z) in the dword of its plane, and in its brick's word (x, y, z: the voxel's own coordinates, their low two bits count)
__device__ __forceinline__ unsigned grid_plane_state_of(unsigned plane, int x, int y) { return plane >> (2 * ((x & 3) + 4 * (y & 3))) & 3u; }
__device__ __forceinline__ unsigned grid_state_of(const uint4 &word, int x, int y, int z) {
    const int lz = z & 3;
    return grid_plane_state_of(lz == 0 ? word.x : (lz == 1 ? word.y : (lz == 2 ? word.z : word.w)), x, y);
}

// ---- mask words: faces and growth --------------------------------------------------------------------------------------------------------
// the bits of a mask word on its faces lx = 0, lx = 3, ly = 0 and ly = 3 (the faces lz = 0 and lz = 3 are its low and high 16 bits)
constexpr unsigned long long GRID_X0 = 0x1111111111111111ull, GRID_X3 = 0x8888888888888888ull, GRID_Y0 = 0x000f000f000f000full,
                             GRID_Y3 = 0xf000f000f000f000ull;
// the six face neighbours, inside the brick, of the set bits of m (m itself not included): a shift along x or y must not wrap into the next row or plane
__device__ __forceinline__ unsigned long long grid_neighbours(unsigned long long m) {
    return (m << 1 & ~GRID_X0) | (m >> 1 & ~GRID_X3) | (m << 4 & ~GRID_Y0) | (m >> 4 & ~GRID_Y3) | m << 16 | m >> 16;
}
// the face neighbours, inside this brick, of the set bits of the six neighbouring bricks' words (x-, x+, y-, y+, z-, z+; 0 where the grid has
// no such brick): each word's facing plane, moved onto this brick's opposite face
__device__ __forceinline__ unsigned long long grid_neighbours_across(unsigned long long xm, unsigned long long xp, unsigned long long ym, unsigned long long yp,
                                                                     unsigned long long zm, unsigned long long zp) {
    return (xm & GRID_X3) >> 3 | (xp & GRID_X0) << 3 | (ym & GRID_Y3) >> 12 | (yp & GRID_Y0) << 12 | zm >> 48 | zp << 48;
}

// ---- launches over voxels ----------------------------------------------------------------------------------------------------------------
// thread = voxel: 256 threads along x, y and z from the launch's grid (hence grid_dims_launchable)
enum { GRID_VOXEL_THREADS = 256 };
static inline dim3 grid_voxel_blocks(const GridDims &d) { return dim3(((unsigned)d.X + GRID_VOXEL_THREADS - 1u) / GRID_VOXEL_THREADS, (unsigned)d.Y, (unsigned)d.Z); }
// false for the threads beyond X
__device__ __forceinline__ bool grid_voxel_of_thread(const GridDims &d, int &x, int &y, int &z) {
    x = (int)(blockIdx.x * (unsigned)GRID_VOXEL_THREADS + threadIdx.x); y = (int)blockIdx.y; z = (int)blockIdx.z;
    return x < d.X;
}

// ---- launches over tiles -----------------------------------------------------------------------------------------------------------------
// workgroup = a tile of 8 x 8 x 8 voxels (2 x 2 x 2 bricks), thread t = voxel (t & 7, t >> 3 & 7, t >> 6) of it.  The tile is staged in LDS with
// an apron of one voxel: cell (px, py, pz) of the 10^3, at index (pz 10 + py) 10 + px, is voxel (8 tx - 1 + px, 8 ty - 1 + py, 8 tz - 1 + pz).
enum { GRID_TILE = 8, GRID_TILE_SIDE = GRID_TILE + 2, GRID_TILE_CELLS = GRID_TILE_SIDE * GRID_TILE_SIDE * GRID_TILE_SIDE,
       GRID_TILE_THREADS = GRID_TILE * GRID_TILE * GRID_TILE };
static inline dim3 grid_tile_blocks(const GridDims &d) {
    return dim3((unsigned)((d.X + GRID_TILE - 1) / GRID_TILE), (unsigned)((d.Y + GRID_TILE - 1) / GRID_TILE), (unsigned)((d.Z + GRID_TILE - 1) / GRID_TILE));
}
__device__ __forceinline__ void grid_tile_cell_of(int c, int &px, int &py, int &pz) {
    px = c % GRID_TILE_SIDE; py = c / GRID_TILE_SIDE % GRID_TILE_SIDE; pz = c / (GRID_TILE_SIDE * GRID_TILE_SIDE);
}
// the cell of thread t's own voxel
__device__ __forceinline__ int grid_tile_cell_of_thread(int t) {
    return (((t >> 6) + 1) * GRID_TILE_SIDE + ((t >> 3 & 7) + 1)) * GRID_TILE_SIDE + ((t & 7) + 1);
}
// neighbour k of the 27 around a voxel, k = (dz + 1) 9 + (dy + 1) 3 + (dx + 1) (13 is the voxel itself): its components, and its distance in cell indices
__host__ __device__ constexpr int grid_dx(int k) { return k % 3 - 1; }
__host__ __device__ constexpr int grid_dy(int k) { return k / 3 % 3 - 1; }
__host__ __device__ constexpr int grid_dz(int k) { return k / 9 - 1; }
__host__ __device__ constexpr int grid_tile_step(int k) { return (grid_dz(k) * GRID_TILE_SIDE + grid_dy(k)) * GRID_TILE_SIDE + grid_dx(k); }

// ---- seeds -------------------------------------------------------------------------------------------------------------------------------
// the seeds of a flood or of a travel field as a kernel argument: n of them (1 .. XS_REACH_MAX_SEEDS, the caller checks), (x, y, z) each
struct GridSeeds { int n; int v[3 * XS_REACH_MAX_SEEDS]; };
static inline GridSeeds grid_seeds(const int *seeds3xN, int n) {
    GridSeeds s;
    memset(&s, 0, sizeof(s));
    s.n = n;
    memcpy(s.v, seeds3xN, (size_t)n * 3 * sizeof(int));
    return s;
}

// ---- rounds to a fixpoint ----------------------------------------------------------------------------------------------------------------
// A monotone relaxation (words that only gain bits, distances or labels that only fall) is run in rounds, one launch each, until a round
// changes nothing.  Rounds go in batches, one `changed` word per round of a batch (a round that changed something stores 1 to its word, a
// plain vector store) and one read-back per batch: the first round that changed nothing ends the loop and is counted (the rounds behind it
// in its batch changed nothing either).  launch_round(changed + k) launches round k of a batch on `st`; `changed` is GRID_CONTROL_BYTES of
// device memory.  Ends because every changing round moves at least one of finitely many bounded values one way.
enum { GRID_ROUNDS_PER_BATCH = 8, GRID_CONTROL_BYTES = 256 };
static_assert(GRID_ROUNDS_PER_BATCH * sizeof(unsigned) <= GRID_CONTROL_BYTES, "one changed word per round of a batch");
template <typename LaunchRound>
static int grid_run_rounds(unsigned *changed, hipStream_t st, int *rounds_out, LaunchRound launch_round) {
    int rounds = 0;
    for (;;) {
        unsigned host_changed[GRID_ROUNDS_PER_BATCH];
        XS_CHECK(hipMemsetAsync(changed, 0, sizeof(host_changed), st));
        for (int k = 0; k < GRID_ROUNDS_PER_BATCH; ++k) {
            launch_round(changed + k);
            XS_CHECK(hipGetLastError());
        }
        XS_CHECK(hipMemcpyAsync(host_changed, changed, sizeof(host_changed), hipMemcpyDeviceToHost, st));
        XS_CHECK(hipStreamSynchronize(st));
        int k = 0;
        while (k < GRID_ROUNDS_PER_BATCH && host_changed[k]) ++k;
        if (k < GRID_ROUNDS_PER_BATCH) { rounds += k + 1; break; }
        rounds += GRID_ROUNDS_PER_BATCH;
    }
    if (rounds_out) *rounds_out = rounds;
    return 0;
}
