// xs_travel.hip — how far it is to a reached voxel, and which way: a geodesic travel-distance field over the REACHED set of xs_reach.hip and
// a walk down it.  Integer arithmetic throughout: the field is the unique fixpoint of d[v] = min(d[v], d[u] + w)
// under the limit, so every result is a pure function of the inputs, two runs give equal bytes, and there is no atomic.
//
// MOVES  the 26 neighbour offsets o, index k = (dz + 1) 9 + (dy + 1) 3 + (dx + 1), cost 3, 4 or 5 for one, two or three non-zero components
// (the <3, 4, 5> chamfer metric: a unit is a third of a voxel edge).  v -> v + o is allowed iff v + o is in the domain and so is every
// v + o' with o' = o with a non-empty proper subset of its non-zero components zeroed (no corner cutting).
//   k_travel_seed    one lane: 0 at the seeds whose bit is set in the reached words (the caller's fill of 0xFF is NONE everywhere else)
//   k_travel_round   workgroup = a tile of 8 x 8 x 8 voxels (2 x 2 x 2 bricks), thread = voxel.  A tile with no reached bit returns at once.
//                    Otherwise the 4 x 4 x 4 brick words around the tile go to LDS (one load per lane of the first wave), then the 10^3 travel
//                    values of tile plus apron (NONE outside the domain), each thread forms its 26-bit allowed-move mask once, and the
//                    tile is relaxed against LDS until nothing in it changes.  Threads write back their own voxel if it fell; one thread
//                    stores 1 to the round's `changed` word.  The apron is read from global memory every round: a stale value delays a
//                    distance by a round and never invents one.  Every barrier is reached by all 512 threads: the empty-tile exit and
//                    the loop's exit are decided by __syncthreads_or.
//   k_travel_path    lane = target: walks down the field by the lowest-index allowed move with travel[v + o] + w(o) = travel[v]
//   k_travel_query   lane = integer voxel: travel[v], NONE outside the volume
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xs_device.h"
#include "xs_grid.h"
#include "../../include/xslam_amd.h"

static_assert(XS_TRAVEL_NONE == 65535 && XS_TRAVEL_MAX == 65534 && XS_TRAVEL_MAX_TARGETS == 64, "the header's bounds");

// move k of the 27 (13 is no move; its components: grid_dx, grid_dy, grid_dz): its cost, and the neighbour bits (k's own included) that must
// all be in the domain
__host__ __device__ constexpr int travel_cost(int k) {
    return 2 + (grid_dx(k) != 0) + (grid_dy(k) != 0) + (grid_dz(k) != 0);
}
__host__ __device__ constexpr unsigned travel_need(int k) {
    unsigned m = 0;
    for (int s = 1; s < 8; ++s) {                                  // s: which components are kept
        const int dx = (s & 1) ? grid_dx(k) : 0, dy = (s & 2) ? grid_dy(k) : 0, dz = (s & 4) ? grid_dz(k) : 0;
        if (dx == 0 && dy == 0 && dz == 0) continue;
        m |= 1u << ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
    }
    return m;
}
static_assert(travel_need(14) == (1u << 14) && travel_need(26) == ((1u << 14) | (1u << 16) | (1u << 17) | (1u << 22) | (1u << 23) | (1u << 25) | (1u << 26)),
              "a face move needs its target, a corner move the three faces, the three edges and the corner");
static_assert(travel_cost(14) == 3 && travel_cost(17) == 4 && travel_cost(26) == 5 && travel_cost(0) == 5, "3, 4, 5");

extern "C" size_t xs_travel_bytes(const int *res) {
    GridDims d;
    return grid_dims_launchable(res, d) ? grid_voxels(d) * sizeof(uint16_t) : 0;
}
extern "C" size_t xs_travel_workspace_bytes(void) { return GRID_CONTROL_BYTES; }   // the `changed` words of grid_run_rounds

__global__ void k_travel_seed(GridSeeds s, GridDims d, const unsigned long long *__restrict__ words, uint16_t *__restrict__ travel) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int k = 0; k < s.n; ++k) {
        const int x = s.v[3 * k], y = s.v[3 * k + 1], z = s.v[3 * k + 2];
        if (!grid_inside(d, x, y, z)) continue;
        if (grid_mask_bit(words, d, x, y, z)) travel[grid_voxel_of(d, x, y, z)] = 0;
    }
}

__global__ void __launch_bounds__(GRID_TILE_THREADS) k_travel_round(uint16_t *travel, const unsigned long long *__restrict__ words, GridDims d, unsigned limit,
                                                                     unsigned *changed) {
    __shared__ unsigned long long dom[64];                         // the 4 x 4 x 4 bricks from brick (2 tx - 1, 2 ty - 1, 2 tz - 1)
    __shared__ uint16_t dist[GRID_TILE_CELLS];                     // the travel values of tile plus apron
    const int t = (int)threadIdx.x;
    const int tx = (int)blockIdx.x, ty = (int)blockIdx.y, tz = (int)blockIdx.z;
    // the brick of lane t < 64 among those 4 x 4 x 4; the tile's own eight are the ones with all three coordinates in {1, 2}
    unsigned long long w = 0ull;
    bool own = false;
    if (t < 64) {
        const int jx = t & 3, jy = t >> 2 & 3, jz = t >> 4;
        const int bx = 2 * tx - 1 + jx, by = 2 * ty - 1 + jy, bz = 2 * tz - 1 + jz;
        if ((unsigned)bx < (unsigned)d.BX && (unsigned)by < (unsigned)d.BY && (unsigned)bz < (unsigned)d.BZ)
            w = words[grid_brick_at(d, bx, by, bz)];
        own = ((jx - 1) | (jy - 1) | (jz - 1)) >> 1 == 0;          // each of jx - 1, jy - 1, jz - 1 is 0 or 1
        dom[t] = w;
    }
    if (!__syncthreads_or(own && w != 0ull)) return;               // (block-uniform; the barrier also publishes dom)
    // cell c of the 10^3 lies at voxel q = cell + 3 of the 16^3 the bricks span
    auto in_domain = [&](int px, int py, int pz) {
        const int qx = px + 3, qy = py + 3, qz = pz + 3;
        return (dom[(qx >> 2) + 4 * (qy >> 2) + 16 * (qz >> 2)] >> grid_bit_of(qx, qy, qz) & 1ull) != 0ull;
    };
    const int x0 = GRID_TILE * tx - 1, y0 = GRID_TILE * ty - 1, z0 = GRID_TILE * tz - 1;
    for (int c = t; c < GRID_TILE_CELLS; c += GRID_TILE_THREADS) {
        int px, py, pz;
        grid_tile_cell_of(c, px, py, pz);
        const int x = x0 + px, y = y0 + py, z = z0 + pz;
        uint16_t v = XS_TRAVEL_NONE;
        if (in_domain(px, py, pz) && grid_inside(d, x, y, z)) v = travel[grid_voxel_of(d, x, y, z)];
        dist[c] = v;
    }
    // this thread's voxel, its cell, the domain bits of the 27 cells around it and from them the allowed moves
    const int lx = t & 7, ly = t >> 3 & 7, lz = t >> 6;
    const int cell = grid_tile_cell_of_thread(t);
    unsigned around = 0u, moves = 0u;
#pragma unroll
    for (int k = 0; k < 27; ++k)
        if (in_domain(lx + 1 + grid_dx(k), ly + 1 + grid_dy(k), lz + 1 + grid_dz(k))) around |= 1u << k;
    if (around >> 13 & 1u) {
#pragma unroll
        for (int k = 0; k < 27; ++k)
            if (k != 13 && (around & travel_need(k)) == travel_need(k)) moves |= 1u << k;
    }
    __syncthreads();
    const unsigned first = dist[cell];
    unsigned mine = first;
    for (;;) {
        unsigned best = mine;
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            if (k == 13 || !(moves >> k & 1u)) continue;
            const unsigned cand = (unsigned)dist[cell + grid_tile_step(k)] + (unsigned)travel_cost(k);
            best = min(best, cand);
        }
        const bool fell = best < mine && best <= limit;           // (NONE + w is above every limit)
        if (fell) { mine = best; dist[cell] = (uint16_t)best; }   // in place: values only fall, each is the length of a real path
        if (!__syncthreads_or(fell)) break;                        // (block-uniform)
    }
    const bool fell = mine < first;
    if (fell) travel[grid_voxel_of(d, x0 + 1 + lx, y0 + 1 + ly, z0 + 1 + lz)] = (uint16_t)mine;   // (in the domain, so inside the volume)
    if (__syncthreads_or(fell) && t == 0) *changed = 1u;
}

extern "C" int xs_travel_build(const void *reach, const int *res, const int *seeds3xN, int seeds, int limit, unsigned short *travel_dev, void *workspace,
                               int *rounds_out, void *stream) {
    GridDims d;
    if (!reach || !seeds3xN || !travel_dev || !workspace) return xs_set_error(hipErrorInvalidValue, "xs_travel_build: null pointer");
    if (!grid_dims_launchable(res, d)) return xs_set_error(hipErrorInvalidValue, "xs_travel_build: bad resolution");
    if (seeds < 1 || seeds > XS_REACH_MAX_SEEDS) return xs_set_error(hipErrorInvalidValue, "xs_travel_build: seeds outside 1 .. XS_REACH_MAX_SEEDS");
    if (limit < 0 || limit > XS_TRAVEL_MAX) return xs_set_error(hipErrorInvalidValue, "xs_travel_build: limit outside 0 .. XS_TRAVEL_MAX");
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long *words = static_cast<const unsigned long long *>(reach);
    unsigned *changed = static_cast<unsigned *>(workspace);
    XS_CHECK(hipMemsetAsync(travel_dev, 0xFF, grid_voxels(d) * sizeof(uint16_t), st));
    hipLaunchKernelGGL(k_travel_seed, dim3(1), dim3(64), 0, st, grid_seeds(seeds3xN, seeds), d, words, travel_dev);
    XS_CHECK(hipGetLastError());
    // every changing round lowers at least one of finitely many bounded integers
    return grid_run_rounds(changed, st, rounds_out, [&](unsigned *changed_k) {
        hipLaunchKernelGGL(k_travel_round, grid_tile_blocks(d), dim3(GRID_TILE_THREADS), 0, st, travel_dev, words, d, (unsigned)limit, changed_k);
    });
}

// ---- the field at integer voxels ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_travel_query(int n, const int *__restrict__ voxel, GridDims d, const uint16_t *__restrict__ travel, uint16_t *__restrict__ out) {
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    if (i >= n) return;
    const int x = voxel[3 * (size_t)i], y = voxel[3 * (size_t)i + 1], z = voxel[3 * (size_t)i + 2];
    out[i] = grid_inside(d, x, y, z) ? travel[grid_voxel_of(d, x, y, z)] : (uint16_t)XS_TRAVEL_NONE;
}

extern "C" int xs_travel_query(int n, const int *voxel3xN_dev, const int *res, const unsigned short *travel_dev, unsigned short *out_dev, void *stream) {
    GridDims d;
    if (!voxel3xN_dev || !travel_dev || !out_dev) return xs_set_error(hipErrorInvalidValue, "xs_travel_query: null pointer");
    if (!grid_dims_launchable(res, d)) return xs_set_error(hipErrorInvalidValue, "xs_travel_query: bad resolution");
    if (n < 1) return xs_set_error(hipErrorInvalidValue, "xs_travel_query: n < 1");
    hipLaunchKernelGGL(k_travel_query, dim3(((unsigned)n + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, n, voxel3xN_dev, d, travel_dev, out_dev);
    XS_CHECK(hipGetLastError());
    return 0;
}

// ---- the walk down the field -------------------------------------------------------------------------------------------------------------
// A serial chain of dependent loads per lane: an export path, not tuned.
__global__ void __launch_bounds__(64) k_travel_path(int n, const int *__restrict__ target, GridDims d, const unsigned long long *__restrict__ words,
                                                    const uint16_t *__restrict__ travel, int max_steps, int capacity, int *__restrict__ path3, int *__restrict__ len_out) {
    const int i = (int)threadIdx.x;
    if (i >= n) return;
    int x = target[3 * i], y = target[3 * i + 1], z = target[3 * i + 2], len = 0;
    auto in_domain = [&](int a, int b, int c) { return grid_inside(d, a, b, c) && grid_mask_bit(words, d, a, b, c); };
    unsigned here = grid_inside(d, x, y, z) ? (unsigned)travel[grid_voxel_of(d, x, y, z)] : (unsigned)XS_TRAVEL_NONE;
    if (here != (unsigned)XS_TRAVEL_NONE) {
        int *out = path3 + (size_t)i * (size_t)capacity * 3;
        for (int step = 0;; ++step) {
            if (len < capacity) { out[3 * (size_t)len] = x; out[3 * (size_t)len + 1] = y; out[3 * (size_t)len + 2] = z; }
            ++len;
            if (here == 0u || step >= max_steps) break;            // (the cap: a corrupt field cannot spin the loop)
            unsigned around = 0u;
            for (int k = 0; k < 27; ++k)
                if (in_domain(x + grid_dx(k), y + grid_dy(k), z + grid_dz(k))) around |= 1u << k;
            int take = -1;
            unsigned next = 0u;
            for (int k = 0; k < 27 && take < 0; ++k) {
                if (k == 13 || (around & travel_need(k)) != travel_need(k)) continue;
                const unsigned there = (unsigned)travel[grid_voxel_of(d, x + grid_dx(k), y + grid_dy(k), z + grid_dz(k))];
                if (there + (unsigned)travel_cost(k) == here) { take = k; next = there; }
            }
            if (take < 0) break;                                   // (not a fixpoint: no move explains the value)
            x += grid_dx(take); y += grid_dy(take); z += grid_dz(take);
            here = next;
        }
    }
    len_out[i] = len;
}

extern "C" int xs_travel_path(int n, const int *target3xN_dev, const int *res, const void *reach, const unsigned short *travel_dev, int limit, int capacity,
                              int *path3_dev, int *len_dev, void *stream) {
    GridDims d;
    if (!target3xN_dev || !reach || !travel_dev || !path3_dev || !len_dev) return xs_set_error(hipErrorInvalidValue, "xs_travel_path: null pointer");
    if (!grid_dims_launchable(res, d)) return xs_set_error(hipErrorInvalidValue, "xs_travel_path: bad resolution");
    if (n < 1 || n > XS_TRAVEL_MAX_TARGETS) return xs_set_error(hipErrorInvalidValue, "xs_travel_path: n outside 1 .. 64");
    if (limit < 0 || limit > XS_TRAVEL_MAX) return xs_set_error(hipErrorInvalidValue, "xs_travel_path: limit outside 0 .. XS_TRAVEL_MAX");
    if (capacity < 1) return xs_set_error(hipErrorInvalidValue, "xs_travel_path: capacity < 1");
    hipLaunchKernelGGL(k_travel_path, dim3(1), dim3(64), 0, (hipStream_t)stream, n, target3xN_dev, d, static_cast<const unsigned long long *>(reach), travel_dev,
                       limit / 3 + 2, capacity, path3_dev, len_dev);
    XS_CHECK(hipGetLastError());
    return 0;
}
