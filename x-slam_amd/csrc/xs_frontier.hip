// xs_frontier.hip — where known free space borders the unknown, and which of those voxels belong together: the frontier mask of the
// observation grid of xs_view.hip, its connected clusters and one record per cluster.  Integer arithmetic on the
// grid's two-bit states throughout: every result is a pure function of the inputs, two runs give equal bytes, and the only atomics are
// integer add / min / max, whose results do not depend on their order.
//
//   k_frontier_mask      lane = brick: the brick's FREE and UNKNOWN words from its 16-byte grid word (overhang bits cleared: padding is not a
//                        state), UNKNOWN grown by the six masked shifts of xs_grid.h plus the facing bits of the six neighbouring
//                        bricks' UNKNOWN words, ANDed with FREE.  One plain launch, no synchronisation.
//   k_frontier_seed      lane = voxel: labels[v] = v on a frontier voxel, NONE elsewhere
//   k_frontier_round     workgroup = a tile of 8 x 8 x 8 voxels (2 x 2 x 2 bricks), thread = voxel.  A tile whose eight mask words have no bit
//                        returns at once.  Otherwise the 10^3 labels of tile plus apron go to LDS (NONE outside the volume and across a
//                        cell boundary; a non-frontier voxel holds NONE already), every frontier thread takes the minimum over itself and
//                        its 26 neighbours until nothing in the tile changes, writes back its own label if it fell, and one thread stores
//                        1 to the round's `changed` word.  The apron is read from global memory every round: a stale label delays a
//                        merge by a round and never invents one.  Every barrier is reached by all 512 threads.
//   k_frontier_roots     lane = brick: the voxels whose label is their own index, compacted through an integer counter
//   k_frontier_accumulate  lane = brick: a voxel finds its record by binary search over the sorted roots; count and coordinate sums by
//                        64-bit integer atomic adds, the bounding box by 32-bit integer atomic min / max (runs of equal labels inside a
//                        brick are added up in registers first)
// (xs_frontier_expand, one byte per voxel, runs xs_reach.hip's k_reach_expand: the mask's words have the reached words' layout.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "xs_device.h"
#include "xs_grid.h"
#include "../../include/xslam_amd.h"

// the workspace begins with GRID_CONTROL_BYTES: the `changed` words of grid_run_rounds, and at FRONTIER_COUNTER_AT the root counter
enum { FRONTIER_COUNTER_AT = 64, FRONTIER_RECORD_WORDS = 8 };
static_assert(XS_FRONTIER_NONE == 0xFFFFFFFFu && XS_FRONTIER_RECORD_WORDS == FRONTIER_RECORD_WORDS, "the header's constants");
static_assert(GRID_ROUNDS_PER_BATCH * sizeof(unsigned) <= FRONTIER_COUNTER_AT && FRONTIER_COUNTER_AT + sizeof(unsigned) <= GRID_CONTROL_BYTES,
              "the root counter behind the changed words, inside the control bytes");

// the resolutions the frontier calls take: the launchable ones of xs_grid.h whose voxels a uint32 label can index, 0xFFFFFFFF kept free for NONE
static inline bool frontier_dims(const int *res, GridDims &d) { return grid_dims_launchable(res, d) && grid_voxels(d) < 0xFFFFFFFFull; }
static inline bool frontier_cell_ok(int cell) { return cell == 0 || (cell >= 8 && cell <= 65528 && cell % 8 == 0); }

extern "C" size_t xs_frontier_mask_bytes(const int *res) {
    GridDims d;
    return frontier_dims(res, d) ? grid_bricks(d) * sizeof(unsigned long long) : 0;
}
extern "C" size_t xs_frontier_label_bytes(const int *res) {
    GridDims d;
    return frontier_dims(res, d) ? grid_voxels(d) * sizeof(unsigned) : 0;
}
// the control words, then `capacity` roots (rounded up to 16 bytes), then six box words per record
static size_t frontier_box_at(int capacity) { return GRID_CONTROL_BYTES + ((size_t)capacity * sizeof(unsigned) + 15) / 16 * 16; }
extern "C" size_t xs_frontier_workspace_bytes(const int *res, int capacity) {
    GridDims d;
    if (!frontier_dims(res, d) || capacity < 0) return 0;
    return frontier_box_at(capacity) + (size_t)capacity * 6 * sizeof(unsigned);
}

// ---- the mask ----------------------------------------------------------------------------------------------------------------------------
// the even bits of a dword (one per two-bit state) as its low 16 bits
__device__ __forceinline__ unsigned frontier_even_bits(unsigned x) {
    x &= 0x55555555u;
    x = (x | x >> 1) & 0x33333333u;
    x = (x | x >> 2) & 0x0f0f0f0fu;
    x = (x | x >> 4) & 0x00ff00ffu;
    x = (x | x >> 8) & 0x0000ffffu;
    return x;
}
// plane lz of a grid word as 16 bits: the voxels whose state is UNKNOWN (0) / FREE (1)
static_assert(GRID_UNKNOWN == 0 && GRID_FREE == 1, "the bit tests below");
__device__ __forceinline__ unsigned frontier_unknown16(unsigned plane) { return frontier_even_bits(~(plane | plane >> 1)); }
__device__ __forceinline__ unsigned frontier_free16(unsigned plane) { return frontier_even_bits(plane & ~(plane >> 1)); }
__device__ __forceinline__ unsigned long long frontier_unknown64(const uint4 w) {
    return (unsigned long long)frontier_unknown16(w.x) | (unsigned long long)frontier_unknown16(w.y) << 16 | (unsigned long long)frontier_unknown16(w.z) << 32 |
           (unsigned long long)frontier_unknown16(w.w) << 48;
}
__device__ __forceinline__ unsigned long long frontier_free64(const uint4 w) {
    return (unsigned long long)frontier_free16(w.x) | (unsigned long long)frontier_free16(w.y) << 16 | (unsigned long long)frontier_free16(w.z) << 32 |
           (unsigned long long)frontier_free16(w.w) << 48;
}
// the bits of brick (bx, by, bz) that stand for voxels inside the volume
__device__ __forceinline__ unsigned long long frontier_inside64(const GridDims &d, int bx, int by, int bz) {
    const int kx = min(4, d.X - 4 * bx), ky = min(4, d.Y - 4 * by), kz = min(4, d.Z - 4 * bz);
    const unsigned long long vx = GRID_X0 * ((1ull << kx) - 1ull);
    const unsigned long long vy = 0x0001000100010001ull * ((1ull << (4 * ky)) - 1ull);
    const unsigned long long vz = kz == 4 ? ~0ull : (1ull << (16 * kz)) - 1ull;
    return vx & vy & vz;
}

__global__ void __launch_bounds__(256) k_frontier_mask(const uint4 *__restrict__ grid, GridDims d, unsigned nbricks, unsigned long long *__restrict__ mask) {
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nbricks) return;
    int bx, by, bz;
    grid_brick_of(d, b, bx, by, bz);
    const unsigned sy = (unsigned)d.BX, sz = (unsigned)d.BX * (unsigned)d.BY;
    const uint4 own = grid[b];
    // A neighbouring brick shares two of this brick's three coordinates, so it overhangs the volume on those axes exactly as this one does,
    // and its facing plane is inside the volume on the third: the AND with `inside` below clears every padding bit it brings.
    const unsigned long long inside = frontier_inside64(d, bx, by, bz);
    const unsigned long long f = frontier_free64(own) & inside;
    if (f == 0ull) { mask[b] = 0ull; return; }
    const unsigned long long u = frontier_unknown64(own) & inside;
    // of the bricks below and above only the facing plane is read and converted: its plane 3 below this brick's plane 0, its plane 0 above
    // this brick's plane 3, each put where grid_neighbours_across looks for it
    const unsigned long long across = grid_neighbours_across(
        bx > 0 ? frontier_unknown64(grid[b - 1u]) : 0ull, bx + 1 < d.BX ? frontier_unknown64(grid[b + 1u]) : 0ull,
        by > 0 ? frontier_unknown64(grid[b - sy]) : 0ull, by + 1 < d.BY ? frontier_unknown64(grid[b + sy]) : 0ull,
        bz > 0 ? (unsigned long long)frontier_unknown16(grid[b - sz].w) << 48 : 0ull, bz + 1 < d.BZ ? (unsigned long long)frontier_unknown16(grid[b + sz].x) : 0ull);
    mask[b] = (grid_neighbours(u) | across) & f;
}

extern "C" int xs_frontier_mask(const void *grid, const int *res, void *mask, void *stream) {
    GridDims d;
    if (!grid || !mask) return xs_set_error(hipErrorInvalidValue, "xs_frontier_mask: null pointer");
    if (!frontier_dims(res, d)) return xs_set_error(hipErrorInvalidValue, "xs_frontier_mask: bad resolution");
    const unsigned nbricks = (unsigned)grid_bricks(d);
    hipLaunchKernelGGL(k_frontier_mask, dim3((nbricks + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, static_cast<const uint4 *>(grid), d, nbricks,
                       static_cast<unsigned long long *>(mask));
    XS_CHECK(hipGetLastError());
    return 0;
}

// the mask's words have the layout of the reach buffer's reached words: xs_reach.hip's kernel expands them
extern "C" int xs_frontier_expand(const void *mask, const int *res, unsigned char *out_dev, void *stream) {
    GridDims d;
    if (!mask || !out_dev) return xs_set_error(hipErrorInvalidValue, "xs_frontier_expand: null pointer");
    if (!frontier_dims(res, d)) return xs_set_error(hipErrorInvalidValue, "xs_frontier_expand: bad resolution");
    return xs_reach_expand(mask, res, 0, out_dev, stream);
}

// ---- the labels --------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(GRID_VOXEL_THREADS) k_frontier_seed(const unsigned long long *__restrict__ words, GridDims d, unsigned *__restrict__ labels) {
    int x, y, z;
    if (!grid_voxel_of_thread(d, x, y, z)) return;
    const size_t v = grid_voxel_of(d, x, y, z);
    labels[v] = grid_mask_bit(words, d, x, y, z) ? (unsigned)v : (unsigned)XS_FRONTIER_NONE;
}

__global__ void __launch_bounds__(GRID_TILE_THREADS) k_frontier_round(unsigned *labels, const unsigned long long *__restrict__ words, GridDims d, int cell,
                                                                       unsigned *changed) {
    __shared__ unsigned lab[GRID_TILE_CELLS];                      // the labels of tile plus apron
    const int t = (int)threadIdx.x;
    const int tx = (int)blockIdx.x, ty = (int)blockIdx.y, tz = (int)blockIdx.z;
    // the tile's own eight bricks, one per lane t < 8
    bool any = false;
    if (t < 8) {
        const int bx = 2 * tx + (t & 1), by = 2 * ty + (t >> 1 & 1), bz = 2 * tz + (t >> 2);
        if (bx < d.BX && by < d.BY && bz < d.BZ) any = words[grid_brick_at(d, bx, by, bz)] != 0ull;
    }
    if (!__syncthreads_or(any)) return;                            // (block-uniform)
    // 8 divides cell, so the tile lies in one cell; a face of the apron is across a cell boundary iff the tile touches that boundary
    const int x0 = GRID_TILE * tx - 1, y0 = GRID_TILE * ty - 1, z0 = GRID_TILE * tz - 1;
    const bool cut_x0 = cell && (x0 + 1) % cell == 0, cut_x1 = cell && (x0 + 1 + GRID_TILE) % cell == 0;
    const bool cut_y0 = cell && (y0 + 1) % cell == 0, cut_y1 = cell && (y0 + 1 + GRID_TILE) % cell == 0;
    const bool cut_z0 = cell && (z0 + 1) % cell == 0, cut_z1 = cell && (z0 + 1 + GRID_TILE) % cell == 0;
    for (int c = t; c < GRID_TILE_CELLS; c += GRID_TILE_THREADS) {
        int px, py, pz;
        grid_tile_cell_of(c, px, py, pz);
        const int x = x0 + px, y = y0 + py, z = z0 + pz;
        const bool across = (px == 0 && cut_x0) || (px == GRID_TILE_SIDE - 1 && cut_x1) || (py == 0 && cut_y0) || (py == GRID_TILE_SIDE - 1 && cut_y1) ||
                            (pz == 0 && cut_z0) || (pz == GRID_TILE_SIDE - 1 && cut_z1);
        unsigned v = (unsigned)XS_FRONTIER_NONE;
        if (!across && grid_inside(d, x, y, z)) v = labels[grid_voxel_of(d, x, y, z)];
        lab[c] = v;
    }
    __syncthreads();
    const int lx = t & 7, ly = t >> 3 & 7, lz = t >> 6;
    const int here = grid_tile_cell_of_thread(t);
    const unsigned first = lab[here];
    const bool frontier = first != (unsigned)XS_FRONTIER_NONE;     // (a voxel outside the volume was staged as NONE)
    unsigned mine = first;
    for (;;) {
        unsigned best = mine;
        if (frontier) {
#pragma unroll
            for (int k = 0; k < 27; ++k)
                best = min(best, lab[here + grid_tile_step(k)]);   // (NONE is the largest value)
        }
        const bool fell = best < mine;
        if (fell) { mine = best; lab[here] = best; }               // in place: labels only fall, each is the index of a voxel of this cluster
        if (!__syncthreads_or(fell)) break;                        // (block-uniform)
    }
    const bool fell = mine < first;
    if (fell) labels[grid_voxel_of(d, x0 + 1 + lx, y0 + 1 + ly, z0 + 1 + lz)] = mine;   // (a frontier voxel, so inside the volume)
    if (__syncthreads_or(fell) && t == 0) *changed = 1u;
}

extern "C" int xs_frontier_label(const void *mask, const int *res, int cell, unsigned *labels_dev, void *workspace, int *rounds_out, void *stream) {
    GridDims d;
    if (!mask || !labels_dev || !workspace) return xs_set_error(hipErrorInvalidValue, "xs_frontier_label: null pointer");
    if (!frontier_dims(res, d)) return xs_set_error(hipErrorInvalidValue, "xs_frontier_label: bad resolution");
    if (!frontier_cell_ok(cell)) return xs_set_error(hipErrorInvalidValue, "xs_frontier_label: cell is 0 or a multiple of 8 in 8 .. 65528");
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long *words = static_cast<const unsigned long long *>(mask);
    unsigned *changed = static_cast<unsigned *>(workspace);
    hipLaunchKernelGGL(k_frontier_seed, grid_voxel_blocks(d), dim3(GRID_VOXEL_THREADS), 0, st, words, d, labels_dev);
    XS_CHECK(hipGetLastError());
    // every changing round lowers at least one of finitely many non-negative integers
    return grid_run_rounds(changed, st, rounds_out, [&](unsigned *changed_k) {
        hipLaunchKernelGGL(k_frontier_round, grid_tile_blocks(d), dim3(GRID_TILE_THREADS), 0, st, labels_dev, words, d, cell, changed_k);
    });
}

// ---- the cluster records -----------------------------------------------------------------------------------------------------------------
// (the voxel of a set bit, grid_voxel_of_bit, is inside the volume where the mask's overhang bits are clear, as xs_frontier_mask leaves them)
__global__ void __launch_bounds__(256) k_frontier_roots(const unsigned long long *__restrict__ words, const unsigned *__restrict__ labels, GridDims d,
                                                        unsigned nbricks, unsigned capacity, unsigned *__restrict__ roots, unsigned *counter) {
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nbricks) return;
    unsigned long long w = words[b];
    if (w == 0ull) return;
    int bx, by, bz;
    grid_brick_of(d, b, bx, by, bz);
    while (w) {
        const int bit = __ffsll((long long)w) - 1;
        w &= w - 1ull;
        int x, y, z;
        grid_voxel_of_bit(bx, by, bz, bit, x, y, z);
        if (!grid_inside(d, x, y, z)) continue;                   // (a mask from elsewhere with overhang bits set: nothing is read out of bounds)
        const unsigned v = (unsigned)grid_voxel_of(d, x, y, z);
        if (labels[v] != v) continue;
        const unsigned i = atomicAdd(counter, 1u);                 // (the slot is arbitrary: the host sorts the list)
        if (i < capacity) roots[i] = v;
    }
}

__global__ void __launch_bounds__(256) k_frontier_records_init(unsigned n, const unsigned *__restrict__ roots, unsigned long long *__restrict__ records,
                                                               unsigned *__restrict__ box) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    unsigned long long *r = records + (size_t)i * FRONTIER_RECORD_WORDS;
    r[0] = roots[i];
#pragma unroll
    for (int k = 1; k < FRONTIER_RECORD_WORDS; ++k) r[k] = 0ull;
    unsigned *q = box + (size_t)i * 6;
    q[0] = q[1] = q[2] = 0xFFFFFFFFu;
    q[3] = q[4] = q[5] = 0u;
}

struct FrontierRun { unsigned label, count, sx, sy, sz, x0, y0, z0, x1, y1, z1; };   // at most 64 voxels of one brick: 32 bits hold every sum

__device__ __forceinline__ void frontier_flush(const FrontierRun &r, unsigned n, const unsigned *__restrict__ roots, unsigned long long *records, unsigned *box) {
    unsigned lo = 0u, hi = n;                                      // the record of the label: the first root that is not below it
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2u;
        if (roots[mid] < r.label) lo = mid + 1u; else hi = mid;
    }
    if (lo >= n || roots[lo] != r.label) return;                   // (labels that are no fixpoint: nothing is added anywhere)
    unsigned long long *rec = records + (size_t)lo * FRONTIER_RECORD_WORDS;
    atomicAdd(rec + 1, (unsigned long long)r.count);
    atomicAdd(rec + 2, (unsigned long long)r.sx);
    atomicAdd(rec + 3, (unsigned long long)r.sy);
    atomicAdd(rec + 4, (unsigned long long)r.sz);
    unsigned *q = box + (size_t)lo * 6;
    atomicMin(q + 0, r.x0); atomicMin(q + 1, r.y0); atomicMin(q + 2, r.z0);
    atomicMax(q + 3, r.x1); atomicMax(q + 4, r.y1); atomicMax(q + 5, r.z1);
}

__global__ void __launch_bounds__(256) k_frontier_accumulate(const unsigned long long *__restrict__ words, const unsigned *__restrict__ labels, GridDims d,
                                                             unsigned nbricks, unsigned n, const unsigned *__restrict__ roots, unsigned long long *records,
                                                             unsigned *box) {
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nbricks) return;
    unsigned long long w = words[b];
    if (w == 0ull) return;
    int bx, by, bz;
    grid_brick_of(d, b, bx, by, bz);
    FrontierRun r;
    r.count = 0u;
    while (w) {
        const int bit = __ffsll((long long)w) - 1;
        w &= w - 1ull;
        int x, y, z;
        grid_voxel_of_bit(bx, by, bz, bit, x, y, z);
        if (!grid_inside(d, x, y, z)) continue;
        const unsigned l = labels[grid_voxel_of(d, x, y, z)];
        if (r.count && l != r.label) { frontier_flush(r, n, roots, records, box); r.count = 0u; }
        if (r.count == 0u) {
            r.label = l; r.count = 1u;
            r.sx = r.x0 = r.x1 = (unsigned)x; r.sy = r.y0 = r.y1 = (unsigned)y; r.sz = r.z0 = r.z1 = (unsigned)z;
        } else {
            ++r.count;
            r.sx += (unsigned)x; r.sy += (unsigned)y; r.sz += (unsigned)z;
            r.x0 = min(r.x0, (unsigned)x); r.y0 = min(r.y0, (unsigned)y); r.z0 = min(r.z0, (unsigned)z);
            r.x1 = max(r.x1, (unsigned)x); r.y1 = max(r.y1, (unsigned)y); r.z1 = max(r.z1, (unsigned)z);
        }
    }
    if (r.count) frontier_flush(r, n, roots, records, box);
}

__global__ void __launch_bounds__(256) k_frontier_records_finish(unsigned n, const unsigned *__restrict__ box, unsigned long long *__restrict__ records) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const unsigned *q = box + (size_t)i * 6;
    unsigned long long *r = records + (size_t)i * FRONTIER_RECORD_WORDS;
    r[5] = (unsigned long long)q[0] | (unsigned long long)q[1] << 16 | (unsigned long long)q[2] << 32;
    r[6] = (unsigned long long)q[3] | (unsigned long long)q[4] << 16 | (unsigned long long)q[5] << 32;
}

extern "C" int xs_frontier_clusters(const void *mask, const unsigned *labels_dev, const int *res, int capacity, unsigned long long *records_dev,
                                    unsigned *count_dev, unsigned *count_host, void *workspace, void *stream) {
    GridDims d;
    if (!mask || !labels_dev || !records_dev || !count_dev || !workspace) return xs_set_error(hipErrorInvalidValue, "xs_frontier_clusters: null pointer");
    if (!frontier_dims(res, d)) return xs_set_error(hipErrorInvalidValue, "xs_frontier_clusters: bad resolution");
    if (capacity < 1) return xs_set_error(hipErrorInvalidValue, "xs_frontier_clusters: capacity < 1");
    if (d.X > 65535) return xs_set_error(hipErrorInvalidValue, "xs_frontier_clusters: X above 65535 does not fit a record's packed box");
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long *words = static_cast<const unsigned long long *>(mask);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    unsigned *counter = reinterpret_cast<unsigned *>(ws + FRONTIER_COUNTER_AT), *roots = reinterpret_cast<unsigned *>(ws + GRID_CONTROL_BYTES);
    unsigned *box = reinterpret_cast<unsigned *>(ws + frontier_box_at(capacity));
    const unsigned nbricks = (unsigned)grid_bricks(d);
    const dim3 over_bricks((nbricks + 255u) / 256u);
    XS_CHECK(hipMemsetAsync(counter, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_frontier_roots, over_bricks, dim3(256), 0, st, words, labels_dev, d, nbricks, (unsigned)capacity, roots, counter);
    XS_CHECK(hipGetLastError());
    unsigned n = 0;
    XS_CHECK(hipMemcpyAsync(count_dev, counter, sizeof(unsigned), hipMemcpyDeviceToDevice, st));
    XS_CHECK(hipMemcpyAsync(&n, counter, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    XS_CHECK(hipStreamSynchronize(st));
    if (count_host) *count_host = n;
    if (n == 0u || n > (unsigned)capacity) return 0;               // (the caller retries with n records)
    // the roots in ascending order: a record's place must not depend on which lane's atomic came first
    std::vector<unsigned> sorted(n);
    XS_CHECK(hipMemcpyAsync(sorted.data(), roots, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    XS_CHECK(hipStreamSynchronize(st));
    std::sort(sorted.begin(), sorted.end());
    XS_CHECK(hipMemcpyAsync(roots, sorted.data(), (size_t)n * sizeof(unsigned), hipMemcpyHostToDevice, st));
    const dim3 over_records((n + 255u) / 256u);
    hipLaunchKernelGGL(k_frontier_records_init, over_records, dim3(256), 0, st, n, roots, records_dev, box);
    XS_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_frontier_accumulate, over_bricks, dim3(256), 0, st, words, labels_dev, d, nbricks, n, roots, records_dev, box);
    XS_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_frontier_records_finish, over_records, dim3(256), 0, st, n, box, records_dev);
    XS_CHECK(hipGetLastError());
    XS_CHECK(hipStreamSynchronize(st));                            // (`sorted` is the source of a copy until here)
    return 0;
}
