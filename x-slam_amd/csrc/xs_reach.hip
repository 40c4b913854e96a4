// xs_reach.hip — how far the nearest obstacle is, and where a body of a given radius can get to, from the observation grid of xs_view.hip
// (DESIGN.md section 4.19).  Everything here is integer arithmetic on the grid's two-bit states: every result is a pure function of the
// inputs, two runs give equal bytes, and there is no floating-point atomic.
//
// CLEARANCE FIELD  field[(z Y + y) X + x] = min(d^2, R^2), uint16: d^2 the least squared integer distance from the voxel to an obstacle
// voxel (OCCUPIED; with unknown_blocks also UNKNOWN and every position outside the volume).  Three separable passes, each a plain launch:
//   k_clear_x      block = a strip of 256 voxels of the four rows (ly) of one brick row at one z.  The rows' obstacle bits, with an apron of
//                  256 bits on either side, are put into LDS as 32-bit masks (one dword of a brick word holds the plane's 4 x 4 states);
//                  a lane finds the nearest set bit to its left and right by clz / ctz over at most nine words a side.  One byte per
//                  voxel: the distance along x, 255 = none within R.
//   k_clear_axis   the windowed minimum of f(j) + (j - i)^2 over |j - i| <= R along y (from the bytes, squared; to uint16 saturated at
//                  65535, which any value above R^2 may be replaced by) and then along z (to the field, capped at R^2).  Block = 64 lanes
//                  along x times four row groups; a tile of T output rows with its R-row aprons sits in LDS ((T + 2R) x 64 elements,
//                  static: 24 KiB of uint16 up to R = 64 with T = 64, 80 KiB up to R = 255 with T = 128), long axes are cut into strips
//                  of T.  Positions outside the volume are not stored: with unknown_blocks the nearest of them along the pass's axis
//                  is (i + 1) or (L - i) away.
// REACHABILITY  one 64-bit mask per brick (bit lx + 4 ly + 16 lz) of the passable voxels (FREE and field >= r2) and one of the reached ones:
//   k_reach_passable   wave = brick, lane = voxel, the mask by ballot
//   k_reach_seed       one lane: the seeds that are inside the volume and passable
//   k_reach_round      lane = brick word: grows the word to its in-brick fixpoint by masked shifts, pulls the facing bits of the six
//                      neighbouring words, grows again, writes its own word and, if it grew, a `changed` word (a plain vector store).
//                      Words only gain bits, a stale read of a neighbour delays a bit and never invents one, the fixpoint is unique.
//                      The host runs the rounds through xs_grid.h's grid_run_rounds.
//   k_reach_expand     one byte per voxel
//   k_reach_query      lane = point: the voxel of the point, its bit, and with snap > 0 the nearest voxel of the mask in the snap cube
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xs_device.h"
#include "xs_grid.h"
#include "../../include/xslam_amd.h"

enum { CLEAR_STRIP = 256, CLEAR_APRON = 256, CLEAR_WORDS = (CLEAR_STRIP + 2 * CLEAR_APRON) / 32, CLEAR_NONE8 = 255, CLEAR_NONE16 = 65535 };
static_assert(XS_REACH_MAX_SEEDS == 64 && XS_REACH_MAX_SNAP == 16 && XS_CLEARANCE_MAX_RADIUS == 255, "the header's bounds");

// ---- clearance ---------------------------------------------------------------------------------------------------------------------------
extern "C" size_t xs_clearance_bytes(const int *res) {
    GridDims d;
    return grid_dims_launchable(res, d) ? grid_voxels(d) * sizeof(uint16_t) : 0;
}
// the bytes of k_clear_x (rounded up to 256), then the uint16 of the y pass
static size_t clear_ws_split(const GridDims &d) { return (grid_voxels(d) + 255) / 256 * 256; }
extern "C" size_t xs_clearance_workspace_bytes(const int *res) {
    GridDims d;
    return grid_dims_launchable(res, d) ? clear_ws_split(d) + grid_voxels(d) * sizeof(uint16_t) : 0;
}

__global__ void __launch_bounds__(CLEAR_STRIP) k_clear_x(const unsigned *__restrict__ grid, GridDims d, int R, int unknown_blocks, unsigned char *__restrict__ dist) {
    __shared__ unsigned bits[4][CLEAR_WORDS];
    const int t = threadIdx.x, x0 = (int)blockIdx.x * CLEAR_STRIP, by = (int)blockIdx.y, z = (int)blockIdx.z;
    if (t < 4 * CLEAR_WORDS) bits[t / CLEAR_WORDS][t % CLEAR_WORDS] = 0u;
    __syncthreads();
    // bit q of a row's masks stands for x = x0 - CLEAR_APRON + q; thread t < 192 brings the brick that holds bits 4 t .. 4 t + 3 (x0 and
    // the apron are multiples of four, so a brick never straddles two threads)
    if (t < (CLEAR_STRIP + 2 * CLEAR_APRON) / 4) {
        const int bx = (x0 - CLEAR_APRON) / 4 + t;                 // (exact: the numerator is a multiple of four, negative or not)
        if (bx >= 0 && bx < d.BX) {
            const unsigned plane = grid[4 * grid_brick_at(d, bx, by, z >> 2) + (size_t)(z & 3)];   // dword lz of the brick word: the 4 x 4 states of plane z
#pragma unroll
            for (int ly = 0; ly < 4; ++ly) {
                unsigned nib = 0;
#pragma unroll
                for (int lx = 0; lx < 4; ++lx) {
                    const unsigned s = grid_plane_state_of(plane, lx, ly);
                    const bool inside = 4 * bx + lx < d.X;         // the padding bits of an overhanging brick are not a state
                    if (inside && (s == GRID_OCCUPIED || (unknown_blocks && s == GRID_UNKNOWN))) nib |= 1u << lx;
                }
                if (nib) atomicOr(&bits[ly][t >> 3], nib << (4 * (t & 7)));
            }
        }
    }
    __syncthreads();
    const int x = x0 + t;
    if (x >= d.X) return;
    const int q = CLEAR_APRON + t, wq = q >> 5, bq = q & 31, nw = (R + 31) / 32 + 1;
#pragma unroll
    for (int ly = 0; ly < 4; ++ly) {
        const int y = 4 * by + ly;
        if (y >= d.Y) break;
        const unsigned *m = bits[ly];
        int best = CLEAR_NONE8;
        // to the left: the highest set bit at or below q
        unsigned w = m[wq] & (0xffffffffu >> (31 - bq));
        for (int k = 0; k < nw; ++k) {
            if (w) { best = q - (32 * (wq - k) + 31 - __clz((int)w)); break; }
            if (wq - k - 1 < 0) break;
            w = m[wq - k - 1];
        }
        // to the right: the lowest set bit above q
        w = bq == 31 ? 0u : m[wq] & (0xffffffffu << (bq + 1));
        for (int k = 0; k < nw; ++k) {
            if (w) { best = min(best, 32 * (wq + k) + (__ffs((int)w) - 1) - q); break; }
            if (wq + k + 1 >= CLEAR_WORDS) break;
            w = m[wq + k + 1];
        }
        if (unknown_blocks) best = min(best, min(x + 1, d.X - x));   // the nearest position outside the volume along x
        if (best > R) best = CLEAR_NONE8;
        dist[grid_voxel_of(d, x, y, z)] = (unsigned char)best;
    }
}

// One pass along an axis of length L whose elements are `stride` apart; `other` (blockIdx.z) runs over the third axis, `ostride` apart.
// In = unsigned char: the x pass's distances, squared here.  cap: what the result saturates at.  ROWS: the tile's rows in LDS, static
// (192 rows for R <= 64 with T = 64, 640 rows — 80 KiB of uint16 — for R <= 255 with T = 128).
template <typename In, int ROWS>
__global__ void __launch_bounds__(256) k_clear_axis(const In *__restrict__ in, uint16_t *__restrict__ out, int X, int L, size_t stride, size_t ostride,
                                                    int R, int T, int unknown_blocks, unsigned cap) {
    __shared__ In tile[ROWS * 64];                                 // [T + 2 R <= ROWS][64]
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int x = (int)blockIdx.x * 64 + lane, i0 = (int)blockIdx.y * T;
    const int lo = max(i0 - R, 0), hi = min(i0 + T + R, L);        // the rows of the axis the tile holds: [lo, hi)
    const size_t base = (size_t)blockIdx.z * ostride + (size_t)x;
    if (x < X)
        for (int j = lo + grp; j < hi; j += 4) tile[(j - lo) * 64 + lane] = in[base + (size_t)j * stride];
    __syncthreads();
    if (x >= X) return;
    const int iend = min(i0 + T, L);
    for (int i = i0 + grp; i < iend; i += 4) {
        unsigned best = 0x7fffffffu;                               // "none": above 3 * 255^2
        const int j0 = max(i - R, lo), j1 = min(i + R, hi - 1);
        for (int j = j0; j <= j1; ++j) {
            unsigned f = (unsigned)tile[(j - lo) * 64 + lane];
            if (sizeof(In) == 1) f *= f;
            const int dj = j - i;
            best = min(best, f + (unsigned)(dj * dj));
        }
        if (unknown_blocks) {
            const unsigned a = (unsigned)(i + 1), b = (unsigned)(L - i);
            best = min(best, min(a * a, b * b));
        }
        out[base + (size_t)i * stride] = (uint16_t)min(best, cap);
    }
}

static int clear_tile_rows(int R) { return R <= 64 ? 64 : 128; }

extern "C" int xs_clearance_build(const void *grid, const int *res, int max_radius, int unknown_blocks, void *workspace, unsigned short *field_dev, void *stream) {
    GridDims d;
    if (!grid || !workspace || !field_dev) return xs_set_error(hipErrorInvalidValue, "xs_clearance_build: null pointer");
    if (!grid_dims_launchable(res, d)) return xs_set_error(hipErrorInvalidValue, "xs_clearance_build: bad resolution");
    if (max_radius < 1 || max_radius > XS_CLEARANCE_MAX_RADIUS) return xs_set_error(hipErrorInvalidValue, "xs_clearance_build: max_radius outside 1 .. 255");
    if (unknown_blocks != 0 && unknown_blocks != 1) return xs_set_error(hipErrorInvalidValue, "xs_clearance_build: unknown_blocks is 0 or 1");
    hipStream_t st = (hipStream_t)stream;
    const int R = max_radius, T = clear_tile_rows(R);
    unsigned char *dx = static_cast<unsigned char *>(workspace);
    uint16_t *dxy = reinterpret_cast<uint16_t *>(dx + clear_ws_split(d));
    hipLaunchKernelGGL(k_clear_x, dim3(((unsigned)d.X + CLEAR_STRIP - 1) / CLEAR_STRIP, (unsigned)d.BY, (unsigned)d.Z), dim3(CLEAR_STRIP), 0, st,
                       static_cast<const unsigned *>(grid), d, R, unknown_blocks, dx);
    XS_CHECK(hipGetLastError());
    const unsigned bxs = ((unsigned)d.X + 63u) / 64u;
    const size_t plane = (size_t)d.X * (size_t)d.Y;
    const dim3 gy(bxs, (unsigned)((d.Y + T - 1) / T), (unsigned)d.Z), gz(bxs, (unsigned)((d.Z + T - 1) / T), (unsigned)d.Y);
    if (R <= 64) {
        hipLaunchKernelGGL((k_clear_axis<unsigned char, 192>), gy, dim3(256), 0, st, dx, dxy, d.X, d.Y, (size_t)d.X, plane, R, T, unknown_blocks, (unsigned)CLEAR_NONE16);
        XS_CHECK(hipGetLastError());
        hipLaunchKernelGGL((k_clear_axis<uint16_t, 192>), gz, dim3(256), 0, st, dxy, field_dev, d.X, d.Z, plane, (size_t)d.X, R, T, unknown_blocks, (unsigned)(R * R));
    } else {
        hipLaunchKernelGGL((k_clear_axis<unsigned char, 640>), gy, dim3(256), 0, st, dx, dxy, d.X, d.Y, (size_t)d.X, plane, R, T, unknown_blocks, (unsigned)CLEAR_NONE16);
        XS_CHECK(hipGetLastError());
        hipLaunchKernelGGL((k_clear_axis<uint16_t, 640>), gz, dim3(256), 0, st, dxy, field_dev, d.X, d.Z, plane, (size_t)d.X, R, T, unknown_blocks, (unsigned)(R * R));
    }
    XS_CHECK(hipGetLastError());
    return 0;
}

// ---- reachability ------------------------------------------------------------------------------------------------------------------------
// The reach buffer: the reached words, the passable words, then GRID_CONTROL_BYTES of `changed` words (grid_run_rounds).
static inline unsigned long long *reach_passable_of(void *reach, size_t nbricks) { return static_cast<unsigned long long *>(reach) + nbricks; }
extern "C" size_t xs_reach_bytes(const int *res) {
    GridDims d;
    return grid_dims_launchable(res, d) ? grid_bricks(d) * 16 + GRID_CONTROL_BYTES : 0;
}

__global__ void __launch_bounds__(256) k_reach_passable(const uint4 *__restrict__ grid, const uint16_t *__restrict__ field, GridDims d, unsigned r2,
                                                        unsigned nbricks, unsigned long long *__restrict__ passable) {
    const unsigned b = blockIdx.x * 4u + (threadIdx.x >> 6);       // wave = brick
    if (b >= nbricks) return;
    const int l = threadIdx.x & 63;                                // lane = the voxel's bit
    int bx, by, bz, x, y, z;
    grid_brick_of(d, b, bx, by, bz);
    grid_voxel_of_bit(bx, by, bz, l, x, y, z);
    bool pass = false;
    if (x < d.X && y < d.Y && z < d.Z) pass = grid_state_of(grid[b], x, y, z) == GRID_FREE && (unsigned)field[grid_voxel_of(d, x, y, z)] >= r2;
    const unsigned long long m = __ballot(pass);
    if (l == 0) passable[b] = m;
}

__global__ void k_reach_seed(GridSeeds s, GridDims d, const unsigned long long *__restrict__ passable, unsigned long long *__restrict__ reach) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int k = 0; k < s.n; ++k) {
        const int x = s.v[3 * k], y = s.v[3 * k + 1], z = s.v[3 * k + 2];
        if (!grid_inside(d, x, y, z)) continue;
        const size_t b = grid_word_of(d, x, y, z);
        const unsigned long long bit = 1ull << grid_bit_of(x, y, z);
        if (passable[b] & bit) reach[b] |= bit;
    }
}

// the word's in-brick fixpoint: the face neighbours of set bits that are passable, until nothing is added (at most 9 steps across a brick,
// more along a winding passage inside it)
__device__ __forceinline__ unsigned long long reach_grow(unsigned long long m, unsigned long long p) {
    for (;;) {
        const unsigned long long g = (m | grid_neighbours(m)) & p;
        if (g == m) return m;
        m = g;
    }
}

__global__ void __launch_bounds__(256) k_reach_round(unsigned long long *reach, const unsigned long long *__restrict__ passable, GridDims d, unsigned nbricks,
                                                     unsigned *changed) {
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nbricks) return;
    const unsigned long long p = passable[b];
    if (p == 0ull) return;
    int bx, by, bz;
    grid_brick_of(d, b, bx, by, bz);
    const unsigned sy = (unsigned)d.BX, sz = (unsigned)d.BX * (unsigned)d.BY;
    const unsigned long long old = reach[b];
    unsigned long long m = reach_grow(old, p);
    // (the neighbours' words as other lanes and workgroups leave them, this round or the last: see the file header)
    const unsigned long long in = grid_neighbours_across(bx > 0 ? reach[b - 1u] : 0ull, bx + 1 < d.BX ? reach[b + 1u] : 0ull, by > 0 ? reach[b - sy] : 0ull,
                                                         by + 1 < d.BY ? reach[b + sy] : 0ull, bz > 0 ? reach[b - sz] : 0ull, bz + 1 < d.BZ ? reach[b + sz] : 0ull);
    m = reach_grow(m | (in & p), p);
    if (m != old) { reach[b] = m; *changed = 1u; }
}

__global__ void __launch_bounds__(GRID_VOXEL_THREADS) k_reach_expand(const unsigned long long *__restrict__ words, GridDims d, unsigned char *__restrict__ out) {
    int x, y, z;
    if (!grid_voxel_of_thread(d, x, y, z)) return;
    out[grid_voxel_of(d, x, y, z)] = (unsigned char)grid_mask_bit(words, d, x, y, z);
}

static int reach_passable_launch(const void *grid, const unsigned short *field, const GridDims &d, int r2, void *reach, hipStream_t st) {
    const unsigned nbricks = (unsigned)grid_bricks(d);
    hipLaunchKernelGGL(k_reach_passable, dim3((nbricks + 3u) / 4u), dim3(256), 0, st, static_cast<const uint4 *>(grid), field, d, (unsigned)r2, nbricks,
                       reach_passable_of(reach, nbricks));
    XS_CHECK(hipGetLastError());
    return 0;
}

extern "C" int xs_reach_passable(const void *grid, const unsigned short *field_dev, const int *res, int r2, void *reach, void *stream) {
    GridDims d;
    if (!grid || !field_dev || !reach) return xs_set_error(hipErrorInvalidValue, "xs_reach_passable: null pointer");
    if (!grid_dims_launchable(res, d)) return xs_set_error(hipErrorInvalidValue, "xs_reach_passable: bad resolution");
    if (r2 < 1 || r2 > 65025) return xs_set_error(hipErrorInvalidValue, "xs_reach_passable: r2 outside 1 .. 255^2");
    return reach_passable_launch(grid, field_dev, d, r2, reach, (hipStream_t)stream);
}

extern "C" int xs_reach_flood(const void *grid, const unsigned short *field_dev, const int *res, int r2, const int *seeds3xN, int seeds, void *reach,
                              int *rounds_out, void *stream) {
    GridDims d;
    if (!grid || !field_dev || !reach || !seeds3xN) return xs_set_error(hipErrorInvalidValue, "xs_reach_flood: null pointer");
    if (!grid_dims_launchable(res, d)) return xs_set_error(hipErrorInvalidValue, "xs_reach_flood: bad resolution");
    if (seeds < 1 || seeds > XS_REACH_MAX_SEEDS) return xs_set_error(hipErrorInvalidValue, "xs_reach_flood: seeds outside 1 .. XS_REACH_MAX_SEEDS");
    if (r2 < 1 || r2 > 65025) return xs_set_error(hipErrorInvalidValue, "xs_reach_flood: r2 outside 1 .. 255^2");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nbricks = (unsigned)grid_bricks(d);
    unsigned long long *words = static_cast<unsigned long long *>(reach), *passable = reach_passable_of(reach, nbricks);
    unsigned *changed = reinterpret_cast<unsigned *>(passable + nbricks);
    if (int rc = reach_passable_launch(grid, field_dev, d, r2, reach, st)) return rc;
    XS_CHECK(hipMemsetAsync(words, 0, (size_t)nbricks * 8, st));
    hipLaunchKernelGGL(k_reach_seed, dim3(1), dim3(64), 0, st, grid_seeds(seeds3xN, seeds), d, passable, words);
    XS_CHECK(hipGetLastError());
    // every changing round sets at least one of finitely many bits
    return grid_run_rounds(changed, st, rounds_out, [&](unsigned *changed_k) {
        hipLaunchKernelGGL(k_reach_round, dim3((nbricks + 255u) / 256u), dim3(256), 0, st, words, passable, d, nbricks, changed_k);
    });
}

extern "C" int xs_reach_expand(const void *reach, const int *res, int passable, unsigned char *out_dev, void *stream) {
    GridDims d;
    if (!reach || !out_dev) return xs_set_error(hipErrorInvalidValue, "xs_reach_expand: null pointer");
    if (!grid_dims_launchable(res, d)) return xs_set_error(hipErrorInvalidValue, "xs_reach_expand: bad resolution");
    const unsigned long long *words = static_cast<const unsigned long long *>(reach) + (passable ? grid_bricks(d) : 0);
    hipLaunchKernelGGL(k_reach_expand, grid_voxel_blocks(d), dim3(GRID_VOXEL_THREADS), 0, (hipStream_t)stream, words, d, out_dev);
    XS_CHECK(hipGetLastError());
    return 0;
}

// ---- point query -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_reach_query(int n, const float *__restrict__ points, float voxel_size, GridDims d, const unsigned long long *__restrict__ words,
                                                    const uint16_t *__restrict__ field, int snap, unsigned char *__restrict__ reachable,
                                                    uint16_t *__restrict__ clear2, int *__restrict__ voxel) {
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    if (i >= n) return;
    const float q0 = floorf(points[3 * (size_t)i] / voxel_size), q1 = floorf(points[3 * (size_t)i + 1] / voxel_size),
                q2 = floorf(points[3 * (size_t)i + 2] / voxel_size);
    unsigned char r = 0;
    uint16_t c = 0;
    int vx = -1, vy = -1, vz = -1;
    // (a NaN compares false: outside)
    if (q0 >= 0.f && q0 < (float)d.X && q1 >= 0.f && q1 < (float)d.Y && q2 >= 0.f && q2 < (float)d.Z) {
        const int sx = (int)q0, sy = (int)q1, sz = (int)q2;
        c = field[grid_voxel_of(d, sx, sy, sz)];
        if (grid_mask_bit(words, d, sx, sy, sz)) { r = 1; vx = sx; vy = sy; vz = sz; }
        else if (snap > 0) {
            // ascending linear index, strict improvement: among equal distances the lowest index stays
            int best = 0x7fffffff;
            for (int z = max(sz - snap, 0); z <= min(sz + snap, d.Z - 1); ++z)
                for (int y = max(sy - snap, 0); y <= min(sy + snap, d.Y - 1); ++y) {
                    const int dyz = (z - sz) * (z - sz) + (y - sy) * (y - sy);
                    if (dyz >= best) continue;
                    for (int x = max(sx - snap, 0); x <= min(sx + snap, d.X - 1); ++x) {
                        const int dd = dyz + (x - sx) * (x - sx);
                        if (dd < best && grid_mask_bit(words, d, x, y, z)) { best = dd; vx = x; vy = y; vz = z; }
                    }
                }
            if (vx >= 0) { r = 1; c = field[grid_voxel_of(d, vx, vy, vz)]; }
        }
    }
    reachable[i] = r;
    clear2[i] = c;
    if (voxel) { voxel[3 * (size_t)i] = vx; voxel[3 * (size_t)i + 1] = vy; voxel[3 * (size_t)i + 2] = vz; }
}

extern "C" int xs_reach_query(int n, const float *points3xN_dev, const int *res, float voxel_size, const void *reach, int over_passable,
                              const unsigned short *field_dev, int snap, unsigned char *reachable_dev, unsigned short *clear2_dev, int *voxel3xN_dev,
                              void *stream) {
    GridDims d;
    if (!points3xN_dev || !reach || !field_dev || !reachable_dev || !clear2_dev) return xs_set_error(hipErrorInvalidValue, "xs_reach_query: null pointer");
    if (!grid_dims_launchable(res, d)) return xs_set_error(hipErrorInvalidValue, "xs_reach_query: bad resolution");
    if (n < 1 || !(voxel_size > 0.f)) return xs_set_error(hipErrorInvalidValue, "xs_reach_query: n < 1 or a voxel size that is not positive");
    if (snap < 0 || snap > XS_REACH_MAX_SNAP) return xs_set_error(hipErrorInvalidValue, "xs_reach_query: snap outside 0 .. XS_REACH_MAX_SNAP");
    const unsigned long long *words = static_cast<const unsigned long long *>(reach) + (over_passable ? grid_bricks(d) : 0);
    hipLaunchKernelGGL(k_reach_query, dim3(((unsigned)n + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, n, points3xN_dev, voxel_size, d, words, field_dev, snap,
                       reachable_dev, clear2_dev, voxel3xN_dev);
    XS_CHECK(hipGetLastError());
    return 0;
}
