// xs_band.hip — the band index of a fixed map and the batched Gauss-Newton pass over it (relocalisation).
//
// The six-pose Gauss-Newton pass (k_tsdf_gauss_newton, xs_residual.hip) scans the whole dense slab to find its band voxels (gt != 0,
// |gt| <= 0.95) and evaluates only those.  The band is a function of gt alone: for a map that does not change, every pass of every query
// frame scans the same gigabytes to find the same voxels.  Here the scan runs once per map version and RECORDS what it deals out:
//   k_band_count / k_band_write  walk the slab exactly as the Gauss-Newton kernel does (walk_band with hess_tiling(heavy_body = true): the
//                                same grid, tiling, interleave, skew and per-wave LDS queue) and store each band voxel in segment
//                                (workgroup b, wave w) at entry 64 k + lane for the lane's k-th take — the order the kernel dealt it in;
//   k_band_gauss_newton          workgroup (b, f) replays segment b's four wave segments for frame f: lane l of wave w takes entries l,
//                                l + 64, ... — the very voxels, in the very order, that lane l of wave w of workgroup b met in the dense
//                                pass — and folds its 29 sums through block_fold_and_finish_of with one ticket per frame.
// Every double addition therefore meets the same operands in the same order as in the dense pass: a frame's 29 sums are bit-identical to
// xs_tsdf_gauss_newton_terms' for its depth and poses, whatever the other frames of the launch are.  The frames go into workgroups, not
// registers (the kernel keeps the dense kernel's 29 accumulators); the index is read F times, from the Infinity Cache after the first.
//
//   k_band_pose_hessian          the exact 6 x 6 pose Hessian of the same loss in one pass over the index: 21
//                                dual-complex poses per frame, one per generator pair a <= b, each band voxel evaluated for all of them.
//                                It has no dense twin to replay: the flat keys / values arrays are dealt out evenly in 64-entry chunks.
//
//   k_band_score_poses           the real-valued loss of ONE depth frame at up to 4096 poses in one pass over the index (DESIGN.md section
//                                4.17): lane = band voxel, the poses in tiles of 64 looped over per chunk, each pose's sum and count kept by
//                                lane (p mod 64) of the wave.  The first question of a relocaliser: which of these hypotheses sees this map?
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "xs_gn_band.h"
#include "../../include/xslam_amd.h"

static_assert(XS_BAND_MAX_FRAMES == 32, "the header's bound");
enum { BAND_RECORD_DOUBLES = 32, BAND_POSES_OFFSET = 256 };
static size_t band_records_offset() { return BAND_POSES_OFFSET + (size_t)XS_BAND_MAX_FRAMES * sizeof(GnPoses); }

__device__ __forceinline__ unsigned long long band_key(int x, int y, int z) {
    return (unsigned long long)x | ((unsigned long long)y << 21) | ((unsigned long long)z << 42);   // BandQueue's packing
}

// segs: [0, nseg) offsets, [nseg, 2 nseg) lengths of the nseg = 4 nblocks wave segments (long long)
template <bool WRITE>
__global__ void __launch_bounds__(256) k_band_record(const HessArgs a, long long *segs, unsigned long long *keys, unsigned *values) {
    const int lane = threadIdx.x, wave = threadIdx.y;
    const unsigned nseg = gridDim.x * 4u, seg = blockIdx.x * 4u + (unsigned)wave;
    const long long base = WRITE ? segs[seg] : 0;
    // walk_band deals sixty-four voxels per take to lanes 0 .. 63 and the last, shorter take to lanes 0 .. n - 1: a lane's k-th call of the body
    // is its wave's k-th take, entry 64 k + lane of the segment
    long long k = 0;
    walk_band(a, [&](int x, int y, int z, size_t, float gt) {
        if (WRITE) {
            const long long e = base + 64 * k + lane;
            keys[e] = band_key(x, y, z);
            values[e] = __float_as_uint(gt);
        }
        ++k;
    });
    if (!WRITE) {
        const unsigned long long n = wave_sum_u64((unsigned long long)k);
        if (lane == 0) segs[nseg + seg] = (long long)n;
    }
}

struct BandGnArgs {
    HessArgs a;                                  // the residual's fields (depth: frame 0's; each workgroup takes its frame's)
    const float *depth[XS_BAND_MAX_FRAMES];
    const unsigned long long *keys;
    const float *values;
    const long long *segs;
    const GnPoses *poses;                        // [F], in the workspace
    double *records;                             // [F][nblocks][32]
    unsigned *tickets;                           // [F], zero between launches
    double *out;                                 // [F][29]
};
__global__ void __launch_bounds__(256) k_band_gauss_newton(const BandGnArgs g) {
    __shared__ GnPoses P;
    const int f = blockIdx.y, lane = threadIdx.x, wave = threadIdx.y;
    const unsigned nblocks = gridDim.x, nseg = 4u * nblocks, seg = blockIdx.x * 4u + (unsigned)wave;
    {
        const float *src = reinterpret_cast<const float *>(g.poses + f);
        float *dst = reinterpret_cast<float *>(&P);
        for (int i = threadIdx.y * 64 + threadIdx.x; i < (int)(sizeof(GnPoses) / sizeof(float)); i += 256) dst[i] = src[i];
        __syncthreads();
    }
    HessArgs a = g.a;
    a.depth = g.depth[f];
    double acc[29];
#pragma unroll
    for (int k = 0; k < 29; ++k) acc[k] = 0.0;
    const long long off = g.segs[seg], n = g.segs[nseg + seg];
    for (long long e = lane; e < n; e += 64) {
        const unsigned long long key = g.keys[off + e];
        const int x = (int)(key & 0x1fffff), y = (int)((key >> 21) & 0x1fffff), z = (int)(key >> 42);
        gn_terms_add(a, P, x, y, z, g.values[off + e], acc);
    }
    block_fold_and_finish_of<29>(acc, g.records + (size_t)f * nblocks * BAND_RECORD_DOUBLES, g.tickets + f, g.out + 29 * f, nullptr, 0, false,
                                 nblocks, blockIdx.x);
}

// the larger of the two grids the slab's walk can take (16-byte aligned gt or not)
extern "C" size_t xs_tsdf_band_segs_bytes(const int *res, int z0, int z1) {
    if (!res || z0 < 0 || z1 > res[2] || z1 <= z0) return 0;
    unsigned most = 0;
    for (uintptr_t addr : {(uintptr_t)256, (uintptr_t)4}) {
        HessArgs a; dim3 grid;
        if (hess_tiling(a, res, reinterpret_cast<const float *>(addr), z0, z1, grid, true)) return 0;
        most = grid.x > most ? grid.x : most;
    }
    return (size_t)most * 4 * 2 * sizeof(long long);
}

extern "C" int xs_tsdf_band_build(const float *gt, const int *res, int z0, int z1, xs_band_index *index, void *stream) {
    if (!gt || !res || !index || !index->segs) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_band_build: null pointer");
    if (z0 < 0 || z1 > res[2] || z1 <= z0) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_band_build: bad slab");
    if (index->capacity > 0 && (!index->keys || !index->values)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_band_build: capacity without arrays");
    if ((long long)res[0] > 0x1fffff || (long long)res[1] > 0x1fffff || (long long)res[2] > 0x3fffff)
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_band_build: volume too large for the packed keys");
    hipStream_t st = (hipStream_t)stream;
    HessArgs a; dim3 grid;
    memset(&a, 0, sizeof(a));
    int rc = hess_tiling(a, res, gt, z0, z1, grid, true);
    if (rc) return rc;
    const unsigned nseg = grid.x * 4u;
    index->count = 0; index->nblocks = 0;
    hipLaunchKernelGGL(k_band_record<false>, grid, dim3(64, 4), 0, st, a, index->segs, nullptr, nullptr);
    XS_CHECK(hipGetLastError());
    std::vector<long long> segs(2 * (size_t)nseg);
    XS_CHECK(hipMemcpyAsync(segs.data() + nseg, index->segs + nseg, nseg * sizeof(long long), hipMemcpyDeviceToHost, st));
    XS_CHECK(hipStreamSynchronize(st));
    long long total = 0;
    for (unsigned s = 0; s < nseg; ++s) { segs[s] = total; total += segs[nseg + s]; }
    index->count = total;
    index->nblocks = (int)grid.x;
    index->res[0] = res[0]; index->res[1] = res[1]; index->res[2] = res[2];
    index->z0 = z0; index->z1 = z1;
    if (total > index->capacity) return XS_BAND_OVER_CAPACITY;
    XS_CHECK(hipMemcpyAsync(index->segs, segs.data(), nseg * sizeof(long long), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_band_record<true>, grid, dim3(64, 4), 0, st, a, index->segs, index->keys, reinterpret_cast<unsigned *>(index->values));
    XS_CHECK(hipGetLastError());
    XS_CHECK(hipStreamSynchronize(st));   // (segs, the host's copy of the offsets, is gone when this returns)
    return 0;
}

extern "C" size_t xs_tsdf_band_workspace_bytes(int frames) {
    if (frames < 1 || frames > XS_BAND_MAX_FRAMES) return 0;
    return band_records_offset() + (size_t)frames * XS_TSDF_REDUCE_MAX_BLOCKS_C * BAND_RECORD_DOUBLES * sizeof(double);
}

extern "C" int xs_tsdf_gauss_newton_terms_band(int frames, const float *const *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4,
                                               float voxel_size, const float *Rv2c108xF, const float *tv2c36xF, float tranc_dist,
                                               const xs_band_index *index, void *workspace, double *out29xF_dev, void *stream) {
    if (frames < 1 || frames > XS_BAND_MAX_FRAMES) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_gauss_newton_terms_band: frames outside 1 .. XS_BAND_MAX_FRAMES");
    if (!depth_scaled || !intr4 || !Rv2c108xF || !tv2c36xF || !index || !workspace || !out29xF_dev)
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_gauss_newton_terms_band: null pointer");
    if (index->nblocks < 1 || index->nblocks > XS_TSDF_REDUCE_MAX_BLOCKS_C || !index->segs || (index->count > 0 && (!index->keys || !index->values)))
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_gauss_newton_terms_band: the index was not built");
    BandGnArgs g;
    memset(&g, 0, sizeof(g));
    for (int f = 0; f < frames; ++f) {
        if (!depth_scaled[f]) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_gauss_newton_terms_band: null depth");
        g.depth[f] = depth_scaled[f];
    }
    HessArgs &a = g.a;   // as hess_common fills them for the dense pass
    a.depth = depth_scaled[0]; a.dstep = scaled_step; a.drows = rows; a.dcols = cols;
    a.voxel_size = voxel_size; a.tranc_dist = tranc_dist; a.tranc_dist_inv = 1.0f / tranc_dist;
    a.intr = Intr{intr4[0], intr4[1], intr4[2], intr4[3]};
    a.X = index->res[0]; a.Y = index->res[1]; a.Z = index->res[2]; a.z0 = index->z0; a.z1 = index->z1;
    std::vector<GnPoses> P((size_t)frames);
    memset(P.data(), 0, P.size() * sizeof(GnPoses));
    for (int f = 0; f < frames; ++f)
        for (int k = 0; k < 6; ++k) { load_mat(Rv2c108xF + 108 * f + 18 * k, P[f].R[k]); load_vec(tv2c36xF + 36 * f + 6 * k, P[f].t[k]); }
    char *ws = static_cast<char *>(workspace);
    g.tickets = reinterpret_cast<unsigned *>(ws);
    g.poses = reinterpret_cast<const GnPoses *>(ws + BAND_POSES_OFFSET);
    g.records = reinterpret_cast<double *>(ws + band_records_offset());
    g.keys = index->keys; g.values = index->values; g.segs = index->segs; g.out = out29xF_dev;
    hipStream_t st = (hipStream_t)stream;
    XS_CHECK(hipMemcpyAsync(ws + BAND_POSES_OFFSET, P.data(), P.size() * sizeof(GnPoses), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_band_gauss_newton, dim3((unsigned)index->nblocks, (unsigned)frames), dim3(64, 4), 0, st, g);
    XS_CHECK(hipGetLastError());
    return 0;
}

// ---- the exact pose Hessian over the index ------------------------------------------------------------------
// Per query frame 21 dual-complex poses, pair (a, b), a <= b, row-major: real part v2c, eps1 along generator a, eps2 along b, eps1 eps2 the
// second-order term of the pose's expansion (the host's newton_seeded_poses).  Every band voxel is evaluated for all 21 (tsdf_loss_d, the
// per-voxel term of k_tsdf_hessian) and counts only if all 21 keep it, so one count serves every entry:
//   out[0 .. 20]  sum loss_ab.hessian()      out[21 .. 26]  sum loss_aa.grad()      out[27]  sum loss_00.value()      out[28]  count
// The pair loop is NOT unrolled (one copy of the dual-complex body); a lane parks a voxel's 28 terms in its own column of LDS until the
// last pair has kept the voxel and then adds them to its 29 double accumulators.
// Order: the entries are cut into chunks of 64; wave w of workgroup b takes chunks 4 b + w, + 4 nblocks, ... and lane l entry l of each —
// a function of the index's count alone, so frame f's additions are the same whatever F, its slot or the other frames are; the fold is
// block_fold_and_finish_of's (registers -> wave -> LDS -> one record per workgroup -> the frame's last workgroup adds the records in
// index order), one ticket per frame.
enum { NEWTON_PAIRS = 21, NEWTON_TERMS = 28, NEWTON_POSES_OFFSET = 256 };
static size_t newton_records_offset() { return NEWTON_POSES_OFFSET + (size_t)XS_BAND_MAX_FRAMES * NEWTON_PAIRS * sizeof(HessPoseD); }
static_assert(sizeof(HessPoseD) == 48 * sizeof(float), "36 + 12 floats per dual-complex pose");

struct BandHessArgs {
    HessArgs a;                                  // the residual's fields (depth: each workgroup takes its frame's)
    const float *depth[XS_BAND_MAX_FRAMES];
    const unsigned long long *keys;
    const float *values;
    long long count;                             // entries of keys / values
    const HessPoseD *poses;                      // [F][21], in the workspace
    double *records;                             // [F][nblocks][32]
    unsigned *tickets;                           // [F], zero between launches
    double *out;                                 // [F][29]
};
__global__ void __launch_bounds__(256) k_band_pose_hessian(const BandHessArgs g) {
    __shared__ HessPoseD P[NEWTON_PAIRS];
    __shared__ float s_term[NEWTON_TERMS][256];  // [term][thread]: a thread reads back only what it wrote itself
    const int f = blockIdx.y, lane = threadIdx.x, wave = threadIdx.y, tid = wave * 64 + lane;
    {
        const float *src = reinterpret_cast<const float *>(g.poses + (size_t)f * NEWTON_PAIRS);
        float *dst = reinterpret_cast<float *>(&P[0]);
        for (int i = tid; i < (int)(NEWTON_PAIRS * sizeof(HessPoseD) / sizeof(float)); i += 256) dst[i] = src[i];
        __syncthreads();
    }
    HessArgs a = g.a;
    a.depth = g.depth[f];
    double acc[29];
#pragma unroll
    for (int k = 0; k < 29; ++k) acc[k] = 0.0;
    const long long nchunks = (g.count + 63) / 64;
    for (long long c = (long long)blockIdx.x * 4 + wave; c < nchunks; c += 4ll * gridDim.x) {
        const long long e = c * 64 + lane;
        if (e >= g.count) continue;              // (the last chunk's tail)
        const unsigned long long key = g.keys[e];
        const int x = (int)(key & 0x1fffff), y = (int)((key >> 21) & 0x1fffff), z = (int)(key >> 42);
        const float gt = g.values[e];
        bool ok = true;
        int pa = 0, pb = 0;
#pragma unroll 1
        for (int p = 0; p < NEWTON_PAIRS; ++p) {
            dcfloat loss;
            if (!tsdf_loss_d(a, P[p], x, y, z, gt, loss)) { ok = false; break; }
            s_term[p][tid] = loss.hessian();
            if (pa == pb) s_term[NEWTON_PAIRS + pa][tid] = loss.grad();
            if (p == 0) s_term[27][tid] = loss.value();
            if (++pb == 6) { ++pa; pb = pa; }
        }
        if (!ok) continue;
#pragma unroll
        for (int k = 0; k < NEWTON_TERMS; ++k) acc[k] += (double)s_term[k][tid];
        acc[28] += 1.0;
    }
    block_fold_and_finish_of<29>(acc, g.records + (size_t)f * gridDim.x * BAND_RECORD_DOUBLES, g.tickets + f, g.out + 29 * f, nullptr, 0, false,
                                 gridDim.x, blockIdx.x);
}

extern "C" size_t xs_tsdf_pose_hessian_workspace_bytes(int frames) {
    if (frames < 1 || frames > XS_BAND_MAX_FRAMES) return 0;
    return newton_records_offset() + (size_t)frames * XS_TSDF_REDUCE_MAX_BLOCKS_C * BAND_RECORD_DOUBLES * sizeof(double);
}

extern "C" int xs_tsdf_pose_hessian_band(int frames, const float *const *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4,
                                         float voxel_size, const float *Rv2c36x21xF, const float *tv2c12x21xF, float tranc_dist,
                                         const xs_band_index *index, void *workspace, double *out29xF_dev, void *stream) {
    if (frames < 1 || frames > XS_BAND_MAX_FRAMES) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_pose_hessian_band: frames outside 1 .. XS_BAND_MAX_FRAMES");
    if (!depth_scaled || !intr4 || !Rv2c36x21xF || !tv2c12x21xF || !index || !workspace || !out29xF_dev)
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_pose_hessian_band: null pointer");
    if (index->nblocks < 1 || index->count < 0 || index->count > index->capacity || (index->count > 0 && (!index->keys || !index->values)))
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_pose_hessian_band: the index was not built");
    if (rows < 4 || cols < 4 || scaled_step < (size_t)cols * sizeof(float)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_pose_hessian_band: bad depth shape");
    BandHessArgs g;
    memset(&g, 0, sizeof(g));
    for (int f = 0; f < frames; ++f) {
        if (!depth_scaled[f]) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_pose_hessian_band: null depth");
        g.depth[f] = depth_scaled[f];
    }
    HessArgs &a = g.a;
    a.depth = depth_scaled[0]; a.dstep = scaled_step; a.drows = rows; a.dcols = cols;
    a.voxel_size = voxel_size; a.tranc_dist = tranc_dist; a.tranc_dist_inv = 1.0f / tranc_dist;
    a.intr = Intr{intr4[0], intr4[1], intr4[2], intr4[3]};
    a.X = index->res[0]; a.Y = index->res[1]; a.Z = index->res[2]; a.z0 = index->z0; a.z1 = index->z1;
    std::vector<HessPoseD> P((size_t)frames * NEWTON_PAIRS);
    for (size_t k = 0; k < P.size(); ++k) {
        const float *p = Rv2c36x21xF + 36 * k, *t = tv2c12x21xF + 12 * k;
        for (int r = 0; r < 3; ++r) {
            P[k].R.data[r].x = dcfloat(p[12 * r + 0], p[12 * r + 1], p[12 * r + 2], p[12 * r + 3]);
            P[k].R.data[r].y = dcfloat(p[12 * r + 4], p[12 * r + 5], p[12 * r + 6], p[12 * r + 7]);
            P[k].R.data[r].z = dcfloat(p[12 * r + 8], p[12 * r + 9], p[12 * r + 10], p[12 * r + 11]);
        }
        P[k].t.x = dcfloat(t[0], t[1], t[2], t[3]);
        P[k].t.y = dcfloat(t[4], t[5], t[6], t[7]);
        P[k].t.z = dcfloat(t[8], t[9], t[10], t[11]);
    }
    // as many workgroups as give every wave a chunk, at most the record workspace's 4096: a function of the index alone
    const long long nchunks = (index->count + 63) / 64, want = (nchunks + 3) / 4;
    const unsigned nblocks = (unsigned)(want < 1 ? 1 : (want > XS_TSDF_REDUCE_MAX_BLOCKS_C ? XS_TSDF_REDUCE_MAX_BLOCKS_C : want));
    char *ws = static_cast<char *>(workspace);
    g.tickets = reinterpret_cast<unsigned *>(ws);
    g.poses = reinterpret_cast<const HessPoseD *>(ws + NEWTON_POSES_OFFSET);
    g.records = reinterpret_cast<double *>(ws + newton_records_offset());
    g.keys = index->keys; g.values = index->values; g.count = index->count; g.out = out29xF_dev;
    hipStream_t st = (hipStream_t)stream;
    XS_CHECK(hipMemcpyAsync(ws + NEWTON_POSES_OFFSET, P.data(), P.size() * sizeof(HessPoseD), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_band_pose_hessian, dim3(nblocks, (unsigned)frames), dim3(64, 4), 0, st, g);
    XS_CHECK(hipGetLastError());
    return 0;
}

// ---- many poses, one frame: the alignment loss of every pose hypothesis in one pass over the index -----------
// The entries are cut into chunks of 64 as for k_band_pose_hessian: wave w of workgroup (b, tile) takes chunks 4 b + w, + 4 nblocks, ...;
// lane l decodes entry l of the chunk once and then meets the tile's poses 64 tile .. 64 tile + 63 one after the other.  The pose index is
// wave-uniform (a loop counter through readfirstlane): the twelve floats of a pose arrive by scalar loads and stay in scalar registers.  Per
// (chunk, pose): loss where tsdf_loss_f keeps the voxel, 0 where it drops it (and in the tail of the last chunk), folded across the wave in a
// fixed six-level pairwise tree — the same additions whatever the other lanes hold — the count by ballot + popcount; lane (p mod 64) adds both
// to the accumulators it keeps in registers for pose p, one double and one unsigned.  Then per workgroup: the four waves' accumulators in
// wave order, one record of 64 doubles + 64 counts, an arrival ticket per tile, and the tile's last workgroup adds the records in index
// order (block_fold_and_finish_of's scheme and hand-off, 64 poses wide).  Every step's order is a function of the index's count alone.
enum { SCORE_TILE = 64, SCORE_POSES_OFFSET = 256, SCORE_MAX_BLOCKS = 1024, SCORE_RECORD_BYTES = SCORE_TILE * (sizeof(double) + sizeof(unsigned)) };
static_assert(XS_SCORE_MAX_POSES / SCORE_TILE * sizeof(unsigned) == SCORE_POSES_OFFSET, "one ticket per tile in the first 256 bytes");
static_assert(sizeof(HessPoseF) == 12 * sizeof(float), "twelve floats per real pose");
static size_t score_records_offset() { return SCORE_POSES_OFFSET + (size_t)XS_SCORE_MAX_POSES * sizeof(HessPoseF); }

struct BandScoreArgs {
    HessArgs a;                                  // the residual's fields
    const unsigned long long *keys;
    const float *values;
    long long count;                             // entries of keys / values
    int poses;
    const HessPoseF *poses_dev;                  // [poses], in the workspace
    char *records;                               // [tiles][nblocks]{64 doubles, 64 unsigned}
    unsigned *tickets;                           // [tiles], zero between launches
    double *out;                                 // [poses][2]
};
__global__ void __launch_bounds__(256) k_band_score_poses(const BandScoreArgs g) {
    __shared__ double s_sum[4][SCORE_TILE];
    __shared__ unsigned s_cnt[4][SCORE_TILE];
    __shared__ unsigned s_last;
    const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(threadIdx.y), tid = wave * 64 + lane;
    const unsigned nblocks = gridDim.x, bid = blockIdx.x, tile = blockIdx.y;
    const int p0 = (int)tile * SCORE_TILE, np = min(SCORE_TILE, g.poses - p0);   // (the last tile may be partial: its other lanes keep zeros)
    const HessPoseF *__restrict__ poses = g.poses_dev + p0;
    double acc = 0.0;
    unsigned cnt = 0;
    const long long nchunks = (g.count + 63) / 64;
    for (long long c = (long long)bid * 4 + wave; c < nchunks; c += 4ll * nblocks) {
        const long long e = c * 64 + lane;
        const bool valid = e < g.count;          // (the last chunk's tail: masked, and it adds zeros)
        unsigned long long key = 0;
        float gt = 0.f;
        if (valid) { key = g.keys[e]; gt = g.values[e]; }
        const int x = (int)(key & 0x1fffff), y = (int)((key >> 21) & 0x1fffff), z = (int)(key >> 42);
#pragma unroll 1
        for (int j = 0; j < np; ++j) {
            const HessPoseF P = poses[__builtin_amdgcn_readfirstlane(j)];
            float loss = 0.f;
            const bool kept = valid && tsdf_loss_f(g.a, P, x, y, z, gt, loss);
            const float s = wave_tree_sum_f32(kept ? loss : 0.f);
            const unsigned n = (unsigned)__popcll(__ballot(kept));
            if (lane == j) { acc += (double)s; cnt += n; }
        }
    }
    // the four waves in wave order, then one record per workgroup: pose lane's sum and count, stored by the lanes of wave 0
    s_sum[wave][lane] = acc;
    s_cnt[wave][lane] = cnt;
    __syncthreads();
    char *tile_records = g.records + (size_t)tile * nblocks * SCORE_RECORD_BYTES;
    if (tid < SCORE_TILE) {
        const double s = ((s_sum[0][tid] + s_sum[1][tid]) + s_sum[2][tid]) + s_sum[3][tid];
        const unsigned n = ((s_cnt[0][tid] + s_cnt[1][tid]) + s_cnt[2][tid]) + s_cnt[3][tid];
        char *rec = tile_records + (size_t)bid * SCORE_RECORD_BYTES;
        __hip_atomic_store(reinterpret_cast<double *>(rec) + tid, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(reinterpret_cast<unsigned *>(rec + SCORE_TILE * sizeof(double)) + tid, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // the hand-off of block_fold_and_finish_of (xs_gn_band.h): write-through record stores by wave 0, acknowledged, then its first lane's ticket
    if (wave == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) {
        const unsigned tk = __hip_atomic_fetch_add(g.tickets + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = tk == nblocks - 1 ? 1u : 0u;
        if (s_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (!s_last) return;
    // the tile's last workgroup: thread (q, l) adds pose l's records q, q + 4, ... in that order, eight loads in flight; the four row groups are
    // then added in group order
    {
        const int l = tid % SCORE_TILE, q = tid / SCORE_TILE;
        double s = 0.0;
        unsigned long long n = 0;
        auto rsum = [&](unsigned b) { return reinterpret_cast<const double *>(tile_records + (size_t)b * SCORE_RECORD_BYTES)[l]; };
        auto rcnt = [&](unsigned b) { return reinterpret_cast<const unsigned *>(tile_records + (size_t)b * SCORE_RECORD_BYTES + SCORE_TILE * sizeof(double))[l]; };
        unsigned b = q;
        for (; b + 4 * 7 < nblocks; b += 4 * 8) {
            double v[8]; unsigned m[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { v[k] = rsum(b + 4 * k); m[k] = rcnt(b + 4 * k); }
#pragma unroll
            for (int k = 0; k < 8; ++k) { s += v[k]; n += m[k]; }
        }
        for (; b < nblocks; b += 4) { s += rsum(b); n += rcnt(b); }
        __shared__ unsigned long long s_n[4][SCORE_TILE];
        s_sum[q][l] = s;   // (wave 0 read its workgroup's own sums before the ticket's barrier)
        s_n[q][l] = n;
        __syncthreads();
        if (tid < np) {
            g.out[2 * (size_t)(p0 + tid)] = ((s_sum[0][tid] + s_sum[1][tid]) + s_sum[2][tid]) + s_sum[3][tid];
            g.out[2 * (size_t)(p0 + tid) + 1] = (double)(((s_n[0][tid] + s_n[1][tid]) + s_n[2][tid]) + s_n[3][tid]);
        }
        // the ticket goes back to zero for the next launch on this workspace (xs_tsdf_reduce_workspace_init zeroes it once)
        if (tid == 0) __hip_atomic_store(g.tickets + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

extern "C" size_t xs_tsdf_score_poses_workspace_bytes(int poses) {
    if (poses < 1 || poses > XS_SCORE_MAX_POSES) return 0;
    const size_t tiles = ((size_t)poses + SCORE_TILE - 1) / SCORE_TILE;
    return score_records_offset() + tiles * SCORE_MAX_BLOCKS * SCORE_RECORD_BYTES;
}

extern "C" int xs_tsdf_score_poses_band(int poses, const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4,
                                        float voxel_size, const float *Rv2c9xP, const float *tv2c3xP, float tranc_dist,
                                        const xs_band_index *index, void *workspace, double *out2xP_dev, void *stream) {
    if (poses < 1 || poses > XS_SCORE_MAX_POSES) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_score_poses_band: poses outside 1 .. XS_SCORE_MAX_POSES");
    if (!depth_scaled || !intr4 || !Rv2c9xP || !tv2c3xP || !index || !workspace || !out2xP_dev)
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_score_poses_band: null pointer");
    if (index->nblocks < 1 || index->count < 0 || index->count > index->capacity || (index->count > 0 && (!index->keys || !index->values)))
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_score_poses_band: the index was not built");
    if (rows < 4 || cols < 4 || scaled_step < (size_t)cols * sizeof(float)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_score_poses_band: bad depth shape");
    BandScoreArgs g;
    memset(&g, 0, sizeof(g));
    HessArgs &a = g.a;
    a.depth = depth_scaled; a.dstep = scaled_step; a.drows = rows; a.dcols = cols;
    a.voxel_size = voxel_size; a.tranc_dist = tranc_dist; a.tranc_dist_inv = 1.0f / tranc_dist;
    a.intr = Intr{intr4[0], intr4[1], intr4[2], intr4[3]};
    a.X = index->res[0]; a.Y = index->res[1]; a.Z = index->res[2]; a.z0 = index->z0; a.z1 = index->z1;
    std::vector<HessPoseF> P((size_t)poses);
    for (int p = 0; p < poses; ++p) {
        for (int i = 0; i < 9; ++i) P[(size_t)p].R[i] = Rv2c9xP[9 * (size_t)p + i];
        for (int i = 0; i < 3; ++i) P[(size_t)p].t[i] = tv2c3xP[3 * (size_t)p + i];
    }
    // as many workgroups per tile as give every wave a chunk, at most the record workspace's 1024: a function of the index alone
    const long long nchunks = (index->count + 63) / 64, want = (nchunks + 3) / 4;
    const unsigned nblocks = (unsigned)(want < 1 ? 1 : (want > SCORE_MAX_BLOCKS ? SCORE_MAX_BLOCKS : want));
    const unsigned tiles = ((unsigned)poses + SCORE_TILE - 1) / SCORE_TILE;
    char *ws = static_cast<char *>(workspace);
    g.tickets = reinterpret_cast<unsigned *>(ws);
    g.poses_dev = reinterpret_cast<const HessPoseF *>(ws + SCORE_POSES_OFFSET);
    g.records = ws + score_records_offset();
    g.keys = index->keys; g.values = index->values; g.count = index->count; g.poses = poses; g.out = out2xP_dev;
    hipStream_t st = (hipStream_t)stream;
    XS_CHECK(hipMemcpyAsync(ws + SCORE_POSES_OFFSET, P.data(), P.size() * sizeof(HessPoseF), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_band_score_poses, dim3(nblocks, tiles), dim3(64, 4), 0, st, g);
    XS_CHECK(hipGetLastError());
    return 0;
}
