// xs_align.hip — the Gauss-Newton terms of aligning a second TSDF map to the volume, over the volume's band index, for gfx950 (DESIGN.md
// section 4.23).  No counterpart in the reference: its maps are only ever aligned to a camera frame.
//
// The residual of a band voxel (x, y, z, gt) of THIS map is "the other map, resampled at the voxel under the affine index map m, minus gt":
// the sample xs_tsdf_merge would average in, at the position it would use.  m is complex: six maps per transform, seeded along the six
// generators of the rigid transform (host/align_host.hpp), and the trilinear interpolation runs in the complex scalars of xs_complex.h, so
// the imaginary part of the residual is h times its derivative along the seed.  What a kept voxel adds is what gn_terms_add adds.
//
// One lane per band entry, dealt out as k_band_pose_hessian deals them: chunks of 64, wave w of workgroup (b, n) takes chunks 4 b + w,
// + 4 nblocks, ..., and the fold is block_fold_and_finish_of with one ticket per transform.  The 144 floats of transform n's maps are read
// into LDS once per workgroup and from there with wave-uniform addresses.  The source is gathered: eight weights, all eight loads issued
// before the first is tested, and — only where all eight carry min_weight — eight values.  Neighbouring entries of the index are spatial
// neighbours (the dense walk deals a wave one 64-voxel run of a row after the other), so their corners share cache lines; no LDS staging.
// Every seed runs the whole complex interpolation: per voxel the float32 results are the contract's bit for bit, and the six real parts
// are not assumed equal (they are, to the last bits, and the voxel counts only if all six keep it).
//
// k_align_score, after it: the same residual without seeds, for up to 4096 transforms in one pass, which finds the
// transform the Gauss-Newton pass above starts from when nobody supplies one.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "xs_gn_band.h"
#include "xs_complex.h"
#include "xs_score_fold.h"
#include "../../include/xslam_amd.h"

static_assert(XS_ALIGN_MAX_TRANSFORMS == 32, "the header's bound");
static_assert(XS_ALIGN_MAX_TRANSFORMS * sizeof(unsigned) <= 256, "one ticket per transform in the first 256 bytes");
enum { ALIGN_MAP_FLOATS = 144, ALIGN_MAPS_OFFSET = 256, ALIGN_RECORD_DOUBLES = 32 };
static size_t align_records_offset() { return ALIGN_MAPS_OFFSET + (size_t)XS_ALIGN_MAX_TRANSFORMS * ALIGN_MAP_FLOATS * sizeof(float); }

struct AlignArgs {
    const unsigned long long *keys;
    const float *values;
    long long count;                             // entries of keys / values
    const float *svalue; const int *sweight; size_t sstep;
    int S[3];
    const float *maps;                           // [N][6][24], in the workspace
    int min_weight;
    float max_residual;
    double *records;                             // [N][nblocks][32]
    unsigned *tickets;                           // [N], zero between launches
    double *out;                                 // [N][29]
};

namespace {
// entry i of seed k's map, from LDS (a wave-uniform address)
__device__ __forceinline__ cfloat map_entry(const float *m, int k, int i) { return cfloat(m[24 * k + 2 * i], m[24 * k + 2 * i + 1]); }

// the per-entry contract of include/xslam_amd.h: adds the voxel's terms to acc if every gate keeps it
__device__ __forceinline__ void align_terms_add(const AlignArgs &g, const float *m, int x, int y, int z, float gt, double (&acc)[29]) {
    const float fx = (float)x, fy = (float)y, fz = (float)z;
    int b[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {   // seed 0's real parts: merge_index's value
        const float gr = ((m[2 * (3 * a)] * fx + m[2 * (3 * a + 1)] * fy) + m[2 * (3 * a + 2)] * fz) + m[2 * (9 + a)];
        if (!(gr >= 0.f && gr < (float)(g.S[a] - 1))) return;
        b[a] = __float2int_rd(gr);               // 0 <= b <= S - 2: both corners of the axis are inside the source
    }
    const int *wrow[4];
    const float *vrow[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {                // d: bit 0 = +y, bit 1 = +z
        const int row = g.S[1] * (b[2] + (d >> 1)) + b[1] + (d & 1);
        wrow[d] = row_ptr(g.sweight, g.sstep, row);
        vrow[d] = row_ptr(g.svalue, g.sstep, row);
    }
    int w[8];                                    // the eight loads in flight together: no test of one decides whether the next is issued
#pragma unroll
    for (int d = 0; d < 8; ++d) w[d] = wrow[d >> 1][b[0] + (d & 1)];
    int ws = w[0];
#pragma unroll
    for (int d = 1; d < 8; ++d) ws = min(ws, w[d]);
    if (ws < g.min_weight) return;
    float v[8];                                  // corner d: bit 0 = +x, bit 1 = +y, bit 2 = +z
#pragma unroll
    for (int d = 0; d < 8; ++d) v[d] = vrow[d >> 1][b[0] + (d & 1)];
    cfloat e[6];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        cfloat f[3], c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const cfloat ga = ((map_entry(m, k, 3 * a) * fx + map_entry(m, k, 3 * a + 1) * fy) + map_entry(m, k, 3 * a + 2) * fz) + map_entry(m, k, 9 + a);
            f[a] = ga - (float)b[a];
            c[a] = 1.0f - f[a];
        }
        // x (real corners times complex fractions), then y, then z
        const cfloat c00 = v[0] * c[0] + v[1] * f[0], c10 = v[2] * c[0] + v[3] * f[0];
        const cfloat c01 = v[4] * c[0] + v[5] * f[0], c11 = v[6] * c[0] + v[7] * f[0];
        const cfloat c0 = c00 * c[1] + c10 * f[1], c1 = c01 * c[1] + c11 * f[1];
        const cfloat F = c0 * c[2] + c1 * f[2];
        e[k] = F - gt;
        ok = ok && !(fabsf(e[k].re) > g.max_residual);
        // one seed at a time, as gn_terms_add: left to itself the scheduler interleaves all six
        asm volatile("" : "+v"(e[k].re), "+v"(e[k].im) :: "memory");
    }
    if (!ok) return;
    const double r = (double)e[0].re;
    int s = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int k = j; k < 6; ++k) acc[s++] += (double)e[j].im * (double)e[k].im;
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[21 + k] += (double)e[k].im * r;
    acc[27] += r * r;
    acc[28] += 1.0;
}
}  // namespace

__global__ void __launch_bounds__(256) k_align_terms(const AlignArgs g) {
    __shared__ float s_map[ALIGN_MAP_FLOATS];
    const int n = blockIdx.y, lane = threadIdx.x, wave = threadIdx.y, tid = wave * 64 + lane;
    if (tid < ALIGN_MAP_FLOATS) s_map[tid] = g.maps[(size_t)n * ALIGN_MAP_FLOATS + tid];
    __syncthreads();
    double acc[29];
#pragma unroll
    for (int k = 0; k < 29; ++k) acc[k] = 0.0;
    const long long nchunks = (g.count + 63) / 64;
    for (long long c = (long long)blockIdx.x * 4 + wave; c < nchunks; c += 4ll * gridDim.x) {
        const long long e = c * 64 + lane;
        if (e >= g.count) continue;              // (the last chunk's tail)
        const unsigned long long key = g.keys[e];
        const int x = (int)(key & 0x1fffff), y = (int)((key >> 21) & 0x1fffff), z = (int)(key >> 42);
        align_terms_add(g, s_map, x, y, z, g.values[e], acc);
    }
    block_fold_and_finish_of<29>(acc, g.records + (size_t)n * gridDim.x * ALIGN_RECORD_DOUBLES, g.tickets + n, g.out + 29 * n, nullptr, 0, false,
                                 gridDim.x, blockIdx.x);
}

extern "C" size_t xs_tsdf_align_workspace_bytes(int transforms) {
    if (transforms < 1 || transforms > XS_ALIGN_MAX_TRANSFORMS) return 0;
    return align_records_offset() + (size_t)transforms * XS_TSDF_REDUCE_MAX_BLOCKS_C * ALIGN_RECORD_DOUBLES * sizeof(double);
}

/* see include/xslam_amd.h */
extern "C" int xs_tsdf_align_terms(int transforms, const xs_band_index *index, const float *src_value, const int *src_weight, size_t src_step,
                                   const int *src_res, const float *maps144xN, int min_weight, float max_residual, void *workspace,
                                   double *out29xN_dev, void *stream) {
    if (transforms < 1 || transforms > XS_ALIGN_MAX_TRANSFORMS)
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_align_terms: transforms outside 1 .. XS_ALIGN_MAX_TRANSFORMS");
    if (!index || !src_value || !src_weight || !src_res || !maps144xN || !workspace || !out29xN_dev)
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_align_terms: null pointer");
    if (index->nblocks < 1 || index->count < 0 || index->count > index->capacity || (index->count > 0 && (!index->keys || !index->values)))
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_align_terms: the index was not built");
    for (int k = 0; k < 3; ++k)
        if (src_res[k] < 2 || src_res[k] > 65535 * 4) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_align_terms: a source axis outside 2 .. 262140");
    if ((long long)src_res[1] * (long long)src_res[2] >= (1ll << 31)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_align_terms: the source's rows do not fit an int");
    if (src_step % 4 != 0 || src_step < (size_t)src_res[0] * 4) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_align_terms: bad pitch");
    if (min_weight < 1) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_align_terms: min_weight below 1");
    if (!(max_residual > 0.f) || !isfinite(max_residual)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_align_terms: max_residual is not finite and positive");
    for (size_t i = 0; i < (size_t)transforms * ALIGN_MAP_FLOATS; ++i)
        if (!isfinite(maps144xN[i])) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_align_terms: a map entry is not finite");
    AlignArgs g;
    memset(&g, 0, sizeof(g));
    g.keys = index->keys; g.values = index->values; g.count = index->count;
    g.svalue = src_value; g.sweight = src_weight; g.sstep = src_step;
    for (int k = 0; k < 3; ++k) g.S[k] = src_res[k];
    g.min_weight = min_weight; g.max_residual = max_residual;
    // as many workgroups as give every wave a chunk, at most the record workspace's 4096: a function of the index alone
    const long long nchunks = (index->count + 63) / 64, want = (nchunks + 3) / 4;
    const unsigned nblocks = (unsigned)(want < 1 ? 1 : (want > XS_TSDF_REDUCE_MAX_BLOCKS_C ? XS_TSDF_REDUCE_MAX_BLOCKS_C : want));
    char *ws = static_cast<char *>(workspace);
    g.tickets = reinterpret_cast<unsigned *>(ws);
    g.maps = reinterpret_cast<const float *>(ws + ALIGN_MAPS_OFFSET);
    g.records = reinterpret_cast<double *>(ws + align_records_offset());
    g.out = out29xN_dev;
    hipStream_t st = (hipStream_t)stream;
    XS_CHECK(hipMemcpyAsync(ws + ALIGN_MAPS_OFFSET, maps144xN, (size_t)transforms * ALIGN_MAP_FLOATS * sizeof(float), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_align_terms, dim3(nblocks, (unsigned)transforms), dim3(64, 4), 0, st, g);
    XS_CHECK(hipGetLastError());
    return 0;
}

// ---- many transforms, no derivative: the loss of every map-to-map hypothesis in one pass over the index ---------
// k_band_score_poses' scheme (xs_band.hip) with the other MAP as what is sampled: the scored entries (every stride-th of the index) are cut
// into chunks of 64; wave w of workgroup (b, tile) takes chunks 4 b + w, + 4 nblocks, ...; lane l decodes scored entry l of the chunk once and
// then meets the tile's transforms 64 tile .. 64 tile + 63 one after the other.  The transform index is wave-uniform (a loop counter through
// readfirstlane): the twelve floats of an index map arrive by scalar loads and stay in scalar registers.  Per (chunk, transform): r * r where
// the per-entry contract of include/xslam_amd.h keeps the entry, 0 where it drops it (and in the tail of the last chunk), folded across the
// wave by wave_tree_sum_f32, the count by ballot + popcount; lane (p mod 64) adds both to the double and the unsigned it keeps for transform
// p.  A wave none of whose lanes lies inside the source, or none of whose lanes passes the weight gate, goes on to the next transform without
// the loads: what it leaves out is the addition of +0.0 to a sum that is never -0.0, and of 0 to a count.  Then per workgroup: the four waves
// in wave order, one record of 64 doubles + 64 counts, an arrival ticket per tile, and the tile's last workgroup adds the records in index
// order (score_tile_fold_and_finish of xs_score_fold.h, shared with k_register_score).  Every step's order is a function of the index's count and the stride alone.
enum { ASCORE_TILE = SCORE_TILE, ASCORE_XFORMS_OFFSET = 256, ASCORE_MAX_BLOCKS = SCORE_MAX_BLOCKS, ASCORE_RECORD_BYTES = SCORE_RECORD_BYTES };   // (xs_score_fold.h)
static_assert(XS_ALIGN_SCORE_MAX_TRANSFORMS / ASCORE_TILE * sizeof(unsigned) == ASCORE_XFORMS_OFFSET, "one ticket per tile in the first 256 bytes");
struct AlignXform { float m[12]; };
static size_t ascore_records_offset() { return ASCORE_XFORMS_OFFSET + (size_t)XS_ALIGN_SCORE_MAX_TRANSFORMS * sizeof(AlignXform); }

struct AlignScoreArgs {
    const unsigned long long *keys;
    const float *values;
    long long scored;                            // ceil(count / stride): scored entry i is index entry stride * i
    long long stride;
    const float *svalue; const int *sweight; size_t sstep;
    int S[3];
    int transforms;
    const AlignXform *xforms;                    // [transforms], in the workspace
    int min_weight;
    float max_residual;
    char *records;                               // [tiles][nblocks]{64 doubles, 64 unsigned}
    unsigned *tickets;                           // [tiles], zero between launches
    double *out;                                 // [transforms][2]
};

__global__ void __launch_bounds__(256) k_align_score(const AlignScoreArgs g) {
    const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const unsigned nblocks = gridDim.x, bid = blockIdx.x, tile = blockIdx.y;
    const int p0 = (int)tile * ASCORE_TILE, np = min(ASCORE_TILE, g.transforms - p0);   // (the last tile may be partial: its other lanes keep zeros)
    const AlignXform *__restrict__ xforms = g.xforms + p0;
    const float top0 = (float)(g.S[0] - 1), top1 = (float)(g.S[1] - 1), top2 = (float)(g.S[2] - 1);
    double acc = 0.0;
    unsigned cnt = 0;
    const long long nchunks = (g.scored + 63) / 64;
    for (long long c = (long long)bid * 4 + wave; c < nchunks; c += 4ll * nblocks) {
        const long long i = c * 64 + lane;
        const bool valid = i < g.scored;         // (the last chunk's tail: masked, and it adds zeros)
        unsigned long long key = 0;
        float gt = 0.f;
        if (valid) { key = g.keys[i * g.stride]; gt = g.values[i * g.stride]; }
        const float fx = (float)(int)(key & 0x1fffff), fy = (float)(int)((key >> 21) & 0x1fffff), fz = (float)(int)(key >> 42);
#pragma unroll 1
        for (int j = 0; j < np; ++j) {
            const AlignXform M = xforms[__builtin_amdgcn_readfirstlane(j)];
            const float *m = M.m;
            const float g0 = ((m[0] * fx + m[1] * fy) + m[2] * fz) + m[9];
            const float g1 = ((m[3] * fx + m[4] * fy) + m[5] * fz) + m[10];
            const float g2 = ((m[6] * fx + m[7] * fy) + m[8] * fz) + m[11];
            const bool inside = valid && (g0 >= 0.f && g0 < top0) && (g1 >= 0.f && g1 < top1) && (g2 >= 0.f && g2 < top2);
            if (__ballot(inside) == 0) continue;                 // the wave misses the source: the zeros it would add change no bit
            int ws = 0, b0 = 0;
            const int *wrow[4];
            const float *vrow[4];
            float f0 = 0.f, f1 = 0.f, f2 = 0.f;
            if (inside) {
                b0 = __float2int_rd(g0);                         // 0 <= b <= S - 2: both corners of the axis are inside the source
                const int b1 = __float2int_rd(g1), b2 = __float2int_rd(g2);
                f0 = g0 - (float)b0; f1 = g1 - (float)b1; f2 = g2 - (float)b2;
#pragma unroll
                for (int d = 0; d < 4; ++d) {                    // d: bit 0 = +y, bit 1 = +z
                    const int row = g.S[1] * (b2 + (d >> 1)) + b1 + (d & 1);
                    wrow[d] = row_ptr(g.sweight, g.sstep, row);
                    vrow[d] = row_ptr(g.svalue, g.sstep, row);
                }
                int w[8];                                        // the eight loads in flight together
#pragma unroll
                for (int d = 0; d < 8; ++d) w[d] = wrow[d >> 1][b0 + (d & 1)];
                ws = w[0];
#pragma unroll
                for (int d = 1; d < 8; ++d) ws = min(ws, w[d]);
            }
            const bool heavy = inside && ws >= g.min_weight;
            if (__ballot(heavy) == 0) continue;                  // no lane passes the weight gate: no value is loaded
            float rr = 0.f;
            bool kept = false;
            if (heavy) {
                float v[8];                                      // corner d: bit 0 = +x, bit 1 = +y, bit 2 = +z
#pragma unroll
                for (int d = 0; d < 8; ++d) v[d] = vrow[d >> 1][b0 + (d & 1)];
                const float c0 = 1.0f - f0, c1 = 1.0f - f1, c2 = 1.0f - f2;
                const float x00 = v[0] * c0 + v[1] * f0, x10 = v[2] * c0 + v[3] * f0;
                const float x01 = v[4] * c0 + v[5] * f0, x11 = v[6] * c0 + v[7] * f0;
                const float y0 = x00 * c1 + x10 * f1, y1 = x01 * c1 + x11 * f1;
                const float F = y0 * c2 + y1 * f2;
                const float r = F - gt;
                kept = fabsf(r) <= g.max_residual;               // (a NaN drops)
                rr = kept ? r * r : 0.f;
            }
            const float s = wave_tree_sum_f32(rr);
            const unsigned n = (unsigned)__popcll(__ballot(kept));
            if (lane == j) { acc += (double)s; cnt += n; }
        }
    }
    score_tile_fold_and_finish(acc, cnt, g.records, g.tickets, g.out, p0, np);   // xs_score_fold.h: the waves, the record, the ticket, the last workgroup's fold
}

extern "C" size_t xs_tsdf_score_transforms_workspace_bytes(int transforms) {
    if (transforms < 1 || transforms > XS_ALIGN_SCORE_MAX_TRANSFORMS) return 0;
    const size_t tiles = ((size_t)transforms + ASCORE_TILE - 1) / ASCORE_TILE;
    return ascore_records_offset() + tiles * ASCORE_MAX_BLOCKS * ASCORE_RECORD_BYTES;
}

/* see include/xslam_amd.h */
extern "C" int xs_tsdf_score_transforms(int transforms, const xs_band_index *index, int stride, const float *src_value, const int *src_weight,
                                        size_t src_step, const int *src_res, const float *xform12xP, int min_weight, float max_residual,
                                        void *workspace, double *out2xP_dev, void *stream) {
    if (transforms < 1 || transforms > XS_ALIGN_SCORE_MAX_TRANSFORMS)
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_score_transforms: transforms outside 1 .. XS_ALIGN_SCORE_MAX_TRANSFORMS");
    if (stride < 1) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_score_transforms: stride below 1");
    if (!index || !src_value || !src_weight || !src_res || !xform12xP || !workspace || !out2xP_dev)
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_score_transforms: null pointer");
    if (index->nblocks < 1 || index->count < 0 || index->count > index->capacity || (index->count > 0 && (!index->keys || !index->values)))
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_score_transforms: the index was not built");
    for (int k = 0; k < 3; ++k)
        if (src_res[k] < 2 || src_res[k] > 65535 * 4) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_score_transforms: a source axis outside 2 .. 262140");
    if ((long long)src_res[1] * (long long)src_res[2] >= (1ll << 31)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_score_transforms: the source's rows do not fit an int");
    if (src_step % 4 != 0 || src_step < (size_t)src_res[0] * 4) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_score_transforms: bad pitch");
    if (min_weight < 1) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_score_transforms: min_weight below 1");
    if (!(max_residual > 0.f) || !isfinite(max_residual)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_score_transforms: max_residual is not finite and positive");
    for (size_t i = 0; i < (size_t)transforms * 12; ++i)
        if (!isfinite(xform12xP[i])) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_score_transforms: a map entry is not finite");
    AlignScoreArgs g;
    memset(&g, 0, sizeof(g));
    g.keys = index->keys; g.values = index->values;
    g.stride = stride; g.scored = (index->count + stride - 1) / stride;
    g.svalue = src_value; g.sweight = src_weight; g.sstep = src_step;
    for (int k = 0; k < 3; ++k) g.S[k] = src_res[k];
    g.transforms = transforms; g.min_weight = min_weight; g.max_residual = max_residual;
    // as many workgroups per tile as give every wave a chunk, at most the record workspace's 1024: a function of the index and the stride alone
    const long long nchunks = (g.scored + 63) / 64, want = (nchunks + 3) / 4;
    const unsigned nblocks = (unsigned)(want < 1 ? 1 : (want > ASCORE_MAX_BLOCKS ? ASCORE_MAX_BLOCKS : want));
    const unsigned tiles = ((unsigned)transforms + ASCORE_TILE - 1) / ASCORE_TILE;
    char *ws = static_cast<char *>(workspace);
    g.tickets = reinterpret_cast<unsigned *>(ws);
    g.xforms = reinterpret_cast<const AlignXform *>(ws + ASCORE_XFORMS_OFFSET);
    g.records = ws + ascore_records_offset();
    g.out = out2xP_dev;
    hipStream_t st = (hipStream_t)stream;
    XS_CHECK(hipMemcpyAsync(ws + ASCORE_XFORMS_OFFSET, xform12xP, (size_t)transforms * sizeof(AlignXform), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_align_score, dim3(nblocks, tiles), dim3(64, 4), 0, st, g);
    XS_CHECK(hipGetLastError());
    return 0;
}
