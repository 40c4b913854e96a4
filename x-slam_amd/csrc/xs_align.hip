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
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "xs_gn_band.h"
#include "xs_complex.h"
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
