// xs_reintegrate.hip — fused frames taken out of the TSDF volume and fused again, for gfx950: observations applied with a sign through the
// per-voxel contract of the integrate kernels (xs_integrate_voxel.h).  No reference counterpart.
#include <string.h>
#include <cmath>
#include "xs_device.h"
#include "xs_integrate_voxel.h"
#include "xs_integrate_args.h"
#include "../../include/xslam_amd.h"

using namespace xs;

// ---- observations applied with a sign (xs_tsdf_reintegrate) ---------------------------------------------------------
// One pass over the planes for up to XS_REINTEGRATE_MAX_OPS observations.  A workgroup is a tile of 64 (x) x 4 (y) x REINT_TZ (z) voxels, a wave
// one row of it: lanes along x, every volume access a 256-byte row segment, a thread walks the tile's planes.  The op table is a kernel argument:
// the ops loop is the outer one and runs over a wave-uniform bit mask (the ops whose frustum can see the wave's box), pose and image pointer of the
// op in hand are scalar loads from the argument segment, once per op and tile.  The column's states (3 x REINT_TZ words) are requested before the
// first op's projection and stay in registers across the ops; an op's observation is voxel_ctx / project_voxel / voxel_tsdf as the integrate
// kernels call them, the +1 update is running_mean itself.
enum { REINT_TZ = 8 };
struct ReintOp { Frustum fr; MatS33 R; cfloat3 t; const float *depth; int sign, pad_; };
struct ReintArgs {
    ReintOp op[XS_REINTEGRATE_MAX_OPS];
    int ops; unsigned flags;
    size_t dstep; int drows, dcols;
    float *value; int *weight; float *grad; size_t vstep;
    int X, Y, z0, z1;
    float tranc_dist, tranc_dist_inv; int max_weight;
    Intr intr; float voxel_size, threshold;
    unsigned long long *counts;
};
static_assert(sizeof(ReintArgs) <= 4096, "the op table travels in the kernel's arguments");
template <bool BILINEAR>
__global__ void __launch_bounds__(256) k_reintegrate(const ReintArgs g) {
    const int zb = g.z0 + blockIdx.z * REINT_TZ, ze = min(zb + REINT_TZ, g.z1);
    const int x0 = blockIdx.x * 64, x1 = min(x0 + 64, g.X), y0 = blockIdx.y * 4;
    const bool cull = !(g.flags & XS_REINTEGRATE_NO_CULL);
    // the workgroup's box first: a tile no op can see leaves here, every thread of it (uniform: block indices alone)
    unsigned wg_seen = 0;
    for (int i = 0; i < g.ops; ++i)
        if (!cull || box_may_pass(g.op[i].fr, x0, x1, y0, min(y0 + 4, g.Y), zb, ze)) wg_seen |= 1u << i;
    if (wg_seen == 0) return;
    const int x = threadIdx.x + x0;
    const int y = __builtin_amdgcn_readfirstlane(threadIdx.y) + y0;   // (a wave is one row: uniform)
    unsigned seen_by = 0;   // bit i: op i's frustum may see the wave's box — wave-uniform
    if (y < g.Y)
        for (unsigned m = wg_seen; m != 0; m &= m - 1) {
            const int i = __builtin_ctz(m);
            if (!cull || box_may_pass(g.op[i].fr, x0, x1, y, y + 1, zb, ze)) seen_by |= 1u << i;
        }
    unsigned n_removed = 0, n_added = 0, n_emptied = 0, n_orphaned = 0;
    if (seen_by != 0 && x < g.X) {
        IntegrateArgs a;   // what the per-voxel functions read of it
        a.drows = g.drows; a.dcols = g.dcols; a.intr = g.intr; a.voxel_size = g.voxel_size; a.threshold = g.threshold;
        a.tranc_dist = g.tranc_dist; a.tranc_dist_inv = g.tranc_dist_inv;
        const size_t plane = (size_t)g.Y * g.vstep;
        const size_t off = ((size_t)(zb - g.z0) * g.Y + y) * g.vstep + (size_t)x * 4;   // bytes, 64 bits: rows lie past 2^31 bytes
        char *const bv = reinterpret_cast<char *>(g.value) + off, *const bw = reinterpret_cast<char *>(g.weight) + off, *const bg = reinterpret_cast<char *>(g.grad) + off;
        const int nz = ze - zb;
        // the tile's column of states, all requested before the first projection: 3 x REINT_TZ loads in flight under it
        float v[REINT_TZ], gr[REINT_TZ];
        int w[REINT_TZ];
#pragma unroll
        for (int j = 0; j < REINT_TZ; ++j) {
            v[j] = 0.0f; gr[j] = 0.0f; w[j] = 0;
            if (j < nz) {
                v[j] = *reinterpret_cast<const float *>(bv + j * plane);
                w[j] = *reinterpret_cast<const int *>(bw + j * plane);
                gr[j] = *reinterpret_cast<const float *>(bg + j * plane);
            }
        }
        unsigned dirty = 0;   // bit j: an op changed the value word of plane j; bit 8 + j: the weight; bit 16 + j: the grad
        for (unsigned m = seen_by; m != 0; m &= m - 1) {
            const ReintOp &op = g.op[__builtin_ctz(m)];
            const PoseRT ps{op.R, op.t};   // (scalar registers: once per op and tile)
            const VoxelCtx k = voxel_ctx(a, ps, x, y);
            const DepthGlobal dimg{op.depth, g.dstep};
            const int sign = op.sign;
#pragma unroll
            for (int j = 0; j < REINT_TZ; ++j) {
                if (j < nz) {
                    VoxelProj p;
                    cfloat t;
                    if (project_voxel<BILINEAR>(a, ps, k, zb + j, p, dimg) && voxel_tsdf(a, k, p, t)) {
                        const float pv = v[j], pg = gr[j];
                        const int pw = w[j];
                        if (sign > 0) {
                            running_mean(g.max_weight, t, pv, pg, pw, v[j], gr[j], w[j]);
                            ++n_added;
                        } else if (pw >= 2) {
                            const cfloat num = unpack_tsdf(pv, pg) * __int2float_rn(pw) - 1.0f * t;
                            // as in running_mean: x / x is exactly 1 and 0 / x exactly 0 (sign kept; den > 0), so free space taken out of free
                            // space — (1 w - 1) / (w - 1), grad 0 — skips both divides, wave by wave
                            float qv, qg;
                            mean_divide(num, __int2float_rn(pw - 1), qv, qg);
                            v[j] = fminf(fmaxf(qv, -1.0f), 1.0f); gr[j] = qg;
                            w[j] = pw - 1;
                            ++n_removed;
                        } else if (pw == 1) {
                            v[j] = 0.0f; gr[j] = 0.0f; w[j] = 0;
                            ++n_removed; ++n_emptied;
                        } else ++n_orphaned;
                        if (__float_as_uint(v[j]) != __float_as_uint(pv)) dirty |= 1u << j;
                        if (w[j] != pw) dirty |= 1u << (8 + j);
                        if (__float_as_uint(gr[j]) != __float_as_uint(pg)) dirty |= 1u << (16 + j);
                    }
                }
            }
        }
        // only words an op changed are stored
#pragma unroll
        for (int j = 0; j < REINT_TZ; ++j) {
            if (dirty & (1u << j)) *reinterpret_cast<float *>(bv + j * plane) = v[j];
            if (dirty & (1u << (8 + j))) *reinterpret_cast<int *>(bw + j * plane) = w[j];
            if (dirty & (1u << (16 + j))) *reinterpret_cast<float *>(bg + j * plane) = gr[j];
        }
    }
    // one add per counter and workgroup
    __shared__ unsigned s_cnt[4][4];
    const unsigned sums[4] = {wave_sum_u32(n_removed), wave_sum_u32(n_added), wave_sum_u32(n_emptied), wave_sum_u32(n_orphaned)};
    if (threadIdx.x == 0)
        for (int c = 0; c < 4; ++c) s_cnt[c][threadIdx.y] = sums[c];
    __syncthreads();
    if (threadIdx.y == 0 && threadIdx.x < 4) {
        const unsigned t = (s_cnt[threadIdx.x][0] + s_cnt[threadIdx.x][1]) + (s_cnt[threadIdx.x][2] + s_cnt[threadIdx.x][3]);
        if (t) atomicAdd(g.counts + threadIdx.x, (unsigned long long)t);
    }
}

extern "C" int xs_tsdf_reintegrate(int ops, const xs_reintegrate_op *ops_host, size_t scaled_step, int rows, int cols, const float *intr4,
                                   int max_weight, const int *res, float voxel_size, float tranc_dist, float threshold,
                                   float *value, int *weight, float *grad, size_t vol_step, int z0, int z1,
                                   unsigned long long *counts4_dev, unsigned flags, void *stream) {
    if (ops < 1 || ops > XS_REINTEGRATE_MAX_OPS) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_reintegrate: ops outside 1 .. XS_REINTEGRATE_MAX_OPS");
    if (!ops_host || !intr4 || !res || !value || !weight || !grad || !counts4_dev) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_reintegrate: null pointer");
    for (int a = 0; a < 3; ++a)
        if (res[a] < 1 || res[a] > 262140) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_reintegrate: an axis outside 1 .. 262140");
    if (z0 < 0 || z1 > res[2] || z1 <= z0 || (vol_step % 4) != 0 || vol_step < (size_t)res[0] * 4)
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_reintegrate: bad plane range or pitch");
    if (max_weight < 1 || max_weight > (1 << 24)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_reintegrate: max_weight outside [1, 1 << 24]");
    if (!(voxel_size > 0.f) || !std::isfinite(voxel_size) || !(tranc_dist > 0.f) || !std::isfinite(tranc_dist))
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_reintegrate: voxel_size or tranc_dist not positive and finite");
    ReintArgs g;
    memset(&g, 0, sizeof(g));
    for (int i = 0; i < ops; ++i) {
        const xs_reintegrate_op &o = ops_host[i];
        if (o.sign != 1 && o.sign != -1) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_reintegrate: a sign other than +1 or -1");
        if (!o.depth_scaled) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_reintegrate: null image");
        for (int k = 0; k < 18; ++k)
            if (!std::isfinite(o.Rv2c18[k])) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_reintegrate: a pose entry is not finite");
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(o.tv2c6[k])) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_reintegrate: a pose entry is not finite");
        IntegrateArgs a;   // the op's padded frustum, as the integrate kernels build it, closed at the far limit of a 5 m depth (far_limit without a frame maximum)
        integrate_args(a, rows, cols, intr4, res, voxel_size, o.Rv2c18, o.tv2c6, tranc_dist, z0, z1, nullptr);
        a.fr.alpha[5] += 5.0f * 1.0001f + 1.05f * tranc_dist;
        g.op[i].fr = a.fr; g.op[i].R = a.R; g.op[i].t = a.t; g.op[i].depth = o.depth_scaled; g.op[i].sign = o.sign;
    }
    g.ops = ops; g.flags = flags;
    g.dstep = scaled_step; g.drows = rows; g.dcols = cols;
    g.value = value; g.weight = weight; g.grad = grad; g.vstep = vol_step;
    g.X = res[0]; g.Y = res[1]; g.z0 = z0; g.z1 = z1;
    g.tranc_dist = tranc_dist; g.tranc_dist_inv = 1.0f / tranc_dist; g.max_weight = max_weight;
    g.intr = Intr{intr4[0], intr4[1], intr4[2], intr4[3]}; g.voxel_size = voxel_size; g.threshold = threshold;
    g.counts = counts4_dev;
    const dim3 grid(div_up(res[0], 64), div_up(res[1], 4), div_up(z1 - z0, REINT_TZ)), block(64, 4);
    if (threshold > 0.0f) hipLaunchKernelGGL(k_reintegrate<true>, grid, block, 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(k_reintegrate<false>, grid, block, 0, (hipStream_t)stream, g);
    XS_CHECK(hipGetLastError());
    return 0;
}
