// xs_residual.hip — the residual kernels over a dense TSDF slab for gfx950: the dual-complex
// Hessian kernel and its real-valued twin, and the six-pose Gauss-Newton pass.  Replaces TsdfFusion.cu:204-283
// (ComputeLocalTsdfHessianKernel) + :286-331 (ComputeLocalTsdf_hessian) and :335-410 + :412-447
// (ComputeLocalTsdfLossKernel / ComputeLocalTsdf_loss).
//
// The reference writes four N^3 scratch volumes (value / grad / hessian / count) and then runs
// four thrust::reduce passes over them: five full-volume passes.  Here the per-voxel terms are
// folded on chip — lane registers, wave shuffles, one LDS exchange, one record per workgroup,
// and the last workgroup adds the records in index order — so the only N^3 traffic is the 4 B
// per voxel of the dense ground-truth TSDF (algorithmic bytes 4*N^3 + 2*W*H).  Sums are kept
// in double and rounded once; thrust's float tree order is unspecified in the reference.
#include <string.h>
#include "xs_gn_band.h"   // HessArgs, the record fold, the band walk, the six-pose residual (shared with xs_band.hip)
#include "xs_mailbox.h"
#include "xs_env.h"
#include "../../include/xslam_amd.h"

// Three waves per SIMD (168 VGPRs; left alone the compiler takes 176 = two waves; four = 128 VGPRs spill): the band's dual-complex evaluation is
// VALU work that only another wave's scan can hide.  0.1035 -> 0.1005 ms at 512^3 alternating on one box; four waves 0.1215 (profiles/r06_hess_scan.txt 6).
#ifndef XS_HESS_WAVES_PER_EU
#define XS_HESS_WAVES_PER_EU 3
#endif
#define XS_HESS_OCC __attribute__((amdgpu_waves_per_eu(XS_HESS_WAVES_PER_EU, XS_HESS_WAVES_PER_EU)))
__global__ void __launch_bounds__(256) XS_HESS_OCC k_tsdf_hessian(const HessArgs a, const HessPoseD Pk) {
    __shared__ HessPoseD P;   // 48 floats of pose through LDS rather than through vector registers (see k_tsdf_gauss_newton)
    {
        const float *src = reinterpret_cast<const float *>(&Pk);
        float *dst = reinterpret_cast<float *>(&P);
        for (int i = threadIdx.y * 64 + threadIdx.x; i < (int)(sizeof(HessPoseD) / sizeof(float)); i += 256) dst[i] = src[i];
    }
    __syncthreads();
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    walk_band(a, [&](int xq, int yq, int z, size_t index, float gt) {
        dcfloat loss;
        if (!tsdf_loss_d(a, P, xq, yq, z, gt, loss)) return;   // (xs_gn_band.h: shared with k_band_pose_hessian)
        if (a.real_out) {
            a.real_out[index] = loss.value(); a.grad_out[index] = loss.grad();
            a.hess_out[index] = loss.hessian(); a.count_out[index] = 1;
        }
        acc[0] += loss.value(); acc[1] += loss.grad(); acc[2] += loss.hessian(); acc[3] += 1.0;
    });
    block_fold_and_finish<4>(acc, a.partials, a.ticket, a.out);
}

__global__ void __launch_bounds__(256) k_tsdf_loss(const HessArgs a, const HessPoseF P) {
    double acc[2] = {0.0, 0.0};
    walk_band(a, [&](int xq, int yq, int z, size_t index, float gt_tsdf) {
        float loss;
        if (!tsdf_loss_f(a, P, xq, yq, z, gt_tsdf, loss)) return;   // (xs_gn_band.h: shared with k_band_score_poses)
        if (a.real_out) { a.real_out[index] = loss; a.count_out[index] = 1; }
        acc[0] += loss; acc[1] += 1.0;
    });
    block_fold_and_finish<2>(acc, a.partials, a.ticket, a.out);
}

// ---- first-order CSFD Gauss-Newton terms of the same residual (BASELINE config 5) ----------------
// The residual of ComputeLocalTsdfHessianKernel (TsdfFusion.cu:204-283) evaluated in complex<float>
// for six poses at once — the pose seeded with i*h along each of its six degrees of freedom — so one
// pass over the volume yields, per voxel, the residual r = Re(error) and the six derivative parts
// d_k = Im(error_k) = h * dr/dtheta_k, and on chip the sums a Gauss-Newton step needs:
//   out[0..20]  sum d_j d_k (upper triangle, rows j <= k),  out[21..26]  sum d_k r,
//   out[27]     sum r^2,                                    out[28]      voxel count
// (the caller divides by h^2 / h).  The reference has no such kernel; its commented ComputeTSDF_hessian
// (KinectFusionReconstruction.cpp:404-434) takes one seeded direction per call and would need 6 passes
// and 6 N^3 scratch volumes for the same matrix.
// POSTED: the launch was enqueued before its poses existed (the host is still solving the previous pass): wave 0 polls the mailbox — six pose
// mailboxes of xs_mailbox.h in a row, written in order, so box 5 carrying the sequence number means boxes 0 .. 4 do — and fills P from it.
// A workgroup that is told to leave (cmd 1) or whose poses never come sums nothing but still takes its arrival ticket, marked: the launch's last
// workgroup then publishes the sequence number with bit 63 set instead of sums (block_fold_and_finish) — one record per launch whatever happened,
// and the ticket back at zero.
#ifdef XS_GN_WAVES_PER_EU   // experiment switch (three waves per SIMD = 168 VGPRs spill 31 registers here: 206 -> 172 relocalisations/s; left at the compiler's 228 = two waves)
#define XS_GN_OCC __attribute__((amdgpu_waves_per_eu(XS_GN_WAVES_PER_EU, XS_GN_WAVES_PER_EU)))
#else
#define XS_GN_OCC
#endif
template <bool POSTED>
__global__ void __launch_bounds__(256) XS_GN_OCC k_tsdf_gauss_newton(const HessArgs a, const GnPoses Pk) {
    // The six poses (144 floats) do not fit the scalar registers next to everything else, and the compiler then keeps them
    // in vector registers for the whole kernel (256 of them: one wave per SIMD).  They go through LDS instead: broadcast
    // reads where an evaluation needs them.
    __shared__ GnPoses P;
    bool left = false;
    if constexpr (POSTED) {
        __shared__ unsigned s_mail[xs::MAILBOX_WORDS];
        __shared__ unsigned s_cmd;
        if (threadIdx.y == 0) {
            const int lane = threadIdx.x;
            const unsigned long long t_resident = wall_clock64();   // (100 MHz: what this launch waits for its poses is the host's side of the loop)
            // (a workgroup of this launch has left already — told to, or it waited its second out: the ones that become resident later do not wait theirs)
            const bool somebody_left = (__hip_atomic_load(a.ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 16) != 0;
            if (!somebody_left) xs::mailbox_wait(a.mailbox + 5 * xs::MAILBOX_WORDS, a.mailbox_seq, s_mail, lane);
            if (a.publish && blockIdx.x == 0 && lane == 0)   // word [30] of the record: ticks from resident to poses seen (the record's sequence word follows ~0.8 ms later)
                __hip_atomic_store(&a.publish[30], (double)(wall_clock64() - t_resident), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            unsigned cmd = somebody_left ? 1u : (unsigned)__builtin_amdgcn_readfirstlane((int)s_mail[1]);
            float *dst = reinterpret_cast<float *>(&P);
            for (int k = 0; k < 6 && cmd == 0; ++k) {   // (issued after box 5's sequence words were seen: complete payloads)
                const unsigned w = __hip_atomic_load(a.mailbox + k * xs::MAILBOX_WORDS + (lane & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                const unsigned s0 = __builtin_amdgcn_readlane(w, 0), s1 = __builtin_amdgcn_readlane(w, 8), s2 = __builtin_amdgcn_readlane(w, 16),
                               s3 = __builtin_amdgcn_readlane(w, 24);
                if (s0 != a.mailbox_seq || s1 != a.mailbox_seq || s2 != a.mailbox_seq || s3 != a.mailbox_seq) { cmd = 2; break; }
                const int f = xs::mailbox_float_of(lane & 31);   // (xs_mailbox.h: four sectors, each {seq, payload})
                if (lane < 32 && f >= 0) dst[f < 18 ? 18 * k + f : 108 + 6 * k + (f - 18)] = __uint_as_float(w);
            }
            if (lane == 0) s_cmd = cmd;
        }
        __syncthreads();
        left = s_cmd != 0;   // (the workgroup still arrives: block_fold_and_finish)
    } else {
        const float *src = reinterpret_cast<const float *>(&Pk);
        float *dst = reinterpret_cast<float *>(&P);
        for (int i = threadIdx.y * 64 + threadIdx.x; i < (int)(sizeof(GnPoses) / sizeof(float)); i += 256) dst[i] = src[i];
        __syncthreads();
    }
    double acc[29];
#pragma unroll
    for (int k = 0; k < 29; ++k) acc[k] = 0.0;
    if (!left) walk_band(a, [&](int xq, int yq, int z, size_t, float gt) { gn_terms_add(a, P, xq, yq, z, gt, acc); });
    block_fold_and_finish<29>(acc, a.partials, a.ticket, a.out, a.publish, a.publish_seq, left);
}

enum { XS_TSDF_REDUCE_MAX_BLOCKS = XS_TSDF_REDUCE_MAX_BLOCKS_C };
extern "C" size_t xs_tsdf_reduce_workspace_bytes(void) { return (size_t)XS_TSDF_REDUCE_MAX_BLOCKS * 32 * sizeof(double) + 256; }
/* Zero the workspace's arrival ticket once after allocation (any zero fill of the first 256 bytes does): every launch of the three residual kernels
 * leaves it zero — their last workgroup resets it — so a launch needs no fill of its own (round 6: that fill was a dispatch in front of every pass).
 * One launch at a time per workspace.  After a launch that did not complete (a device fault), initialise again. */
extern "C" int xs_tsdf_reduce_workspace_init(void *workspace, void *stream) {
    if (!workspace) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_reduce_workspace_init: null pointer");
    XS_CHECK(hipMemsetAsync(workspace, 0, 256, (hipStream_t)stream));
    return 0;
}

static int hess_common(HessArgs &a, const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4, const int *res,
                       float voxel_size, float tranc_dist, const float *gt, int z0, int z1, void *workspace, double *out_dev, dim3 &grid,
                       void *stream, bool heavy_body) {
    if (!depth_scaled || !intr4 || !res || !gt || !workspace || !out_dev) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_hessian/loss: null pointer");
    if (z0 < 0 || z1 > res[2] || z1 <= z0) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_hessian/loss: bad slab");
    a.depth = depth_scaled; a.dstep = scaled_step; a.drows = rows; a.dcols = cols;
    a.voxel_size = voxel_size; a.tranc_dist = tranc_dist; a.tranc_dist_inv = 1.0f / tranc_dist;
    a.intr = Intr{intr4[0], intr4[1], intr4[2], intr4[3]};
    a.publish = nullptr; a.publish_seq = 0; a.mailbox = nullptr; a.mailbox_seq = 0;
    a.ticket = (unsigned *)workspace; a.partials = (double *)((char *)workspace + 256); a.out = out_dev;
    return hess_tiling(a, res, gt, z0, z1, grid, heavy_body);
}
// The walk's shape for the slab [z0, z1) of gt (the band index of xs_band.hip records the same walk: it calls this with heavy_body = true)
int hess_tiling(HessArgs &a, const int *res, const float *gt, int z0, int z1, dim3 &grid, bool heavy_body) {
    a.X = res[0]; a.Y = res[1]; a.Z = res[2]; a.z0 = z0; a.z1 = z1;
    a.gt = gt;
    // Tiles of 64 x 4 columns x zchunk planes, one column per lane (256 x 4 with four columns per lane: a.wide); the workgroups stride
    // over them.  (While every workgroup paid an L2 write-back for its record, 4096 of them halved the streaming rate against 1024; the
    // records now leave with write-through stores: block_fold_and_finish.)
    static const int env_blocks = exp_env_int("XS_HESS_BLOCKS", 0);  // tuning aid
    static const bool env_narrow = exp_env_set("XS_HESS_NARROW");    // A/B aid: the one-column-per-lane scan whatever the shape
    // sixteen bytes per lane where the rows allow it (for_band_voxels_wide): X a multiple of four and the slab's first voxel 16-byte aligned
    // Which planes a workgroup takes: runs of consecutive planes stream fastest (eight ADJACENT planes per request: 6.1 TB/s scan alone at
    // 512^3 against 5.7 for planes four apart), but a band is a thin sheet and a wall across z then lies in ONE workgroup's run per column — the
    // kernels whose band voxels are expensive (dual-complex Hessian, six-pose Gauss-Newton) take five interleaved groups of planes (below), the
    // loss kernel takes runs (profiles/r06_hess_scan.txt).
    static const int env_ilg = exp_env_int("XS_HESS_IL", 1);   // tuning aid: consecutive planes a group takes together (pairs measured the same or worse)
    a.il = (env_ilg == 2 || env_ilg == 4 || env_ilg == 8) ? env_ilg : 1;
    static const int env_il = exp_env_int("XS_HESS_INTERLEAVE", -1);   // A/B aid: 0 = runs, 1 = interleaved, whatever the kernel
    const bool interleave = env_il < 0 ? heavy_body : env_il != 0;
    a.wide = (a.X % 4 == 0 && (reinterpret_cast<uintptr_t>(gt) % 16) == 0 && !env_narrow) ? (interleave ? 2 : 1) : 0;
    int gx = div_up(a.X, a.wide ? 256 : 64), gy = div_up(a.Y, 4), nz = z1 - z0, zsplit = 1;
    // one workgroup per column of tiles while that gives 1024 .. 4096 of them (512^3: 1024, 1024^3: 4096 — measured best:
    // the Gauss-Newton pass at 1024^3 runs 15 % faster with 4096 workgroups walking one column each than with 1024 walking
    // four); fewer columns are split along z, more are strided over
    const long long cols_xy = (long long)gx * gy;
    // (in the bare scan 4096 workgroups streamed 4 % faster than 1024; in the kernels, which pay a record and a ticket per workgroup, 8-12 % slower)
    const int cap = env_blocks > 0 && env_blocks <= XS_TSDF_REDUCE_MAX_BLOCKS ? env_blocks
                    : a.wide == 2 ? (int)XS_TSDF_REDUCE_MAX_BLOCKS   // (one workgroup per tile up to 4096: 512^3 has 1024 tiles, 1024^3 4096)
                    : a.wide ? (int)(cols_xy < 1024 ? 1024 : (cols_xy > XS_TSDF_REDUCE_MAX_BLOCKS ? XS_TSDF_REDUCE_MAX_BLOCKS : cols_xy))
                    : (int)(cols_xy < 1024 ? 1024 : (cols_xy > XS_TSDF_REDUCE_MAX_BLOCKS ? XS_TSDF_REDUCE_MAX_BLOCKS : cols_xy));
    if (a.wide == 2) {
        // FIVE z groups per column of tiles, their planes interleaved one by one (a tile: 256 x 4 columns x every fifth plane).  A kernel is as
        // slow as its busiest wave, and a wave that lies IN a surface holds nothing but band voxels: a wall across z is a sheet one or two planes
        // thick — plane by plane it goes to different groups; a floor (a wall along z and x) fills whole rows of a column — with whole columns per
        // wave (round 5: 64 x 1024 voxels at 1024^3; 256 x 1024 with four columns per lane) the box room's floor kept a few dozen waves busy long
        // after the rest had left: 0.89 ms per Gauss-Newton pass of the relocalisation workload then, 2.0 ms with four columns per lane and whole
        // columns, 0.80 ms now.  More, smaller groups balance better and stream worse (32-plane groups: 0.139 ms for the Hessian kernel at 512^3
        // against 0.097).  FIVE, not four: the eight requests of a batch lie G planes apart, and with a power of two between them (4 MiB at 512^3,
        // 16 MiB at 1024^3) the scan alone loses 10 % at 512^3 (0.098 against 0.087 ms with three or six groups: the requests of a lane fall on the
        // same memory channels) — five keeps the balance of four and the rate of an odd stride: Gauss-Newton 1024^3 0.79 -> 0.73 ms, relocalisation
        // 206 -> 209 frames/s, Hessian 512^3 0.098 -> 0.097 (profiles/r06_hess_scan.txt 5, 7).  Workgroup b takes tiles b, b + grid, ... of an
        // enumeration with the z group fastest, skewed by one group per round (walk_band).
        static const int env_zt = exp_env_int("XS_HESS_TILE_PLANES", 0);   // tuning aid: planes per group
        int G = nz >= 80 ? 5 : (nz >= 48 ? 3 : (nz >= 24 ? 2 : 1));
        if (env_zt >= 8) { G = 1; while (G * 2 * env_zt <= nz) G *= 2; }
        static const int env_g = exp_env_int("XS_HESS_GROUPS", 0);   // tuning aid: G itself (any number)
        if (env_g >= 1 && env_g * 8 <= nz) G = env_g;
        a.tiles_x = gx; a.tiles_y = gy; a.tiles_z = G; a.zchunk = div_up(nz, G);
    } else {
        while ((long long)gx * gy * zsplit < cap && zsplit < nz && nz / (zsplit * 2) >= 16) zsplit *= 2;
        a.zchunk = div_up(nz, zsplit);
        a.tiles_x = gx; a.tiles_y = gy; a.tiles_z = div_up(nz, a.zchunk);
    }
    const long long ntiles = (long long)a.tiles_x * a.tiles_y * a.tiles_z;
    grid = dim3((unsigned)(ntiles < cap ? ntiles : cap));
    if ((long long)grid.x * grid.y * grid.z > XS_TSDF_REDUCE_MAX_BLOCKS) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_hessian/loss: volume too large for the reduce workspace");
    return 0;
}

/* float4 ComputeLocalTsdf_hessian(const PtrStepSz<ushort>& depth, const Intr&, DeviceArray2D<float>& depthScaled,
 *     const int3& res, float voxel_size, const MatD33& Rv2c, const devDComplex3& tv2c, float tranc_dist,
 *     float threshold, float k, thrustDvec<float>& gt, real, grad, hessian, thrustDvec<int>& count)
 *                                                        TsdfFusion.h:55-60, TsdfFusion.cu:286-331
 * depth_scaled: output of xs_scale_depth.  Rv2c36 / tv2c12: MatD33 / devDComplex3 as groups of
 * (re.re, re.im, im.re, im.im).  gt: dense unpitched TSDF of the slab [z0, z1).  out4_dev: 4
 * doubles {loss, grad, hessian, count} (the reference returns them narrowed to float4).  The
 * four per-voxel volumes are optional (all four or none).  threshold and k are unused by the
 * reference kernel.  No synchronisation. */
extern "C" int xs_compute_local_tsdf_hessian(const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4,
                                             const int *res, float voxel_size, const float *Rv2c36, const float *tv2c12,
                                             float tranc_dist, const float *gt, float *real_out, float *grad_out, float *hess_out,
                                             int *count_out, int z0, int z1, void *workspace, double *out4_dev, void *stream) {
    HessArgs a; dim3 grid;
    int rc = hess_common(a, depth_scaled, scaled_step, rows, cols, intr4, res, voxel_size, tranc_dist, gt, z0, z1, workspace, out4_dev, grid, stream, true);
    if (rc) return rc;
    if (!Rv2c36 || !tv2c12) return xs_set_error(hipErrorInvalidValue, "xs_compute_local_tsdf_hessian: null pose");
    const bool all = real_out && grad_out && hess_out && count_out, none = !real_out && !grad_out && !hess_out && !count_out;
    if (!all && !none) return xs_set_error(hipErrorInvalidValue, "xs_compute_local_tsdf_hessian: pass all four volumes or none");
    a.real_out = real_out; a.grad_out = grad_out; a.hess_out = hess_out; a.count_out = count_out;
    HessPoseD P;
    for (int r = 0; r < 3; ++r) {
        const float *p = Rv2c36 + r * 12;
        P.R.data[r].x = dcfloat(p[0], p[1], p[2], p[3]);
        P.R.data[r].y = dcfloat(p[4], p[5], p[6], p[7]);
        P.R.data[r].z = dcfloat(p[8], p[9], p[10], p[11]);
    }
    P.t.x = dcfloat(tv2c12[0], tv2c12[1], tv2c12[2], tv2c12[3]);
    P.t.y = dcfloat(tv2c12[4], tv2c12[5], tv2c12[6], tv2c12[7]);
    P.t.z = dcfloat(tv2c12[8], tv2c12[9], tv2c12[10], tv2c12[11]);
    hipLaunchKernelGGL(k_tsdf_hessian, grid, dim3(64, 4), 0, (hipStream_t)stream, a, P);
    XS_CHECK(hipGetLastError());
    return 0;
}

/* float2 ComputeLocalTsdf_loss(..., const Mat33& Rv2c, const float3& tv2c, ..., gt, real, count)
 *                                                        TsdfFusion.h:48-52, TsdfFusion.cu:412-447
 * out2_dev: {loss, count} as doubles. */
extern "C" int xs_compute_local_tsdf_loss(const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4,
                                          const int *res, float voxel_size, const float *Rv2c9, const float *tv2c3, float tranc_dist,
                                          const float *gt, float *real_out, int *count_out, int z0, int z1, void *workspace,
                                          double *out2_dev, void *stream) {
    HessArgs a; dim3 grid;
    int rc = hess_common(a, depth_scaled, scaled_step, rows, cols, intr4, res, voxel_size, tranc_dist, gt, z0, z1, workspace, out2_dev, grid, stream, false);
    if (rc) return rc;
    if (!Rv2c9 || !tv2c3) return xs_set_error(hipErrorInvalidValue, "xs_compute_local_tsdf_loss: null pose");
    if ((real_out == nullptr) != (count_out == nullptr)) return xs_set_error(hipErrorInvalidValue, "xs_compute_local_tsdf_loss: pass both volumes or none");
    a.real_out = real_out; a.grad_out = nullptr; a.hess_out = nullptr; a.count_out = count_out;
    HessPoseF P;
    for (int i = 0; i < 9; ++i) P.R[i] = Rv2c9[i];
    for (int i = 0; i < 3; ++i) P.t[i] = tv2c3[i];
    hipLaunchKernelGGL(k_tsdf_loss, grid, dim3(64, 4), 0, (hipStream_t)stream, a, P);
    XS_CHECK(hipGetLastError());
    return 0;
}

/* First-order CSFD Gauss-Newton terms of the Hessian kernel's residual for six seeded poses in one pass
 * (BASELINE config 5; no counterpart launcher in the reference).  Rv2c108 / tv2c36: six MatS33 / devComplex3
 * (pose k carries i*h on degree of freedom k; real parts equal).  out29_dev: 29 doubles — sum d_j d_k for
 * j <= k (21, row-major upper triangle), sum d_k r (6), sum r^2, count — with d_k = Im(error_k), r =
 * Re(error_0); voxels are those with gt != 0, |gt| <= 0.95 that pass the kernel's gates for all six poses.
 * gt / depth_scaled / slab arguments as xs_compute_local_tsdf_hessian.  No synchronisation. */
extern "C" int xs_tsdf_gauss_newton_terms(const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4, const int *res,
                                          float voxel_size, const float *Rv2c108, const float *tv2c36, float tranc_dist, const float *gt, int z0,
                                          int z1, void *workspace, double *out29_dev, void *stream) {
    return xs_tsdf_gauss_newton_terms_ex(depth_scaled, scaled_step, rows, cols, intr4, res, voxel_size, Rv2c108, tv2c36, tranc_dist, gt, z0, z1, workspace,
                                         out29_dev, nullptr, stream);
}
/* ... with the loop protocol of the ICP iterations (opts; NULL = none of it):
 *   publish_host / publish_seq   host-coherent pinned memory of xs_gn_publish_bytes(): the last workgroup stores the 29 sums there and then the
 *                                64-bit word [32] = publish_seq — the host spins on that word instead of copying and draining the stream;
 *   pose_mailbox / mailbox_seq   Rv2c108 / tv2c36 NULL: the launch is enqueued before its poses exist and takes them from the mailbox
 *                                (xs_icp_mailbox_alloc; xs_gn_post_poses writes it).  cmd 1 or a pose that never comes (about a second): nothing is
 *                                summed, publish word = publish_seq | 1 << 63. */
extern "C" int xs_tsdf_gauss_newton_terms_ex(const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4, const int *res,
                                             float voxel_size, const float *Rv2c108, const float *tv2c36, float tranc_dist, const float *gt, int z0,
                                             int z1, void *workspace, double *out29_dev, const xs_gn_opts *opts, void *stream) {
    if (opts && opts->struct_bytes != sizeof(xs_gn_opts)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_gauss_newton_terms_ex: opts->struct_bytes is not sizeof(xs_gn_opts)");
    HessArgs a; dim3 grid;
    int rc = hess_common(a, depth_scaled, scaled_step, rows, cols, intr4, res, voxel_size, tranc_dist, gt, z0, z1, workspace, out29_dev, grid, stream, true);
    if (rc) return rc;
    const bool posted = opts && opts->pose_mailbox && !Rv2c108 && !tv2c36;
    if (!posted && (!Rv2c108 || !tv2c36)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_gauss_newton_terms: give the six poses or a mailbox");
    a.real_out = nullptr; a.grad_out = nullptr; a.hess_out = nullptr; a.count_out = nullptr;
    if (opts) { a.publish = opts->publish_host; a.publish_seq = opts->publish_seq; }
    GnPoses P;
    memset(&P, 0, sizeof(P));
    if (posted) {
        a.mailbox = static_cast<const unsigned *>(opts->pose_mailbox); a.mailbox_seq = opts->mailbox_seq;
        hipLaunchKernelGGL(k_tsdf_gauss_newton<true>, grid, dim3(64, 4), 0, (hipStream_t)stream, a, P);
    } else {
        for (int k = 0; k < 6; ++k) { load_mat(Rv2c108 + 18 * k, P.R[k]); load_vec(tv2c36 + 6 * k, P.t[k]); }
        hipLaunchKernelGGL(k_tsdf_gauss_newton<false>, grid, dim3(64, 4), 0, (hipStream_t)stream, a, P);
    }
    XS_CHECK(hipGetLastError());
    return 0;
}
extern "C" size_t xs_gn_publish_bytes(void) { return 33 * sizeof(double); }
extern "C" size_t xs_gn_mailbox_bytes(void) { return 6 * xs::MAILBOX_WORDS * sizeof(unsigned); }
/* Host: the six seeded poses (or a command: cmd 1 = leave) for the launch that polls `mailbox_host` for `mailbox_seq` — six mailboxes of the
 * xs_icp_post_pose layout in a row, posted as one (mailbox_post, xs_mailbox.h: the launch polls the LAST box and then reads all six, checking
 * each one's sequence words). */
extern "C" void xs_gn_post_poses(void *mailbox_host, const float *Rv2c108, const float *tv2c36, unsigned mailbox_seq, int cmd) {
    alignas(64) unsigned img[6][xs::MAILBOX_WORDS];
    for (int k = 0; k < 6; ++k) mailbox_image(img[k], Rv2c108 ? Rv2c108 + 18 * k : nullptr, tv2c36 ? tv2c36 + 6 * k : nullptr, mailbox_seq, cmd);
    mailbox_post(mailbox_host, img, 6);
}
__global__ void k_publish_sums(const double *sums, int n, double *publish, unsigned long long seq) {
    const int tid = threadIdx.x;
    if (tid < n) __hip_atomic_store(&publish[tid], sums[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    if (tid == 0) __hip_atomic_store(reinterpret_cast<unsigned long long *>(publish) + 32, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
/* Shard mode: the sums as they stand in device memory AFTER the stream's all-reduce, published the same way (n <= 32 doubles, then word [32] = seq). */
extern "C" int xs_gn_publish_sums(const double *sums_dev, int n, double *publish_host, unsigned long long seq, void *stream) {
    if (!sums_dev || !publish_host || n < 1 || n > 32) return xs_set_error(hipErrorInvalidValue, "xs_gn_publish_sums: bad argument");
    hipLaunchKernelGGL(k_publish_sums, dim3(1), dim3(64), 0, (hipStream_t)stream, sums_dev, n, publish_host, seq);
    XS_CHECK(hipGetLastError());
    return 0;
}
