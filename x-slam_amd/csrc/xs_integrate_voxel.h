// xs_integrate_voxel.h — the per-voxel fusion contract that the integrate kernels (xs_integrate.hip), the box classifier
// (xs_integrate_classify.hip) and signed re-integration (xs_reintegrate.hip) share: the brick geometry, the launch arguments, the frustum
// and its column clip, and the reference's per-voxel body (TsdfFusion.cu:110-168) in the pieces the kernels call.
#pragma once
#include "xs_device.h"
#include "xs_signmap.h"
#include "xs_depth_tiles.h"

using namespace xs;   // (Frustum, ClipPlanes and IntegrateArgs stay at global scope: they are part of the kernels' mangled names)

// Brick geometry: 64 (x) x 4 (y) x 8 (z) voxels = one 256-thread workgroup, lane = x, so every
// volume access of a wave is one 256-byte row segment.
#ifndef XS_BRICK_X
#define XS_BRICK_X 32
#endif
enum { BRICK_X = XS_BRICK_X, BRICK_Y = 256 / XS_BRICK_X, BRICK_Z = 8 };   // thread t of the workgroup: column t % BRICK_X, row t / BRICK_X

// Half-spaces of the (padded) view frustum in the volume's voxel-index space, built on the
// host and passed as kernel arguments (wave-uniform: they live in scalar registers).  Along any
// direction the camera-frame position is affine in the voxel index (real parts), so each side
// of the image window, the camera plane and the far limit is
//     alpha + bx*i + by*j + bz*k >= -slack,   (i, j, k) = voxel index + 0.5.
// The window is the reference's in-image test (TsdfFusion.cu:123-124) padded by three pixels,
// the slack is 2e-3 of the term magnitudes: voxels outside provably fail the exact tests;
// voxels inside still take them.  Plane 5 is the far limit c <= cfar; cfar comes from the
// frame's largest depth on the device (alpha[5] holds everything but cfar).
struct Frustum {
    float alpha[6], bx[6], by[6], bz[6], slack[6];
};

// The same half-spaces solved for k, as the column clip wants them: plane p bounds k at
//     root_p(i, j) = A + B*i + C*j     (kind +1: k >= root, -1: k <= root),
// or, where the plane does not depend on k (kind 0), excludes the column when A + B*i + C*j < 0.
// A already holds the slack.  Three scalars per plane instead of six: the integrate kernels are
// short of scalar registers (72 at eight waves per SIMD).
struct ClipPlanes {
    float A[6], B[6], C[6];
    float far_scale;  // what a unit of the far limit adds to A[5]
    int kinds;        // two bits per plane: 0 = no k dependence, 1 = lower bound, 2 = upper bound
};

struct IntegrateArgs {
    Frustum fr;
    ClipPlanes cp;
    const float *depth; size_t dstep; int drows, dcols;
    float *value; int *weight; float *grad; size_t vstep;
    int X, Y, Z;        // full resolution
    int z0, z1;         // slab owned by this launch; storage starts at z0
    int zchunk;         // z range per blockIdx.z (column-walk kernel)
    float tranc_dist, tranc_dist_inv; int max_weight;
    MatS33 R; cfloat3 t;
    Intr intr; float voxel_size, threshold;
    unsigned long long *updated;  // optional device counter
    const float *depth_max;       // optional: largest valid depth of the frame (device)
    int *brick_list; unsigned *brick_count;  // work list of the two-phase path: the region the integrate kernel reads, the workspace header
    unsigned *count_room;                    // the brick kernel's update counts, a word per workgroup (room_count_add)
    unsigned list_cap, pair_word;            // entries a list region holds; header word of the ListPair that goes with brick_list (PAIR_*)
    int bricks_x, bricks_y, bricks_z, brick_z;  // brick_z: planes per brick (runtime; BRICK_Z by default)
    unsigned kflags;              // KF_*
    float near_margin;            // pixels: how near a half-integer a streamed voxel's approximate image coordinate may come before the exact path decides (stream_margins)
    unsigned char *signmap;       // xs_signmap.h buffer (whole-volume launches) or null: bricks that receive a negative value are marked
    DepthTiles dt;                // per-tile depth range of the frame (k_scale_depth), for k_classify_boxes
    unsigned *box_class;          // [list entry][BOXES_PER_BRICK] box_word (k_classify_boxes) or null: every box takes the exact walk
    size_t probe_offset;          // XS_EXPERIMENTS + XS_WG_TIMES only: bytes from box_class to the record area
};
// KF_ALWAYS_STORE: write every updated voxel's three words even where the bits do not change (measurement aid)
// KF_COUNT_CLASSES: the classification counts its boxes in the workspace header, words CLASS_COUNT_WORD + 0..3, + 6, + 7: boxes wholly free /
//                   wholly empty / with planes to walk, planes walked, planes streamed with the in-image test (EDGE), with the validity test (SPECKLE)
// KF_FAR_FIRST:     the list is taken from its end (see k_integrate_bricks)
// KF_NO_TESTED_STREAM: the numeric shortcuts of the EDGE / SPECKLE classes are not proven for this launch (sensor too large or imaginary pose
//                   parts too large: stream_margins): such boxes take the exact walk
enum { KF_ALWAYS_STORE = 1u, KF_COUNT_CLASSES = 2u, KF_FAR_FIRST = 4u, KF_NO_TESTED_STREAM = 8u };
// the smallest camera depth c at which a box may be classed EDGE / SPECKLE: the streamed paths' shortcuts are derived for voxels that are
// not at the camera (xs_integrate_stream.h), the classifier and stream_margins (xs_integrate_args.h) both bound with it
#define XS_EDGE_CMIN 0.05f

namespace {
// device side of the frustum: add the far limit (see struct Frustum).  Behind the farthest
// surface by more than the truncation band nothing is written: v_c_1 = Dp*(xl, yl, 1) lies on
// the voxel's own ray, so sdf = (Dp - c) * |v_c|/c with |v_c|/c >= 1 and Dp <= Dmax; c > Dmax +
// trunc therefore gives sdf < -trunc.  Without a frame maximum the valid-depth gate of
// scaleDepth (5 m, TsdfFusion.cu:77) bounds Dp.
__device__ __forceinline__ float far_limit(const IntegrateArgs &a) {
    const float dmax = a.depth_max ? *a.depth_max : 5.0f;
    return dmax * 1.0001f + 1.05f * a.tranc_dist;
}
__device__ __forceinline__ Frustum device_frustum(const IntegrateArgs &a) {
    Frustum f = a.fr;
    f.alpha[5] += far_limit(a);
    return f;
}
// z interval [zb, ze) of column (x, y) that can pass the tests, padded by two voxels.  Branch-free per
// lane: the plane kinds are wave-uniform.
__device__ __forceinline__ void clip_column(const ClipPlanes &c, float far, int x, int y, int &zb, int &ze) {
    float lo = (float)zb, hi = (float)ze;
    const float i = x + 0.5f, j = y + 0.5f;
    bool empty = false;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const float a0 = (p == 5) ? c.A[5] + far * c.far_scale : c.A[p];
        const float root = a0 + c.B[p] * i + c.C[p] * j;
        const int kind = (c.kinds >> (2 * p)) & 3;
        if (kind == 1) lo = fmaxf(lo, root);
        else if (kind == 2) hi = fminf(hi, root);
        else empty = empty || (root < 0.f);
    }
    zb = max(zb, (int)floorf(lo - 0.5f) - 2);
    ze = empty ? zb : min(ze, (int)ceilf(hi - 0.5f) + 3);
}
// can any voxel of the index box [x0,x1) x [y0,y1) x [z0,z1) pass?  (all corners outside one
// half-space => no)
__device__ __forceinline__ bool box_may_pass(const Frustum &f, int x0, int x1, int y0, int y1, int z0, int z1) {
    const float xa = x0 + 0.5f, xb = x1 - 0.5f, ya = y0 + 0.5f, yb = y1 - 0.5f, za = z0 + 0.5f, zb = z1 - 0.5f;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        // maximum of the affine form over the box: pick the favourable end per axis
        const float m = f.alpha[p] + (f.bx[p] > 0 ? f.bx[p] * xb : f.bx[p] * xa) + (f.by[p] > 0 ? f.by[p] * yb : f.by[p] * ya) +
                        (f.bz[p] > 0 ? f.bz[p] * zb : f.bz[p] * za);
        if (m < -f.slack[p] * 1.5f) return false;
    }
    return true;
}

// The reference's per-voxel body (TsdfFusion.cu:110-168) for one voxel whose current state
// (value, grad, weight) has already been loaded.  Returns true and the new state if the voxel is
// written.
struct PoseRT { MatS33 R; cfloat3 t; };   // volume-to-camera pose (the kernel argument's)
struct VoxelCtx {
    cfloat base[3];
    float fx, fy, cx, cy, ulo, uhi, vlo, vhi;
};
struct VoxelProj {  // what the projection hands to the update
    cfloat3 v_c; cfloat image_x, image_y, Dp; float c;
};
// how project_voxel reads the scaled depth image: plain global loads (64-bit per-lane addresses), or buffer loads through a
// wave-uniform descriptor with a 32-bit per-lane byte offset (no 64-bit multiply-add per gather)
struct DepthGlobal {
    const float *depth; size_t dstep;
    struct __attribute__((packed, aligned(4))) pair { float a, b; };
    __device__ __forceinline__ float one(int y, int x) const { return row_ptr(depth, dstep, y)[x]; }
    __device__ __forceinline__ void two(int y, int x, float &a, float &b) const {
        const pair r = *reinterpret_cast<const pair *>(row_ptr(depth, dstep, y) + x); a = r.a; b = r.b;
    }
};
struct DepthBuffer {
    __amdgpu_buffer_rsrc_t rsrc; int dstep;
    __device__ __forceinline__ float one(int y, int x) const {
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, y * dstep + x * 4, 0, 0));
    }
    __device__ __forceinline__ void two(int y, int x, float &a, float &b) const {
        const auto r = __builtin_amdgcn_raw_buffer_load_b64(rsrc, y * dstep + x * 4, 0, 0);
        a = __builtin_bit_cast(float, r[0]); b = __builtin_bit_cast(float, r[1]);
    }
};
enum { BUFFER_RSRC_FLAGS = 0x00020000 };   // gfx9 raw buffer, dword 3: 32-bit data format
// phase 1 (TsdfFusion.cu:110-143): project the voxel, fetch its depth.  false = not written.
// In pieces so that a caller can take one alone (the streamed columns of xs_integrate_stream.h run voxel_pixel where their shortcut is unsure):
// voxel_pixel — camera-frame point, image coordinates, the pixel (TsdfFusion.cu:110-127); pixel_depth — the depth sample(s) as loaded
// words; voxel_depth — Dp from those words (:128-143).  project_voxel is the three in a row.
struct VoxelPixel { int coo_x, coo_y, near_x, near_y; };
__device__ __forceinline__ bool voxel_pixel(const IntegrateArgs &a, const PoseRT &ps, const VoxelCtx &k, int z, VoxelProj &o, VoxelPixel &px_) {
    const float vgz = (z + 0.5f) * a.voxel_size;
    o.v_c.x = (k.base[0] + ps.R.data[0].z * vgz) + ps.t.x;
    o.v_c.y = (k.base[1] + ps.R.data[1].z * vgz) + ps.t.y;
    o.v_c.z = (k.base[2] + ps.R.data[2].z * vgz) + ps.t.z;
    const float c = o.v_c.z.re;
    o.c = c;
    if (c < 0) return false;  // Re(1/v_c.z) < 0
    const cfloat px = o.v_c.x * k.fx, py = o.v_c.y * k.fy;
    // early reject before the divides: |true image coordinate - (px/c + cx)| << 1 pixel
    // (one min-chain and a single compare instead of four compare-and-branch pairs)
    const float margin = fminf(fminf(px.re - k.ulo * c, k.uhi * c - px.re), fminf(py.re - k.vlo * c, k.vhi * c - py.re));
    if (c > 0 && margin < 0) return false;
    const cfloat inv_z = 1.0f / o.v_c.z;
    o.image_x = px * inv_z + k.cx;
    o.image_y = py * inv_z + k.cy;
    px_.coo_x = __float2int_rd(o.image_x.re - 0.5f);
    px_.coo_y = __float2int_rd(o.image_y.re - 0.5f);
    if (!(px_.coo_x > 1 && px_.coo_y > 1 && px_.coo_x < a.dcols - 1 && px_.coo_y < a.drows - 1)) return false;
    px_.near_x = __float2int_rn(o.image_x.re); px_.near_y = __float2int_rn(o.image_y.re);
    return true;
}
// what a column's voxels share: the z-invariant part of dot(R.row, v_g): (row.x*vgx) + (row.y*vgy) — v_g has zero imaginary part, so each
// complex product is (re*vg, im*vg) — and the conservative image window in un-divided form (one pixel of slack on each side)
__device__ __forceinline__ VoxelCtx voxel_ctx(const IntegrateArgs &a, const PoseRT &ps, int x, int y) {
    const float vgx = (x + 0.5f) * a.voxel_size;
    const float vgy = (y + 0.5f) * a.voxel_size;
    VoxelCtx k;
#pragma unroll
    for (int r = 0; r < 3; ++r) k.base[r] = ps.R.data[r].x * vgx + ps.R.data[r].y * vgy;
    k.fx = a.intr.fx; k.fy = a.intr.fy; k.cx = a.intr.cx; k.cy = a.intr.cy;
    k.ulo = 1.5f - k.cx; k.uhi = (a.dcols - 0.5f) - k.cx + 1.0f;
    k.vlo = 1.5f - k.cy; k.vhi = (a.drows - 0.5f) - k.cy + 1.0f;
    return k;
}
template <bool BILINEAR> struct DepthWords;
template <> struct DepthWords<false> { float n; };
template <> struct DepthWords<true> { float d00, d10, d01, d11; };
template <bool BILINEAR, class Depth>
__device__ __forceinline__ void pixel_depth(const VoxelPixel &q, const Depth &dimg, DepthWords<BILINEAR> &w) {
    if constexpr (BILINEAR) {
        // the four corners as two 8-byte loads (the pair (coo_x, coo_x + 1) is contiguous; 4-byte alignment is all a
        // global load needs); the nearest pixel is always one of them — coo = floor(image - 0.5), so rn(image) is coo or
        // coo + 1 on each axis (ties included) — and is picked from the registers instead of being gathered a fifth time:
        // two address-unit trips per voxel where there were five
        dimg.two(q.coo_y, q.coo_x, w.d00, w.d10);
        dimg.two(q.coo_y + 1, q.coo_x, w.d01, w.d11);
    } else {
        w.n = dimg.one(q.near_y, q.near_x);
    }
}
template <bool BILINEAR>
__device__ __forceinline__ bool voxel_depth(const IntegrateArgs &a, const VoxelPixel &q, const DepthWords<BILINEAR> &w, VoxelProj &o) {
    cfloat Dp;
    if constexpr (BILINEAR) {
        const float d00 = w.d00, d10 = w.d10, d01 = w.d01, d11 = w.d11;
        const int coo_x = q.coo_x, coo_y = q.coo_y;
        const float n0 = q.near_x == coo_x ? d00 : d10, n1 = q.near_x == coo_x ? d01 : d11;
        Dp = cfloat(q.near_y == coo_y ? n0 : n1, 0.0f);
        const float gmax = fmaxf(d00, fmaxf(d01, fmaxf(d10, d11)));
        const float gmin = fminf(d00, fminf(d01, fminf(d10, d11)));
        if (gmax - gmin < a.threshold && d00 != 0.0f && d01 != 0.0f && d10 != 0.0f && d11 != 0.0f) {
            const cfloat one(1.0f, 0.0f);
            const cfloat fa = o.image_x - cfloat(coo_x + 0.5f, 0.0f);
            const cfloat fb = o.image_y - cfloat(coo_y + 0.5f, 0.0f);
            Dp = d00 * (one - fa) * (one - fb) + d10 * fa * (one - fb) + d01 * (one - fa) * fb + d11 * fa * fb;
        }
    } else Dp = cfloat(w.n, 0.0f);
    o.Dp = Dp;
    return Dp.re > 0;  // the update needs Re Dp > 0 (TsdfFusion.cu:150)
}
template <bool BILINEAR, class Depth>
__device__ __forceinline__ bool project_voxel(const IntegrateArgs &a, const PoseRT &ps, const VoxelCtx &k, int z, VoxelProj &o, const Depth &dimg) {
    VoxelPixel q;
    if (!voxel_pixel(a, ps, k, z, o, q)) return false;
    DepthWords<BILINEAR> w;
    pixel_depth<BILINEAR>(q, dimg, w);
    return voxel_depth<BILINEAR>(a, q, w, o);
}
// The divide of a running mean, (out_v, out_g) = num / den component-wise by a real divisor den > 0.  x / x is exactly 1 and 0 / x is
// exactly 0 (sign kept) in IEEE arithmetic, so the two divides are skipped where the numerator equals the divisor or is zero — the steady
// state of free space (value 1, derivative 0), i.e. most written voxels.
__device__ __forceinline__ void mean_divide(cfloat num, float den, float &out_v, float &out_g) {
    const bool div_v = !(num.re == den), div_g = !(num.im == 0.0f);
    out_v = 1.0f; out_g = num.im;
    if (__builtin_amdgcn_ballot_w64(div_v || div_g) != 0) {  // wave-uniform: whole waves of steady free space skip both divides
        if (div_v) out_v = num.re / den;
        if (div_g) out_g = num.im / den;
    }
}
// phase 2 (TsdfFusion.cu:144-167): signed distance, truncation, running mean.
__device__ __forceinline__ bool update_voxel(const IntegrateArgs &a, const VoxelCtx &k, const VoxelProj &p, float pre_v, float pre_g,
                                             int pre_w, float &out_v, float &out_g, int &out_w) {
    // v_c_1 = Dp*(xl, yl, 1) lies on the voxel's own ray (xl = v_c.x / v_c.z), so
    // sdf = |v_c_1| - |v_c| = (Dp - c) * |v_c|/c with |v_c|/c >= 1.  Beyond the truncation band by
    // a safe margin (0.1 % of the band + 10 um, ~30x the float error of the two norms) the side is
    // decided by the depth difference alone: behind the surface nothing is written, in front the
    // value is the truncated constant (1, 0) — exactly what the reference computes — and the
    // two complex norms (6 complex products, 2 square roots, 6 divides) are only evaluated
    // inside the band.
    const float depth_diff = p.Dp.re - p.c;
    const float band = a.tranc_dist * 1.001f + 1e-5f;
    if (depth_diff < -band) return false;
    cfloat tsdf(1.0f, 0.0f);
    if (!(depth_diff > band)) {
        const cfloat xl = (p.image_x - k.cx) / k.fx;
        const cfloat yl = (p.image_y - k.cy) / k.fy;
        const cfloat3 v_c_1 = mk3(p.Dp * xl, p.Dp * yl, p.Dp);
        const cfloat sdf = norm(v_c_1) - norm(p.v_c);
        if (!(sdf.re >= -a.tranc_dist)) return false;
        if (!(sdf.re > a.tranc_dist)) tsdf = sdf * a.tranc_dist_inv;
    }
    // running mean (TsdfFusion.cu:161-167): (prev * w + tsdf) / (w + 1)
    const cfloat tsdf_prev = unpack_tsdf(pre_v, pre_g);
    const cfloat num = tsdf_prev * __int2float_rn(pre_w) + 1.0f * tsdf;
    mean_divide(num, __int2float_rn(pre_w + 1), out_v, out_g);
    out_w = min(pre_w + 1, a.max_weight);
    return true;
}
// update_voxel in two halves, for the kernel that decides first and touches the volume afterwards.
// voxel_tsdf is everything of TsdfFusion.cu:144-159 — it needs no voxel state: false = not written, else the frame's tsdf;
// running_mean is :161-167 on the loaded state.  The two state the same operations in the same order as update_voxel and are kept beside
// it ON PURPOSE: with update_voxel written as voxel_tsdf + running_mean the compiler schedules the integrate kernels differently — 468,
// 573, 833 and 607 of the about 5 000-5 300 assembly lines of the four k_integrate_bricks instances change, and 28 of each k_integrate,
// when the split of xs_integrate.hip was proposed; 603, 561, 835 and 454 of 4 500-4 800, and 26, by profiles/tools/compare_kernel_text.py's
// count on the split tree — and the walk is bound by instruction issue, so each of these kernels would have to be measured again.  A
// change to one of the three is a change to all three (profiles/integrate_split_kernels.txt lists this among the dedupes tried; the one
// piece the three could share with identical kernel text is mean_divide).
__device__ __forceinline__ bool voxel_tsdf(const IntegrateArgs &a, const VoxelCtx &k, const VoxelProj &p, cfloat &tsdf) {
    const float depth_diff = p.Dp.re - p.c;
    const float band = a.tranc_dist * 1.001f + 1e-5f;
    if (depth_diff < -band) return false;
    tsdf = cfloat(1.0f, 0.0f);
    if (!(depth_diff > band)) {
        const cfloat xl = (p.image_x - k.cx) / k.fx;
        const cfloat yl = (p.image_y - k.cy) / k.fy;
        const cfloat3 v_c_1 = mk3(p.Dp * xl, p.Dp * yl, p.Dp);
        const cfloat sdf = norm(v_c_1) - norm(p.v_c);
        if (!(sdf.re >= -a.tranc_dist)) return false;
        if (!(sdf.re > a.tranc_dist)) tsdf = sdf * a.tranc_dist_inv;
    }
    return true;
}
__device__ __forceinline__ void running_mean(int max_weight, cfloat tsdf, float pre_v, float pre_g, int pre_w, float &out_v,
                                             float &out_g, int &out_w) {
    const cfloat tsdf_prev = unpack_tsdf(pre_v, pre_g);
    const cfloat num = tsdf_prev * __int2float_rn(pre_w) + 1.0f * tsdf;
    mean_divide(num, __int2float_rn(pre_w + 1), out_v, out_g);
    out_w = min(pre_w + 1, max_weight);
}
// Only the words whose bits change are stored (same volume, fewer bytes: in free space in front of a surface the running mean of (1, 0)
// with (1, 0) is (1, 0) again, and a saturated weight stays).  always: 1 with KF_ALWAYS_STORE, else 0.
// The voxel is at byte offset off of the three arrays bv / bw / bg (a caller that holds the voxel's three pointers passes them with offset 0).
// Written with the addresses formed INSIDE the three branches: formed in front of them, at the call, the compiler hoists them and 900 to
// 1 228 lines of each k_integrate_bricks instance change (profiles/integrate_split_kernels.txt).
__device__ __forceinline__ void store_changed(char *bv, char *bw, char *bg, unsigned off, float ov, int ow, float og, float v0, int w0, float g0, unsigned always) {
    if ((__float_as_uint(ov) ^ __float_as_uint(v0)) | always) *reinterpret_cast<float *>(bv + off) = ov;
    if ((unsigned)(ow ^ w0) | always) *reinterpret_cast<int *>(bw + off) = ow;
    if ((__float_as_uint(og) ^ __float_as_uint(g0)) | always) *reinterpret_cast<float *>(bg + off) = og;
}
template <bool BILINEAR>
__device__ __forceinline__ bool integrate_voxel(const IntegrateArgs &a, const PoseRT &ps, const VoxelCtx &k, int z, float pre_v, float pre_g, int pre_w,
                                                float &out_v, float &out_g, int &out_w) {
    VoxelProj p;
    if (!project_voxel<BILINEAR>(a, ps, k, z, p, DepthGlobal{a.depth, a.dstep})) return false;
    return update_voxel(a, k, p, pre_v, pre_g, pre_w, out_v, out_g, out_w);
}

// z in [zb, ze) of column (x, y).  The voxel's current state (coalesced 256 B rows) is requested
// before the projection arithmetic so its HBM latency runs under it.  (Two planes per trip with
// six reads in flight was measured slower: 102 VGPRs halve the resident waves.)
// OFF32 (the brick kernel): the three arrays are addressed as a wave-uniform base (the brick's first voxel: scalar registers) + one 32-bit
// byte offset per lane that advances by a plane per trip — one VALU instruction per trip for the addresses instead of the six of three
// 64-bit pointers.  ubase: byte offset of the brick's voxel (0, 0, zb0) in each array; zb0: the brick's first plane.
template <bool BILINEAR, bool OFF32 = false, bool SIGN = false>   // SIGN: a.signmap is marked (a template parameter: the walk is bound by instruction issue)
__device__ __forceinline__ unsigned integrate_span(const IntegrateArgs &a, const PoseRT &ps, int x, int y, int zb, int ze, size_t ubase = 0, int zb0 = 0, unsigned lane_off = 0) {
    unsigned n_upd = 0;
    const VoxelCtx k = voxel_ctx(a, ps, x, y);
    const size_t row = (size_t)(zb - a.z0) * a.Y + y;
    float *pos = row_ptr(a.value, a.vstep, 0) + row * (a.vstep / 4) + x;
    int *wpos = row_ptr(a.weight, a.vstep, 0) + row * (a.vstep / 4) + x;
    float *gpos = row_ptr(a.grad, a.vstep, 0) + row * (a.vstep / 4) + x;
    const size_t zstride = (size_t)a.Y * (a.vstep / 4);
    const unsigned always = (a.kflags & KF_ALWAYS_STORE) ? 1u : 0u;
    float vmin = 0.0f;   // smallest value written by this span (sign map: one v_min per written voxel, one test per span)
    if constexpr (OFF32) {
        char *bv = reinterpret_cast<char *>(a.value) + ubase, *bw = reinterpret_cast<char *>(a.weight) + ubase, *bg = reinterpret_cast<char *>(a.grad) + ubase;
        const unsigned plane = (unsigned)a.Y * (unsigned)a.vstep;
        unsigned off = lane_off + (unsigned)(zb - zb0) * plane;
        for (int z = zb; z < ze; ++z, off += plane) {
            float *pos = reinterpret_cast<float *>(bv + off), *gpos = reinterpret_cast<float *>(bg + off);
            int *wpos = reinterpret_cast<int *>(bw + off);
            const float v0 = *pos, g0 = *gpos;
            const int w0 = *wpos;
            float ov, og; int ow;
            if (integrate_voxel<BILINEAR>(a, ps, k, z, v0, g0, w0, ov, og, ow)) {
                store_changed(bv, bw, bg, off, ov, ow, og, v0, w0, g0, always);
                if (SIGN) vmin = fminf(vmin, ov);
                ++n_upd;
            }
            else asm volatile("" ::"v"(v0), "v"(g0), "v"(w0));
        }
        if (SIGN && vmin < 0.0f) signmap_mark_span(a.signmap, x, y, zb, ze);
        return n_upd;
    }
    // (Requesting the state of voxel z+1 one trip ahead, in front of or behind the depth gather, was
    // measured slower: loads return in issue order and the extra live registers cost a wave.)
    for (int z = zb; z < ze; ++z, pos += zstride, wpos += zstride, gpos += zstride) {
        const float v0 = *pos, g0 = *gpos;
        const int w0 = *wpos;
        float ov, og; int ow;
        if (integrate_voxel<BILINEAR>(a, ps, k, z, v0, g0, w0, ov, og, ow)) {
            store_changed(reinterpret_cast<char *>(pos), reinterpret_cast<char *>(wpos), reinterpret_cast<char *>(gpos), 0u, ov, ow, og, v0, w0, g0, always);
            if (SIGN) vmin = fminf(vmin, ov);
            ++n_upd;
        }
        else asm volatile("" ::"v"(v0), "v"(g0), "v"(w0));
        // (the empty asm consumes the three loads on the paths that left early: without it they are
        // still in flight at the loop head, and the wait the compiler puts there to protect their
        // registers also waits for the previous trip's stores to be acknowledged)
    }
    if (SIGN && vmin < 0.0f) signmap_mark_span(a.signmap, x, y, zb, ze);
    return n_upd;
}
}  // namespace
