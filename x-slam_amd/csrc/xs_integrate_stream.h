// xs_integrate_stream.h — the three streamed-column paths of k_integrate_bricks (xs_integrate.hip): what a wave does with the planes of a box
// that the classification (xs_integrate_boxes.h has the classes) found free — FREE: the running mean alone; EDGE: behind the in-image test;
// SPECKLE: behind the validity test of the voxel's own pixel.
#pragma once
#include "xs_integrate_voxel.h"

#ifndef XS_FREE_CHUNK
#define XS_FREE_CHUNK 1
#endif
enum { FREE_CHUNK = XS_FREE_CHUNK };

namespace {
// FREE box: voxels (x, y, zb .. ze - 1) of this lane's column (which lies in the volume).  A rolling pipeline over groups of FREE_CHUNK
// planes: the next group's state is requested before the current group is updated and stored, so the wave always has reads in flight
// (a wave's memory operations complete in issue order: the stores of one group would otherwise stand between two groups of reads).
// Addressed like the OFF32 walk: wave-uniform array bases + one 32-bit byte offset per lane and plane, shared by the three arrays.
// off: the column's first voxel (plane zb); plane: bytes between planes.
struct FreeGroup { float v[FREE_CHUNK], g[FREE_CHUNK]; int w[FREE_CHUNK]; };
__device__ __forceinline__ void free_group_load(FreeGroup &s, const char *bv, const char *bw, const char *bg, unsigned off, unsigned plane, int left) {
#pragma unroll
    for (int j = 0; j < FREE_CHUNK; ++j)
        if (j < left) {
            s.v[j] = *reinterpret_cast<const float *>(bv + (off + j * plane));
            s.g[j] = *reinterpret_cast<const float *>(bg + (off + j * plane));
            s.w[j] = *reinterpret_cast<const int *>(bw + (off + j * plane));
        }
}
__device__ __forceinline__ void free_group_store(const IntegrateArgs &a, const FreeGroup &s, char *bv, char *bw, char *bg, unsigned off, unsigned plane, int left,
                                                 unsigned always) {
#pragma unroll
    for (int j = 0; j < FREE_CHUNK; ++j)
        if (j < left) {
            float ov, og; int ow;
            running_mean(a.max_weight, cfloat(1.0f, 0.0f), s.v[j], s.g[j], s.w[j], ov, og, ow);
            store_changed(bv, bw, bg, off + j * plane, ov, ow, og, s.v[j], s.w[j], s.g[j], always);
        }
}
// (The streamed planes never mark the sign map: the running mean of a value with (1, 0) is negative only if the value was — and then the
// launch that wrote that negative value marked the brick, the map's bytes are never cleared, and a value that reached the array any other
// way obliges its owner to rebuild the map (xs_signmap.h).  One v_min per voxel and a dependent byte load per column less; 1024^3 -2 us.)
__device__ __forceinline__ unsigned integrate_free_column(const IntegrateArgs &a, char *bv, char *bw, char *bg, unsigned off, unsigned plane, int zb, int ze) {
    const unsigned always = (a.kflags & KF_ALWAYS_STORE) ? 1u : 0u;
    FreeGroup A, B;
    free_group_load(A, bv, bw, bg, off, plane, ze - zb);
#pragma unroll 1
    for (int z = zb; z < ze; z += 2 * FREE_CHUNK, off += 2 * FREE_CHUNK * plane) {
        free_group_load(B, bv, bw, bg, off + FREE_CHUNK * plane, plane, ze - z - FREE_CHUNK);
        free_group_store(a, A, bv, bw, bg, off, plane, ze - z, always);
        free_group_load(A, bv, bw, bg, off + 2 * FREE_CHUNK * plane, plane, ze - z - 2 * FREE_CHUNK);
        free_group_store(a, B, bv, bw, bg, off + FREE_CHUNK * plane, plane, ze - z - FREE_CHUNK, always);
    }
    return (unsigned)(ze - zb);
}


// EDGE box: like integrate_free_column, but a voxel is updated only if it passes the reference's in-image test (TsdfFusion.cu:123-124) —
// the one per-voxel decision left (see BOX_EDGE_BIT).  The exact path (voxel_pixel) decides it from
//     image_x = Re(px * (1 / v_c.z)) + cx,   coo_x = floor(image_x - 0.5),   1 < coo_x < cols - 1   <=>   2.5 <= image_x < cols - 0.5
// (and the same in y).  Here the real parts X, Y, c of v_c are formed with the exact path's own operations (the real part of each complex
// sum and product: the same bits), and the window is tested on the un-divided coordinates with a margin of EDGE_MARGIN pixels: the float
// image_x differs from fx X / c + cx in real arithmetic by < 3e-4 px (three roundings of magnitudes <= 640, the imaginary products ~1e-14),
// the un-divided terms by < 1e-4 px — two hundred times inside the margin, at any c >= XS_EDGE_CMIN.  A voxel inside the window by the
// margin is in the image, one outside by the margin is not, and the few in between (a strip 2 x EDGE_MARGIN px wide along the image
// border: a few per cent of the rows of an edge box) run the exact test itself — wave-uniformly skipped where no lane needs it.
#define XS_EDGE_MARGIN 0.03125f
struct EdgeWindow { float ulo, uhi, vlo, vhi; };   // the window shrunk by the margin, relative to the principal point
__device__ __forceinline__ EdgeWindow edge_window(const IntegrateArgs &a, const VoxelCtx &k) {
    EdgeWindow w;
    w.ulo = (2.5f + XS_EDGE_MARGIN) - k.cx; w.uhi = ((a.dcols - 0.5f) - XS_EDGE_MARGIN) - k.cx;
    w.vlo = (2.5f + XS_EDGE_MARGIN) - k.cy; w.vhi = ((a.drows - 0.5f) - XS_EDGE_MARGIN) - k.cy;
    return w;
}
// the real parts of voxel z's camera-frame point, by the exact path's own operations (voxel_pixel): the depth c and the un-divided image
// coordinates pxr = X fx, pyr = Y fy
struct RealPoint { float c, pxr, pyr; };
__device__ __forceinline__ RealPoint real_point(const IntegrateArgs &a, const PoseRT &ps, const VoxelCtx &k, int z) {
    const float vgz = (z + 0.5f) * a.voxel_size;
    const float X = (k.base[0].re + ps.R.data[0].z.re * vgz) + ps.t.x.re;
    const float Y = (k.base[1].re + ps.R.data[1].z.re * vgz) + ps.t.y.re;
    const float c = (k.base[2].re + ps.R.data[2].z.re * vgz) + ps.t.z.re;
    return RealPoint{c, X * k.fx, Y * k.fy};
}
__device__ __forceinline__ bool edge_in_image(const IntegrateArgs &a, const PoseRT &ps, const VoxelCtx &k, const EdgeWindow &w, int z) {
    const RealPoint rp = real_point(a, ps, k, z);
    const float c = rp.c, pxr = rp.pxr, pyr = rp.pyr;
    const float d = fminf(fminf(pxr - w.ulo * c, w.uhi * c - pxr), fminf(pyr - w.vlo * c, w.vhi * c - pyr));   // >= 0: inside by the margin
    bool in = d >= 0.0f;
    const bool unsure = !in && !(d < -2.0f * XS_EDGE_MARGIN * c);   // (NaN: unsure — the exact test decides)
    if (__builtin_amdgcn_ballot_w64(unsure) != 0) {
        if (unsure) { VoxelProj p; VoxelPixel q; in = voxel_pixel(a, ps, k, z, p, q); }
    }
    return in;
}
__device__ __forceinline__ unsigned integrate_edge_column(const IntegrateArgs &a, const PoseRT &ps, char *bv, char *bw, char *bg, unsigned off, unsigned plane,
                                                          int x, int y, int zb, int ze) {
    const unsigned always = (a.kflags & KF_ALWAYS_STORE) ? 1u : 0u;
    const VoxelCtx k = voxel_ctx(a, ps, x, y);
    const EdgeWindow w = edge_window(a, k);
    unsigned n = 0;
    // the free column's rolling pipeline, one plane per group: the next plane's test and state request go out before this plane's stores
    FreeGroup A, B;
    bool inA = edge_in_image(a, ps, k, w, zb), inB = false;
    if (inA) free_group_load(A, bv, bw, bg, off, plane, 1);
#pragma unroll 1
    for (int z = zb; z < ze; z += 2, off += 2 * plane) {
        inB = z + 1 < ze && edge_in_image(a, ps, k, w, z + 1);
        if (inB) free_group_load(B, bv, bw, bg, off + plane, plane, 1);
        if (inA) { free_group_store(a, A, bv, bw, bg, off, plane, 1, always); ++n; }
        inA = z + 2 < ze && edge_in_image(a, ps, k, w, z + 2);
        if (inA) free_group_load(A, bv, bw, bg, off + 2 * plane, plane, 1);
        if (inB) { free_group_store(a, B, bv, bw, bg, off + plane, plane, 1, always); ++n; }
    }
    return n;
}


// SPECKLE box (and EDGE + SPECKLE): a voxel of a free plane is written iff it is in the image AND its nearest pixel is valid (BOX_SPECKLE_BIT).
// The exact path finds that pixel from image_x = Re(px * (1 / v_c.z)) + cx, near_x = rn(image_x).  Here u = pxr * rcp(c) + cx from the same
// real parts (edge_in_image has the argument): the two differ by < 2.5e-4 px — the exact one carries five roundings of magnitudes <= 640
// (1.4e-4), this one v_rcp_f32's ulp, a product and a sum (1.0e-4) — so wherever u lies further than the margin (1 / 2048 px at that size) from a
// half-integer both round to the same pixel, and the ~0.2 % of voxels that lie nearer (one plane of a wave in eight) take the exact
// voxel_pixel, wave-uniformly skipped where no lane needs it.  THOSE FIGURES ARE THE 640 x 480 SENSOR'S: every rounding above is half an ulp
// of a magnitude up to E = max(cols + |cx|, rows + |cy|), so the margin is a launch parameter, a.near_margin = 8 ulp(E) (never below
// 1 / 2048: E < 1024 gives exactly that), against a worst case of 4 ulp(E) by the count above and 2 ulp(E) measured over 2e7 random voxels
// per width; and the argument drops the imaginary parts' contribution to the real part of px * (1 / v_c.z), which is
// <= E (Im c / c)^2 + |fx Im X| |Im c| / c^2 (1e-7 px for a first-order seed of 1e-7): stream_margins bounds it with c >= XS_EDGE_CMIN from
// the launch's pose and, where it exceeds a sixteenth of the margin or E >= 8192, sets KF_NO_TESTED_STREAM — no box is then classed EDGE or
// SPECKLE, they walk (INTEGRATION.md "Sensor size").  The in-image test is edge_in_image's (skipped for a box whose range is
// inside the image: need_image false).  One 4-byte depth gather per voxel; the state loads go out with it, a plane ahead of the stores.
struct ValidSlot { float v, g, d; int w; bool in; };
template <class Depth>
__device__ __forceinline__ void valid_slot_request(ValidSlot &s, const IntegrateArgs &a, const PoseRT &ps, const VoxelCtx &k, const EdgeWindow &win, bool need_image,
                                                   const Depth &dimg, const char *bv, const char *bw, const char *bg, unsigned off, int z, bool live) {
    s.in = false;
    if (__builtin_amdgcn_ballot_w64(live) == 0) return;
    const RealPoint rp = real_point(a, ps, k, z);
    const float c = rp.c, pxr = rp.pxr, pyr = rp.pyr;
    bool in = live, unsure = false;
    if (need_image) {
        const float d = fminf(fminf(pxr - win.ulo * c, win.uhi * c - pxr), fminf(pyr - win.vlo * c, win.vhi * c - pyr));
        in = live && d >= 0.0f;
        unsure = live && !in && !(d < -2.0f * XS_EDGE_MARGIN * c);
    }
    const float rc = __builtin_amdgcn_rcpf(c);
    const float u = pxr * rc + k.cx, v = pyr * rc + k.cy;
    const float ru = rintf(u), rv = rintf(v);
    const float sure = 0.5f - a.near_margin;
    unsure = unsure || (in && !(fabsf(u - ru) < sure && fabsf(v - rv) < sure));   // (NaN: unsure)
    int nx = (int)ru, ny = (int)rv;
    if (__builtin_amdgcn_ballot_w64(unsure) != 0) {
        if (unsure) { VoxelProj p; VoxelPixel q; in = voxel_pixel(a, ps, k, z, p, q); nx = q.near_x; ny = q.near_y; }
    }
    s.in = in;
    if (in) {
        s.d = dimg.one(ny, nx);
        s.v = *reinterpret_cast<const float *>(bv + off); s.g = *reinterpret_cast<const float *>(bg + off); s.w = *reinterpret_cast<const int *>(bw + off);
    }
}
__device__ __forceinline__ unsigned valid_slot_retire(const ValidSlot &s, const IntegrateArgs &a, char *bv, char *bw, char *bg, unsigned off, unsigned always) {
    if (!(s.in && s.d > 0.0f)) return 0u;   // (Dp = 0: TsdfFusion.cu:150)
    float ov, og; int ow;
    running_mean(a.max_weight, cfloat(1.0f, 0.0f), s.v, s.g, s.w, ov, og, ow);
    store_changed(bv, bw, bg, off, ov, ow, og, s.v, s.w, s.g, always);
    return 1u;
}
__device__ __forceinline__ unsigned integrate_valid_column(const IntegrateArgs &a, const PoseRT &ps, bool need_image, char *bv, char *bw, char *bg, unsigned off,
                                                           unsigned plane, int x, int y, int zb, int ze) {
    const unsigned always = (a.kflags & KF_ALWAYS_STORE) ? 1u : 0u;
    const VoxelCtx k = voxel_ctx(a, ps, x, y);
    const EdgeWindow w = edge_window(a, k);
    const DepthGlobal dimg{a.depth, a.dstep};
    unsigned n = 0;
    ValidSlot A, B;
    valid_slot_request(A, a, ps, k, w, need_image, dimg, bv, bw, bg, off, zb, true);
#pragma unroll 1
    for (int z = zb; z < ze; z += 2, off += 2 * plane) {
        valid_slot_request(B, a, ps, k, w, need_image, dimg, bv, bw, bg, off + plane, z + 1, z + 1 < ze);
        n += valid_slot_retire(A, a, bv, bw, bg, off, always);
        valid_slot_request(A, a, ps, k, w, need_image, dimg, bv, bw, bg, off + 2 * plane, z + 2, z + 2 < ze);
        n += valid_slot_retire(B, a, bv, bw, bg, off + plane, always);
    }
    return n;
}

}  // namespace
