// merge_host.hpp — the host's side of merging a second TSDF map into the volume: the affine map from this volume's
// voxel indices to the other volume's continuous voxel indices, the rigid transform between two maps from one camera frame posed in both, the
// source index box of a destination tile that the kernel's cull uses, and the descriptor of a second map with the one rule that accepts it.
// No device call and no HIP header: the orchestrator uses it in front of the launch, csrc/xs_merge_sample.h (xs_merge.hip, xs_diff.hip) compiles merge_tile_box for the device from this same text, and tests/cxx/merge_selftest.cpp runs all of it
// under the sanitizers without a GPU.
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define XS_MERGE_HD __host__ __device__
#else
#define XS_MERGE_HD
#endif

namespace xs_host {

// xform12 of xs_tsdf_merge from a rigid (or similar) transform.  T16: a real 4 x 4, row-major, taking a point of THIS map's volume frame (metres)
// to the OTHER map's volume frame, p_other = T p_this.  Voxel i of a volume has its centre at (i + 0.5) vs, so the continuous index of the other
// volume under destination voxel d is (R ((d + 0.5) vs_dst) + t) / vs_src - 0.5: the matrix block is R vs_dst / vs_src and the offset
// (R (0.5 vs_dst (1, 1, 1)) + t) / vs_src - 0.5.  Float64 throughout, one rounding to float32 at the end.  False, with nothing written, for an entry
// of T (rows 0 .. 2) that is not finite or a voxel size that is not finite and positive.
inline bool merge_affine(const double *T16, double dst_voxel_size, double src_voxel_size, float *out12) {
    if (!T16 || !out12 || !(dst_voxel_size > 0.0) || !(src_voxel_size > 0.0) || !std::isfinite(dst_voxel_size) || !std::isfinite(src_voxel_size)) return false;
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(T16[i])) return false;
    double m[12];
    for (int a = 0; a < 3; ++a) {
        const double *R = T16 + 4 * a;
        for (int b = 0; b < 3; ++b) m[3 * a + b] = R[b] * dst_voxel_size / src_voxel_size;
        const double half = 0.5 * dst_voxel_size;
        m[9 + a] = (((R[0] * half + R[1] * half) + R[2] * half) + R[3]) / src_voxel_size - 0.5;
    }
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite((double)(float)m[i])) return false;
    for (int i = 0; i < 12; ++i) out12[i] = (float)m[i];
    return true;
}

// T = c2v_other c2v_this^-1 from the real parts of two camera-to-volume poses of the SAME camera frame (4 x 4, row-major, rigid): a point of this
// map's volume frame goes to the camera and from there into the other map's volume frame.  The inverse of a rigid pose is (R^T, -R^T t).
inline void map_transform(const double *c2v_this16, const double *c2v_other16, double *T16) {
    double inv[16] = {0};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) inv[4 * r + c] = c2v_this16[4 * c + r];
        inv[4 * r + 3] = -((c2v_this16[r] * c2v_this16[3] + c2v_this16[4 + r] * c2v_this16[7]) + c2v_this16[8 + r] * c2v_this16[11]);
    }
    inv[15] = 1.0;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += (r < 3 ? c2v_other16[4 * r + k] : (k == 3 ? 1.0 : 0.0)) * inv[4 * k + c];
            T16[4 * r + c] = s;
        }
}

// The second map of a map-level call (merge, align, score, search, diff): a whole volume in device memory in the project's layout, the arrays at
// plane 0 with one pitch of `step` bytes; its resolution and voxel size may differ from this map's.  It is only read.  It comes from
// the caller's pointers, from another instance of the process or from a checkpoint file of a whole volume in either format
// (KinectFusionReconstruction.h: OtherInstanceMap, OpenCheckpointMap).
struct SecondMap {
    const float *value = nullptr;
    const int *weight = nullptr;
    const float *grad = nullptr;   // only a merge reads it
    size_t step = 0;
    int res[3] = {0, 0, 0};
    float voxel_size = 0.f, tranc_dist = 0.f;
};

// Whether an operation takes the map: no null array (grad only where it is needed), every axis at least min_axis (1 where the map is sampled, 2
// where its differences are), a finite positive voxel size, this map's truncation distance exactly (stored values are normalised by it, so
// another is refused, not rescaled), no array that is this map's own, and a pitch that is a multiple of 4 holding a row.  Every refusal is the
// caller's -1.
inline bool second_map_ok(const SecondMap &m, int min_axis, bool need_grad, float this_tranc_dist, const float *this_value, const int *this_weight,
                          const float *this_grad) {
    if (!m.value || !m.weight || (need_grad && !m.grad)) return false;
    for (int a = 0; a < 3; ++a)
        if (m.res[a] < min_axis) return false;
    if (!(m.voxel_size > 0.f) || !std::isfinite(m.voxel_size) || m.tranc_dist != this_tranc_dist) return false;
    if (m.value == this_value || m.weight == this_weight || (need_grad && m.grad == this_grad)) return false;
    return m.step % 4 == 0 && m.step >= (size_t)m.res[0] * 4;
}

// One axis of the per-voxel contract's step 1, float32 in the order written (both builds compile with -ffp-contract=off).
XS_MERGE_HD inline float merge_index(const float *m12, int a, int x, int y, int z) {
    return ((m12[3 * a] * (float)x + m12[3 * a + 1] * (float)y) + m12[3 * a + 2] * (float)z) + m12[9 + a];
}

// The source index box of the destination tile lo .. hi (inclusive voxel indices per axis): box6 = {lo x, lo y, lo z, hi x, hi y, hi z}, inclusive,
// inside [0, S - 1], containing every source voxel that any voxel of the tile reads.  False when no voxel of the tile passes the contract's step 2
// (the tile misses the source).  Every float32 operation of merge_index is monotone in each of x, y and z (a rounded product with a fixed factor
// and a rounded sum are), so the computed index of every voxel of the tile lies between the computed indices of the tile's eight corners:
// the bounds are exact for the arithmetic the kernel runs, and one voxel of margin is added on both sides all the same.  A corner that is not finite
// (an overflow) gives the whole source.
XS_MERGE_HD inline bool merge_tile_box(const float *m12, const int *lo3, const int *hi3, const int *S3, int *box6) {
    bool whole = false;
    float gmin[3], gmax[3];
    for (int a = 0; a < 3; ++a) {
        for (int c = 0; c < 8; ++c) {
            const float g = merge_index(m12, a, (c & 1) ? hi3[0] : lo3[0], (c & 2) ? hi3[1] : lo3[1], (c & 4) ? hi3[2] : lo3[2]);
            if (!(g - g == 0.f)) whole = true;   // an infinity or a NaN
            if (c == 0 || g < gmin[a]) gmin[a] = g;
            if (c == 0 || g > gmax[a]) gmax[a] = g;
        }
    }
    for (int a = 0; a < 3; ++a) {
        const float top = (float)(S3[a] - 1);
        if (whole) { box6[a] = 0; box6[3 + a] = S3[a] - 1; continue; }
        if (gmax[a] < 0.f || gmin[a] > top) return false;
        const float l = gmin[a] < 0.f ? 0.f : gmin[a], h = gmax[a] > top ? top : gmax[a];
        const int bl = (int)floorf(l) - 1, bh = (int)floorf(h) + 2;   // floor(h) + 1 is the upper corner; one voxel of margin either side
        box6[a] = bl < 0 ? 0 : bl;
        box6[3 + a] = bh > S3[a] - 1 ? S3[a] - 1 : bh;
    }
    return true;
}

}  // namespace xs_host
