// xs_trilinear.h — F(P), the trilinear value of a volume at a point in metres, stated once for xs_render.hip (the refinement of a crossing and
// the six samples of a normal) and xs_sample.hip (caller-supplied points): the rule written out under xs_render_views in include/xslam_amd.h.
// xs_merge_sample.h keeps its own statement: it starts from an affine map of integer voxel indices and has a cull of its own.
#pragma once
#include "xs_device.h"

namespace xs {

// the volume as F reads it: rows in (z * Y + y) order, one pitch of `step` bytes for every array, the pointers at plane 0
struct TrilinearVolume {
    const float *value; const int *weight;
    const float *second;             // a second array interpolated over the same corners (the grad volume), or null
    size_t step;
    int X, Y, Z;
    float voxel_size;
    int min_weight;
};

enum { TRI_OUTSIDE = 0,              // refused by the range test (a NaN or an infinite coordinate is outside)
       TRI_UNSEEN = 1,               // refused by the weight test: the smallest weight among the needed corners < min_weight
       TRI_OK = 2 };

// g[c] = P[c] / voxel_size - 0.5f must lie in 0 .. S[c] - 1; only the corners on axes with a fraction > 0 are read; x, then y, then z, a stage
// being lo * (1 - f) + hi * f and its lower operand itself on an axis with fraction 0 (-0 stays -0).  With SECOND, `second` is put through the
// same stages with the same fractions into out2.  out and out2 are written only with TRI_OK.
template <bool SECOND>
__device__ __forceinline__ int trilinear_sample(const TrilinearVolume &a, float p0, float p1, float p2, float &out, float &out2) {
    const float p[3] = {p0, p1, p2};
    const int S[3] = {a.X, a.Y, a.Z};
    int b[3];
    float f[3];
    bool need[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float g = p[k] / a.voxel_size - 0.5f;
        if (!(g >= 0.f && g <= (float)(S[k] - 1))) return TRI_OUTSIDE;
        b[k] = __float2int_rd(g);
        f[k] = g - (float)b[k];
        need[k] = f[k] > 0.f;            // then g < S - 1 and b + 1 is inside the volume
    }
    const int needmask = (need[0] ? 1 : 0) | (need[1] ? 2 : 0) | (need[2] ? 4 : 0);
    int ws = 0x7fffffff;
#pragma unroll
    for (int d = 0; d < 8; ++d)
        if ((d & ~needmask) == 0) ws = min(ws, row_ptr(a.weight, a.step, a.Y * (b[2] + (d >> 2)) + b[1] + (d >> 1 & 1))[b[0] + (d & 1)]);
    if (ws < a.min_weight) return TRI_UNSEEN;
    float v[8], q[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        v[d] = 0.f; q[d] = 0.f;
        if ((d & ~needmask) == 0) {
            const int row = a.Y * (b[2] + (d >> 2)) + b[1] + (d >> 1 & 1);
            v[d] = row_ptr(a.value, a.step, row)[b[0] + (d & 1)];
            if (SECOND) q[d] = row_ptr(a.second, a.step, row)[b[0] + (d & 1)];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int stride = 1 << k;
        const float fk = f[k], gk = 1.0f - fk;
#pragma unroll
        for (int d = 0; d < 8; d += 2 * stride) {
            v[d] = need[k] ? v[d] * gk + v[d + stride] * fk : v[d];
            if (SECOND) q[d] = need[k] ? q[d] * gk + q[d + stride] * fk : q[d];
        }
    }
    out = v[0];
    if (SECOND) out2 = q[0];
    return TRI_OK;
}

}  // namespace xs
