// xs_sample_at.h — every output of one sampled point, stated once for xs_sample.hip (the caller's points and a depth frame's pixels) and
// xs_register.hip (the Gauss-Newton terms of a point cloud): the value F(P) of xs_trilinear.h, the grad array beside it where dvalue is wanted,
// and the gradient from the six samples at +- half a voxel.  The contract is xs_tsdf_sample_points' in include/xslam_amd.h.
#pragma once
#include "xs_trilinear.h"

namespace xs {

struct SampleResult { int status; float value, dvalue, grad[3]; };

// every output of one point P; the NaN 0x7fffffff wherever the contract says so.  The centre sample first, then, where a gradient is wanted
// and the centre is OK, the six samples at +- half a voxel: seven evaluations of up to eight corners each, all gathers; nothing is kept
// between them.
template <bool SECOND>
__device__ __forceinline__ void sample_at(const TrilinearVolume &vol, bool want_gradient, float p0, float p1, float p2, SampleResult &r) {
    r.value = qnan_f(); r.dvalue = qnan_f(); r.grad[0] = r.grad[1] = r.grad[2] = qnan_f();
    float v = 0.f, q = 0.f;
    r.status = trilinear_sample<SECOND>(vol, p0, p1, p2, v, q);
    if (r.status != TRI_OK) return;
    r.value = v;
    if (SECOND) r.dvalue = q;
    if (!want_gradient) return;
    const float h = 0.5f * vol.voxel_size;
    float G[3] = {0.f, 0.f, 0.f};
    bool ok = true;
#pragma unroll 1
    for (int c = 0; c < 3 && ok; ++c) {
        float Fp = 0.f, Fm = 0.f, unused;
        ok = trilinear_sample<false>(vol, c == 0 ? p0 + h : p0, c == 1 ? p1 + h : p1, c == 2 ? p2 + h : p2, Fp, unused) == TRI_OK &&
             trilinear_sample<false>(vol, c == 0 ? p0 - h : p0, c == 1 ? p1 - h : p1, c == 2 ? p2 - h : p2, Fm, unused) == TRI_OK;
        const float g = Fp - Fm;
        if (c == 0) G[0] = g; else if (c == 1) G[1] = g; else G[2] = g;
    }
    if (ok) { r.grad[0] = G[0] / vol.voxel_size; r.grad[1] = G[1] / vol.voxel_size; r.grad[2] = G[2] / vol.voxel_size; }
}

}  // namespace xs
