// xs_render.hip — depth, normal and shaded views of a map from poses the caller picks, many views in one launch, for gfx950 (DESIGN.md
// section 4.28).  No counterpart in the reference, whose only ray caster is the tracker's.
//
// The contract is in include/xslam_amd.h (xs_render_views), operation by operation; what the call refuses, the sample count and the
// workspace's layout are ../host/render_host.hpp's, shared with the orchestrator and the host selftest.
//   k_render_mask_build  wave = one word of the brick mask: 32 bricks of 8 x 8 x 8 voxels in a row along x, that is up to four segments of
//                        64 voxels by 64 rows (8 y by 8 z).  A row is one coalesced 256-byte load of the values and one of the weights; the
//                        wave's ballot of "value < 0 && weight >= min_weight" is the row's 64 voxels, the ballots of a segment are OR-ed and
//                        each byte of the result is one brick.  Every word has one writer: no atomics, no clearing beforehand.
//   k_render_views       lane = pixel, wave = workgroup = an 8 x 8 pixel tile of ONE view (blockIdx.z; its twelve pose floats arrive by
//                        scalar loads), so a wave's rays stay in neighbouring bricks.  The march keeps the previous sample's state in
//                        registers; with the cull a sample in a brick without a negative voxel is not read unless its neighbour turns out
//                        negative (the mask word is read through L2 and kept in a register while the ray stays in the same 32 bricks).  The
//                        crossing is refined after the loop, by every lane of the wave that found one at once, then the six samples of
//                        the normal.  The trilinear sample is xs_trilinear.h's, shared with xs_sample.hip (xs_merge_sample.h keeps its
//                        own: DESIGN.md says why).  Four class counts per wave by ballot and popcount, one integer atomic each.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "xs_merge_sample.h"   // merge_res_ok
#include "xs_trilinear.h"
#include "../host/render_host.hpp"

using namespace xs;
using namespace xs_host;

static_assert(XS_RENDER_MAX_VIEWS == RENDER_MAX_VIEWS, "the header's bound");
static_assert(sizeof(RenderHeader) <= RENDER_HEADER_BYTES, "the header fits its bytes");

extern "C" size_t xs_render_workspace_bytes(const int *res) { return render_workspace_bytes(res); }

__global__ void __launch_bounds__(256) k_render_mask_build(const float *__restrict__ value, const int *__restrict__ weight, size_t step, int X, int Y, int Z,
                                                           int WX, int BY, unsigned nwords, int min_weight, unsigned *__restrict__ mask) {
    const int lane = threadIdx.x;
    const unsigned w = blockIdx.x * 4u + threadIdx.y;   // (uniform over the wave)
    if (w >= nwords) return;
    const int wx = (int)(w % (unsigned)WX), by = (int)(w / (unsigned)WX % (unsigned)BY), bz = (int)(w / ((unsigned)WX * (unsigned)BY));
    unsigned bits = 0;
    for (int seg = 0; seg < 4; ++seg) {
        const int x0 = wx * 256 + seg * 64;
        if (x0 >= X) break;
        const int x = x0 + lane;
        unsigned long long acc = 0ull;
        for (int r = 0; r < 64; ++r) {
            const int y = by * 8 + (r & 7), z = bz * 8 + (r >> 3);
            bool neg = false;
            if (y < Y && z < Z && x < X) {
                const int row = Y * z + y;
                neg = row_ptr(value, step, row)[x] < 0.f && row_ptr(weight, step, row)[x] >= min_weight;
            }
            acc |= __ballot(neg);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (acc >> (8 * i) & 0xFFull) bits |= 1u << (seg * 8 + i);
    }
    if (lane == 0) mask[w] = bits;
}

extern "C" int xs_render_mask_build(const float *value, const int *weight, size_t vol_step, const int *res, int min_weight, void *workspace, void *stream) {
    if (!value || !weight || !res || !workspace) return xs_set_error(hipErrorInvalidValue, "xs_render_mask_build: null pointer");
    RenderMaskDims m;
    if (!merge_res_ok(res) || !render_mask_dims(res, m) || m.words >= ((size_t)1 << 31)) return xs_set_error(hipErrorInvalidValue, "xs_render_mask_build: bad resolution");
    if (vol_step % 4 != 0 || vol_step < (size_t)res[0] * 4) return xs_set_error(hipErrorInvalidValue, "xs_render_mask_build: bad pitch");
    const int mw = min_weight < 1 ? 1 : min_weight;
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    hipLaunchKernelGGL(k_render_mask_build, dim3((unsigned)((m.words + 3) / 4)), dim3(64, 4), 0, st, value, weight, vol_step, res[0], res[1], res[2], m.WX, m.BY,
                       (unsigned)m.words, mw, reinterpret_cast<unsigned *>(ws + render_mask_offset()));
    XS_CHECK(hipGetLastError());
    const RenderHeader h = {RENDER_MAGIC, {res[0], res[1], res[2]}, mw};
    XS_CHECK(hipMemcpyAsync(ws, &h, sizeof(h), hipMemcpyHostToDevice, st));   // (pageable: staged before the call returns)
    return 0;
}

// ---- the render kernel -----------------------------------------------------------------------------------------------------------------
struct RenderArgs {
    const float *value; const int *weight; size_t step;
    int X, Y, Z;
    const float *poses;                          // [P][12]: R row-major, then t (camera to volume), in the workspace's staging area
    const unsigned *mask;
    int WX, BY;
    int rows, cols, tiles_x, samples;
    float fx, fy, cx, cy, t_near, dt, voxel_size;
    int min_weight, cull;
    float *depth; unsigned short *depth16; float *normal; unsigned char *shade; unsigned *counts;
};

enum { RAY_HIT = 0, RAY_BACKFACE = 1, RAY_REJECTED = 2, RAY_NONE = 3, RAY_REFINE = 4 };   // (RAY_REFINE: between the march and the refinement)
enum { ST_NONE = 0, ST_VALUE = 1, ST_DEFERRED = 2 };   // ST_DEFERRED: inside, in a brick without a negative voxel, not read yet

// the voxel of point p: false where it lies outside the volume (or is no number)
__device__ __forceinline__ bool render_voxel(const RenderArgs &a, float p0, float p1, float p2, int &x, int &y, int &z) {
    const float q0 = p0 / a.voxel_size, q1 = p1 / a.voxel_size, q2 = p2 / a.voxel_size;
    if (!(q0 >= 0.f && q0 < (float)a.X && q1 >= 0.f && q1 < (float)a.Y && q2 >= 0.f && q2 < (float)a.Z)) return false;
    x = __float2int_rd(q0); y = __float2int_rd(q1); z = __float2int_rd(q2);
    return true;
}
// the state of voxel (x, y, z), inside the volume: ST_VALUE with its value, or ST_NONE below min_weight
__device__ __forceinline__ int render_state(const RenderArgs &a, int x, int y, int z, float &v) {
    const int row = a.Y * z + y;
    if (row_ptr(a.weight, a.step, row)[x] < a.min_weight) return ST_NONE;
    v = row_ptr(a.value, a.step, row)[x];
    return ST_VALUE;
}

// F(P) of the contract (xs_trilinear.h, shared with xs_sample.hip) on the value array.  False where it is refused.
__device__ __forceinline__ bool render_trilinear(const RenderArgs &a, float p0, float p1, float p2, float &out) {
    const TrilinearVolume vol = {a.value, a.weight, nullptr, a.step, a.X, a.Y, a.Z, a.voxel_size, a.min_weight};
    float unused;
    return trilinear_sample<false>(vol, p0, p1, p2, out, unused) == TRI_OK;
}

__global__ void __launch_bounds__(64) k_render_views(const RenderArgs a) {
    const int lane = threadIdx.x;
    const int tile = blockIdx.x, ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const unsigned view = blockIdx.z;
    const float *__restrict__ P = a.poses + (size_t)view * RENDER_POSE_FLOATS;   // wave-uniform: scalar loads
    const float R00 = P[0], R01 = P[1], R02 = P[2], R10 = P[3], R11 = P[4], R12 = P[5], R20 = P[6], R21 = P[7], R22 = P[8];
    const float t0 = P[9], t1 = P[10], t2 = P[11];
    const int i = tx * 8 + (lane & 7), j = ty * 8 + (lane >> 3);
    const bool active = i < a.cols && j < a.rows;
    int cls = RAY_NONE;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    int kh = 0;                                  // the crossing lies between samples kh and kh + 1
    if (active) {
        const float dx = ((float)i - a.cx) / a.fx, dy = ((float)j - a.cy) / a.fy;
        d0 = (R00 * dx + R01 * dy) + R02; d1 = (R10 * dx + R11 * dy) + R12; d2 = (R20 * dx + R21 * dy) + R22;
        int pk = ST_NONE, px = 0, py = 0, pz = 0;
        float pv = 0.f;
        unsigned word = 0;
        int cur = -1;                            // the mask word `word` holds
        bool was_inside = false;
        for (int k = 0; k < a.samples; ++k) {
            const float t = a.t_near + (float)k * a.dt;
            int x = 0, y = 0, z = 0, ck = ST_NONE;
            float cv = 0.f;
            if (!render_voxel(a, t0 + t * d0, t1 + t * d1, t2 + t * d2, x, y, z)) {
                // outside: NONE.  Every coordinate is monotone in k, so a ray that has left the volume stays outside and nothing ends it.
                if (was_inside) break;
            } else {
                was_inside = true;
                bool read = true;
                if (a.cull) {
                    const int wi = (a.BY * (z >> 3) + (y >> 3)) * a.WX + (x >> 8);
                    if (wi != cur) { word = a.mask[wi]; cur = wi; }
                    read = word >> (x >> 3 & 31) & 1u;
                }
                ck = read ? render_state(a, x, y, z, cv) : (int)ST_DEFERRED;
            }
            // a deferred sample is NONE or a value >= 0: it matters only beside a negative value, and is read then
            if (ck == ST_VALUE && cv < 0.f && pk == ST_DEFERRED) pk = render_state(a, px, py, pz, pv);
            if (pk == ST_VALUE && pv < 0.f && ck == ST_DEFERRED) ck = render_state(a, x, y, z, cv);
            if (pk == ST_VALUE && ck == ST_VALUE) {
                if (pv < 0.f && cv > 0.f) { cls = RAY_BACKFACE; break; }
                if (pv > 0.f && cv < 0.f) { cls = RAY_REFINE; kh = k - 1; break; }
            }
            pk = ck; pv = cv; px = x; py = y; pz = z;
        }
    }
    float ts = 0.f;
    if (cls == RAY_REFINE) {
        const float ta = a.t_near + (float)kh * a.dt, tb = a.t_near + (float)(kh + 1) * a.dt;
        float F0 = 0.f, F1 = 0.f;
        const bool ok0 = render_trilinear(a, t0 + ta * d0, t1 + ta * d1, t2 + ta * d2, F0);
        const bool ok1 = render_trilinear(a, t0 + tb * d0, t1 + tb * d1, t2 + tb * d2, F1);
        cls = RAY_REJECTED;
        if (ok0 && ok1 && F0 >= 0.f && F1 <= 0.f) {
            const float den = F1 - F0;
            if (!(den == 0.f)) { ts = ta - a.dt * (F0 / den); cls = RAY_HIT; }
        }
    }
    const bool hit = cls == RAY_HIT;
    float n0 = qnan_f(), n1 = n0, n2 = n0;
    bool have_normal = false;
    if (hit && (a.normal || a.shade)) {
        const float q[3] = {t0 + ts * d0, t1 + ts * d1, t2 + ts * d2};
        const float h = 0.5f * a.voxel_size;
        float G[3] = {0.f, 0.f, 0.f};
        bool ok = true;
#pragma unroll 1
        for (int c = 0; c < 3 && ok; ++c) {
            float Fp = 0.f, Fm = 0.f;
            ok = render_trilinear(a, c == 0 ? q[0] + h : q[0], c == 1 ? q[1] + h : q[1], c == 2 ? q[2] + h : q[2], Fp) &&
                 render_trilinear(a, c == 0 ? q[0] - h : q[0], c == 1 ? q[1] - h : q[1], c == 2 ? q[2] - h : q[2], Fm);
            const float g = Fp - Fm;
            if (c == 0) G[0] = g; else if (c == 1) G[1] = g; else G[2] = g;
        }
        const float gg = (G[0] * G[0] + G[1] * G[1]) + G[2] * G[2];
        if (ok && gg > 0.f) {
            const float len = sqrtf(gg);
            n0 = G[0] / len; n1 = G[1] / len; n2 = G[2] / len;
            have_normal = true;
        }
    }
    if (active) {
        const size_t plane = (size_t)a.rows * (size_t)a.cols, pix = (size_t)j * (size_t)a.cols + (size_t)i;
        if (a.depth) a.depth[(size_t)view * plane + pix] = hit ? ts : 0.f;
        if (a.depth16) {
            const float r = rintf(ts * 1000.0f);
            a.depth16[(size_t)view * plane + pix] = hit && r >= 1.f && r <= 65535.f ? (unsigned short)(int)r : (unsigned short)0;
        }
        if (a.normal) {
            float *n = a.normal + (size_t)view * 3 * plane + pix;
            n[0] = n0; n[plane] = n1; n[2 * plane] = n2;
        }
        if (a.shade) {
            unsigned char s = 0;
            if (have_normal) {
                const float nd = (n0 * d0 + n1 * d1) + n2 * d2, dd = (d0 * d0 + d1 * d1) + d2 * d2;
                s = (unsigned char)(int)rintf(255.0f * fminf(1.0f, fabsf(nd) / sqrtf(dd)));
            }
            a.shade[(size_t)view * plane + pix] = s;
        }
    }
    if (a.counts) {
        const unsigned c_hit = (unsigned)__popcll(__ballot(active && cls == RAY_HIT)), c_back = (unsigned)__popcll(__ballot(active && cls == RAY_BACKFACE));
        const unsigned c_rej = (unsigned)__popcll(__ballot(active && cls == RAY_REJECTED)), c_none = (unsigned)__popcll(__ballot(active && cls == RAY_NONE));
        if (lane == 0) {
            unsigned *o = a.counts + 4 * (size_t)view;
            if (c_hit) atomicAdd(o + 0, c_hit);
            if (c_back) atomicAdd(o + 1, c_back);
            if (c_rej) atomicAdd(o + 2, c_rej);
            if (c_none) atomicAdd(o + 3, c_none);
        }
    }
}

/* see include/xslam_amd.h */
extern "C" int xs_render_views(int views, const float *Rc2v9xP, const float *tc2v3xP, const float *intr4, int rows, int cols, const float *value,
                               const int *weight, size_t vol_step, const int *res, float voxel_size, const xs_render_opts *opts, void *workspace,
                               float *depth_f32, uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4xP, void *stream) {
    xs_render_opts o;
    memset(&o, 0, sizeof(o));
    o.struct_bytes = sizeof(o);
    if (opts) o = *opts;
    RenderPlan plan;
    const int why = render_validate(views, Rc2v9xP, tc2v3xP, intr4, rows, cols, value && weight, vol_step, res, voxel_size, o.struct_bytes, (unsigned)sizeof(xs_render_opts),
                                    o.t_near, o.t_far, o.step, o.min_weight, o.shade_mode, workspace != nullptr,
                                    depth_f32 || depth_u16 || normal || shade || counts4xP, plan);
    if (why != RENDER_OK || !merge_res_ok(res)) {
        char msg[160];
        snprintf(msg, sizeof(msg), "xs_render_views: %s", render_refusal_str(why != RENDER_OK ? why : (int)RENDER_RES));
        return xs_set_error(hipErrorInvalidValue, msg);
    }
    RenderMaskDims m;
    render_mask_dims(res, m);
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    if (o.cull) {
        RenderHeader h;
        XS_CHECK(hipMemcpyAsync(&h, ws, sizeof(h), hipMemcpyDeviceToHost, st));
        XS_CHECK(hipStreamSynchronize(st));
        if (!render_mask_usable(h, res, plan.min_weight)) return xs_set_error(hipErrorInvalidValue, "xs_render_views: the cull needs a mask built in this workspace for this resolution");
    }
    RenderArgs a;
    memset(&a, 0, sizeof(a));
    a.value = value; a.weight = weight; a.step = vol_step;
    a.X = res[0]; a.Y = res[1]; a.Z = res[2];
    float *staging = reinterpret_cast<float *>(ws + RENDER_HEADER_BYTES);
    a.poses = staging;
    a.mask = reinterpret_cast<const unsigned *>(ws + render_mask_offset());
    a.WX = m.WX; a.BY = m.BY;
    a.rows = rows; a.cols = cols; a.tiles_x = (cols + 7) / 8; a.samples = plan.samples;
    a.fx = intr4[0]; a.fy = intr4[1]; a.cx = intr4[2]; a.cy = intr4[3];
    a.t_near = plan.t_near; a.dt = plan.step; a.voxel_size = voxel_size;
    a.min_weight = plan.min_weight; a.cull = o.cull ? 1 : 0;
    a.depth = depth_f32; a.depth16 = depth_u16; a.normal = normal; a.shade = shade; a.counts = counts4xP;
    std::vector<float> P((size_t)views * RENDER_POSE_FLOATS);
    for (int p = 0; p < views; ++p) {
        for (int k = 0; k < 9; ++k) P[(size_t)p * RENDER_POSE_FLOATS + k] = Rc2v9xP[9 * (size_t)p + k];
        for (int k = 0; k < 3; ++k) P[(size_t)p * RENDER_POSE_FLOATS + 9 + k] = tc2v3xP[3 * (size_t)p + k];
    }
    XS_CHECK(hipMemcpyAsync(staging, P.data(), P.size() * sizeof(float), hipMemcpyHostToDevice, st));   // (pageable: staged before the call returns)
    if (counts4xP) XS_CHECK(hipMemsetAsync(counts4xP, 0, (size_t)views * 4 * sizeof(unsigned), st));
    const unsigned tiles = (unsigned)a.tiles_x * (unsigned)((rows + 7) / 8);
    hipLaunchKernelGGL(k_render_views, dim3(tiles, 1, (unsigned)views), dim3(64), 0, st, a);
    XS_CHECK(hipGetLastError());
    return 0;
}
