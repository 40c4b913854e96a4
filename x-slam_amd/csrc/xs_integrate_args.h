// xs_integrate_args.h — host only: how an IntegrateArgs (xs_integrate_voxel.h) is filled.  The frustum and its column clip, the streamed
// classes' margins, and the one builder the integrate call, the classification entry points and re-integration start from.
#pragma once
#include <string.h>
#include <algorithm>
#include <cmath>
#include "xs_integrate_voxel.h"
#include "xs_env.h"

// the padded view frustum of a's pose as half-spaces of the voxel-index space, and the same planes solved for k (struct Frustum, ClipPlanes)
static void set_plane(Frustum &f, int P, const float T[3], const float M[3][3], float cxk, float cyk, float czk, float sl) {
    f.alpha[P] = cxk * T[0] + cyk * T[1] + czk * T[2];  // cxk*X + cyk*Y + czk*c >= -sl
    f.bx[P] = cxk * M[0][0] + cyk * M[1][0] + czk * M[2][0];
    f.by[P] = cxk * M[0][1] + cyk * M[1][1] + czk * M[2][1];
    f.bz[P] = cxk * M[0][2] + cyk * M[1][2] + czk * M[2][2];
    f.slack[P] = sl;
}
static void host_frustum(IntegrateArgs &a) {
    Frustum &f = a.fr;
    const float vs = a.voxel_size, fx = a.intr.fx, fy = a.intr.fy;
    const float ul = (1.5f - a.intr.cx) - 2.f, uh = ((a.dcols - 0.5f) - a.intr.cx + 1.0f) + 2.f;
    const float vl = (1.5f - a.intr.cy) - 2.f, vh = ((a.drows - 0.5f) - a.intr.cy + 1.0f) + 2.f;
    // camera coordinates (real parts): p_r = t_r + vs * (R_r0*i + R_r1*j + R_r2*k)
    const float T[3] = {a.t.x.re, a.t.y.re, a.t.z.re};
    const float M[3][3] = {{a.R.data[0].x.re * vs, a.R.data[0].y.re * vs, a.R.data[0].z.re * vs},
                           {a.R.data[1].x.re * vs, a.R.data[1].y.re * vs, a.R.data[1].z.re * vs},
                           {a.R.data[2].x.re * vs, a.R.data[2].y.re * vs, a.R.data[2].z.re * vs}};
    const float ext = (float)std::max(a.X, std::max(a.Y, a.Z));
    const float mag0 = fabsf(T[0]) + (fabsf(M[0][0]) + fabsf(M[0][1]) + fabsf(M[0][2])) * ext;
    const float mag1 = fabsf(T[1]) + (fabsf(M[1][0]) + fabsf(M[1][1]) + fabsf(M[1][2])) * ext;
    const float mag2 = fabsf(T[2]) + (fabsf(M[2][0]) + fabsf(M[2][1]) + fabsf(M[2][2])) * ext;
    const float rel = 2e-3f;
    set_plane(f, 0, T, M, 0.f, 0.f, 1.f, rel * mag2);                                      // c >= 0
    set_plane(f, 1, T, M, fx, 0.f, -ul, rel * (fabsf(fx) * mag0 + fabsf(ul) * mag2));      // fx*X >= ul*c
    set_plane(f, 2, T, M, -fx, 0.f, uh, rel * (fabsf(fx) * mag0 + fabsf(uh) * mag2));      // fx*X <= uh*c
    set_plane(f, 3, T, M, 0.f, fy, -vl, rel * (fabsf(fy) * mag1 + fabsf(vl) * mag2));      // fy*Y >= vl*c
    set_plane(f, 4, T, M, 0.f, -fy, vh, rel * (fabsf(fy) * mag1 + fabsf(vh) * mag2));      // fy*Y <= vh*c
    set_plane(f, 5, T, M, 0.f, 0.f, -1.f, rel * mag2);                                     // c <= cfar (cfar added on the device)
    // the column clip's form of the same planes (see ClipPlanes)
    ClipPlanes &c = a.cp;
    c.kinds = 0; c.far_scale = 1.0f;
    for (int p = 0; p < 6; ++p) {
        // a slope along z too small to divide by is dropped from the column clip; what it could
        // contribute over the whole column goes into the slack instead
        const float scale = fabsf(f.alpha[p]) + (fabsf(f.bx[p]) + fabsf(f.by[p])) * ext + f.slack[p] + (p == 5 ? 6.f : 0.f);
        if (fabsf(f.bz[p]) * ext <= 1e-6f * scale) {
            f.slack[p] += fabsf(f.bz[p]) * ext;
            c.A[p] = f.alpha[p] + f.slack[p]; c.B[p] = f.bx[p]; c.C[p] = f.by[p];
        } else {
            const double s = -1.0 / (double)f.bz[p];
            c.A[p] = (float)(((double)f.alpha[p] + (double)f.slack[p]) * s);
            c.B[p] = (float)(f.bx[p] * s); c.C[p] = (float)(f.by[p] * s);
            if (p == 5) c.far_scale = (float)s;
            c.kinds |= (f.bz[p] > 0.f ? 1 : 2) << (2 * p);
        }
    }
}

// Where the streamed classes' numeric shortcuts hold (valid_slot_request, xs_integrate_stream.h, has the derivation): the margin for this
// sensor — never below 1 / 2048 px — and whether the launch may class boxes EDGE / SPECKLE at all.  Needs a.drows / dcols / intr / R / t /
// X / Y / Z / voxel_size.
#define XS_NEAR_MARGIN_MIN 0.00048828125f
static void stream_margins(IntegrateArgs &a) {
    const float E = fmaxf((float)a.dcols + fabsf(a.intr.cx), (float)a.drows + fabsf(a.intr.cy));
    int e = 0;
    (void)frexpf(E, &e);                                       // E = m 2^e, m in [0.5, 1): ulp(E) = 2^(e - 24)
    a.near_margin = fmaxf(ldexpf(1.0f, e - 21), XS_NEAR_MARGIN_MIN);   // 8 ulp(E)
    const double ext[3] = {(double)a.X * a.voxel_size, (double)a.Y * a.voxel_size, (double)a.Z * a.voxel_size};
    auto im_row = [&](const cfloat3 &r, const cfloat &t) { return fabs((double)r.x.im) * ext[0] + fabs((double)r.y.im) * ext[1] + fabs((double)r.z.im) * ext[2] + fabs((double)t.im); };
    const double imX = im_row(a.R.data[0], a.t.x), imY = im_row(a.R.data[1], a.t.y), imC = im_row(a.R.data[2], a.t.z);
    const double cmin = XS_EDGE_CMIN;
    const double bound = (double)E * (imC / cmin) * (imC / cmin) + fmax(fabs((double)a.intr.fx) * imX, fabs((double)a.intr.fy) * imY) * imC / (cmin * cmin);
    if (!(E < 8192.0f) || !(bound <= (double)a.near_margin / 16.0)) a.kflags |= KF_NO_TESTED_STREAM;   // (NaN: no)
}
// What the arguments of every launch that goes through the per-voxel contract have in common — the integrate call, the classification on its
// own and each op of a re-integration: the image size, the volume and the slab, the band, pose and intrinsics, the frustum with its column
// clip, the streamed classes' margin (which may set KF_NO_TESTED_STREAM: a caller ORs its own flags into kflags afterwards) and the brick
// grid.  Everything else is zero; a caller then sets what is its alone.
static void integrate_args(IntegrateArgs &a, int rows, int cols, const float *intr4, const int *res, float voxel_size, const float *Rv2c18,
                           const float *tv2c6, float tranc_dist, int z0, int z1, const float *depth_max_dev) {
    memset(&a, 0, sizeof(a));
    a.drows = rows; a.dcols = cols;
    a.X = res[0]; a.Y = res[1]; a.Z = res[2]; a.z0 = z0; a.z1 = z1;
    a.tranc_dist = tranc_dist; a.tranc_dist_inv = 1.0f / tranc_dist;
    load_mat(Rv2c18, a.R); load_vec(tv2c6, a.t);
    a.intr = Intr{intr4[0], intr4[1], intr4[2], intr4[3]};
    a.voxel_size = voxel_size; a.depth_max = depth_max_dev;
    host_frustum(a);
    stream_margins(a);
    static const int env_bz = exp_env_int("XS_BRICK_Z", 0);  // tuning aid: planes per brick
    a.brick_z = (env_bz >= 2 && env_bz <= 64) ? env_bz : BRICK_Z;
    a.bricks_x = div_up(a.X, BRICK_X); a.bricks_y = div_up(a.Y, BRICK_Y); a.bricks_z = div_up(z1 - z0, a.brick_z);
}
