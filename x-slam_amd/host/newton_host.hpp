// newton_host.hpp — the host's side of the exact-Hessian (Newton) relocalisation: the 21 dual-complex seeded poses of one pass of
// xs_tsdf_pose_hessian_band and the step taken on its 29 sums.  Pure host code, no device call: the orchestrator
// uses it between launches and the C ABI exposes it as xs_host_newton_seeded_poses / xs_host_newton_step so it is tested without a GPU.
#pragma once
#include "gn_host.hpp"

namespace xs_host {

constexpr double NEWTON_H = 1e-6;   // the dual-complex seed step (DoubleComplex.cpp:61-66)

// se(3) generator k of the twist (t_x, t_y, t_z, omega_x, omega_y, omega_z) as a 4 x 4 matrix
inline void newton_generator(int k, double G[4][4]) {
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) G[i][j] = 0.0;
    if (k < 3) { G[k][3] = 1.0; return; }
    const int a = k - 3, b = (a + 1) % 3, c = (a + 2) % 3;   // hat(e_a): (c, b) = +1, (b, c) = -1
    G[c][b] = 1.0; G[b][c] = -1.0;
}
inline void newton_matmul4(const double A[4][4], const double B[4][4], double C[4][4]) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += A[i][k] * B[k][j];
            C[i][j] = s;
        }
}

// The 21 dual-complex volume-to-camera poses of one pass, pair (a, b), a <= b, row-major: with v2c = inverse(camera2volume) (one 4 x 4
// inverse, its real part as float) and G_k the generators,
//     real v2c      eps1  -h v2c G_a      eps2  -h v2c G_b      eps1 eps2  h^2 v2c (G_a G_b + G_b G_a) / 2,
// the expansion of inverse(se3Exp(theta) camera2volume) = v2c exp(-theta^) to second order: hessian() / h^2 of the loss is then the exact
// d2L / dtheta_a dtheta_b at theta = 0, in the parameterisation the step updates in.  The eps parts are formed in double from the float v2c
// and rounded once; every column of G_a and of G_a G_b + G_b G_a has at most one entry that is not zero, so each is one rounded product.
// All 21 real parts are the same bits by construction (the kernel counts a voxel only if every evaluation keeps it).
// R: 36 floats per pose (3 x 3 groups of (re.re, re.im, im.re, im.im)), t: 12.
inline void newton_seeded_poses(const Matrix4cf &camera2volume, float R[21][36], float t[21][12]) {
    const Matrix4cf inv = inverse(camera2volume);
    double M[4][4], G[6][4][4];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) M[i][j] = (double)inv.m[i][j].real();
    for (int k = 0; k < 6; ++k) newton_generator(k, G[k]);
    const double h = NEWTON_H;
    double Mh[4][4], Mhh[4][4], E[6][4][4];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { Mh[i][j] = -h * M[i][j]; Mhh[i][j] = h * h * M[i][j]; }
    for (int k = 0; k < 6; ++k) newton_matmul4(Mh, G[k], E[k]);
    int p = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++p) {
            double AB[4][4], BA[4][4], S[4][4], X[4][4];
            newton_matmul4(G[a], G[b], AB);
            newton_matmul4(G[b], G[a], BA);
            for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) S[i][j] = AB[i][j] + BA[i][j];
            newton_matmul4(Mhh, S, X);
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 4; ++j) {
                    float *g = j < 3 ? &R[p][(i * 3 + j) * 4] : &t[p][i * 4];
                    g[0] = (float)M[i][j]; g[1] = (float)E[a][i][j]; g[2] = (float)E[b][i][j]; g[3] = (float)(X[i][j] / 2.0);
                }
            }
        }
}

// the kernel's raw sums -> derivatives: H / h^2, g / h
inline void newton_scale_sums(const double *raw, double out29[29]) {
    const double ih = 1.0 / NEWTON_H;
    for (int i = 0; i < 21; ++i) out29[i] = raw[i] * ih * ih;
    for (int i = 21; i < 27; ++i) out29[i] = raw[i] * ih;
    out29[27] = raw[27]; out29[28] = raw[28];
}

// One Newton step on the scaled sums s = {H upper triangle (21), g (6), sum r^2, count}: gn_host.hpp's damped step with the exact Hessian.
// false, camera2volume untouched: fewer than six voxels, or the damped system is not positive definite (away from the optimum the exact
// Hessian can be indefinite; the caller then takes a Gauss-Newton step).
inline bool newton_step(const double s[29], double damping, Matrix4cf &camera2volume) { return damped_spd6_step(s, damping, camera2volume); }

}  // namespace xs_host
