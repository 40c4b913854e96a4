// align_host.hpp — the host's side of aligning a second TSDF map to the volume: the six complex-seeded index maps of a
// Gauss-Newton pass over the band and the damped step on its sums.  No device call and no HIP header: the orchestrator uses it between
// launches and tests/cxx/align_selftest.cpp runs all of it under the sanitizers without a GPU.
#pragma once
#include "gn_host.hpp"
#include "merge_host.hpp"

namespace xs_host {

// the report of an alignment call that has no result (yet): zeros, and -1 where the winner's index goes
inline void align_report_clear(double *report, int n) {
    if (!report) return;
    for (int i = 0; i < n; ++i) report[i] = 0.0;
    report[0] = -1.0;
}

// The six seeded maps of one pass: T_k = (I + i h G_k) T, k = 0 .. 5 (G_k: unit translation along axis k, or the hat matrix of axis k - 3:
// gn_seeded_poses' order), each put through merge_affine's formula.  out[k]: the 12 entries of xform12 as (re, im) pairs.  The real part of T_k
// is T itself, so the 12 real parts are merge_affine(T) bit for bit for every k; the seed goes into the imaginary parts alone: Im T_k = h G_k T
// has, for a translation, h at (k, 3) and nothing else, and for a rotation about axis a (b = a + 1, c = a + 2 mod 3; hat(e_a): (c, b) = +1,
// (b, c) = -1) row c = h T(b, :) and row b = -h T(c, :).  merge_affine's formula is linear in T apart from its constant - 0.5, which has no
// imaginary part.  Float64 throughout, each part rounded once to float32.  h is GN_H as the kernels hold it (a float32), so that gn_scale_sums
// undoes it exactly.  False, nothing written: merge_affine's refusals.
inline bool align_seeded_maps(const double *T16, double vs_this, double vs_other, float out[6][24]) {
    float re[12];
    if (!out || !merge_affine(T16, vs_this, vs_other, re)) return false;
    const double h = (double)(float)GN_H, half = 0.5 * vs_this;
    for (int k = 0; k < 6; ++k) {
        double I[3][4] = {};   // rows 0 .. 2 of Im T_k
        if (k < 3) {
            I[k][3] = h;
        } else {
            const int a = k - 3, b = (a + 1) % 3, c = (a + 2) % 3;
            for (int j = 0; j < 4; ++j) { I[c][j] = h * T16[4 * b + j]; I[b][j] = -(h * T16[4 * c + j]); }
        }
        double im[12];
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) im[3 * a + b] = I[a][b] * vs_this / vs_other;
            im[9 + a] = (((I[a][0] * half + I[a][1] * half) + I[a][2] * half) + I[a][3]) / vs_other;
        }
        for (int i = 0; i < 12; ++i) { out[k][2 * i] = re[i]; out[k][2 * i + 1] = (float)im[i]; }
    }
    return true;
}

// exp of the twist delta = (v, omega) as a real 4 x 4, row-major, float64: R = I + A W + B W^2, t = (I + B W + C W^2) v with W = hat(omega),
// A = sin(th) / th, B = (1 - cos(th)) / th^2, C = (th - sin(th)) / th^3; below th = 1e-4 the three by their series (the next terms are th^4
// / 120 and smaller: under 1e-18)
inline void align_se3_exp(const double delta[6], double E[16]) {
    const double *v = delta, *w = delta + 3;
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = std::sqrt(th2);
    double A, B, C;
    if (th < 1e-4) { A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; C = 1.0 / 6.0 - th2 / 120.0; }
    else { A = std::sin(th) / th; B = (1.0 - std::cos(th)) / th2; C = (th - std::sin(th)) / (th2 * th); }
    const double W[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
    double W2[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W2[i][j] = (W[i][0] * W[0][j] + W[i][1] * W[1][j]) + W[i][2] * W[2][j];
    for (int i = 0; i < 3; ++i) {
        double t = 0.0;
        for (int j = 0; j < 3; ++j) {
            const double id = i == j ? 1.0 : 0.0;
            E[4 * i + j] = (id + A * W[i][j]) + B * W2[i][j];
            t += ((id + B * W[i][j]) + C * W2[i][j]) * v[j];
        }
        E[4 * i + 3] = t;
    }
    E[12] = 0.0; E[13] = 0.0; E[14] = 0.0; E[15] = 1.0;
}

// One damped step on the scaled sums s = {A upper triangle (21), g (6), sum r^2, count}: damped_spd6_step's algebra, (A + damping diag(A)) delta
// = -g by Cholesky, then T <- exp(delta) T (rows 0 .. 2; the last row of T is kept).  false, T untouched: fewer than six voxels, or the damped
// system is not positive definite, or a step that is not finite.
inline bool align_step(const double s[29], double damping, double T16[16]) {
    if (!s || !T16 || s[28] < 6) return false;
    double A[36], b[6], x[6];
    int q = 0;
    for (int j = 0; j < 6; ++j)
        for (int k = j; k < 6; ++k, ++q) { A[j * 6 + k] = s[q]; A[k * 6 + j] = s[q]; }
    for (int k = 0; k < 6; ++k) { A[k * 6 + k] *= 1.0 + damping; b[k] = -s[21 + k]; }
    if (!solve_spd6(A, b, x)) return false;
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(x[k])) return false;
    double E[16], out[12];
    align_se3_exp(x, E);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            out[4 * i + j] = ((E[4 * i] * T16[j] + E[4 * i + 1] * T16[4 + j]) + E[4 * i + 2] * T16[8 + j]) + (j == 3 ? E[4 * i + 3] : 0.0);
            if (!std::isfinite(out[4 * i + j])) return false;
        }
    for (int i = 0; i < 12; ++i) T16[i] = out[i];
    return true;
}

}  // namespace xs_host
