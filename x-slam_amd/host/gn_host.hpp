// gn_host.hpp — the host's side of Gauss-Newton relocalisation (DESIGN.md sections 4.15, 4.16): the six seeded poses of a pass, the scaling of its
// sums, the damped 6 x 6 step that Gauss-Newton and Newton (newton_host.hpp) share, the batched loop both run, and the multi-start loop over it that
// the map alignment and the point registration run.  Pure host code, no device call and no HIP header: the orchestrator uses it between launches
// and tests/cxx/gn_selftest.cpp runs it under the sanitizers without a GPU.
#pragma once
#include "host_algebra.hpp"
#include <algorithm>
#include <vector>

namespace xs_host {

constexpr double GN_H = 1e-7;   // the complex seed step: H_ of xs_types.hpp (Internal.h:42)

// The six seeded volume-to-camera poses of one Gauss-Newton pass: v2c_k = inverse(se3Exp(i h e_k) * camera2volume), k = 0 .. 5.
// For a single seeded generator se3Exp takes its small-angle branch and is EXACTLY I + i h G_k (G_k: unit translation along axis k, or the hat matrix
// of axis k - 3), whose inverse is I - i h G_k up to a REAL term h^2 G_k^2 (1e-14: below the rounding of every entry it would touch).  So
//     v2c_k = v2c - i h (v2c G_k),        v2c = inverse(camera2volume) once,
// and v2c G_k is a column of v2c (translations) or two columns of its rotation swapped and signed (rotations): one 4x4 inverse and a few dozen products
// instead of six complex 4x4 products and six complex 4x4 cofactor inverses (4.9 -> 0.5 us on the build container's core; the host's side of a pass is
// what stands between two kernels).  The six poses share their real parts bit for bit by construction (the kernel counts a voxel only if every seeded
// evaluation keeps it): the seed goes into the imaginary parts alone — subtracting the whole product would also subtract its real part, a zero, and
// turn a real part of -0 into +0.  The imaginary parts equal those of the long form to rounding (tests/test_gauss_newton_gpu.py: the oracle twin, which inverts in
// double, and the analytic seeds of the per-pass test).
inline void gn_seeded_poses(const Matrix4cf &camera2volume, float R[6][18], float t[6][6]) {
    const Matrix4cf v2c = inverse(camera2volume);
    const hostComplex ih(0.f, (float)GN_H);
    for (int k = 0; k < 6; ++k) {
        hostComplex Rk[3][3], tk[3];
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) Rk[i][j] = v2c.m[i][j]; tk[i] = v2c.m[i][3]; }
        if (k < 3) {
            for (int i = 0; i < 3; ++i) tk[i].imag(tk[i].imag() - (ih * v2c.m[i][k]).imag());   // (v2c G_k): column 3 = column k of the rotation
        } else {
            const int a = k - 3, b = (a + 1) % 3, c = (a + 2) % 3;                           // hat(e_a): (c, b) = +1, (b, c) = -1
            for (int i = 0; i < 3; ++i) {
                Rk[i][b].imag(Rk[i][b].imag() - (ih * v2c.m[i][c]).imag());                  // (R hat)(i, b) = R(i, c)
                Rk[i][c].imag(Rk[i][c].imag() + (ih * v2c.m[i][b]).imag());                  // (R hat)(i, c) = -R(i, b)
            }
        }
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) { R[k][(i * 3 + j) * 2] = Rk[i][j].real(); R[k][(i * 3 + j) * 2 + 1] = Rk[i][j].imag(); }
            t[k][2 * i] = tk[i].real(); t[k][2 * i + 1] = tk[i].imag();
        }
    }
}
// the kernel's sums of the seeded imaginary parts -> derivative sums: divided by h^2 (J^T J) and h (J^T r)
inline void gn_scale_sums(const double *raw, double out29[29]) {
    const double ih = 1.0 / (double)(float)GN_H;
    for (int i = 0; i < 21; ++i) out29[i] = raw[i] * ih * ih;
    for (int i = 21; i < 27; ++i) out29[i] = raw[i] * ih;
    out29[27] = raw[27]; out29[28] = raw[28];
}

// One damped step on the scaled sums s = {A upper triangle (21), g (6), sum r^2, count}: (A + damping diag(A)) delta = -g by Cholesky, then
// camera2volume <- se3Exp(delta) camera2volume.  false, camera2volume untouched: fewer than six voxels (nothing to align to), or the damped
// system is not positive definite.
inline bool damped_spd6_step(const double s[29], double damping, Matrix4cf &camera2volume) {
    if (s[28] < 6) return false;
    double A[36], b[6], x[6];
    int q = 0;
    for (int j = 0; j < 6; ++j)
        for (int k = j; k < 6; ++k, ++q) { A[j * 6 + k] = s[q]; A[k * 6 + j] = s[q]; }
    for (int k = 0; k < 6; ++k) { A[k * 6 + k] *= 1.0 + damping; b[k] = -s[21 + k]; }
    if (!solve_spd6(A, b, x)) return false;
    hostComplex xi[6];
    for (int k = 0; k < 6; ++k) xi[k] = hostComplex((float)x[k], 0.f);
    camera2volume = se3Exp(xi) * camera2volume;
    return true;
}

// One host step of the Gauss-Newton loop on pass p's sums: the loss goes into the history; then 1 = the loop is finished (p was the final loss
// pass), -1 = it failed (nothing to align to, or the damped system is not positive definite), 0 = camera2volume took the step, go on.
inline int gn_loop_step(const double s[29], int p, int iterations, float damping, xs_host::Matrix4cf &camera2volume, std::vector<double> *loss_history) {
    if (loss_history) loss_history->push_back(s[28] > 0 ? s[27] / s[28] : 0.0);
    if (p == iterations) return 1;                        // the final loss pass
    return damped_spd6_step(s, (double)damping, camera2volume) ? 0 : -1;
}

// The batched loop of F frames against a fixed map.  evaluate(frames, n, sums) runs one launch for the n <= chunk frames `frames` and writes
// their n x 29 scaled sums; step(f, s, p) steps frame f's pose on its sums s of pass p and says whether it did.  A pass evaluates the frames
// still active in chunks, in order; a frame's loss goes into loss_history[f] (null: no history, and no final loss pass); a frame with fewer
// than six voxels, or whose step fails, drops out with ok[f] = 0; one that took its last step, or reached the loss pass, ends with ok[f] = 1.
// Returns the number of frames that ended ok.
template <class Evaluate, class Step>
int gn_batch_loop(int F, int iterations, std::vector<double> *loss_history, int *ok, int chunk, Evaluate &&evaluate, Step &&step) {
    for (int f = 0; f < F; ++f) ok[f] = 0;
    const int passes = iterations + (loss_history ? 1 : 0);   // (the last one only reports the loss the loop ended at)
    if (passes <= 0) { for (int f = 0; f < F; ++f) ok[f] = 1; return F; }
    std::vector<int> active((size_t)F);
    for (int f = 0; f < F; ++f) active[(size_t)f] = f;
    std::vector<double> sums((size_t)chunk * 29);
    for (int p = 0; p < passes && !active.empty(); ++p) {
        std::vector<int> next;
        for (size_t c0 = 0; c0 < active.size(); c0 += (size_t)chunk) {   // one launch per chunk of the frames still active
            const int n = (int)std::min(active.size() - c0, (size_t)chunk);
            evaluate(&active[c0], n, sums.data());
            for (int i = 0; i < n; ++i) {
                const int f = active[c0 + (size_t)i];
                const double *s = &sums[(size_t)i * 29];
                if (loss_history) loss_history[f].push_back(s[28] > 0 ? s[27] / s[28] : 0.0);
                if (p == iterations) { ok[f] = 1; continue; }   // the final loss pass
                if (s[28] < 6 || !step(f, s, p)) continue;      // nothing to align to, or no step: the frame fails
                if (p + 1 == passes) ok[f] = 1;                 // (no loss pass: the last step ends the loop)
                else next.push_back(f);
            }
        }
        active.swap(next);
    }
    return (int)std::count(ok, ok + F, 1);
}

struct GnMultistart {
    int win = -1, ended_ok = 0, passes = 0;   // the winning start (-1: none), the starts that could have won, the evaluate calls made
    double sums[29] = {};                      // the winner's sums of its last pass
    std::vector<double> history;               // and its loss per pass
};
// gn_batch_loop over the N starts of one problem (evaluate and step as it takes them), and the start that wins: the one that ended ok, with at
// least six voxels in its last pass too (gn_batch_loop lets the loss pass end ok whatever it counts: a start that its last step, or no step at
// all, left off the map is no result), with the highest S = count - sum r^2 (relocalize_global's score; ties: the lower index).  loss_pass: a
// last pass that only reports the loss, so the winner is picked where it ended; without it the sums are those the last step was taken from,
// and iterations = 0 launches nothing and nobody wins.
template <class Evaluate, class Step>
GnMultistart gn_multistart(int N, int iterations, int chunk, bool loss_pass, Evaluate &&evaluate, Step &&step) {
    GnMultistart r;
    std::vector<std::vector<double>> history((size_t)N);
    std::vector<double> last((size_t)N * 29, 0.0);
    std::vector<int> ok((size_t)N, 0);
    gn_batch_loop(N, iterations, loss_pass ? history.data() : nullptr, ok.data(), chunk, [&](const int *starts, int n, double *sums) {
        evaluate(starts, n, sums);
        ++r.passes;
        for (int i = 0; i < n; ++i) std::copy(sums + 29 * i, sums + 29 * i + 29, &last[(size_t)starts[i] * 29]);
    }, step);
    auto S = [&](int n) { return last[(size_t)n * 29 + 28] - last[(size_t)n * 29 + 27]; };
    for (int n = 0; n < N; ++n) {
        if (!ok[(size_t)n] || last[(size_t)n * 29 + 28] < 6) continue;
        ++r.ended_ok;
        if (r.win < 0 || S(n) > S(r.win)) r.win = n;
    }
    if (r.win < 0) return r;
    std::copy(&last[(size_t)r.win * 29], &last[(size_t)r.win * 29] + 29, r.sums);
    r.history = history[(size_t)r.win];
    return r;
}
// report[0 .. 5] of a multi-start call: {the winner's index, its count, sum r^2 and mean loss (as the caller cleared them without a winner),
// evaluate calls, starts that ended ok}
inline void gn_multistart_report(const GnMultistart &r, double *report) {
    if (!report) return;
    report[4] = (double)r.passes; report[5] = (double)r.ended_ok;
    if (r.win >= 0) { report[0] = (double)r.win; report[1] = r.sums[28]; report[2] = r.sums[27]; report[3] = r.sums[28] > 0 ? r.sums[27] / r.sums[28] : 0.0; }
}

}  // namespace xs_host
