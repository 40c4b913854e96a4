// align_search_host.hpp — the host's side of aligning two TSDF maps with no initial guess: the candidate transforms
// that xs_tsdf_score_transforms scores (a low-discrepancy cover of SO(3) with centroid-matched translations, and boxes about a kept transform),
// their ranking, and the centroid of a band index.  No device call and no HIP header, float64 and deterministic: the orchestrator uses it
// between launches and tests/cxx/align_search_selftest.cpp runs all of it under the sanitizers without a GPU.
// T everywhere: a real 4 x 4, row-major, taking a point of THIS map's volume frame (metres) to the OTHER map's, as merge_affine takes it.
#pragma once
#include <cmath>
#include <vector>
#include "score_host.hpp"

namespace xs_host {

// the radical inverse of i >= 1 in `base`
inline double align_halton(unsigned long long i, unsigned base) {
    double f = 1.0, r = 0.0;
    while (i > 0) {
        f /= (double)base;
        r += f * (double)(i % base);
        i /= base;
    }
    return r;
}

// Shoemake's map of the unit cube to uniformly distributed unit quaternions, as a rotation matrix (row-major)
inline void align_shoemake(double u1, double u2, double u3, double R[9]) {
    const double two_pi = 6.283185307179586476925286766559;
    const double a = std::sqrt(1.0 - u1), b = std::sqrt(u1);
    const double x = a * std::sin(two_pi * u2), y = a * std::cos(two_pi * u2), z = b * std::sin(two_pi * u3), w = b * std::cos(two_pi * u3);
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - z * w);       R[2] = 2.0 * (x * z + y * w);
    R[3] = 2.0 * (x * y + z * w);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - x * w);
    R[6] = 2.0 * (x * z - y * w);       R[7] = 2.0 * (y * z + x * w);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// exp of the axis-angle vector w as a rotation matrix (Rodrigues; the series below 1e-4 rad, as align_se3_exp)
inline void align_so3_exp(const double w[3], double R[9]) {
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = std::sqrt(th2);
    double A, B;
    if (th < 1e-4) { A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; }
    else { A = std::sin(th) / th; B = (1.0 - std::cos(th)) / th2; }
    const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double W2 = (W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j]) + W[3 * i + 2] * W[6 + j];
            R[3 * i + j] = ((i == j ? 1.0 : 0.0) + A * W[3 * i + j]) + B * W2;
        }
}

// n candidates with no guess: candidate i's rotation is Shoemake's map of (halton(i + 1, 2), halton(i + 1, 3), halton(i + 1, 5)); its
// translation takes this map's centroid onto the other's, c_other - R c_this, plus box_t (2 halton(i + 1, {7, 11, 13}) - 1).  False, nothing
// written: n < 1, a null pointer, an input that is not finite or a negative box.
inline bool align_search_free(int n, const double *centroid_this, const double *centroid_other, double box_t, double *T16xN) {
    if (n < 1 || !centroid_this || !centroid_other || !T16xN || !(box_t >= 0.0) || !std::isfinite(box_t)) return false;
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(centroid_this[a]) || !std::isfinite(centroid_other[a])) return false;
    static const unsigned tb[3] = {7, 11, 13};
    for (int i = 0; i < n; ++i) {
        const unsigned long long k = (unsigned long long)i + 1;
        double R[9];
        align_shoemake(align_halton(k, 2), align_halton(k, 3), align_halton(k, 5), R);
        double *T = T16xN + 16 * (size_t)i;
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) T[4 * a + b] = R[3 * a + b];
            const double Rc = (R[3 * a] * centroid_this[0] + R[3 * a + 1] * centroid_this[1]) + R[3 * a + 2] * centroid_this[2];
            T[4 * a + 3] = (centroid_other[a] - Rc) + box_t * (2.0 * align_halton(k, tb[a]) - 1.0);
        }
        T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
    }
    return true;
}

// n candidates about T: entry 0 is T itself (its 16 numbers copied); entry i >= 1, with u = 2 halton(i, {2, 3, 5, 7, 11, 13}) - 1, turns T by
// E = exp(box_r u[3:6]) about the image q = T pivot of `pivot` and shifts it by box_t u[0:3]: x -> E (T x - q) + q + box_t u[0:3].  False,
// nothing written: n < 1, a null pointer, an entry of T (rows 0 .. 2), a pivot or a box that is not finite, or a negative box.
inline bool align_search_around(const double *T16, const double *pivot, double box_t, double box_r, int n, double *T16xN) {
    if (n < 1 || !T16 || !pivot || !T16xN || !(box_t >= 0.0) || !(box_r >= 0.0) || !std::isfinite(box_t) || !std::isfinite(box_r)) return false;
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(T16[i])) return false;
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(pivot[a])) return false;
    double q[3];
    for (int a = 0; a < 3; ++a) q[a] = ((T16[4 * a] * pivot[0] + T16[4 * a + 1] * pivot[1]) + T16[4 * a + 2] * pivot[2]) + T16[4 * a + 3];
    for (int k = 0; k < 16; ++k) T16xN[k] = T16[k];
    static const unsigned base[6] = {2, 3, 5, 7, 11, 13};
    for (int i = 1; i < n; ++i) {
        double u[6], w[3], E[9];
        for (int k = 0; k < 6; ++k) u[k] = 2.0 * align_halton((unsigned long long)i, base[k]) - 1.0;
        for (int a = 0; a < 3; ++a) w[a] = box_r * u[3 + a];
        align_so3_exp(w, E);
        double *T = T16xN + 16 * (size_t)i;
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) T[4 * a + b] = (E[3 * a] * T16[b] + E[3 * a + 1] * T16[4 + b]) + E[3 * a + 2] * T16[8 + b];
            // E (t - q) + q + box_t u
            const double d0 = T16[3] - q[0], d1 = T16[7] - q[1], d2 = T16[11] - q[2];
            T[4 * a + 3] = (((E[3 * a] * d0 + E[3 * a + 1] * d1) + E[3 * a + 2] * d2) + q[a]) + box_t * u[a];
        }
        T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
    }
    return true;
}

// The min(keep, P) candidates with the highest S = count - sum r^2, best first, equal scores in index order: relocalize_global's rule
// (score_top_k).  Returns how many indices it wrote.
inline int align_search_rank(const double *out2xP, int P, int keep, int *idx_out) {
    if (!out2xP || !idx_out) return 0;
    const std::vector<int> order = score_top_k(out2xP, P, keep);
    for (size_t i = 0; i < order.size(); ++i) idx_out[i] = order[i];
    return (int)order.size();
}

// The centroid of the voxel centres of a band index's keys (x | y << 21 | z << 42): exact 64-bit integer sums, then (sum / count + 0.5)
// voxel_size in double.  False, nothing written: no entry, a null pointer.
inline bool band_centroid(const unsigned long long *keys, long long count, double voxel_size, double *out3) {
    if (!keys || !out3 || count < 1) return false;
    unsigned long long s[3] = {0, 0, 0};   // count < 2^42 entries of 21 / 22 bits each: no overflow
    for (long long i = 0; i < count; ++i) {
        const unsigned long long k = keys[i];
        s[0] += k & 0x1fffff; s[1] += (k >> 21) & 0x1fffff; s[2] += k >> 42;
    }
    for (int a = 0; a < 3; ++a) out3[a] = ((double)s[a] / (double)count + 0.5) * voxel_size;
    return true;
}

}  // namespace xs_host
