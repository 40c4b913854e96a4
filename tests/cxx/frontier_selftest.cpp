// frontier_selftest.cpp — the frontier side of x-slam_amd/host/view_host.hpp (no GPU) built with -fsanitize=address,undefined and run:
// the voxel-centre round trip over the index range a volume can have, centroids of cluster records, the Halton directions and standpoints,
// the look-at rotation with its fallback hint, and the selection by size.
//
// Float bounds, each from the operation count (eps = 2^-24, the relative error of one float32 rounding):
//   direction   computed in float64 and rounded once per component: |d| = 1 within 3 roundings of components below 1 -> 3 eps, taken as 4 eps
//   standpoint  p = c + s d: one product and one sum per axis, so |p - c| = s |d| within (2 eps per axis of magnitude <= |c| + s) -> the
//               distance is s within s * 4 eps + 2 sqrt(3) eps (|c| + s)
//   look_at     float64 throughout, nine final roundings of entries below 1 in magnitude: each entry is off by at most eps, so a dot
//               product of two columns is off by at most 2 eps sum |a_r| |b_r| <= 2 eps (+ float64 noise), an entry of x cross y by 4 eps
//               -> 8 eps for both; the optical axis is off from the true direction by a vector of length at most sqrt(3) eps, so its
//               cross product with that direction is no longer -> 2 eps
#include "view_host.hpp"
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

using namespace xs_host;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static const double EPS = 5.9604644775390625e-8;   // 2^-24

static void check_rotation(const float R[9], const float pos[3], const float target[3]) {
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double dot = 0.0;
            for (int r = 0; r < 3; ++r) dot += (double)R[3 * r + a] * (double)R[3 * r + b];
            CHECK(std::fabs(dot - (a == b ? 1.0 : 0.0)) <= 8.0 * EPS);
        }
    // right-handed: x cross y = z
    const double cx = (double)R[3] * R[7] - (double)R[6] * R[4], cy = (double)R[6] * R[1] - (double)R[0] * R[7], cz = (double)R[0] * R[4] - (double)R[3] * R[1];
    CHECK(std::fabs(cx - R[2]) <= 8.0 * EPS && std::fabs(cy - R[5]) <= 8.0 * EPS && std::fabs(cz - R[8]) <= 8.0 * EPS);
    double d[3], n = 0.0;
    for (int a = 0; a < 3; ++a) { d[a] = (double)target[a] - (double)pos[a]; n += d[a] * d[a]; }
    n = std::sqrt(n);
    const double z[3] = {R[2], R[5], R[8]};
    const double px = (z[1] * d[2] - z[2] * d[1]) / n, py = (z[2] * d[0] - z[0] * d[2]) / n, pz = (z[0] * d[1] - z[1] * d[0]) / n;
    CHECK(std::sqrt(px * px + py * py + pz * pz) <= 2.0 * EPS);                   // parallel to target - pos ...
    CHECK(z[0] * d[0] + z[1] * d[1] + z[2] * d[2] > 0.0);                        // ... and towards it
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // the voxel-centre round trip: every index a volume can have (Y and Z end at 65535; X beyond that leaves no room for the others), at
    // binary and at awkward voxel sizes, the test scenes' among them
    for (float vs : {0.125f, 0.12f, 3.0f / 64.0f, 0.005859375f, 0.0117f, 0.03f, 1e-3f, 0.7f, 3.0f}) {
        int bad = 0;
        for (int v = 0; v <= 65535; ++v) bad += (int)std::floor(voxel_centre(v, vs) / vs) != v;
        CHECK(bad == 0);
    }
    CHECK(voxel_centre(0, 0.125f) == 0.0625f && voxel_centre(7, 0.5f) == 3.75f);
    // centroids: sums over count, half a voxel up
    const unsigned long long one[8] = {300, 1500, 1500ull * 299 / 2, 1500, 3000, 0, 0, 0};
    float c[3];
    CHECK(frontier_centroid(one, 0.5f, c) && c[0] == (149.5f + 0.5f) * 0.5f && c[1] == 1.5f * 0.5f && c[2] == 2.5f * 0.5f);
    const unsigned long long third[8] = {7, 3, 1, 2, 65535ull * 3, 0, 0, 0};
    CHECK(frontier_centroid(third, 0.12f, c) && c[0] == ((float)(1.0 / 3.0) + 0.5f) * 0.12f && c[1] == ((float)(2.0 / 3.0) + 0.5f) * 0.12f && c[2] == 65535.5f * 0.12f);
    const unsigned long long empty[8] = {7, 0, 0, 0, 0, 0, 0, 0};
    c[0] = -1.f;
    CHECK(!frontier_centroid(empty, 0.12f, c) && c[0] == -1.f);
    // the largest sums a record can hold convert without overflow
    const unsigned long long big[8] = {0, 4294967294ull, 4294967294ull * 65535ull, 0, 4294967294ull, 0, 0, 0};
    CHECK(frontier_centroid(big, 1.f, c) && c[0] == 65535.5f && c[1] == 0.5f && c[2] == 1.5f);
    // Halton: the first elements, exactly for base 2
    CHECK(halton(1, 2) == 0.5 && halton(2, 2) == 0.25 && halton(3, 2) == 0.75 && halton(4, 2) == 0.125 && halton(0, 2) == 0.0);
    CHECK(std::fabs(halton(1, 3) - 1.0 / 3.0) < 1e-15 && std::fabs(halton(2, 3) - 2.0 / 3.0) < 1e-15 && std::fabs(halton(3, 3) - 1.0 / 9.0) < 1e-15);
    // directions: unit length, z = 1 - 2 u, all different; standpoints: the standoff distance
    std::vector<float> seen;
    const float cen[3] = {3.84f, 1.2f, 6.5f};
    for (int j = 0; j < 64; ++j) {
        float d[3], p[3];
        frontier_direction(j, d);
        const double n = std::sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]);
        CHECK(std::fabs(n - 1.0) <= 4.0 * EPS);
        CHECK(d[2] == (float)(1.0 - 2.0 * halton((unsigned)j + 1u, 2u)));
        for (size_t k = 0; k + 2 < seen.size(); k += 3) CHECK(!(seen[k] == d[0] && seen[k + 1] == d[1] && seen[k + 2] == d[2]));
        seen.insert(seen.end(), d, d + 3);
        for (float s : {0.f, 0.25f, 1.f, 2.5f}) {
            frontier_standpoint(cen, s, j, p);
            double dist = 0.0, cn = 0.0;
            for (int a = 0; a < 3; ++a) { dist += ((double)p[a] - cen[a]) * ((double)p[a] - cen[a]); cn += (double)cen[a] * cen[a]; }
            CHECK(std::fabs(std::sqrt(dist) - s) <= s * 4.0 * EPS + 2.0 * std::sqrt(3.0) * EPS * (std::sqrt(cn) + s));
            CHECK(s != 0.f || (p[0] == cen[0] && p[1] == cen[1] && p[2] == cen[2]));
        }
    }
    float d0[3];
    frontier_direction(0, d0);                                                  // u = 1/2, v = 1/3: z = 0, phi = 120 degrees
    CHECK(d0[2] == 0.f && std::fabs(d0[0] + 0.5) <= EPS && std::fabs(d0[1] - std::sqrt(0.75)) <= EPS);
    // look_at: orthonormal, right-handed, the optical axis towards the target, image-down as close to the hint as it can be
    const float down[3] = {0.f, 1.f, 0.f}, side[3] = {1.f, 0.f, 0.f};
    float R[9];
    for (int j = 0; j < 64; ++j) {
        float p[3];
        frontier_standpoint(cen, 1.5f, j, p);
        CHECK(look_at(p, cen, down, side, R));
        check_rotation(R, p, cen);
        const double along = ((double)cen[1] - p[1]) / 1.5;                     // the hint's component along the view
        if (std::fabs(along) <= 0.98) CHECK(R[4] > 0.f && R[3] == 0.f);            // y has a positive component along the hint, x none
    }
    // the fallback: looking straight along the hint (and within 8.1 degrees of it, either way round) the side hint is used instead
    const float origin[3] = {0.f, 0.f, 0.f};
    for (float sgn : {1.f, -1.f})
        for (float tilt : {0.f, 0.1f, 0.14f}) {                                 // atan(0.14) = 7.97 degrees
            const float tgt[3] = {0.f, sgn, tilt};
            CHECK(look_at(origin, tgt, down, side, R));
            check_rotation(R, origin, tgt);
            CHECK(R[0] == 0.f);                                                  // x is across the side hint ...
            CHECK(std::fabs((double)R[1] - 1.0) <= 8.0 * EPS);                   // ... and image-down is the side hint itself (it is orthogonal to z here)
        }
    const float tgt_out[3] = {0.f, 1.f, 0.15f};                                 // atan(0.15) = 8.53 degrees: the hint holds
    CHECK(look_at(origin, tgt_out, down, side, R));
    check_rotation(R, origin, tgt_out);
    CHECK(std::fabs((double)R[0] - 1.0) <= 8.0 * EPS && R[4] > 0.f);             // x = down cross z = +x, y keeps a component along the hint
    // refusals: nothing is written
    R[0] = 42.f;
    CHECK(!look_at(origin, origin, down, side, R) && R[0] == 42.f);
    const float bad[3] = {nan, 0.f, 0.f}, zero[3] = {0.f, 0.f, 0.f}, up[3] = {0.f, 0.f, 1.f};
    CHECK(!look_at(origin, bad, down, side, R) && !look_at(bad, cen, down, side, R) && R[0] == 42.f);
    CHECK(!look_at(origin, up, zero, bad, R) && !look_at(origin, up, up, up, R) && R[0] == 42.f);
    CHECK(look_at(origin, up, zero, side, R) && look_at(origin, up, bad, side, R));   // an unusable first hint: the second
    // selection by size
    const std::vector<unsigned long long> recs = {5, 3, 0, 0, 0, 0, 0, 0, 9, 8, 0, 0, 0, 0, 0, 0, 11, 1, 0, 0, 0, 0, 0, 0, 40, 8, 0, 0, 0, 0, 0, 0};
    int keep[4] = {-1, -1, -1, -1};
    CHECK(frontier_select(recs.data(), 4, 8, keep) == 2 && keep[0] == 1 && keep[1] == 3 && keep[2] == -1);
    CHECK(frontier_select(recs.data(), 4, 0, keep) == 4 && frontier_select(recs.data(), 4, 9, keep) == 0 && frontier_select(recs.data(), 0, 0, keep) == 0);
    if (!failures) std::printf("all checks held\n");
    return failures ? 1 : 0;
}
