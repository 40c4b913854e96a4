// xs_host_capi.cpp — the C ABI's calls that take no instance (include/xslam_amd_pipeline.h): the two complex tables, the flat-YAML probe and
// every xs_host_*, the host's side of the kernels' contracts as the tests and the Python wrappers reach it.  CPU only, no device call.
#include "../../include/xslam_amd_pipeline.h"
#include "../csrc/xs_complex.h"
#include "DoubleComplex.h"
#include "kf_internal.hpp"
#include "align_host.hpp"
#include "align_search_host.hpp"
#include "merge_host.hpp"
#include "newton_host.hpp"
#include "register_host.hpp"
#include "register_search_host.hpp"
#include "sample_host.hpp"
#include <exception>

extern "C" {

// host DoubleComplex over arrays of (re.re, re.im, im.re, im.im) groups
int xs_host_double_complex_table(int op, long n, const float *a, const float *b, float *out) {
    for (long i = 0; i < n; ++i) {
        const DoubleComplex x(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]), y(b[4 * i], b[4 * i + 1], b[4 * i + 2], b[4 * i + 3]);
        DoubleComplex r;
        switch (op) {
            case 0: r = x + y; break;
            case 1: r = x - y; break;
            case 2: r = x * y; break;
            case 3: r = x / y; break;
            case 4: r = sqrt(x); break;
            case 5: r = DoubleComplex(abs(x)); break;
            case 6: r = exp(x); break;
            case 7: r = log(x); break;
            case 8: r = sin(x); break;
            case 9: r = cos(x); break;
            case 10: r = pow(x, y.real().real()); break;
            case 11: { const DoubleComplex s = x + y; r = s * s; break; }  // f1 of test_CSFD/main.cpp:8-11
            case 12: r = conj(x); break;
            case 13: r = DoubleComplex(norm(x)); break;
            case 14: r = DoubleComplex(SingleComplex((x > y) ? 1.f : 0.f, (x < y) ? 1.f : 0.f)); break;
            default: return -1;
        }
        out[4 * i] = r.real().real(); out[4 * i + 1] = r.real().imag(); out[4 * i + 2] = r.imag().real(); out[4 * i + 3] = r.imag().imag();
    }
    return 0;
}

// csrc/xs_complex.h compiled for the host (the DeviceArray operator API is __host__ __device__ in the
// reference too, cuda_complex.hpp:12-16): n interleaved (re, im) pairs, op codes of xs_complex_table
int xs_host_complex_table(int op, long n, const float *a, const float *b, float *out) {
    using namespace xs;
    for (long i = 0; i < n; ++i) {
        const cfloat x(a[2 * i], a[2 * i + 1]), y(b[2 * i], b[2 * i + 1]);
        cfloat r(0.f, 0.f);
        switch (op) {
            case 0: r = x + y; break;
            case 1: r = x - y; break;
            case 2: r = x * y; break;
            case 3: r = x / y; break;
            case 4: r = sqrt(x); break;
            case 5: r = cfloat(abs(x), 0.f); break;
            case 6: r = exp(x); break;
            case 7: r = log(x); break;
            case 8: r = pow(x, y); break;
            case 9: r = sin(x); break;
            case 10: r = cos(x); break;
            case 11: r = sinh(x); break;
            case 12: r = cosh(x); break;
            case 13: r = sin_new(x); break;
            case 14: r = sinh_new(x); break;
            case 15: r = cfloat(norm(x), 0.f); break;
            case 16: r = cfloat(arg(x), 0.f); break;
            case 17: r = conj(x); break;
            case 18: r = polar(x.re, y.re); break;
            case 19: r = x / y.re; break;
            case 20: r = y.re / x; break;
            case 21: r = x * y.re; break;
            case 22: r = y.re - x; break;
            case 23: r = proj(x); break;
            case 24: r = log10(x); break;
            case 25: r = tanh(x); break;
            case 26: r = tan(x); break;
            case 27: r = asinh(x); break;
            case 28: r = acosh(x); break;
            case 29: r = atanh(x); break;
            case 30: r = asin(x); break;
            case 31: r = acos(x); break;
            case 32: r = atan(x); break;
            default: return -1;
        }
        out[2 * i] = r.re; out[2 * i + 1] = r.im;
    }
    return 0;
}

// flat-YAML reader probe: value of `key` in `yaml_text` as the reader sees it
int xs_flat_yaml_get(const char *yaml_text, const char *key, char *out, int capacity) {
    try {
        const xs_host::FlatYaml y = xs_host::FlatYaml::Load(yaml_text ? yaml_text : "");
        if (!y.has(key)) return -1;
        const std::string v = y.as<std::string>(key);
        if ((int)v.size() + 1 > capacity) return -2;
        std::memcpy(out, v.c_str(), v.size() + 1);
        return (int)v.size();
    } catch (const std::exception &) {
        return -3;
    }
}

int xs_host_newton_seeded_poses(const float *c2v32, float *R36x21, float *t12x21) {
    if (!c2v32 || !R36x21 || !t12x21) return -1;
    xs_host::newton_seeded_poses(pose_of(c2v32), reinterpret_cast<float (*)[36]>(R36x21), reinterpret_cast<float (*)[12]>(t12x21));
    return 0;
}
int xs_host_newton_step(const double *s29, double damping, float *c2v32) {
    if (!s29 || !c2v32) return -1;
    xs_host::Matrix4cf m = pose_of(c2v32);
    if (!xs_host::newton_step(s29, damping, m)) return -1;
    pose_to(m, c2v32);
    return 0;
}
int xs_host_checkpoint_info(const char *path, double *out32) { return xs_host::checkpoint_info(path, out32); }
int xs_host_align_seeded_maps(const double *T16, double vs_this, double vs_other, float *out144) {
    return xs_host::align_seeded_maps(T16, vs_this, vs_other, reinterpret_cast<float (*)[24]>(out144)) ? 0 : -1;
}
int xs_host_align_step(const double *s29, double damping, double *T16) { return xs_host::align_step(s29, damping, T16) ? 0 : -1; }
int xs_host_sample_compose(const double *T_a2v16, const double *T_p2a16, double *T16) {
    if (!T_a2v16 || !T_p2a16 || !T16) return -1;
    xs_host::sample_compose(T_a2v16, T_p2a16, T16);
    return 0;
}
int xs_host_register_step(const double *s29, double damping, double *T16) { return xs_host::register_step(s29, damping, T16) ? 0 : -1; }
int xs_host_align_search_free(int n, const double *centroid_this3, const double *centroid_other3, double box_t, double *T16xN) {
    return xs_host::align_search_free(n, centroid_this3, centroid_other3, box_t, T16xN) ? 0 : -1;
}
int xs_host_align_search_around(const double *T16, const double *pivot3, double box_t, double box_r, int n, double *T16xN) {
    return xs_host::align_search_around(T16, pivot3, box_t, box_r, n, T16xN) ? 0 : -1;
}
int xs_host_align_search_rank(const double *out2xP, int P, int keep, int *idx_out) { return xs_host::align_search_rank(out2xP, P, keep, idx_out); }
int xs_host_band_centroid(const unsigned long long *keys, long long count, double voxel_size, double *out3) {
    return xs_host::band_centroid(keys, count, voxel_size, out3) ? 0 : -1;
}
int xs_host_points_centroid(const float *points, long long n, int stride, double *out3) { return xs_host::points_centroid(points, n, stride, out3) ? 0 : -1; }
int xs_host_merge_affine(const double *T16, double dst_voxel_size, double src_voxel_size, float *out12) {
    return xs_host::merge_affine(T16, dst_voxel_size, src_voxel_size, out12) ? 0 : -1;
}
int xs_host_map_transform(const double *c2v_this16, const double *c2v_other16, double *T16) {
    if (!c2v_this16 || !c2v_other16 || !T16) return -1;
    xs_host::map_transform(c2v_this16, c2v_other16, T16);
    return 0;
}
int xs_host_merge_tile_box(const float *xform12, const int *lo3, const int *hi3, const int *src_res, int *box6) {
    if (!xform12 || !lo3 || !hi3 || !src_res || !box6) return -1;
    return xs_host::merge_tile_box(xform12, lo3, hi3, src_res, box6) ? 1 : 0;
}

}  // extern "C"
