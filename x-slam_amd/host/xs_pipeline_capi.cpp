// xs_pipeline_capi.cpp — C ABI over KinectFusionReconstruction (include/xslam_amd_pipeline.h).
#include "../../include/xslam_amd_pipeline.h"
#include "../csrc/xs_complex.h"
#include "DoubleComplex.h"
#include "KinectFusionReconstruction.h"
#include "align_host.hpp"
#include "align_search_host.hpp"
#include "merge_host.hpp"
#include "newton_host.hpp"
#include "pack_host.hpp"
#include "register_host.hpp"
#include "sample_host.hpp"
#include <cstring>
#include <exception>
#include <fstream>
#include <memory>
#include <vector>

typedef KinectFusionReconstruction KF;
using xs_host::Matrix4cf;

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

// flat-YAML reader probe (CPU only): value of `key` in `yaml_text` as the reader sees it
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

void xs_kf_set_stream(void *stream) { xs_host::current_stream() = (hipStream_t)stream; }

void *xs_kf_create_sharded(const char *yaml_text, int rank, int count, void (*collective)(void *, int, void *, long), void *user) {
    try {
        std::unique_ptr<KF> k(new KF());
        k->SetSharding(rank, count, collective, user);
        k->SetYamlParameters(xs_host::FlatYaml::Load(yaml_text ? yaml_text : ""));
        return k.release();
    } catch (const std::exception &e) {
        printf("xs_kf_create_sharded: %s\n", e.what());
        return nullptr;
    }
}
void xs_kf_shard_planes(void *kf, int *owned2, int *stored2) {
    KF *k = (KF *)kf;
    if (owned2) { owned2[0] = k->zo0; owned2[1] = k->zo1; }
    if (stored2) { stored2[0] = k->zs0; stored2[1] = k->zs1; }
}
void *xs_kf_create(const char *yaml_text) {
    try {
        std::unique_ptr<KF> k(new KF());   // (a configuration SetYamlParameters refuses leaves nothing behind)
        k->SetYamlParameters(xs_host::FlatYaml::Load(yaml_text ? yaml_text : ""));
        return k.release();
    } catch (const std::exception &e) {
        printf("xs_kf_create: %s\n", e.what());
        return nullptr;
    }
}
void xs_kf_destroy(void *kf) { delete (KF *)kf; }

void xs_kf_set_gt_poses(void *kf, int n, const float *c2w32) {
    KF *k = (KF *)kf;
    k->gt_poses.resize(n);
    for (int i = 0; i < n; ++i) std::memcpy(static_cast<void *>(&k->gt_poses[i]), c2w32 + 32 * i, 32 * sizeof(float));
}

int xs_kf_process_frame(void *kf, const uint16_t *depth_dev, size_t step_bytes) {
    KF *k = (KF *)kf;
    DeviceArray2D<ushort> view(k->depth_height, k->depth_width, (void *)depth_dev, step_bytes);  // borrowed, not counted
    return k->ProcessFrame(view);
}
void xs_kf_hint_next_frame(void *kf, const uint16_t *depth_dev, size_t step_bytes) { ((KF *)kf)->HintNextFrame(depth_dev, step_bytes); }
int xs_kf_process_frame_host(void *kf, const uint16_t *depth_host) { return ((KF *)kf)->ProcessFrameHost(depth_host); }
uint16_t *xs_kf_ingest_buffer(void *kf) { return ((KF *)kf)->IngestBuffer(); }
void xs_kf_get_camera2volume(void *kf, float *out32) {
    const auto m = ((KF *)kf)->getCamera2Volume();
    std::memcpy(out32, &m, 32 * sizeof(float));
}
static DeviceArray2D<ushort> wrap_depth(KF *k, const uint16_t *depth_dev, size_t step_bytes) {
    return DeviceArray2D<ushort>(k->depth_height, k->depth_width, const_cast<uint16_t *>(depth_dev), step_bytes);
}
int xs_kf_gauss_newton_terms(void *kf, const uint16_t *depth_dev, size_t step_bytes, const float *c2v32, double *out29) {
    KF *k = (KF *)kf;
    xs_host::Matrix4cf m;
    std::memcpy(static_cast<void *>(&m), c2v32, 32 * sizeof(float));
    return k->GaussNewtonTerms(wrap_depth(k, depth_dev, step_bytes), m, out29);
}
int xs_kf_relocalize(void *kf, const uint16_t *depth_dev, size_t step_bytes, float *c2v32, int iterations, float damping, double *loss_out) {
    KF *k = (KF *)kf;
    xs_host::Matrix4cf m;
    std::memcpy(static_cast<void *>(&m), c2v32, 32 * sizeof(float));
    std::vector<double> hist;
    const int rc = k->RelocalizeGaussNewton(wrap_depth(k, depth_dev, step_bytes), m, iterations, damping, loss_out ? &hist : nullptr);
    std::memcpy(c2v32, &m, 32 * sizeof(float));
    if (loss_out) for (size_t i = 0; i < hist.size() && i <= (size_t)iterations; ++i) loss_out[i] = hist[i];
    return rc;
}
int xs_kf_relocalize_batch(void *kf, int frames, const uint16_t *const *depth_dev, size_t step_bytes, float *c2v32xF, int iterations, float damping,
                           double *loss_out, int *ok_out) {
    KF *k = (KF *)kf;
    if (frames < 0 || (frames > 0 && (!depth_dev || !c2v32xF || !ok_out))) return -1;
    std::vector<DeviceArray2D<ushort>> depths;
    std::vector<Matrix4cf> m((size_t)frames);
    for (int f = 0; f < frames; ++f) {
        depths.push_back(wrap_depth(k, depth_dev[f], step_bytes));
        std::memcpy(static_cast<void *>(&m[(size_t)f]), c2v32xF + 32 * (size_t)f, 32 * sizeof(float));
    }
    std::vector<std::vector<double>> hist(loss_out ? (size_t)frames : 0);
    const int n = k->RelocalizeGaussNewtonBatch(depths, m.data(), iterations, damping, ok_out, loss_out ? hist.data() : nullptr);
    for (int f = 0; f < frames; ++f) {
        std::memcpy(c2v32xF + 32 * (size_t)f, &m[(size_t)f], 32 * sizeof(float));
        if (loss_out)
            for (size_t i = 0; i < hist[(size_t)f].size() && i <= (size_t)iterations; ++i) loss_out[(size_t)f * (iterations + 1) + i] = hist[(size_t)f][i];
    }
    return n;
}
int xs_host_newton_seeded_poses(const float *c2v32, float *R36x21, float *t12x21) {
    if (!c2v32 || !R36x21 || !t12x21) return -1;
    Matrix4cf m;
    std::memcpy(static_cast<void *>(&m), c2v32, 32 * sizeof(float));
    xs_host::newton_seeded_poses(m, reinterpret_cast<float (*)[36]>(R36x21), reinterpret_cast<float (*)[12]>(t12x21));
    return 0;
}
int xs_host_newton_step(const double *s29, double damping, float *c2v32) {
    if (!s29 || !c2v32) return -1;
    Matrix4cf m;
    std::memcpy(static_cast<void *>(&m), c2v32, 32 * sizeof(float));
    if (!xs_host::newton_step(s29, damping, m)) return -1;
    std::memcpy(c2v32, &m, 32 * sizeof(float));
    return 0;
}
int xs_kf_pose_hessian_terms(void *kf, const uint16_t *depth_dev, size_t step_bytes, const float *c2v32, double *out29) {
    KF *k = (KF *)kf;
    Matrix4cf m;
    std::memcpy(static_cast<void *>(&m), c2v32, 32 * sizeof(float));
    return k->PoseHessianTerms(wrap_depth(k, depth_dev, step_bytes), m, out29);
}
int xs_kf_relocalize_newton_batch(void *kf, int frames, const uint16_t *const *depth_dev, size_t step_bytes, float *c2v32xF, int iterations, float damping,
                                  double *loss_out, int *ok_out, int *fallbacks_out) {
    KF *k = (KF *)kf;
    if (frames < 0 || (frames > 0 && (!depth_dev || !c2v32xF || !ok_out))) return -1;
    std::vector<DeviceArray2D<ushort>> depths;
    std::vector<Matrix4cf> m((size_t)frames);
    for (int f = 0; f < frames; ++f) {
        depths.push_back(wrap_depth(k, depth_dev[f], step_bytes));
        std::memcpy(static_cast<void *>(&m[(size_t)f]), c2v32xF + 32 * (size_t)f, 32 * sizeof(float));
    }
    std::vector<std::vector<double>> hist(loss_out ? (size_t)frames : 0);
    const int n = k->RelocalizeNewtonBatch(depths, m.data(), iterations, damping, ok_out, loss_out ? hist.data() : nullptr, fallbacks_out);
    for (int f = 0; f < frames; ++f) {
        std::memcpy(c2v32xF + 32 * (size_t)f, &m[(size_t)f], 32 * sizeof(float));
        if (loss_out)
            for (size_t i = 0; i < hist[(size_t)f].size() && i <= (size_t)iterations; ++i) loss_out[(size_t)f * (iterations + 1) + i] = hist[(size_t)f][i];
    }
    return n;
}
int xs_kf_relocalize_newton(void *kf, const uint16_t *depth_dev, size_t step_bytes, float *c2v32, int iterations, float damping, double *loss_out,
                            int *fallbacks_out) {
    int ok = 0;
    const int n = xs_kf_relocalize_newton_batch(kf, 1, &depth_dev, step_bytes, c2v32, iterations, damping, loss_out, &ok, fallbacks_out);
    return n < 0 ? n : ok;
}
int xs_kf_score_poses(void *kf, const uint16_t *depth_dev, size_t step_bytes, int poses, const float *c2v32xP, double *out2xP) {
    KF *k = (KF *)kf;
    if (poses < 0 || (poses > 0 && (!depth_dev || !c2v32xP || !out2xP))) return -1;
    std::vector<Matrix4cf> m((size_t)poses);
    for (int p = 0; p < poses; ++p) std::memcpy(static_cast<void *>(&m[(size_t)p]), c2v32xP + 32 * (size_t)p, 32 * sizeof(float));
    return k->ScorePoses(wrap_depth(k, depth_dev, step_bytes), m.data(), poses, out2xP);
}
int xs_kf_relocalize_global(void *kf, const uint16_t *depth_dev, size_t step_bytes, int poses, const float *c2v32xP, int keep, int iterations,
                            float damping, float *best_c2v32, double *report8) {
    KF *k = (KF *)kf;
    if (poses < 0 || !report8 || !best_c2v32 || (poses > 0 && (!depth_dev || !c2v32xP))) return -1;
    std::vector<Matrix4cf> m((size_t)poses);
    for (int p = 0; p < poses; ++p) std::memcpy(static_cast<void *>(&m[(size_t)p]), c2v32xP + 32 * (size_t)p, 32 * sizeof(float));
    Matrix4cf best;
    std::memcpy(static_cast<void *>(&best), best_c2v32, 32 * sizeof(float));
    const int rc = k->RelocalizeGlobal(wrap_depth(k, depth_dev, step_bytes), m.data(), poses, keep, iterations, damping, best, report8);
    std::memcpy(best_c2v32, &best, 32 * sizeof(float));
    return rc;
}
static std::vector<Matrix4cf> poses_of(const float *c2v32xP, int poses) {
    std::vector<Matrix4cf> m((size_t)(poses > 0 ? poses : 0));
    for (int p = 0; p < poses; ++p) std::memcpy(static_cast<void *>(&m[(size_t)p]), c2v32xP + 32 * (size_t)p, 32 * sizeof(float));
    return m;
}
int xs_kf_score_views(void *kf, int poses, const float *c2v32xP, const xs_view_opts *opts, int min_weight, unsigned *out4xP) {
    if (poses < 0 || (poses > 0 && (!c2v32xP || !out4xP))) return -1;
    return ((KF *)kf)->ScoreViews(poses_of(c2v32xP, poses).data(), poses, opts, min_weight, out4xP);
}
int xs_kf_next_best_view(void *kf, int poses, const float *c2v32xP, const xs_view_opts *opts, int min_weight, unsigned min_hits, unsigned *out4xP) {
    if (poses < 0 || (poses > 0 && !c2v32xP)) return -3;
    return ((KF *)kf)->NextBestView(poses_of(c2v32xP, poses).data(), poses, opts, min_weight, min_hits, out4xP);
}
int xs_kf_clearance_field(void *kf, int max_radius_vox, int unknown_blocks, int min_weight, uint16_t *host_out) {
    return ((KF *)kf)->ClearanceField(max_radius_vox, unknown_blocks, min_weight, host_out);
}
int xs_kf_reachable(void *kf, const float *start_c2v32_or_null, float radius_m, int snap_vox, int unknown_blocks, int min_weight, int P, const float *c2v32xP,
                    unsigned char *reachable, unsigned short *clear2) {
    if (P < 0 || (P > 0 && (!c2v32xP || !reachable || !clear2))) return -1;
    const std::vector<Matrix4cf> start = poses_of(start_c2v32_or_null, start_c2v32_or_null ? 1 : 0);
    return ((KF *)kf)->Reachable(start.empty() ? nullptr : start.data(), radius_m, snap_vox, unknown_blocks, min_weight, P, poses_of(c2v32xP, P).data(),
                                 reachable, clear2);
}
int xs_kf_next_reachable_view(void *kf, int poses, const float *c2v32xP, const xs_view_opts *opts, int min_weight, unsigned min_hits, unsigned *out4xP,
                              float radius_m, int snap_vox, int unknown_blocks, unsigned char *reachable) {
    if (poses < 0 || (poses > 0 && !c2v32xP)) return -3;
    return ((KF *)kf)->NextReachableView(poses_of(c2v32xP, poses).data(), poses, opts, min_weight, min_hits, out4xP, radius_m, snap_vox, unknown_blocks,
                                         reachable);
}
int xs_kf_travel(void *kf, const float *start_c2v32_or_null, float radius_m, int snap_vox, int unknown_blocks, int min_weight, float max_travel_m, int P,
                 const float *c2v32xP, unsigned char *reachable, unsigned short *clear2, unsigned short *travel3) {
    if (P < 0 || (P > 0 && (!c2v32xP || !reachable || !clear2 || !travel3))) return -1;
    const std::vector<Matrix4cf> start = poses_of(start_c2v32_or_null, start_c2v32_or_null ? 1 : 0);
    return ((KF *)kf)->Travel(start.empty() ? nullptr : start.data(), radius_m, snap_vox, unknown_blocks, min_weight, max_travel_m, P, poses_of(c2v32xP, P).data(),
                              reachable, clear2, travel3);
}
int xs_kf_path_to(void *kf, const float *start_c2v32_or_null, float radius_m, int snap_vox, int unknown_blocks, int min_weight, float max_travel_m,
                  const float *target_c2v32, int capacity, int *voxels3, float *points3, int *needed_out) {
    if (!target_c2v32) return -1;
    const std::vector<Matrix4cf> start = poses_of(start_c2v32_or_null, start_c2v32_or_null ? 1 : 0);
    return ((KF *)kf)->PathTo(start.empty() ? nullptr : start.data(), radius_m, snap_vox, unknown_blocks, min_weight, max_travel_m, poses_of(target_c2v32, 1)[0],
                              capacity, voxels3, points3, needed_out);
}
int xs_kf_next_view_by_travel(void *kf, int poses, const float *c2v32xP, const xs_view_opts *opts, int min_weight, unsigned min_hits, unsigned *out4xP,
                              float radius_m, int snap_vox, int unknown_blocks, float max_travel_m, float bias_m, unsigned short *travel3_out) {
    if (poses < 0 || (poses > 0 && !c2v32xP)) return -3;
    return ((KF *)kf)->NextViewByTravel(poses_of(c2v32xP, poses).data(), poses, opts, min_weight, min_hits, out4xP, radius_m, snap_vox, unknown_blocks,
                                        max_travel_m, bias_m, travel3_out);
}
int xs_kf_frontiers(void *kf, int cell, unsigned long long min_size, int min_weight, int capacity, unsigned long long *records8, int *count_out) {
    return ((KF *)kf)->Frontiers(cell, min_size, min_weight, capacity, records8, count_out);
}
int xs_kf_propose_views(void *kf, float radius_m, int start_snap_vox, int unknown_blocks, int min_weight, int cell, unsigned long long min_size,
                        int views_per_cluster, float standoff_m, int snap_vox, int capacity, float *c2v32xP_out, int *cluster_out, int *count_out) {
    if (capacity < 0 || (capacity > 0 && !c2v32xP_out)) return -1;
    std::vector<Matrix4cf> m((size_t)capacity);
    const int rc = ((KF *)kf)->ProposeViews(radius_m, start_snap_vox, unknown_blocks, min_weight, cell, min_size, views_per_cluster, standoff_m, snap_vox, capacity,
                                            m.data(), cluster_out, count_out);
    if (rc == 1)
        for (int p = 0; p < *count_out; ++p) std::memcpy(c2v32xP_out + 32 * (size_t)p, &m[(size_t)p], 32 * sizeof(float));
    return rc;
}
long long xs_kf_relocalization_index_voxels(void *kf) { return ((KF *)kf)->RelocalizationIndexVoxels(); }
long long xs_kf_export_point_cloud(void *kf, int max_buffer, float *points_host, float *normals_host) {
    const auto pc = ((KF *)kf)->ExportPointCloud(max_buffer);
    if (points_host && pc.size()) std::memcpy(points_host, pc.positions.data(), pc.positions.size() * sizeof(float));
    if (normals_host && pc.size()) std::memcpy(normals_host, pc.normals.data(), pc.normals.size() * sizeof(float));
    return (long long)pc.size();
}
long long xs_kf_export_ply(void *kf, int max_buffer, const char *filename) {
    const auto pc = ((KF *)kf)->ExportPointCloud(max_buffer);
    return pc.exportPly(filename) ? (long long)pc.size() : -1;
}
long long xs_kf_export_mesh(void *kf, int min_weight, long long vertex_capacity, long long triangle_capacity, float *vertices_host,
                            float *normals_host, float *vertex_im_host, unsigned long long *edge_keys_host, int *triangles_host,
                            long long *triangle_count, int *has_im) {
    const auto m = ((KF *)kf)->ExportMesh(min_weight);
    const long long nv = (long long)m.vertices(), nt = (long long)m.faces();
    if (triangle_count) *triangle_count = nt;
    if (has_im) *has_im = m.has_im ? 1 : 0;
    if (nv > vertex_capacity || nt > triangle_capacity) return nv;   // counts only: the caller allocates and calls again
    if (vertices_host && nv) std::memcpy(vertices_host, m.positions.data(), m.positions.size() * sizeof(float));
    if (normals_host && nv) std::memcpy(normals_host, m.normals.data(), m.normals.size() * sizeof(float));
    if (vertex_im_host && m.has_im && nv) std::memcpy(vertex_im_host, m.vertex_im.data(), m.vertex_im.size() * sizeof(float));
    if (edge_keys_host && nv) std::memcpy(edge_keys_host, m.edge_keys.data(), m.edge_keys.size() * sizeof(unsigned long long));
    if (triangles_host && nt) std::memcpy(triangles_host, m.triangles.data(), m.triangles.size() * sizeof(int));
    return nv;
}
long long xs_kf_export_mesh_ply(void *kf, const char *filename) {
    const auto m = ((KF *)kf)->ExportMesh(1);
    return m.exportPly(filename) ? (long long)m.vertices() : -1;
}
void xs_kf_synchronize(void *kf) { ((KF *)kf)->synchronize(); }

int xs_kf_frame_id(void *kf) { return ((KF *)kf)->frame_id; }
int xs_kf_num_poses(void *kf) { return (int)((KF *)kf)->world2camera_record.size(); }
void xs_kf_get_world2camera(void *kf, int idx, float *out32) {
    KF *k = (KF *)kf;
    if (idx < 0) idx += (int)k->world2camera_record.size();
    std::memcpy(out32, &k->world2camera_record[idx], 32 * sizeof(float));
}
float xs_kf_tranc_dist(void *kf) { return ((KF *)kf)->tsdf_volume_d_ptr->getTsdfTruncDist(); }
long long xs_kf_last_updated_voxels(void *kf) { return ((KF *)kf)->lastUpdatedVoxels(); }
long long xs_kf_last_raycast_hits(void *kf) { return ((KF *)kf)->lastRaycastHits(); }
int xs_kf_icp_log(void *kf, double *out, int capacity) {
    KF *k = (KF *)kf;
    const int n = (int)k->icp_log.size();
    if (out && capacity >= n && n) std::memcpy(out, k->icp_log.data(), n * sizeof(double));
    return n;
}

int xs_kf_download_volume(void *kf, float *value, int *weight, float *grad) {
    KF *k = (KF *)kf;
    const int X = k->volume_resolution[0];
    if (value) k->tsdf_volume_d_ptr->value().download(value, X * sizeof(float));
    if (weight) k->tsdf_volume_d_ptr->weight().download(weight, X * sizeof(int));
    if (grad) k->tsdf_volume_d_ptr->grad().download(grad, X * sizeof(float));
    return 0;
}
int xs_kf_download_map(void *kf, int which, int level, float *out) {
    KF *k = (KF *)kf;
    if (level < 0 || level >= k->num_levels) return -1;
    MapArr *m = nullptr;
    switch (which) {
        case 0: m = &k->depths_curr_d[level]; break;
        case 1: m = &k->vmaps_curr_d[level]; break;
        case 2: m = &k->nmaps_curr_d[level]; break;
        case 3: m = &k->vmaps_g_prev_d[level]; break;
        case 4: m = &k->nmaps_g_prev_d[level]; break;
        default: return -1;
    }
    m->download(out, m->cols() * sizeof(devComplex));
    return 0;
}
void *xs_kf_volume_ptr(void *kf, int which, size_t *step_bytes) {
    KF *k = (KF *)kf;
    if (which == 1) { auto a = k->tsdf_volume_d_ptr->weight(); if (step_bytes) *step_bytes = a.step(); return a.ptr(); }
    auto a = which == 0 ? k->tsdf_volume_d_ptr->value() : k->tsdf_volume_d_ptr->grad();
    if (step_bytes) *step_bytes = a.step();
    if (which == 0) { k->MarkSignMapStale(); ++k->volume_generation; }   // a caller that writes values through this pointer need not know about the sign map
                                                                          // or the relocalisation index
    return a.ptr();
}

void xs_kf_set_profiling(void *kf, int level) { ((KF *)kf)->set_profiling(level); }
void xs_kf_stage_times(void *kf, double *ms6, long long *calls6) {
    KF *k = (KF *)kf;
    if (k->profiling) k->collect_stage_times();
    for (int i = 0; i < KF::ST_COUNT; ++i) { if (ms6) ms6[i] = k->stage_ms[i]; if (calls6) calls6[i] = k->stage_calls[i]; }
}
void xs_kf_cumulative_counters(void *kf, long long *updated, long long *hits) {
    KF *k = (KF *)kf;
    if (k->profiling) k->collect_stage_times();
    if (updated) *updated = k->cum_updated;
    if (hits) *hits = k->cum_hits;
}
void xs_kf_reset_stage_times(void *kf) {
    KF *k = (KF *)kf;
    if (k->profiling) k->collect_stage_times();
    k->cum_updated = 0; k->cum_hits = 0;
    for (int i = 0; i < KF::ST_COUNT; ++i) { k->stage_ms[i] = 0; k->stage_calls[i] = 0; }
    for (int i = 0; i < 4; ++i) { k->icp_level_us[i] = 0; k->icp_level_calls[i] = 0; k->tail_host_us[i] = 0; }
    k->tail_host_calls = 0;
}
void xs_kf_tail_host_times(void *kf, double *us4, long long *frames) {
    KF *k = (KF *)kf;
    for (int i = 0; i < 4; ++i) if (us4) us4[i] = k->tail_host_us[i];
    if (frames) *frames = k->tail_host_calls;
}
void xs_kf_icp_iteration_times(void *kf, double *us4, long long *calls4) {
    KF *k = (KF *)kf;
    for (int i = 0; i < 4; ++i) { if (us4) us4[i] = k->icp_level_us[i]; if (calls4) calls4[i] = k->icp_level_calls[i]; }
}
void xs_kf_set_gn_post_pose(void *kf, int on) { ((KF *)kf)->gn_post_pose = on != 0; }
void xs_kf_gn_poll_times(void *kf, double *poll_us, long long *poll_passes, int reset) {
    KF *k = (KF *)kf;
    if (poll_us) *poll_us = k->gn_poll_us;
    if (poll_passes) *poll_passes = k->gn_poll_passes;
    if (reset) { k->gn_poll_us = 0; k->gn_poll_passes = 0; }
}
void xs_kf_gn_times(void *kf, double *pass_us, long long *passes, double *kernel_ms, long long *kernel_calls, int reset) {
    KF *k = (KF *)kf;
    if (pass_us) *pass_us = k->gn_pass_us;
    if (passes) *passes = k->gn_passes;
    if (kernel_ms) *kernel_ms = k->gn_kernel_ms;
    if (kernel_calls) *kernel_calls = k->gn_kernel_calls;
    if (reset) { k->gn_pass_us = 0; k->gn_passes = 0; k->gn_kernel_ms = 0; k->gn_kernel_calls = 0; }
}
void xs_kf_debug_set_icp_sequence(void *kf, unsigned long long v) { ((KF *)kf)->DebugSetIcpSequence(v); }
void xs_kf_debug_fail_icp_iteration(void *kf, int n) { ((KF *)kf)->debug_fail_icp_iteration_ = n; }
void xs_kf_debug_post_delay(void *kf, int min_us, int max_us) { ((KF *)kf)->debug_post_delay_us_[0] = min_us; ((KF *)kf)->debug_post_delay_us_[1] = max_us; }
void xs_kf_rebuild_sign_map(void *kf) { ((KF *)kf)->RebuildSignMap(); }
long long xs_kf_composite_bytes(void *kf) { return ((KF *)kf)->composite_bytes_; }
void xs_kf_list_cover_counts(void *kf, long long *counts4) {
    if (counts4) for (int i = 0; i < 4; ++i) counts4[i] = ((KF *)kf)->list_cover_counts_[i];
}

long long xs_kf_volume_generation(void *kf) { return (long long)((KF *)kf)->volume_generation; }
int xs_kf_save_checkpoint(void *kf, const char *path) { ((KF *)kf)->saveCheckpoint(path); return 0; }
int xs_kf_load_checkpoint(void *kf, const char *path) { return ((KF *)kf)->loadCheckpoint(path) ? 0 : -1; }
int xs_kf_save_tsdf_volume(void *kf, const char *path) { ((KF *)kf)->saveTSDFVolume(path); return 0; }
int xs_kf_save_checkpoint_sparse(void *kf, const char *path, unsigned long long *stats12) {
    if (!kf || !path) return -1;
    return ((KF *)kf)->saveCheckpointSparse(path, stats12) ? 0 : -1;
}
long long xs_kf_checkpoint_staging_words(void *kf, unsigned long long words) {
    if (!kf || (words != 0 && words < xs_host::PACK_MAX_BRICK_WORDS) || words > (1ull << 40)) return -1;
    if (words) ((KF *)kf)->checkpoint_staging_words = words;
    return (long long)((KF *)kf)->checkpoint_staging_words;
}
int xs_host_checkpoint_info(const char *path, double *out32) {
    using namespace xs_host;
    if (!path || !out32) return -1;
    for (int i = 0; i < 32; ++i) out32[i] = 0.0;
    std::ifstream f(path, std::ios::binary);
    if (!f) return -1;
    f.seekg(0, std::ios::end);
    const long long file_bytes = (long long)f.tellg();
    f.seekg(0, std::ios::beg);
    PackHeader h{};
    if (file_bytes < (long long)sizeof(CkptPrefix)) return -1;
    f.read(reinterpret_cast<char *>(&h.p), sizeof(h.p));
    if (!f) return -1;
    const bool v3 = pack_magic_is(h.p.magic, "XSTSDF3"), v2 = pack_magic_is(h.p.magic, "XSTSDF2");
    if (!v2 && !v3) return -1;
    const CkptPrefix &p = h.p;
    out32[0] = v3 ? 3.0 : 2.0;
    for (int i = 0; i < 3; ++i) out32[2 + i] = p.res[i];
    out32[5] = p.voxel_size; out32[6] = p.tranc_dist; out32[7] = p.frame_id; out32[8] = p.n_poses; out32[9] = p.zs0; out32[10] = p.zs1;
    out32[11] = p.shard_rank; out32[12] = p.shard_count;
    out32[27] = (double)file_bytes;
    PackError e = PACK_OK;
    if (v2) {
        uint64_t words = 0;
        e = pack_validate_dense(p, (uint64_t)file_bytes, &words);
        out32[26] = (double)words;
    } else {
        if (file_bytes < (long long)sizeof(PackHeader)) e = PACK_BAD_LENGTH;
        else {
            f.read(reinterpret_cast<char *>(&h) + sizeof(h.p), sizeof(h) - sizeof(h.p));
            out32[13] = h.brick_edge; out32[14] = h.nbx; out32[15] = h.nby; out32[16] = h.nbz;
            out32[17] = (double)h.nbricks; out32[26] = (double)h.payload_words;
            uint64_t head = 0;
            e = f ? pack_validate_header(h, &head) : PACK_BAD_LENGTH;
            if (e == PACK_OK) {
                if ((uint64_t)file_bytes < head) e = PACK_BAD_LENGTH;
                else {
                    std::vector<unsigned char> cls((size_t)pack_class_bytes_padded(h.nbricks));
                    f.seekg((std::streamoff)(sizeof(PackHeader) + (uint64_t)p.n_poses * PACK_POSE_BYTES), std::ios::beg);
                    f.read(reinterpret_cast<char *>(cls.data()), (std::streamsize)cls.size());
                    uint64_t hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    e = f ? pack_validate(h, cls.data(), (uint64_t)file_bytes, hist) : PACK_BAD_LENGTH;
                    for (int c = 0; c < 8; ++c) out32[18 + c] = (double)hist[c];
                }
            }
        }
    }
    out32[1] = e == PACK_OK ? 1.0 : 0.0;
    out32[28] = (double)e;
    return 0;
}

// ---- the calls that take a second map: from the caller's pointers (*_volume), from another instance (*_map) or from a file (*_checkpoint) ----
static xs_host::SecondMap second_map(const float *value, const int *weight, const float *grad, size_t step, const int *res, float voxel_size, float tranc_dist) {
    xs_host::SecondMap m{value, weight, grad, step, {0, 0, 0}, voxel_size, tranc_dist};   // (a null res stays 0 x 0 x 0, which every operation refuses)
    for (int a = 0; res && a < 3; ++a) m.res[a] = res[a];
    return m;
}
int xs_kf_merge_volume(void *kf, const float *src_value, const int *src_weight, const float *src_grad, size_t src_step, const int *src_res,
                       float src_voxel_size, float src_tranc_dist, const double *T16, int min_weight, unsigned long long *written) {
    return ((KF *)kf)->MergeVolume(second_map(src_value, src_weight, src_grad, src_step, src_res, src_voxel_size, src_tranc_dist), T16, min_weight, written);
}
int xs_kf_merge_checkpoint(void *kf, const char *path, const double *T16, int min_weight, unsigned long long *written) {
    if (!path) return -1;
    KF::CheckpointMap c;
    const int rc = ((KF *)kf)->OpenCheckpointMap(path, c);
    return rc != 1 ? rc : ((KF *)kf)->MergeVolume(c.map, T16, min_weight, written);
}
int xs_kf_merge_map(void *kf, void *other_kf, const double *T16, int min_weight, unsigned long long *written) {
    xs_host::SecondMap m;
    const int rc = ((KF *)kf)->OtherInstanceMap((KF *)other_kf, true, m);
    return rc != 1 ? rc : ((KF *)kf)->MergeVolume(m, T16, min_weight, written);
}
int xs_kf_reintegrate(void *kf, int n, const uint16_t *const *depth_dev, size_t step_bytes, const float *c2v_old32xN, const float *c2v_new32xN,
                      const int *mode, const int *frame_index, unsigned long long *counts4) {
    KF *k = (KF *)kf;
    if (n < 1 || !depth_dev || !mode) return -1;
    std::vector<DeviceArray2D<ushort>> depths;
    for (int i = 0; i < n; ++i) depths.push_back(wrap_depth(k, depth_dev[i], step_bytes));
    const std::vector<Matrix4cf> olds = poses_of(c2v_old32xN, c2v_old32xN ? n : 0), news = poses_of(c2v_new32xN, c2v_new32xN ? n : 0);
    return k->ReintegrateFrames(n, depths.data(), olds.empty() ? nullptr : olds.data(), news.empty() ? nullptr : news.data(), mode, frame_index, counts4);
}
static int align_call(KF *k, const xs_host::SecondMap &m, const double *T16xN, int N, int iterations, double damping, int min_weight, float max_residual,
                      double *T16_out, double *report8, double *loss_history) {
    std::vector<double> history;
    const int rc = k->AlignVolume(m, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report8, loss_history ? &history : nullptr);
    if (loss_history) std::copy(history.begin(), history.end(), loss_history);   // at most iterations + 1 entries
    return rc;
}
int xs_kf_align_map(void *kf, void *other_kf, const double *T16xN, int N, int iterations, double damping, int min_weight, float max_residual,
                    double *T16_out, double *report8, double *loss_history) {
    xs_host::SecondMap m;
    const int rc = ((KF *)kf)->OtherInstanceMap((KF *)other_kf, false, m);
    return rc != 1 ? rc : align_call((KF *)kf, m, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report8, loss_history);
}
int xs_kf_align_checkpoint(void *kf, const char *path, const double *T16xN, int N, int iterations, double damping, int min_weight, float max_residual,
                           double *T16_out, double *report8, double *loss_history) {
    if (!path) return -1;
    xs_host::align_report_clear(report8, 8);
    KF::CheckpointMap c;
    const int rc = ((KF *)kf)->OpenCheckpointMap(path, c);
    return rc != 1 ? rc : align_call((KF *)kf, c.map, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report8, loss_history);
}
int xs_host_align_seeded_maps(const double *T16, double vs_this, double vs_other, float *out144) {
    return xs_host::align_seeded_maps(T16, vs_this, vs_other, reinterpret_cast<float (*)[24]>(out144)) ? 0 : -1;
}
int xs_host_align_step(const double *s29, double damping, double *T16) { return xs_host::align_step(s29, damping, T16) ? 0 : -1; }
void xs_kf_align_search_defaults(void *kf, xs_align_search_opts *opts) { ((KF *)kf)->AlignSearchDefaults(opts); }
int xs_kf_score_transforms(void *kf, void *other_kf, int P, const double *T16xP, int stride, int min_weight, float max_residual, double *out2xP) {
    xs_host::SecondMap m;
    const int rc = ((KF *)kf)->OtherInstanceMap((KF *)other_kf, false, m);
    return rc != 1 ? rc : ((KF *)kf)->ScoreTransformsVolume(m, T16xP, P, stride, min_weight, max_residual, out2xP);
}
int xs_kf_score_transforms_checkpoint(void *kf, const char *path, int P, const double *T16xP, int stride, int min_weight, float max_residual, double *out2xP) {
    if (!path) return -1;
    KF::CheckpointMap c;
    const int rc = ((KF *)kf)->OpenCheckpointMap(path, c);
    return rc != 1 ? rc : ((KF *)kf)->ScoreTransformsVolume(c.map, T16xP, P, stride, min_weight, max_residual, out2xP);
}
int xs_kf_align_map_global(void *kf, void *other_kf, const xs_align_search_opts *opts, double *T16_out, double *report12) {
    xs_host::SecondMap m;
    const int rc = ((KF *)kf)->OtherInstanceMap((KF *)other_kf, false, m);
    return rc != 1 ? rc : ((KF *)kf)->AlignVolumeGlobal(m, opts, T16_out, report12);
}
int xs_kf_align_checkpoint_global(void *kf, const char *path, const xs_align_search_opts *opts, double *T16_out, double *report12) {
    if (!path) return -1;
    xs_host::align_report_clear(report12, 12);
    KF::CheckpointMap c;
    const int rc = ((KF *)kf)->OpenCheckpointMap(path, c);
    return rc != 1 ? rc : ((KF *)kf)->AlignVolumeGlobal(c.map, opts, T16_out, report12);
}
int xs_kf_diff_volume(void *kf, const float *src_value, const int *src_weight, size_t src_step, const int *src_res, float src_voxel_size, float src_tranc_dist,
                      const double *T16, int min_weight, float lo, float hi, int cell, unsigned long long min_size, int capacity,
                      unsigned long long *this_records8, int *this_count, unsigned long long *other_records8, int *other_count, unsigned long long *counts3,
                      unsigned char *this_dense, unsigned char *other_dense) {
    return ((KF *)kf)->DiffVolume(second_map(src_value, src_weight, nullptr, src_step, src_res, src_voxel_size, src_tranc_dist), T16, min_weight, lo, hi, cell,
                                  min_size, capacity, this_records8, this_count, other_records8, other_count, counts3, this_dense, other_dense);
}
int xs_kf_diff_map(void *kf, void *other_kf, const double *T16, int min_weight, float lo, float hi, int cell, unsigned long long min_size, int capacity,
                   unsigned long long *this_records8, int *this_count, unsigned long long *other_records8, int *other_count, unsigned long long *counts3,
                   unsigned char *this_dense, unsigned char *other_dense) {
    xs_host::SecondMap m;
    const int rc = ((KF *)kf)->OtherInstanceMap((KF *)other_kf, false, m);
    return rc != 1 ? rc : ((KF *)kf)->DiffVolume(m, T16, min_weight, lo, hi, cell, min_size, capacity, this_records8, this_count, other_records8, other_count,
                                                 counts3, this_dense, other_dense);
}
int xs_kf_diff_checkpoint(void *kf, const char *path, const double *T16, int min_weight, float lo, float hi, int cell, unsigned long long min_size, int capacity,
                          unsigned long long *this_records8, int *this_count, unsigned long long *other_records8, int *other_count,
                          unsigned long long *counts3, unsigned char *this_dense, unsigned char *other_dense) {
    if (!path) return -1;
    KF::CheckpointMap c;
    const int rc = ((KF *)kf)->OpenCheckpointMap(path, c);
    return rc != 1 ? rc : ((KF *)kf)->DiffVolume(c.map, T16, min_weight, lo, hi, cell, min_size, capacity, this_records8, this_count, other_records8, other_count,
                                                 counts3, this_dense, other_dense);
}
static KF::RenderOutputs render_outputs(float *depth, uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4) {
    KF::RenderOutputs o;
    o.depth = depth; o.depth_u16 = depth_u16; o.normal = normal; o.shade = shade; o.counts = counts4;
    return o;
}
int xs_kf_render_views(void *kf, int views, const float *c2v, int complex_poses, const float *intr4, int rows, int cols, const xs_render_opts *opts, float *depth,
                       uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4, int on_device) {
    return ((KF *)kf)->RenderViews(c2v, complex_poses ? 2 : 1, views, intr4, rows, cols, opts, render_outputs(depth, depth_u16, normal, shade, counts4), on_device);
}
int xs_kf_render_volume(void *kf, const float *src_value, const int *src_weight, size_t src_step, const int *src_res, float src_voxel_size, float src_tranc_dist,
                        int views, const float *c2v, int complex_poses, const float *intr4, int rows, int cols, const xs_render_opts *opts, float *depth,
                        uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4, int on_device) {
    return ((KF *)kf)->RenderSecondMap(second_map(src_value, src_weight, nullptr, src_step, src_res, src_voxel_size, src_tranc_dist), c2v, complex_poses ? 2 : 1, views,
                                       intr4, rows, cols, opts, render_outputs(depth, depth_u16, normal, shade, counts4), on_device);
}
int xs_kf_render_map(void *kf, void *other_kf, int views, const float *c2v, int complex_poses, const float *intr4, int rows, int cols, const xs_render_opts *opts,
                     float *depth, uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4, int on_device) {
    xs_host::SecondMap m;
    const int rc = ((KF *)kf)->OtherInstanceMap((KF *)other_kf, false, m);
    return rc != 1 ? rc : ((KF *)kf)->RenderSecondMap(m, c2v, complex_poses ? 2 : 1, views, intr4, rows, cols, opts,
                                                      render_outputs(depth, depth_u16, normal, shade, counts4), on_device);
}
int xs_kf_render_checkpoint(void *kf, const char *path, int views, const float *c2v, int complex_poses, const float *intr4, int rows, int cols,
                            const xs_render_opts *opts, float *depth, uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4, int on_device) {
    if (!path) return -1;
    KF::CheckpointMap c;
    const int rc = ((KF *)kf)->OpenCheckpointMap(path, c);
    return rc != 1 ? rc : ((KF *)kf)->RenderSecondMap(c.map, c2v, complex_poses ? 2 : 1, views, intr4, rows, cols, opts,
                                                      render_outputs(depth, depth_u16, normal, shade, counts4), on_device);
}
static KF::SampleOutputs sample_outputs(unsigned char *status, float *value, float *dvalue, float *gradient, unsigned long long *counts4) {
    KF::SampleOutputs o;
    o.status = status; o.value = value; o.dvalue = dvalue; o.gradient = gradient; o.counts = counts4;
    return o;
}
int xs_kf_sample_points(void *kf, long long n, const float *points, const double *T16, int min_weight, unsigned char *status, float *value, float *dvalue,
                        float *gradient, unsigned long long *counts4, int on_device) {
    return ((KF *)kf)->SamplePoints(points, n, T16, min_weight, sample_outputs(status, value, dvalue, gradient, counts4), on_device);
}
int xs_kf_sample_volume(void *kf, const float *src_value, const int *src_weight, const float *src_grad, size_t src_step, const int *src_res, float src_voxel_size,
                        float src_tranc_dist, long long n, const float *points, const double *T16, int min_weight, unsigned char *status, float *value,
                        float *dvalue, float *gradient, unsigned long long *counts4, int on_device) {
    return ((KF *)kf)->SampleSecondMap(second_map(src_value, src_weight, src_grad, src_step, src_res, src_voxel_size, src_tranc_dist), points, n, T16, min_weight,
                                       sample_outputs(status, value, dvalue, gradient, counts4), on_device);
}
int xs_kf_sample_map(void *kf, void *other_kf, long long n, const float *points, const double *T16, int min_weight, unsigned char *status, float *value,
                     float *dvalue, float *gradient, unsigned long long *counts4, int on_device) {
    xs_host::SecondMap m;
    const int rc = ((KF *)kf)->OtherInstanceMap((KF *)other_kf, dvalue != nullptr, m);
    return rc != 1 ? rc : ((KF *)kf)->SampleSecondMap(m, points, n, T16, min_weight, sample_outputs(status, value, dvalue, gradient, counts4), on_device);
}
int xs_kf_sample_checkpoint(void *kf, const char *path, long long n, const float *points, const double *T16, int min_weight, unsigned char *status, float *value,
                            float *dvalue, float *gradient, unsigned long long *counts4, int on_device) {
    if (!path) return -1;
    KF::CheckpointMap c;
    const int rc = ((KF *)kf)->OpenCheckpointMap(path, c);
    return rc != 1 ? rc : ((KF *)kf)->SampleSecondMap(c.map, points, n, T16, min_weight, sample_outputs(status, value, dvalue, gradient, counts4), on_device);
}
int xs_kf_frame_residuals(void *kf, const unsigned short *depth, size_t depth_step, const float *c2v, int complex_poses, const float *intr4, int rows, int cols,
                          int min_weight, unsigned char *status, float *value, float *dvalue, float *gradient, unsigned long long *counts4, int on_device) {
    return ((KF *)kf)->FrameResiduals(depth, depth_step, c2v, complex_poses ? 2 : 1, intr4, rows, cols, min_weight,
                                      sample_outputs(status, value, dvalue, gradient, counts4), on_device);
}
int xs_host_sample_compose(const double *T_a2v16, const double *T_p2a16, double *T16) {
    if (!T_a2v16 || !T_p2a16 || !T16) return -1;
    xs_host::sample_compose(T_a2v16, T_p2a16, T16);
    return 0;
}
static int register_call(KF *k, const xs_host::SecondMap *m, long long n, const float *points, int on_device, const double *T16xN, int N, int iterations,
                         double damping, int min_weight, float max_residual, double *T16_out, double *report7, double *loss_history) {
    std::vector<double> history;
    std::vector<double> *h = loss_history ? &history : nullptr;
    const int rc = m ? k->RegisterSecondMap(*m, points, n, on_device, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report7, h)
                     : k->RegisterPoints(points, n, on_device, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report7, h);
    if (loss_history) std::copy(history.begin(), history.end(), loss_history);   // at most iterations + 1 entries
    return rc;
}
int xs_kf_register_points(void *kf, long long n, const float *points, int on_device, const double *T16xN, int N, int iterations, double damping,
                          int min_weight, float max_residual, double *T16_out, double *report7, double *loss_history) {
    return register_call((KF *)kf, nullptr, n, points, on_device, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report7, loss_history);
}
int xs_kf_register_map(void *kf, void *other_kf, long long n, const float *points, int on_device, const double *T16xN, int N, int iterations,
                       double damping, int min_weight, float max_residual, double *T16_out, double *report7, double *loss_history) {
    xs_host::register_report_clear(report7);
    xs_host::SecondMap m;
    const int rc = ((KF *)kf)->OtherInstanceMap((KF *)other_kf, false, m);
    return rc != 1 ? rc : register_call((KF *)kf, &m, n, points, on_device, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report7, loss_history);
}
int xs_kf_register_checkpoint(void *kf, const char *path, long long n, const float *points, int on_device, const double *T16xN, int N, int iterations,
                              double damping, int min_weight, float max_residual, double *T16_out, double *report7, double *loss_history) {
    if (!path) return -1;
    xs_host::register_report_clear(report7);
    KF::CheckpointMap c;
    const int rc = ((KF *)kf)->OpenCheckpointMap(path, c);
    return rc != 1 ? rc : register_call((KF *)kf, &c.map, n, points, on_device, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report7, loss_history);
}
int xs_host_register_step(const double *s29, double damping, double *T16) { return xs_host::register_step(s29, damping, T16) ? 0 : -1; }
int xs_kf_fuse_points(void *kf, long long n, const float *points, int on_device, const double *T16, const float *origin3, float min_range, float max_range,
                      int carve, int weight, unsigned long long *counts5) {
    return ((KF *)kf)->FusePoints(points, n, on_device, T16, origin3, min_range, max_range, carve, weight, counts5);
}
void xs_kf_release_fuse_scratch(void *kf) { ((KF *)kf)->ReleaseFuseScratch(); }
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
