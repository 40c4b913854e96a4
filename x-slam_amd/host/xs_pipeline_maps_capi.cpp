// xs_pipeline_maps_capi.cpp — the C ABI's calls that take a second map or edit or query a map (include/xslam_amd_pipeline.h): merge, align, score,
// diff, render, sample and register with the map from the caller's pointers (*_volume), from another instance (*_map) or from a file
// (*_checkpoint), a cloud's transforms scored and a cloud registered with no guess against this instance's map, another's or a file's, and
// reintegrate, fuse and frame_residuals on this instance's own map.  None of it runs during tracking.
#include "../../include/xslam_amd_pipeline.h"
#include "kf_internal.hpp"
#include "align_host.hpp"
#include "register_host.hpp"

typedef KinectFusionReconstruction KF;
using xs_host::Matrix4cf;
using xs_host::SecondMap;

namespace {
SecondMap second_map(const float *value, const int *weight, const float *grad, size_t step, const int *res, float voxel_size, float tranc_dist) {
    SecondMap m{value, weight, grad, step, {0, 0, 0}, voxel_size, tranc_dist};   // (a null res stays 0 x 0 x 0, which every operation refuses)
    for (int a = 0; res && a < 3; ++a) m.res[a] = res[a];
    return m;
}
// The two other sources of a second map: resolved, then fn(map) and its code; a source that is refused returns the resolver's code (-2, 0, -1)
// and fn does not run.  What an entry point does to its outputs before the source is looked at is the entry point's own.
template <class Fn>
int with_other_map(void *kf, void *other_kf, bool with_grad, Fn &&fn) {
    SecondMap m;
    const int rc = ((KF *)kf)->OtherInstanceMap((KF *)other_kf, with_grad, m);
    return rc != 1 ? rc : fn(m);
}
template <class Fn>
int with_checkpoint_map(void *kf, const char *path, Fn &&fn) {
    if (!path) return -1;
    KF::CheckpointMap c;   // (the temporary device volume lives until fn returns)
    const int rc = ((KF *)kf)->OpenCheckpointMap(path, c);
    return rc != 1 ? rc : fn(c.map);
}
// the two multi-start calls: the winner's loss history goes to the caller's array (at most iterations + 1 entries)
template <class Run>
int with_history(double *loss_history, Run &&run) {
    std::vector<double> history;
    const int rc = run(loss_history ? &history : nullptr);
    if (loss_history) std::copy(history.begin(), history.end(), loss_history);
    return rc;
}
}  // namespace

extern "C" {

// ---- merge ----
int xs_kf_merge_volume(void *kf, const float *src_value, const int *src_weight, const float *src_grad, size_t src_step, const int *src_res,
                       float src_voxel_size, float src_tranc_dist, const double *T16, int min_weight, unsigned long long *written) {
    return ((KF *)kf)->MergeVolume(second_map(src_value, src_weight, src_grad, src_step, src_res, src_voxel_size, src_tranc_dist), T16, min_weight, written);
}
int xs_kf_merge_checkpoint(void *kf, const char *path, const double *T16, int min_weight, unsigned long long *written) {
    return with_checkpoint_map(kf, path, [&](const SecondMap &m) { return ((KF *)kf)->MergeVolume(m, T16, min_weight, written); });
}
int xs_kf_merge_map(void *kf, void *other_kf, const double *T16, int min_weight, unsigned long long *written) {
    return with_other_map(kf, other_kf, true, [&](const SecondMap &m) { return ((KF *)kf)->MergeVolume(m, T16, min_weight, written); });
}
// ---- align, score, align with no guess ----
int xs_kf_align_map(void *kf, void *other_kf, const double *T16xN, int N, int iterations, double damping, int min_weight, float max_residual,
                    double *T16_out, double *report8, double *loss_history) {
    return with_other_map(kf, other_kf, false, [&](const SecondMap &m) {
        return with_history(loss_history, [&](std::vector<double> *h) {
            return ((KF *)kf)->AlignVolume(m, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report8, h);
        });
    });
}
int xs_kf_align_checkpoint(void *kf, const char *path, const double *T16xN, int N, int iterations, double damping, int min_weight, float max_residual,
                           double *T16_out, double *report8, double *loss_history) {
    if (!path) return -1;   // (before the report is cleared)
    xs_host::align_report_clear(report8, 8);
    return with_checkpoint_map(kf, path, [&](const SecondMap &m) {
        return with_history(loss_history, [&](std::vector<double> *h) {
            return ((KF *)kf)->AlignVolume(m, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report8, h);
        });
    });
}
void xs_kf_align_search_defaults(void *kf, xs_align_search_opts *opts) { ((KF *)kf)->AlignSearchDefaults(opts); }
int xs_kf_score_transforms(void *kf, void *other_kf, int P, const double *T16xP, int stride, int min_weight, float max_residual, double *out2xP) {
    return with_other_map(kf, other_kf, false,
                          [&](const SecondMap &m) { return ((KF *)kf)->ScoreTransformsVolume(m, T16xP, P, stride, min_weight, max_residual, out2xP); });
}
int xs_kf_score_transforms_checkpoint(void *kf, const char *path, int P, const double *T16xP, int stride, int min_weight, float max_residual, double *out2xP) {
    return with_checkpoint_map(kf, path, [&](const SecondMap &m) { return ((KF *)kf)->ScoreTransformsVolume(m, T16xP, P, stride, min_weight, max_residual, out2xP); });
}
int xs_kf_align_map_global(void *kf, void *other_kf, const xs_align_search_opts *opts, double *T16_out, double *report12) {
    return with_other_map(kf, other_kf, false, [&](const SecondMap &m) { return ((KF *)kf)->AlignVolumeGlobal(m, opts, T16_out, report12); });
}
int xs_kf_align_checkpoint_global(void *kf, const char *path, const xs_align_search_opts *opts, double *T16_out, double *report12) {
    if (!path) return -1;   // (before the report is cleared)
    xs_host::align_report_clear(report12, 12);
    return with_checkpoint_map(kf, path, [&](const SecondMap &m) { return ((KF *)kf)->AlignVolumeGlobal(m, opts, T16_out, report12); });
}
// ---- diff ----
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
    return with_other_map(kf, other_kf, false, [&](const SecondMap &m) {
        return ((KF *)kf)->DiffVolume(m, T16, min_weight, lo, hi, cell, min_size, capacity, this_records8, this_count, other_records8, other_count, counts3, this_dense,
                                      other_dense);
    });
}
int xs_kf_diff_checkpoint(void *kf, const char *path, const double *T16, int min_weight, float lo, float hi, int cell, unsigned long long min_size, int capacity,
                          unsigned long long *this_records8, int *this_count, unsigned long long *other_records8, int *other_count,
                          unsigned long long *counts3, unsigned char *this_dense, unsigned char *other_dense) {
    return with_checkpoint_map(kf, path, [&](const SecondMap &m) {
        return ((KF *)kf)->DiffVolume(m, T16, min_weight, lo, hi, cell, min_size, capacity, this_records8, this_count, other_records8, other_count, counts3, this_dense,
                                      other_dense);
    });
}
// ---- render ----
int xs_kf_render_views(void *kf, int views, const float *c2v, int complex_poses, const float *intr4, int rows, int cols, const xs_render_opts *opts, float *depth,
                       uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4, int on_device) {
    return ((KF *)kf)->RenderViews(c2v, complex_poses ? 2 : 1, views, intr4, rows, cols, opts, KF::RenderOutputs{depth, depth_u16, normal, shade, counts4}, on_device);
}
int xs_kf_render_volume(void *kf, const float *src_value, const int *src_weight, size_t src_step, const int *src_res, float src_voxel_size, float src_tranc_dist,
                        int views, const float *c2v, int complex_poses, const float *intr4, int rows, int cols, const xs_render_opts *opts, float *depth,
                        uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4, int on_device) {
    return ((KF *)kf)->RenderSecondMap(second_map(src_value, src_weight, nullptr, src_step, src_res, src_voxel_size, src_tranc_dist), c2v, complex_poses ? 2 : 1, views,
                                       intr4, rows, cols, opts, KF::RenderOutputs{depth, depth_u16, normal, shade, counts4}, on_device);
}
int xs_kf_render_map(void *kf, void *other_kf, int views, const float *c2v, int complex_poses, const float *intr4, int rows, int cols, const xs_render_opts *opts,
                     float *depth, uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4, int on_device) {
    return with_other_map(kf, other_kf, false, [&](const SecondMap &m) {
        return ((KF *)kf)->RenderSecondMap(m, c2v, complex_poses ? 2 : 1, views, intr4, rows, cols, opts, KF::RenderOutputs{depth, depth_u16, normal, shade, counts4}, on_device);
    });
}
int xs_kf_render_checkpoint(void *kf, const char *path, int views, const float *c2v, int complex_poses, const float *intr4, int rows, int cols,
                            const xs_render_opts *opts, float *depth, uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4, int on_device) {
    return with_checkpoint_map(kf, path, [&](const SecondMap &m) {
        return ((KF *)kf)->RenderSecondMap(m, c2v, complex_poses ? 2 : 1, views, intr4, rows, cols, opts, KF::RenderOutputs{depth, depth_u16, normal, shade, counts4}, on_device);
    });
}
// ---- sample ----
int xs_kf_sample_points(void *kf, long long n, const float *points, const double *T16, int min_weight, unsigned char *status, float *value, float *dvalue,
                        float *gradient, unsigned long long *counts4, int on_device) {
    return ((KF *)kf)->SamplePoints(points, n, T16, min_weight, KF::SampleOutputs{status, value, dvalue, gradient, counts4}, on_device);
}
int xs_kf_sample_volume(void *kf, const float *src_value, const int *src_weight, const float *src_grad, size_t src_step, const int *src_res, float src_voxel_size,
                        float src_tranc_dist, long long n, const float *points, const double *T16, int min_weight, unsigned char *status, float *value,
                        float *dvalue, float *gradient, unsigned long long *counts4, int on_device) {
    return ((KF *)kf)->SampleSecondMap(second_map(src_value, src_weight, src_grad, src_step, src_res, src_voxel_size, src_tranc_dist), points, n, T16, min_weight,
                                       KF::SampleOutputs{status, value, dvalue, gradient, counts4}, on_device);
}
int xs_kf_sample_map(void *kf, void *other_kf, long long n, const float *points, const double *T16, int min_weight, unsigned char *status, float *value,
                     float *dvalue, float *gradient, unsigned long long *counts4, int on_device) {
    return with_other_map(kf, other_kf, dvalue != nullptr, [&](const SecondMap &m) {   // (the grad array only where dvalue is wanted)
        return ((KF *)kf)->SampleSecondMap(m, points, n, T16, min_weight, KF::SampleOutputs{status, value, dvalue, gradient, counts4}, on_device);
    });
}
int xs_kf_sample_checkpoint(void *kf, const char *path, long long n, const float *points, const double *T16, int min_weight, unsigned char *status, float *value,
                            float *dvalue, float *gradient, unsigned long long *counts4, int on_device) {
    return with_checkpoint_map(kf, path, [&](const SecondMap &m) {
        return ((KF *)kf)->SampleSecondMap(m, points, n, T16, min_weight, KF::SampleOutputs{status, value, dvalue, gradient, counts4}, on_device);
    });
}
int xs_kf_frame_residuals(void *kf, const unsigned short *depth, size_t depth_step, const float *c2v, int complex_poses, const float *intr4, int rows, int cols,
                          int min_weight, unsigned char *status, float *value, float *dvalue, float *gradient, unsigned long long *counts4, int on_device) {
    return ((KF *)kf)->FrameResiduals(depth, depth_step, c2v, complex_poses ? 2 : 1, intr4, rows, cols, min_weight,
                                      KF::SampleOutputs{status, value, dvalue, gradient, counts4}, on_device);
}
// ---- register ----
int xs_kf_register_points(void *kf, long long n, const float *points, int on_device, const double *T16xN, int N, int iterations, double damping,
                          int min_weight, float max_residual, double *T16_out, double *report7, double *loss_history) {
    return with_history(loss_history, [&](std::vector<double> *h) {
        return ((KF *)kf)->RegisterPoints(points, n, on_device, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report7, h);
    });
}
int xs_kf_register_map(void *kf, void *other_kf, long long n, const float *points, int on_device, const double *T16xN, int N, int iterations,
                       double damping, int min_weight, float max_residual, double *T16_out, double *report7, double *loss_history) {
    xs_host::register_report_clear(report7);   // (before the source is looked at)
    return with_other_map(kf, other_kf, false, [&](const SecondMap &m) {
        return with_history(loss_history, [&](std::vector<double> *h) {
            return ((KF *)kf)->RegisterSecondMap(m, points, n, on_device, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report7, h);
        });
    });
}
int xs_kf_register_checkpoint(void *kf, const char *path, long long n, const float *points, int on_device, const double *T16xN, int N, int iterations,
                              double damping, int min_weight, float max_residual, double *T16_out, double *report7, double *loss_history) {
    if (!path) return -1;   // (before the report is cleared)
    xs_host::register_report_clear(report7);
    return with_checkpoint_map(kf, path, [&](const SecondMap &m) {
        return with_history(loss_history, [&](std::vector<double> *h) {
            return ((KF *)kf)->RegisterSecondMap(m, points, n, on_device, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report7, h);
        });
    });
}
// ---- score a cloud's transforms, register with no guess (the map: this instance's through a null source, another instance's, a file's) ----
int xs_kf_score_point_transforms(void *kf, long long n, const float *points, int on_device, int P, const double *T16xP, int stride, int min_weight,
                                 float max_residual, double *out2xP) {
    return ((KF *)kf)->ScorePointTransforms(nullptr, points, n, on_device, T16xP, P, stride, min_weight, max_residual, out2xP);
}
int xs_kf_score_point_transforms_map(void *kf, void *other_kf, long long n, const float *points, int on_device, int P, const double *T16xP, int stride,
                                     int min_weight, float max_residual, double *out2xP) {
    return with_other_map(kf, other_kf, false, [&](const SecondMap &m) {
        return ((KF *)kf)->ScorePointTransforms(&m, points, n, on_device, T16xP, P, stride, min_weight, max_residual, out2xP);
    });
}
int xs_kf_score_point_transforms_checkpoint(void *kf, const char *path, long long n, const float *points, int on_device, int P, const double *T16xP,
                                            int stride, int min_weight, float max_residual, double *out2xP) {
    return with_checkpoint_map(kf, path, [&](const SecondMap &m) {
        return ((KF *)kf)->ScorePointTransforms(&m, points, n, on_device, T16xP, P, stride, min_weight, max_residual, out2xP);
    });
}
void xs_kf_register_search_defaults(void *kf, xs_register_search_opts *opts) { ((KF *)kf)->RegisterSearchDefaults(opts); }
int xs_kf_register_points_global(void *kf, long long n, const float *points, int on_device, const xs_register_search_opts *opts, double *T16_out,
                                 double *report12) {
    return ((KF *)kf)->RegisterPointsGlobal(nullptr, points, n, on_device, opts, T16_out, report12);
}
int xs_kf_register_points_global_map(void *kf, void *other_kf, long long n, const float *points, int on_device, const xs_register_search_opts *opts,
                                     double *T16_out, double *report12) {
    xs_host::align_report_clear(report12, 12);   // (before the source is looked at)
    return with_other_map(kf, other_kf, false, [&](const SecondMap &m) { return ((KF *)kf)->RegisterPointsGlobal(&m, points, n, on_device, opts, T16_out, report12); });
}
int xs_kf_register_points_global_checkpoint(void *kf, const char *path, long long n, const float *points, int on_device,
                                            const xs_register_search_opts *opts, double *T16_out, double *report12) {
    if (!path) return -1;   // (before the report is cleared)
    xs_host::align_report_clear(report12, 12);
    return with_checkpoint_map(kf, path, [&](const SecondMap &m) { return ((KF *)kf)->RegisterPointsGlobal(&m, points, n, on_device, opts, T16_out, report12); });
}
// ---- the edits of this instance's own map ----
int xs_kf_reintegrate(void *kf, int n, const uint16_t *const *depth_dev, size_t step_bytes, const float *c2v_old32xN, const float *c2v_new32xN,
                      const int *mode, const int *frame_index, unsigned long long *counts4) {
    KF *k = (KF *)kf;
    if (n < 1 || !depth_dev || !mode) return -1;
    std::vector<DeviceArray2D<ushort>> depths;
    for (int i = 0; i < n; ++i) depths.push_back(DeviceArray2D<ushort>(k->depth_height, k->depth_width, const_cast<uint16_t *>(depth_dev[i]), step_bytes));   // borrowed
    const std::vector<Matrix4cf> olds = poses_of(c2v_old32xN, c2v_old32xN ? n : 0), news = poses_of(c2v_new32xN, c2v_new32xN ? n : 0);
    return k->ReintegrateFrames(n, depths.data(), olds.empty() ? nullptr : olds.data(), news.empty() ? nullptr : news.data(), mode, frame_index, counts4);
}
int xs_kf_fuse_points(void *kf, long long n, const float *points, int on_device, const double *T16, const float *origin3, float min_range, float max_range,
                      int carve, int weight, unsigned long long *counts5) {
    return ((KF *)kf)->FusePoints(points, n, on_device, T16, origin3, min_range, max_range, carve, weight, counts5);
}
void xs_kf_release_fuse_scratch(void *kf) { ((KF *)kf)->ReleaseFuseScratch(); }

}  // extern "C"
