// xs_pipeline_capi.cpp — C ABI over KinectFusionReconstruction (include/xslam_amd_pipeline.h): create and destroy, the frame path, relocalisation,
// planning, export, statistics, debug and the instance's own checkpoints.  The calls that take no instance are in xs_host_capi.cpp, the ones
// that take a second map or edit or query a map in xs_pipeline_maps_capi.cpp.
#include "../../include/xslam_amd_pipeline.h"
#include "kf_internal.hpp"
#include <exception>
#include <memory>

typedef KinectFusionReconstruction KF;
using xs_host::Matrix4cf;

static DeviceArray2D<ushort> wrap_depth(KF *k, const uint16_t *depth_dev, size_t step_bytes) {   // borrowed, not counted
    return DeviceArray2D<ushort>(k->depth_height, k->depth_width, const_cast<uint16_t *>(depth_dev), step_bytes);
}
// The two batched relocalisations: `run(depths, poses, histories or null)` is RelocalizeGaussNewtonBatch or RelocalizeNewtonBatch; the poses
// come back in place and frame f's loss history goes to loss_out + f (iterations + 1).
template <class Run>
static int relocalize_batch(KF *k, int frames, const uint16_t *const *depth_dev, size_t step_bytes, float *c2v32xF, int iterations, double *loss_out, int *ok_out,
                            Run &&run) {
    if (frames < 0 || (frames > 0 && (!depth_dev || !c2v32xF || !ok_out))) return -1;
    std::vector<DeviceArray2D<ushort>> depths;
    for (int f = 0; f < frames; ++f) depths.push_back(wrap_depth(k, depth_dev[f], step_bytes));
    std::vector<Matrix4cf> m = poses_of(c2v32xF, frames);
    std::vector<std::vector<double>> hist(loss_out ? (size_t)frames : 0);
    const int n = run(depths, m.data(), loss_out ? hist.data() : nullptr);
    for (int f = 0; f < frames; ++f) {
        pose_to(m[(size_t)f], c2v32xF + 32 * (size_t)f);
        if (loss_out)
            for (size_t i = 0; i < hist[(size_t)f].size() && i <= (size_t)iterations; ++i) loss_out[(size_t)f * (iterations + 1) + i] = hist[(size_t)f][i];
    }
    return n;
}
// an optional start pose: null stays null
static const Matrix4cf *start_of(const std::vector<Matrix4cf> &start) { return start.empty() ? nullptr : start.data(); }

extern "C" {

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

void xs_kf_set_gt_poses(void *kf, int n, const float *c2w32) { ((KF *)kf)->gt_poses = poses_of(c2w32, n); }
// ---- the frame path ----
int xs_kf_process_frame(void *kf, const uint16_t *depth_dev, size_t step_bytes) {
    KF *k = (KF *)kf;
    DeviceArray2D<ushort> view(k->depth_height, k->depth_width, (void *)depth_dev, step_bytes);  // borrowed, not counted
    return k->ProcessFrame(view);
}
void xs_kf_hint_next_frame(void *kf, const uint16_t *depth_dev, size_t step_bytes) { ((KF *)kf)->HintNextFrame(depth_dev, step_bytes); }
int xs_kf_process_frame_host(void *kf, const uint16_t *depth_host) { return ((KF *)kf)->ProcessFrameHost(depth_host); }
uint16_t *xs_kf_ingest_buffer(void *kf) { return ((KF *)kf)->IngestBuffer(); }
void xs_kf_get_camera2volume(void *kf, float *out32) { pose_to(((KF *)kf)->getCamera2Volume(), out32); }
// ---- relocalisation ----
int xs_kf_gauss_newton_terms(void *kf, const uint16_t *depth_dev, size_t step_bytes, const float *c2v32, double *out29) {
    KF *k = (KF *)kf;
    return k->GaussNewtonTerms(wrap_depth(k, depth_dev, step_bytes), pose_of(c2v32), out29);
}
int xs_kf_relocalize(void *kf, const uint16_t *depth_dev, size_t step_bytes, float *c2v32, int iterations, float damping, double *loss_out) {
    KF *k = (KF *)kf;
    Matrix4cf m = pose_of(c2v32);
    std::vector<double> hist;
    const int rc = k->RelocalizeGaussNewton(wrap_depth(k, depth_dev, step_bytes), m, iterations, damping, loss_out ? &hist : nullptr);
    pose_to(m, c2v32);
    if (loss_out) for (size_t i = 0; i < hist.size() && i <= (size_t)iterations; ++i) loss_out[i] = hist[i];
    return rc;
}
int xs_kf_relocalize_batch(void *kf, int frames, const uint16_t *const *depth_dev, size_t step_bytes, float *c2v32xF, int iterations, float damping,
                           double *loss_out, int *ok_out) {
    KF *k = (KF *)kf;
    return relocalize_batch(k, frames, depth_dev, step_bytes, c2v32xF, iterations, loss_out, ok_out,
                            [&](const std::vector<DeviceArray2D<ushort>> &depths, Matrix4cf *m, std::vector<double> *hist) {
                                return k->RelocalizeGaussNewtonBatch(depths, m, iterations, damping, ok_out, hist);
                            });
}
int xs_kf_pose_hessian_terms(void *kf, const uint16_t *depth_dev, size_t step_bytes, const float *c2v32, double *out29) {
    KF *k = (KF *)kf;
    return k->PoseHessianTerms(wrap_depth(k, depth_dev, step_bytes), pose_of(c2v32), out29);
}
int xs_kf_relocalize_newton_batch(void *kf, int frames, const uint16_t *const *depth_dev, size_t step_bytes, float *c2v32xF, int iterations, float damping,
                                  double *loss_out, int *ok_out, int *fallbacks_out) {
    KF *k = (KF *)kf;
    return relocalize_batch(k, frames, depth_dev, step_bytes, c2v32xF, iterations, loss_out, ok_out,
                            [&](const std::vector<DeviceArray2D<ushort>> &depths, Matrix4cf *m, std::vector<double> *hist) {
                                return k->RelocalizeNewtonBatch(depths, m, iterations, damping, ok_out, hist, fallbacks_out);
                            });
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
    return k->ScorePoses(wrap_depth(k, depth_dev, step_bytes), poses_of(c2v32xP, poses).data(), poses, out2xP);
}
int xs_kf_relocalize_global(void *kf, const uint16_t *depth_dev, size_t step_bytes, int poses, const float *c2v32xP, int keep, int iterations,
                            float damping, float *best_c2v32, double *report8) {
    KF *k = (KF *)kf;
    if (poses < 0 || !report8 || !best_c2v32 || (poses > 0 && (!depth_dev || !c2v32xP))) return -1;
    Matrix4cf best = pose_of(best_c2v32);
    const int rc = k->RelocalizeGlobal(wrap_depth(k, depth_dev, step_bytes), poses_of(c2v32xP, poses).data(), poses, keep, iterations, damping, best, report8);
    pose_to(best, best_c2v32);
    return rc;
}
long long xs_kf_relocalization_index_voxels(void *kf) { return ((KF *)kf)->RelocalizationIndexVoxels(); }
// ---- planning ----
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
    return ((KF *)kf)->Reachable(start_of(start), radius_m, snap_vox, unknown_blocks, min_weight, P, poses_of(c2v32xP, P).data(), reachable, clear2);
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
    return ((KF *)kf)->Travel(start_of(start), radius_m, snap_vox, unknown_blocks, min_weight, max_travel_m, P, poses_of(c2v32xP, P).data(), reachable, clear2,
                              travel3);
}
int xs_kf_path_to(void *kf, const float *start_c2v32_or_null, float radius_m, int snap_vox, int unknown_blocks, int min_weight, float max_travel_m,
                  const float *target_c2v32, int capacity, int *voxels3, float *points3, int *needed_out) {
    if (!target_c2v32) return -1;
    const std::vector<Matrix4cf> start = poses_of(start_c2v32_or_null, start_c2v32_or_null ? 1 : 0);
    return ((KF *)kf)->PathTo(start_of(start), radius_m, snap_vox, unknown_blocks, min_weight, max_travel_m, pose_of(target_c2v32), capacity, voxels3, points3,
                              needed_out);
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
        for (int p = 0; p < *count_out; ++p) pose_to(m[(size_t)p], c2v32xP_out + 32 * (size_t)p);
    return rc;
}
// ---- export ----
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
// ---- state, statistics and debug ----
int xs_kf_frame_id(void *kf) { return ((KF *)kf)->frame_id; }
int xs_kf_num_poses(void *kf) { return (int)((KF *)kf)->world2camera_record.size(); }
void xs_kf_get_world2camera(void *kf, int idx, float *out32) {
    KF *k = (KF *)kf;
    if (idx < 0) idx += (int)k->world2camera_record.size();
    pose_to(k->world2camera_record[idx], out32);
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
// ---- the instance's own checkpoints ----
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

}  // extern "C"
