// KinectFusionReconstruction.h — host orchestrator of the XKinectFusion CSFD pipeline on one
// MI355X.  Same class name, public fields and method names as the reference
// (XKinectFusion/include/KinectFusionReconstruction.h:19-174), so a caller of the reference's
// class (Experiments/test_xkinect_fusion/main.cpp:38-58) drives this one the same way:
//     KinectFusionReconstruction kinfu;  kinfu.SetYamlParameters(config);
//     kinfu.ProcessFrame(depth_frame_d);  kinfu.world2camera_record.back();
// Host algebra comes from host_algebra.hpp (no Eigen), config from flat_yaml.hpp (no yaml-cpp).
//
// Additions: the CSFD seed is a parameter (keys csfd_seed_row / csfd_seed_col / csfd_seed_h; the
// reference has the seed line commented out, KinectFusionReconstruction.cpp:22); per-stage HIP
// event timing; counters of updated voxels and raycast hits; volume checkpoint save / load.
#pragma once
#include "TsdfVolume.h"
#include "flat_yaml.hpp"
#include "merge_host.hpp"   // SecondMap
#include "../csrc/xs_host_wait.h"
#include <chrono>
#include <string>
#include <vector>

struct xs_align_search_opts;   // include/xslam_amd_pipeline.h
struct xs_register_search_opts;

class KinectFusionReconstruction {
public:
    typedef xs_host::Matrix3cf Matrix3frm;  // row-major complex 3x3
    typedef xs_host::Matrix4cf Matrix4cf;
    typedef xs_host::Vector3cf Vector3cf;
    enum Stage { ST_SURFACE = 0, ST_ICP, ST_SCALE, ST_INTEGRATE, ST_RAYCAST, ST_RESIZE, ST_COUNT };

    xs_host::FlatYaml config;
    int num_levels = 3;
    Matrix4cf world2camera;
    Matrix4cf world2volume;
    std::vector<Matrix4cf> world2camera_record;
    int frame_id = 0;
    int frame_step = 1;
    std::vector<Matrix4cf> gt_poses{};  // camera-to-world; complex so a CSFD seed can ride on a given pose

    Intr kinect_intrinsic;
    int depth_width = 0, depth_height = 0;

    Vector3i volume_resolution;
    float voxel_size{};
    TsdfVolume *tsdf_volume_d_ptr = nullptr;
    int max_integration_weight = 0;

    int icp_iterations[3]{};
    float distThres{};
    float angleThres{};
    DeviceArray2D<devComplexICP> g_buf;  // kept for signature compatibility; unused by the fused reduction
    DeviceArray<devComplexICP> sum_buf;

    float trunc_logistic_k = 0.f;
    float biInterpolate_threshold{0.005f};

    std::vector<DeviceArray2D<devComplex>> depths_curr_d, vmaps_curr_d, nmaps_curr_d, vmaps_g_prev_d, nmaps_g_prev_d;
    DeviceArray2D<float> depthRawScaled_d;
    // the current-frame maps' real parts as float planes (their imaginary parts are zeros: the depth image is real) — what the
    // ICP reduction reads (half the bytes); YAML icp_real_current_maps, default true
    std::vector<DeviceArray2D<float>> vreal_curr_d, nreal_curr_d;
    bool icp_real_current_maps = true;
    // the integrate call's brick classification enqueued behind the last ICP launch, with the pose that launch starts from (YAML
    // integrate_classify_ahead, default true; single GPU with the posted ICP loop): IntegrateFrame then finds the list ready
    bool integrate_classify_ahead = true;
    // (the other schedules of the classification and the integrate launch that were measured and not adopted: DESIGN.md Appendix A)
    long long list_cover_counts_[4] = {0, 0, 0, 0};   // what xs_integrate_list_covers said of the lists classified ahead (xs_kf_list_cover_counts)
    long long composite_bytes_ = 0;   // bytes this rank received through the raycast composite's collectives so far (ring all-reduce: 2 (N - 1) / N x size; gather: the other ranks' parts)
    float integrate_classify_slack = 2.0f;   // YAML integrate_classify_slack: how much wider than its own the list's frustum slack is (1 = every frame falls back)
    // The sign map of the ray march (include/xslam_amd.h, csrc/xs_signmap.h; YAML raycast_sign_map, default true; raycast_sign_map_shift, default 0 =
    // the finest bricks the march can use: 8^3 voxels at 512^3): the integrate kernel marks the bricks it writes negative values into, the march starts every ray at the first
    // step that can end it — the same maps bit for bit (tests/test_signmap_gpu.py), about a fifth of the volume reads.  A rank of a sharded
    // volume keeps a map of the planes it stores (owned slab + halo) and its slab march evaluates the iterations that map leaves.
    bool raycast_sign_map = true;
    int raycast_sign_map_shift = 0;
    void RebuildSignMap();   // call after writing the value array through xs_kf_volume_ptr
    // the value array's address has been handed out (xs_kf_volume_ptr): whoever holds it may write the volume behind the integrate kernels'
    // back, after which the sign map is no longer a superset — it is rebuilt from the volume in front of the next raycast
    void MarkSignMapStale() { sign_map_stale_ = true; }
    bool sign_map_stale_ = false;
    // Look-ahead of the map preparation (no counterpart in the reference, whose main.cpp:50-58 reads, uploads and processes one frame at a
    // time): the caller names the depth image it will pass to the NEXT ProcessFrame call — device memory, unchanged until then — and that
    // frame's bilateral filter and depth pyramid are built during this frame's ICP loop.  A ProcessFrame call with any other image simply
    // prepares its own maps as always.  Same results bit for bit (tests/test_pipeline_gpu.py).
    void HintNextFrame(const ushort *depth_dev, size_t step_bytes) {
        if (next_stage_ != 0) EnqueueAnnouncedFrame(true);   // (an announcement half enqueued is finished first: never expected)
        next_hint_ptr_ = depth_dev; next_hint_step_ = step_bytes;
    }
    void EnqueueAnnouncedFrame(bool all);
    int next_stage_ = 0;
    void EnqueueMapsFromPyramid();
    void EnqueueScale(const DeviceArray2D<ushort> &depth_frame_d);
    void SwapMapSets();
    bool list_ready_ = false;
    float list_Rv2c_[18]{}, list_tv2c_[6]{};
    void ClassifyAhead(const Matrix3frm &Rcurr, const Vector3cf &tcurr);
    bool real_maps_valid_ = false;

    bool use_gtPose = false;

    // CSFD seed: i*h on world2camera(row, col); row < 0 disables
    int csfd_seed_row = -1, csfd_seed_col = -1;
    float csfd_seed_h = 1e-7f;

    // z-slab / pixel-row sharding across GPUs (no counterpart in the single-GPU
    // reference).  Rank r of G owns z planes [zo0, zo1) and stores [zs0, zs1) = owned + halo; it
    // integrates its own storage, evaluates the ICP rows [r*H/G, (r+1)*H/G) of each level and the
    // march steps of every ray that land in its planes.  collective(user, op, dev_ptr, count)
    // must all-reduce in place over the ranks on the current stream: op 0 = sum of doubles,
    // 1 = min of int32, 2 = sum of int32.
    typedef void (*collective_fn)(void *user, int op, void *dev_ptr, long count);
    enum { HALO = 6 };
    int shard_rank = 0, shard_count = 1;
    int zo0 = 0, zo1 = 0, zs0 = 0, zs1 = 0;
    collective_fn collective = nullptr;
    void *collective_user = nullptr;
    void SetSharding(int rank, int count, collective_fn fn, void *user);  // call before SetYamlParameters

    // false (default): the reference's shape, one host solve per ICP iteration (the host spins on a
    // completion word the kernel writes into pinned memory; with icp_post_pose below the next launch is
    // already resident when the solve ends: ICP stage 0.24 ms).  true: the pose update runs on the device
    // (xs_icp_iterate) and the host waits once per frame — slower on this machine (a serial
    // double-precision Cholesky + substitution is ~9000 cycles for one wave, plus a second launch per
    // iteration: 0.35 ms), kept for hosts that cannot spin.  YAML key icp_solve_on_device.
    bool icp_solve_on_device = false;
    // true (default): each iteration's launch is enqueued while the previous one is still running and
    // receives its pose through a pinned-memory mailbox once the host has solved for it
    // (xs_icp_accumulate_posted / xs_icp_post_pose): the launch latency leaves the per-iteration
    // turnaround.  Same kernel arithmetic, same poses.  false: launch after the solve (the reference's
    // order).  Applies when this rank evaluates whole images (not with icp_shard_rows).  YAML key
    // icp_post_pose.
    bool icp_post_pose = true;
    int icp_lookahead = 1;   // posted launches kept in the queue ahead of the one the host waits for (>= 1; more measured the same)
    // The final addition of an ICP reduction on the host (xs_icp_accumulate_records / xs_icp_sum_records): every
    // workgroup writes its record of 55 partial sums straight into pinned host memory and leaves; the host — which is
    // spinning for the result anyway — adds the records in index order.  Takes the cross-XCD gather (write-back, ticket,
    // last workgroup reading every record from memory) out of the launch.  Measured no faster than the device gather
    // (profiles/r02_ab_icp_fold.txt: 2 270-2 540 against 2 530-2 550 frames/s — 90-512 workgroups each pushing 448 bytes
    // and a system-scope release over PCIe cost what the agent-scope publish + final sum cost), so it is off by default.
    // YAML key icp_host_fold.
    bool icp_host_fold = false;
    // Every ICP sum reaches the host as one 16-byte store {sequence number, sum} (XS_ICP_PUBLISH_PAIRS, include/xslam_amd.h): no completion word that
    // has to be ordered behind the sums — the kernel's last workgroup skips the wait for its stores' acknowledgement, a barrier and a release store
    // per launch.  YAML key icp_publish_pairs; the launches of the host-solve loop only (not icp_host_fold, not the device solve).
    bool icp_publish_pairs = true;
    // Sharded runs (SetSharding): false (default) — every rank evaluates the whole ICP itself; all ranks hold
    // the same current-frame maps and the composited previous-frame maps, the reduction is deterministic,
    // so they reach the same pose bit for bit with no collective inside the ICP loop.  true — pixel rows
    // are split across ranks and the 55 sums are all-reduced every iteration: 12
    // latency-bound collectives + host waits per frame to save < 0.1 ms of kernel time.  YAML key
    // icp_shard_rows.
    bool icp_shard_rows = false;
    // test aid: take the slab raycast + composite (and its collectives) even with a single rank
    bool force_shard_composite = false;

    // instrumentation
    bool profiling = false;
    double stage_ms[ST_COUNT] = {0, 0, 0, 0, 0, 0};
    long long stage_calls[ST_COUNT] = {0, 0, 0, 0, 0, 0};
    std::vector<double> icp_log;  // per ICP iteration of the last frame: 54 sums + inliers
    long long cum_updated = 0, cum_hits = 0;  // summed over profiled frames (read back with the stage times)

    KinectFusionReconstruction();
    ~KinectFusionReconstruction();

    int getFrame() const { return frame_id; }
    int getVolumeSize() const { return volume_resolution[0] * volume_resolution[1] * volume_resolution[2]; }
    const int *res3() const { return volume_resolution.v; }   // the resolution as the launchers take it
    Matrix4cf getCamera2Volume() { return world2volume * xs_host::inverse(world2camera); }

    void AllocateBuffers();
    void ReleaseBuffers();
    void SetYamlParameters(const xs_host::FlatYaml &config_);
    int ProcessFrame(const DeviceArray2D<ushort> &depth_frame_d);
    int ProcessFrameHost(const ushort *depth_host);  // dense rows of depth_width u16; pinned or pageable
    ushort *IngestBuffer();                          // next host-pinned staging buffer (decode into it, then ProcessFrameHost(it))
    void SurfaceMeasure(const DeviceArray2D<ushort> &depth_frame_d);
    int PoseEstimate(Matrix3frm Rcurr, Vector3cf tcurr, Matrix3frm Rprev_inv, Vector3cf tprev);
    int AlignDepthToReconstruction(const DeviceArray2D<ushort> &depth_frame_d, bool use_LM = false);
    int IntegrateFrame(const DeviceArray2D<ushort> &depth_frame_d);
    static int SmoothDepthFrame(MapArr &dst_d, const DeviceArray2D<ushort> &src_d);
    int CalculatePointCloud(MapArr &xyz_g_d, MapArr &normal_g_d);
    void ModelMapPyramid();

    static inline Vector3cf GetTranslation(Matrix4cf &trans_mat) { return xs_host::GetTranslation(trans_mat); }
    static inline Matrix3frm GetRotation(Matrix4cf &trans_mat) { return xs_host::GetRotation(trans_mat); }

    // Pose refinement against the map by Gauss-Newton on the TSDF residual of ComputeLocalTsdf_hessian, with the
    // Jacobian from first-order CSFD: six poses seeded with i*h along the generators of a left perturbation
    // camera2volume <- se3Exp(xi) * camera2volume, all evaluated in one pass over the volume
    // (xs_tsdf_gauss_newton_terms).  BASELINE config 5; the reference only has the commented single-direction
    // ComputeTSDF_loss / ComputeTSDF_hessian (:374-434).  A sharded rank evaluates its slab and the 29 sums are
    // all-reduced.  GaussNewtonTerms fills {JtJ upper triangle (21), Jtr (6), sum r^2, count}, already divided by h.
    int GaussNewtonTerms(const DeviceArray2D<ushort> &depth_frame_d, const Matrix4cf &camera2volume, double out29[29]);
    int RelocalizeGaussNewton(const DeviceArray2D<ushort> &depth_frame_d, Matrix4cf &camera2volume, int iterations, float damping,
                              std::vector<double> *loss_history = nullptr);
    // the loop protocol of the Gauss-Newton passes (see RelocalizeGaussNewton): YAML gn_post_pose, default true
    bool gn_post_pose = true;
    bool gn_publish_sharded = true;   // shard mode: the all-reduced sums reach the host through a publish kernel + pinned record (false: copy + stream drain)
    double gn_pass_us = 0, gn_kernel_ms = 0;       // wall clock of the passes RelocalizeGaussNewton ran (from its first kernel enqueued to its last sums seen) / kernel durations of the profiled passes
    long long gn_passes = 0, gn_kernel_calls = 0;
    double gn_poll_us = 0;             // summed over the passes enqueued ahead: what the resident kernel waited for its poses (its own 100 MHz clock): the host's side of a pass
    long long gn_poll_passes = 0;
    const float *GaussNewtonPrepare(const DeviceArray2D<ushort> &depth_frame_d);
    void GaussNewtonEnqueue(const DeviceArray2D<ushort> &depth_frame_d, const float *gt, const float (*R)[18], const float (*t)[6], unsigned mail_seq,
                            unsigned long long seq);
    bool GaussNewtonWait(unsigned long long seq, double out29[29]);
    void GaussNewtonCollectEvents();
    // Batched relocalisation against a fixed map: the band voxels of the owned planes are compacted once per volume
    // generation into an index in the six-pose kernel's own dealing order (xs_tsdf_band_build), and every pass evaluates the index for all frames
    // still active, at most XS_BAND_MAX_FRAMES per launch (xs_tsdf_gauss_newton_terms_band).  Frame f's sums are bit-identical to the dense pass's,
    // and the host step is RelocalizeGaussNewton's own (gn_host.hpp: damped_spd6_step inside gn_batch_loop): ok[f], camera2volume[f] and loss_history[f] are what RelocalizeGaussNewton
    // returns for that frame alone.  A frame that fails or finishes drops out of the launches.  In shard mode the F x 29 sums are all-reduced.
    // loss_history: null, or F vectors (each gets the losses RelocalizeGaussNewton would give it).  Returns the number of frames that succeeded.
    int RelocalizeGaussNewtonBatch(const std::vector<DeviceArray2D<ushort>> &depths, Matrix4cf *camera2volume, int iterations, float damping,
                                   int *ok, std::vector<double> *loss_history = nullptr);
    // The exact pose Hessian and Newton relocalisation: one launch of xs_tsdf_pose_hessian_band over the band index gives,
    // per frame, the 6 x 6 Hessian and the gradient of L = sum r^2 in the twist of camera2volume <- se3Exp(theta) * camera2volume (21 dual-complex
    // seeded poses, newton_host.hpp).  PoseHessianTerms fills {H upper triangle (21), g (6), sum r^2, count}, divided by h^2 / h.  The loops are
    // RelocalizeGaussNewtonBatch's with the step (H + damping diag H) delta = -g; a frame whose damped Hessian is not positive definite takes the
    // Gauss-Newton step for that iteration (fallbacks[f] counts them).  No posted poses: copy + stream drain per pass.  Sharded: the sums are all-reduced.
    int PoseHessianTerms(const DeviceArray2D<ushort> &depth_frame_d, const Matrix4cf &camera2volume, double out29[29]);
    int RelocalizeNewtonBatch(const std::vector<DeviceArray2D<ushort>> &depths, Matrix4cf *camera2volume, int iterations, float damping, int *ok,
                              std::vector<double> *loss_history = nullptr, int *fallbacks = nullptr);
    // Global relocalisation: the camera is lost and there are pose hypotheses.  ScorePoses evaluates the real-valued
    // alignment loss of one depth frame at P camera2volume poses in one pass over the band index per chunk of XS_SCORE_MAX_POSES
    // (xs_tsdf_score_poses_band): out2xP + 2 p = {sum loss, count} at the real part of inverse(camera2volume[p]) — the bits newton_seeded_poses
    // puts in its real parts.  Sharded: a chunk's 2 n doubles are all-reduced.  Returns 1, or 0 without a volume.
    // RelocalizeGlobal scores the P candidates, keeps the min(keep, P) with the highest S = count - sum loss (score_host.hpp), refines them with
    // RelocalizeGaussNewtonBatch (the same depth in every slot), scores the refined poses and returns in `best` the one with the highest S
    // among those whose loop ended ok.  report: {winner's candidate index, its S before, its S after, sum loss after, count after, number of
    // the kept that ended ok, band voxels in the index, 0}.  Returns 1, or 0 with `best` untouched when none ended ok.
    int ScorePoses(const DeviceArray2D<ushort> &depth_frame_d, const Matrix4cf *camera2volume, int P, double *out2xP);
    int RelocalizeGlobal(const DeviceArray2D<ushort> &depth_frame_d, const Matrix4cf *candidates, int P, int keep, int iterations, float damping,
                         Matrix4cf &best, double report[8]);
    // Next best view: what would the camera see from each of P hypothetical camera2volume poses?  ScoreViews casts a
    // lattice of rays per pose through the observation grid of the volume (two bits per voxel: unknown / free / occupied at `min_weight`;
    // allocated on first use, rebuilt when volume_generation or min_weight differ from what it was built at) in one launch of xs_score_views
    // per chunk of XS_VIEW_MAX_POSES: out4xP + 4 p = {unknown, free, hits, frontier} at the real part of camera2volume[p].  opts: null for the
    // defaults (80 x 60 rays of the level-0 camera, depths 0.2 .. 5.0 in steps of a voxel).  NextBestView scores and returns the index of the
    // pose with the most unknown samples among those with hits >= min_hits (view_host.hpp), -1 when none qualifies; out4xP may be null.
    // ScoreViews returns 1 when it ran, 0 without a volume, -1 on bad arguments or options; NextBestView -3 on those and -1 without a volume.
    // Both return -2 in shard mode with nothing done: occlusion along a ray is not additive over z-slabs.
    int ScoreViews(const Matrix4cf *camera2volume, int P, const xs_view_opts *opts, int min_weight, unsigned *out4xP);
    int NextBestView(const Matrix4cf *camera2volume, int P, const xs_view_opts *opts, int min_weight, unsigned min_hits, unsigned *out4xP);
    // Clearance and reachability: can the camera be at a candidate, and get there?  ClearanceField builds (or takes
    // from its cache) the field of xs_clearance_build over the observation grid at `min_weight` — min(d^2, R^2) per voxel to the nearest
    // obstacle, R = max_radius_vox — and copies its X * Y * Z uint16 to host_out.  Reachable floods the known free space a body of
    // radius_m fits in (r2 and R by view_host.hpp's reach_radius) from `start` (null: the current camera2volume), whose translation's voxel is
    // first snapped to the nearest passable voxel within snap_vox (the sensor observes nothing at its own centre); no such voxel: nothing is
    // reachable, which is a result.  reachable[p] = 1 iff the centre voxel of camera2volume[p] (not snapped) was reached, clear2[p] the
    // field there (0 outside the volume).  NextReachableView scores like NextBestView and picks by the same rule among the reachable
    // candidates (view_host.hpp's next_reachable_view), starting from the current camera; reachable (optional) receives the flags.
    // The field, the reach buffer and the flood are cached and redone when volume_generation, min_weight, unknown_blocks, R, r2 or the
    // snapped seed differ from what they were built with.  ClearanceField and Reachable return 1 when they ran, 0 without a volume, -1 on
    // bad arguments (R or snap out of range among them); NextReachableView -3 on those and -1 when nobody qualifies or there is no volume.
    // All return -2 in shard mode with nothing done: distance and connectivity are not additive over z-slabs.
    int ClearanceField(int max_radius_vox, int unknown_blocks, int min_weight, unsigned short *host_out);
    int Reachable(const Matrix4cf *start, float radius_m, int snap_vox, int unknown_blocks, int min_weight, int P, const Matrix4cf *camera2volume,
                  unsigned char *reachable, unsigned short *clear2);
    int NextReachableView(const Matrix4cf *camera2volume, int P, const xs_view_opts *opts, int min_weight, unsigned min_hits, unsigned *out4xP,
                          float radius_m, int snap_vox, int unknown_blocks, unsigned char *reachable);
    // Travel cost and shortest collision-free path: how far is a candidate, and which way?  Travel is Reachable plus
    // travel3[p], the uint16 cost of xs_travel_build's field (include/xslam_amd.h: the contract; units of a third of a voxel edge) at the centre
    // voxel of camera2volume[p] (not snapped), 65535 where unreachable or beyond the limit view_host.hpp's travel_limit derives from
    // max_travel_m (<= 0: none).  The field is built from the flood's snapped seed.  PathTo returns the number of voxels of the path from the
    // start to the centre voxel of `target`, start first and target last: voxels3 (int32) and points3 (the voxel centres (v + 0.5) voxel_size in
    // volume coordinates) are optional; 0 when the target is not reached (or beyond the limit, or there is no volume), -1 on bad arguments, -4
    // with nothing written when the path is longer than `capacity`; *needed_out (optional) receives the length whenever a walk ran.
    // NextViewByTravel scores like NextBestView and picks by view_host.hpp's next_view_by_travel with bias3 = travel_bias(bias_m), starting
    // from the current camera; travel3_out (optional) receives the costs.  Its return codes are NextReachableView's.  The field is cached
    // under the flood's key and the limit.  All three return -2 in shard mode and do nothing.
    int Travel(const Matrix4cf *start, float radius_m, int snap_vox, int unknown_blocks, int min_weight, float max_travel_m, int P,
               const Matrix4cf *camera2volume, unsigned char *reachable, unsigned short *clear2, unsigned short *travel3);
    int PathTo(const Matrix4cf *start, float radius_m, int snap_vox, int unknown_blocks, int min_weight, float max_travel_m, const Matrix4cf &target,
               int capacity, int *voxels3, float *points3, int *needed_out);
    int NextViewByTravel(const Matrix4cf *camera2volume, int P, const xs_view_opts *opts, int min_weight, unsigned min_hits, unsigned *out4xP,
                         float radius_m, int snap_vox, int unknown_blocks, float max_travel_m, float bias_m, unsigned short *travel3_out);
    // Frontier clusters and the views proposed from them: where should the camera go next, with no candidates from
    // the caller?  Frontiers labels the frontier voxels of the observation grid at min_weight into clusters within cells of `cell` voxels
    // (include/xslam_amd.h: the contract) and returns the records of the clusters with at least min_size voxels, in ascending label order:
    // records8 (capacity x 8 uint64, optional when capacity is 0) and *count_out, their number.  ProposeViews floods as Reachable does from the
    // current camera (its start snapped within start_snap_vox), takes those clusters, puts views_per_cluster standpoints around each
    // centroid at standoff_m (view_host.hpp: frontier_standpoint), snaps each to the nearest REACHED voxel within snap_vox (dropping those
    // that find none, and a standpoint whose voxel an earlier one of the same cluster already gave), and emits for each survivor the pose
    // at that voxel's centre looking at the centroid (view_host.hpp: look_at; image-down hint: the current camera's y axis) with the
    // cluster's index in Frontiers' list: c2v_out and cluster_out (capacity each) and *count_out.  Mask, labels and records are cached and
    // redone when volume_generation, min_weight or cell differ.  Both return 1 when they ran, 0 without a volume, -1 on bad arguments, -4
    // with the needed count in *count_out (and nothing else written) when capacity is too small, -2 in shard mode, doing nothing.
    int Frontiers(int cell, unsigned long long min_size, int min_weight, int capacity, unsigned long long *records8, int *count_out);
    int ProposeViews(float radius_m, int start_snap_vox, int unknown_blocks, int min_weight, int cell, unsigned long long min_size, int views_per_cluster,
                     float standoff_m, int snap_vox, int capacity, Matrix4cf *c2v_out, int *cluster_out, int *count_out);
    long long RelocalizationIndexVoxels() const { return reloc_.band_key.generation >= 0 ? reloc_.band.count : 0; }   // the index as last built, 0 before any
    // bumped by everything that writes the volume: integrate calls, loadCheckpoint, xs_kf_volume_ptr(kf, 0, .), RebuildSignMap (the band index is rebuilt
    // when its generation differs)
    long long volume_generation = 0;

    // ExportPointCloud (reference :334-372, main.cpp:78-80): zero-crossing points of the TSDF with
    // normals, at most max_buffer of them; a sharded rank exports the planes it owns.
    struct CPointCloud {
        std::vector<float> positions, normals;   // xyz triples
        size_t size() const { return positions.size() / 3; }
        bool exportPly(const std::string &filename) const;  // CPointCloud.cpp:42-67: ascii, x y z nx ny nz
    };
    CPointCloud ExportPointCloud(int max_buffer);
    // ExportMesh (no working counterpart in the reference; xs_extract_mesh in include/xslam_amd.h): the marching-cubes mesh of the
    // TSDF, vertices in ascending edge key, triangles in cube order.  vertex_im (Im of every vertex, raw: divide by csfd_seed_h) only
    // while a CSFD seed is active, else empty.  The orchestrator's sign map lets the kernel skip bricks without a negative voxel.  A
    // sharded rank meshes the cubes of its owned planes [zo0, min(zo1, Z - 1)), reading plane zo1 from its halo: vertices on a shared
    // plane appear in both neighbours' meshes with the same bits and key.
    struct CMesh {
        std::vector<float> positions, normals, vertex_im;   // xyz triples
        std::vector<unsigned long long> edge_keys;
        std::vector<int> triangles;                          // index triples
        bool has_im = false;                                 // a CSFD seed was active: vertex_im holds every vertex's Im
        size_t vertices() const { return edge_keys.size(); }
        size_t faces() const { return triangles.size() / 3; }
        bool exportPly(const std::string &filename) const;   // binary little-endian: x y z nx ny nz [dx dy dz]; list uchar int vertex_indices
    };
    CMesh ExportMesh(int min_weight = 1);

    // volume checkpoint: raw float32 value (+ grad, + int32 weight), X*Y*Z each, dense
    // (the reference's saveTSDFVolume writes value only and res[0]*res[2]*res[2] floats,
    // KinectFusionReconstruction.cpp:438-447)
    void saveTSDFVolume(const std::string &tsdf_filename);
    void saveCheckpoint(const std::string &filename);
    bool loadCheckpoint(const std::string &filename);   // either format: it looks at the magic
    // The brick-sparse checkpoint XSTSDF3 (pack_host.hpp: the format), lossless: the volume is classified and compacted on the
    // device (xs_tsdf_pack_classify, xs_tsdf_pack_gather) and leaves through one pinned staging buffer of checkpoint_staging_words words, chunk by chunk;
    // the host never holds the whole volume.  A rank of a sharded run saves its own planes, as saveCheckpoint does.  stats12 (optional): bricks, the
    // bricks of classes 0 .. 7, payload words, file bytes, gather chunks.  False when the file cannot be written (or there is no volume).
    bool saveCheckpointSparse(const std::string &filename, unsigned long long *stats12);
    // The staging buffer of sparse saves and loads in 32-bit words: 16 Mi words (64 MiB) unless set; at least one brick's 1536.  It bounds the pinned
    // host buffer and the device buffer of a chunk whatever the volume's size (a volume whose payload is smaller allocates only that).
    unsigned long long checkpoint_staging_words = 16ull << 20;
    // ---- the calls that take a second map (kf_second_map.cpp) ----
    // The second map is a SecondMap (merge_host.hpp): a whole volume in device memory in the project's layout (the arrays at plane 0, one pitch)
    // whose resolution and voxel size may differ from this map's; it is only read.  Every operation below refuses it with -1 when
    // second_map_ok does: a null or aliasing array, an axis below the operation's minimum, a voxel size that is not finite and positive, a pitch
    // that holds no row, or a truncation distance different from this map's (stored values are normalised by it, so it is refused, not
    // rescaled).  Every operation returns -2 in shard mode before anything else, then 0 without a volume, then -1 on bad arguments, doing
    // nothing; 1 when it ran.  A T16 is a real 4 x 4, row-major, taking a point of THIS map's volume frame (metres) to the second map's volume
    // frame; an entry of its rows 0 .. 2 that is not finite is a bad argument.  Two ways to obtain the map besides the caller's own pointers:
    // OtherInstanceMap: the volume of another instance of this process, which is synchronised and only read (grad only with_grad: a merge).
    // 1; -1 for null or this instance itself, -2 for a sharded instance, -1 for one without a volume or with arrays of unequal pitch.
    int OtherInstanceMap(KinectFusionReconstruction *other, bool with_grad, xs_host::SecondMap &out) const;
    // OpenCheckpointMap: a checkpoint file of a whole volume in either format (saveCheckpoint, saveCheckpointSparse), read and validated in
    // full before anything is allocated — the format's rules (pack_host.hpp), axes 1 .. 65535, shard_count 1, every plane, this map's
    // truncation distance — then written into a temporary device volume that `out` owns and out.map views; it is freed with `out`.
    // 1; -2 in shard mode, 0 without a volume, -1 for any other file; nothing of this instance is touched.
    struct CheckpointMap {
        DeviceArray2D<float> dv, dg;
        DeviceArray2D<int> dw;
        xs_host::SecondMap map;
    };
    int OpenCheckpointMap(const std::string &filename, CheckpointMap &out);
    // Merging (xs_tsdf_merge in include/xslam_amd.h: the contract).  The map's grad array is needed; axes >= 1.
    // The device is drained, xform12 built by merge_host.hpp's merge_affine, the kernel run with max_integration_weight, and everything
    // derived from the volume follows as after loadCheckpoint: volume_generation, the sign map, the cached planning and relocalisation
    // maps, the previous frame's model maps at the current pose.  Poses, frame_id and the trajectory record are untouched.  *written
    // (optional): the voxels written.  -1 also for min_weight < 1.
    int MergeVolume(const xs_host::SecondMap &src, const double *T16, int min_weight, unsigned long long *written);
    // Taking fused frames out of the volume and fusing them again at corrected poses (kf_reintegrate.cpp; DESIGN.md section 4.27;
    // xs_tsdf_reintegrate in include/xslam_amd.h: the contract).  Entry i: the depth frame depths[i] (u16, device), mode[i] bit 0: take it out at
    // c2v_old[i], bit 1: put it in at c2v_new[i] (camera2volume, seeds included; the pointer of a mode that is not asked for may be null);
    // frame_index (optional) per entry: >= 0 replaces that frame's world2camera_record entry by the pose that gives c2v_new[i] (and world2camera
    // with the last entry), < 0 leaves the record alone.  The device is drained, each distinct image scaled into a buffer of the call's own, the
    // ops issued in entry order (an entry's removal before its addition) in launches of at most XS_REINTEGRATE_MAX_OPS with
    // max_integration_weight and biInterpolate_threshold, and everything derived from the volume follows as after MergeVolume.  frame_id and the
    // number of poses are untouched.  counts4 (optional) = {removed, added, emptied, orphaned} voxels over all ops.  Returns 1, 0 without a
    // volume, -1 on bad arguments (n < 1, a null frame, a mode outside 1 .. 3, a missing pose or one that is not finite, a frame index past
    // the record) with the state unchanged, -2 in shard mode.
    int ReintegrateFrames(int n, const DeviceArray2D<ushort> *depths, const Matrix4cf *c2v_old, const Matrix4cf *c2v_new, const int *mode,
                          const int *frame_index, unsigned long long counts4[4]);
    // Aligning a second map to the volume before it is merged (xs_tsdf_align_terms in include/xslam_amd.h: the
    // contract).  Axes >= 2.  T16xN: N >= 1 starting transforms.
    // The device is drained, the band index of THIS map prepared, and gn_multistart (gn_host.hpp) run over the starts:
    // a pass is one xs_tsdf_align_terms launch per chunk of the starts still active, a step align_host.hpp's align_step.  T16_out receives
    // the start that ended ok — at least six voxels on every pass, the last one included, and a positive definite system on every step —
    // with the highest S = count - sum r^2 (ties: the lower index; S is relocalize_global's truncated-quadratic score for max_residual <= 1: above
    // that a kept voxel can subtract more than it adds); report = {its index, its count, its sum r^2,
    // its mean loss, launches run, starts that ended ok, band voxels in the index, 0}; loss_history (optional) its loss per pass, the
    // last entry the loss it ended at.  Nothing of either map is modified: volume_generation, poses and frame_id stay.  0 also when no start
    // ended ok (T16_out untouched, report[0] = -1); -1 also for N < 1, iterations < 0, min_weight < 1, a damping or max_residual that is not
    // finite, max_residual <= 0.
    int AlignVolume(const xs_host::SecondMap &src, const double *T16xN, int N, int iterations, double damping, int min_weight, float max_residual,
                    double *T16_out, double report[8], std::vector<double> *loss_history);
    // Many transforms against the other map in one band pass each, and alignment with no initial guess (DESIGN.md section 4.24;
    // xs_tsdf_score_transforms in include/xslam_amd.h: the contract).  Axes >= 2.
    // ScoreTransformsVolume: the device is drained, the band index of THIS map prepared, every T16xP + 16 p put through merge_affine and
    // scored over every stride-th band entry in launches of XS_ALIGN_SCORE_MAX_TRANSFORMS; out2xP + 2 p = {sum r^2, count}.  *launches
    // (optional) is advanced by the launches run.  -1 also for AlignVolume's min_weight and max_residual, P < 1, stride < 1.
    // AlignVolumeGlobal: the search of align_search_host.hpp on top of it.  Both maps' band centroids (this map's from its index, the
    // other's from one xs_tsdf_band_build over the source into temporary buffers), round 0 over align_search_free's candidates (or the
    // caller's, when opts gives any), `rounds` rounds of align_search_around about each kept transform with the boxes halved per round,
    // each scored and ranked by align_search_rank, then AlignVolume from the kept transforms over the full band: its winner and its
    // "ended ok" decide.  opts null: the defaults (AlignSearchDefaults).  report12 = {the winner's rank after the last round, its S
    // before refinement on the strided band, its count, sum r^2 and mean loss after refinement, scoring launches, alignment passes,
    // starts that ended ok, band voxels, scored entries per transform, the distance of the other map's centroid from this map's under
    // the winner, 0}.  Nothing of either map is modified.  Returns AlignVolume's codes (0 also when a map has an empty band); -1 also for
    // candidates < 1, keep outside 1 .. 32, rounds < 0, stride < 1, a box that is negative or not finite, a wrong opts->struct_bytes.
    int ScoreTransformsVolume(const xs_host::SecondMap &src, const double *T16xP, int P, int stride, int min_weight, float max_residual, double *out2xP,
                              int *launches = nullptr);
    void AlignSearchDefaults(struct xs_align_search_opts *opts) const;
    int AlignVolumeGlobal(const xs_host::SecondMap &src, const struct xs_align_search_opts *opts, double *T16_out, double report[12]);
    // What differs between this map and a second map, as clusters (xs_tsdf_diff in include/xslam_amd.h: the contract).
    // Axes >= 1.  The output arguments are checked before the volume.  The device is drained, xform12 built by merge_affine, the two
    // masks written by xs_tsdf_diff (only_this: this map has matter where the other is firmly free; only_other: the reverse), each labelled
    // and clustered by the frontier's calls within cells of `cell` voxels (the frontier's rule), and the clusters with count >= min_size
    // (frontier_select) returned in the frontier's record format: this_records8 / other_records8 (capacity x 8 uint64 each; may be null when
    // capacity is 0) with *this_count / *other_count.  counts3 (optional) = {compared, only_this, only_other} voxels; this_dense /
    // other_dense (optional, host, X * Y * Z bytes each) the masks expanded to a byte per voxel.  Every buffer is the call's own: nothing of
    // either map is modified, volume_generation, the sign map, the band index and the planning caches stay.  -1 also for min_weight < 1, lo or
    // hi not finite or lo > hi, a bad cell, a negative capacity, a volume the frontier calls cannot label; -4 when a list does not fit
    // capacity, with both needed counts returned and nothing else written.
    int DiffVolume(const xs_host::SecondMap &src, const double *T16, int min_weight, float lo, float hi, int cell, unsigned long long min_size, int capacity,
                   unsigned long long *this_records8, int *this_count, unsigned long long *other_records8, int *other_count, unsigned long long counts3[3],
                   unsigned char *this_dense, unsigned char *other_dense);

    // Depth, normal and shaded views of a map from poses the caller picks (kf_render.cpp; xs_render_views in
    // include/xslam_amd.h: the contract).  c2v: P camera2volume matrices, 4 x 4 row-major with `stride` floats per entry (1: real, 2: (re, im)
    // pairs, the real part used).  intr4 null: the configuration's level-0 intrinsics; rows, cols 0, 0: its image size.  opts null: the
    // defaults with the cull on.  The outputs are view-major arrays as the contract lays them out, each optional (null: not wanted), on the
    // host, or with on_device != 0 in device memory, where the call leaves them without copying.  The device is drained, the views rendered in
    // launches of XS_RENDER_MAX_VIEWS, and the stream drained again: the outputs are complete on return.
    // RenderViews renders THIS map.  Its brick mask lives in a workspace that is cached under (volume_generation, min_weight) the way the
    // observation grid is, and dropped with it whenever the volume is edited.  RenderSecondMap renders another map (axes >= 1), with a
    // workspace of the call's own whose mask is built per call; nothing of this instance is touched.
    // Both return 1, -2 in shard mode (a ray's first crossing is not additive over the ranks' z-slabs), 0 without a volume, -1 on bad
    // arguments (P < 1, a null c2v, a stride other than 1 or 2, every output null, whatever xs_render_views refuses).
    struct RenderOutputs { float *depth = nullptr; uint16_t *depth_u16 = nullptr; float *normal = nullptr; unsigned char *shade = nullptr; unsigned *counts = nullptr; };
    int RenderViews(const float *c2v, int stride, int P, const float *intr4, int rows, int cols, const xs_render_opts *opts, const RenderOutputs &out,
                    int on_device);
    int RenderSecondMap(const xs_host::SecondMap &src, const float *c2v, int stride, int P, const float *intr4, int rows, int cols, const xs_render_opts *opts,
                        const RenderOutputs &out, int on_device);

    // The map asked at points the caller supplies, and at the pixels of a depth frame (kf_sample.cpp; DESIGN.md section 4.29;
    // xs_tsdf_sample_points and xs_tsdf_sample_depth in include/xslam_amd.h: the contract).  points: n x 3 float32 metres in a frame that T16 (a
    // real 4 x 4, row-major; null: none, the points' bits as they are) takes to the sampled map's volume frame.  The outputs are the contract's
    // arrays, each optional (null: not wanted).  on_device bit 0: the points (the depth image) are device memory, bit 1: the outputs are, and
    // the call leaves them there without copying.  The device is drained, one launch run, and the stream drained again: the outputs are
    // complete on return.  Nothing of either map or of any cache is modified, and no cache is needed.
    // SamplePoints asks THIS map, SampleSecondMap another one (axes >= 1; its grad array only where dvalue is wanted).  FrameResiduals asks
    // this map at the points of a depth frame (u16 millimetres, depth_step bytes per row, 0: packed) seen from camera2volume c2v (4 x 4 with
    // `stride` floats per entry, as RenderViews takes it; intr4 null: the configuration's, rows, cols 0, 0: its image size): value is the
    // frame's signed residual against the map in units of the truncation distance, images [rows][cols] and [3][rows][cols].
    // All return 1, -2 in shard mode (a point's eight corners may straddle two ranks' z-slabs), 0 without a volume, -1 on bad arguments
    // (whatever the kernels' calls refuse, a T16 entry that is not finite, a second map that is not taken).
    struct SampleOutputs { unsigned char *status = nullptr; float *value = nullptr; float *dvalue = nullptr; float *gradient = nullptr; unsigned long long *counts = nullptr; };
    int SamplePoints(const float *points, long long n, const double *T16, int min_weight, const SampleOutputs &out, int on_device);
    int SampleSecondMap(const xs_host::SecondMap &src, const float *points, long long n, const double *T16, int min_weight, const SampleOutputs &out, int on_device);
    int FrameResiduals(const unsigned short *depth, size_t depth_step, const float *c2v, int stride, const float *intr4, int rows, int cols, int min_weight,
                       const SampleOutputs &out, int on_device);

    // A point cloud registered to a map (kf_register.cpp; xs_tsdf_register_terms in include/xslam_amd.h: the contract;
    // register_host.hpp: the host's side).  points: n x 3 float32 metres (on_device bit 0: device memory) in a frame that each of the N starts
    // T16xN (real 4 x 4, row-major) takes to the map's volume frame.  The starts run through gn_multistart: per pass one
    // xs_tsdf_register_terms launch over the starts still active and one fetch of their sums, then register_step on each.  The winner, the
    // "ended ok" rule, iterations = 0 and the return codes are AlignVolume's; report7 = {its index, its count, its sum r^2, its mean loss,
    // launches run, starts that ended ok, n}.  The device is drained before and the stream after.  Nothing of any map or cache is modified.
    // RegisterPoints asks THIS map, RegisterSecondMap another one (axes >= 1, no grad array needed).
    int RegisterPoints(const float *points, long long n, int on_device, const double *T16xN, int N, int iterations, double damping, int min_weight,
                       float max_residual, double *T16_out, double report[7], std::vector<double> *loss_history);
    int RegisterSecondMap(const xs_host::SecondMap &src, const float *points, long long n, int on_device, const double *T16xN, int N, int iterations,
                          double damping, int min_weight, float max_residual, double *T16_out, double report[7], std::vector<double> *loss_history);
    // Many transforms of a cloud scored against a map, and registration with no starting guess (kf_register.cpp; DESIGN.md section 4.32;
    // xs_tsdf_score_points in include/xslam_amd.h: the contract; register_search_host.hpp: the host's side).  src: the map (null: THIS map,
    // through OwnMap, so that all sources take one path).  ScorePointTransforms: every T16xP + 16 p rounded by register_xform12, launches of
    // XS_REGISTER_SCORE_MAX_TRANSFORMS over every stride-th point, {sum r^2, count} per transform.  RegisterPointsGlobal: AlignVolumeGlobal's
    // rounds and ranking with the cloud as "this" (its centroid: points_centroid over the scored points, for a device cloud over a strided
    // copy of them) and the map as "other" (second_map_centroid, for this instance's map too: no cache is touched), then RegisterVolume's
    // loop over all n points from the kept transforms.  opts null: RegisterSearchDefaults.  report12 as AlignVolumeGlobal's with [8] = n,
    // [9] = scored points per transform, [10] = the distance of the map's band centroid from the image of the cloud's under the winner.
    // Both: 1; 0 without a volume (the search also when nothing ended ok or the map has no band voxel, T16_out untouched); -1 on bad
    // arguments (the search also for more than 2^24 scored points: raise the stride); -2 in shard mode.  Nothing is modified.
    int ScorePointTransforms(const xs_host::SecondMap *src, const float *points, long long n, int on_device, const double *T16xP, int P, int stride,
                             int min_weight, float max_residual, double *out2xP);
    void RegisterSearchDefaults(struct xs_register_search_opts *opts) const;
    int RegisterPointsGlobal(const xs_host::SecondMap *src, const float *points, long long n, int on_device, const struct xs_register_search_opts *opts,
                             double *T16_out, double report[12]);

    // A registered point cloud fused into THIS map (kf_fuse.cpp; xs_tsdf_fuse_points_accumulate and
    // xs_tsdf_fuse_points_fold in include/xslam_amd.h: the contract; fuse_host.hpp: the host's side).  points: n x 3 float32 metres (on_device
    // bit 0: device memory) and origin3, the sensor's position, in a frame that T16 (a real 4 x 4, row-major; null: none, the bits as they are)
    // takes to the volume frame; it is rounded by register_xform12's rule, so RegisterPoints' T16_out is fused at the bits it was scored at.
    // Rays shorter than min_range or longer than max_range are dropped; with carve the rays write free space from the sensor on; `weight` is
    // the observation's weight (1 .. max_integration_weight).  The device is drained; the cloud goes through in fuse_host.hpp's runs of at
    // most 2^24 - 1 points, one accumulate and one fold over the whole volume each (a voxel touched by two runs thus receives two
    // observations); then everything derived from the volume follows as after ReintegrateFrames: volume_generation, the sign map, the cached
    // planning and relocalisation maps, the previous frame's model maps.  Poses, frame_id and the trajectory record are untouched.
    // counts5 (optional) = {points used, points dropped, visits, samples outside, voxels written}.  The accumulator (8 bytes per voxel: 1 GiB at
    // 512^3) is allocated and zeroed on first use and kept with the instance; ReleaseFuseScratch frees it, and the next call allocates it again.
    // Returns 1, -2 in shard mode (a ray crosses the ranks' z-slabs), 0 without a volume, -1 on bad arguments (whatever the two calls refuse,
    // a T16 entry that is not finite, a null pointer, arrays of unequal pitch) with the state unchanged.
    int FusePoints(const float *points, long long n, int on_device, const double *T16, const float *origin3, float min_range, float max_range, int carve,
                   int weight, unsigned long long counts5[5]);
    void ReleaseFuseScratch() { fuse_acc_.release(); }

    // counters of the last frame (synchronise the stream)
    long long lastUpdatedVoxels();
    long long lastRaycastHits();
    long long last_frame_counter(int which);
    void synchronize();

private:
    // Per-frame diagnostics counters ([0] updated voxels, [1] raycast hits) live in a device ring, one slot
    // per frame; half of the ring is cleared by one fill every COUNTER_RING / 2 frames instead of one fill
    // (and, when profiling, one download) per frame on the critical stream.
    enum { COUNTER_RING = 512 };
    DeviceArray<unsigned long long> counters_;  // [COUNTER_RING][2]
    long long counter_frame_ = 0;               // frames integrated so far = next slot to use
    unsigned long long *frame_counters() { return counters_.ptr() + 2 * (size_t)(counter_frame_ % COUNTER_RING); }
    unsigned long long *hits_counter_ = nullptr;  // set while IntegrateFrame runs the raycast
    DeviceArray<float> depth_max_;              // [0] largest valid depth of the frame (scale kernel -> integrate far clip)
    DeviceArray<unsigned char> integrate_ws_;  // brick work list of the integrate kernel
    DeviceArray<unsigned char> icp_ws_;        // per-workgroup partial records of the ICP reduction
    DeviceArray<double> icp_sums_;             // 27 complex sums + inlier count
    DeviceArray<unsigned char> icp_pose_;      // device-resident pose of the ICP loop (xs_icp_iterate)
    // What each derived map was built with (generation -1: not built, or no longer to be trusted); a map is rebuilt when its key differs.
    struct BandKey { long long generation = -1; bool operator==(const BandKey &o) const { return generation == o.generation; } };
    struct GridKey { long long generation = -1; int min_weight = 0; bool operator==(const GridKey &o) const { return generation == o.generation && min_weight == o.min_weight; } };
    struct ClearKey { GridKey grid; int R = 0, unknown = -1; bool operator==(const ClearKey &o) const { return grid == o.grid && R == o.R && unknown == o.unknown; } };
    struct ReachKey {   // the field flooded, the body's r2 and the snapped seed
        ClearKey field; int r2 = 0, seed[3] = {-1, -1, -1};
        bool operator==(const ReachKey &o) const { return field == o.field && r2 == o.r2 && seed[0] == o.seed[0] && seed[1] == o.seed[1] && seed[2] == o.seed[2]; }
    };
    struct TravelKey { ReachKey reach; int limit = -1; bool operator==(const TravelKey &o) const { return reach == o.reach && limit == o.limit; } };
    struct FrontierKey { GridKey grid; int cell = -1; bool operator==(const FrontierKey &o) const { return grid == o.grid && cell == o.cell; } };
    // Relocalisation against the map (kf_relocalize.cpp): nothing the frame path touches.
    struct Reloc {
        DeviceArray<double> gn_sums;               // 29 Gauss-Newton sums (+ pad)
        double *gn_publish = nullptr;              // pinned: the 29 sums + sequence word a pass publishes (xs_gn_publish_bytes)
        void *gn_mailbox = nullptr;                // the six-pose mailbox of the passes enqueued ahead (xs_gn_post_poses)
        int gn_mailbox_in_device = 0;
        unsigned long long gn_seq = 0;
        unsigned gn_mail_seq = 0;
        std::vector<std::pair<hipEvent_t, hipEvent_t>> gn_events;
        DeviceArray<float> gn_dense;               // packed copy of the owned planes when the volume is pitched
        DeviceArray<unsigned char> gn_ws;          // reduce workspace of the dense Gauss-Newton kernel
        xs_band_index band = {};                   // band index of the owned planes (RelocalizeGaussNewtonBatch)
        BandKey band_key;                          // the volume_generation it was built at
        DeviceArray<unsigned long long> band_keys;
        DeviceArray<float> band_values;
        DeviceArray<long long> band_segs;
        DeviceArray<unsigned char> band_ws;        // xs_tsdf_band_workspace_bytes(XS_BAND_MAX_FRAMES)
        DeviceArray<double> band_sums;             // XS_BAND_MAX_FRAMES x 29
        std::vector<DeviceArray2D<float>> band_depth;   // the batch's scaled depths, one per frame
        DeviceArray<unsigned char> newton_ws;      // xs_tsdf_pose_hessian_workspace_bytes(XS_BAND_MAX_FRAMES)
        DeviceArray<double> newton_sums;           // XS_BAND_MAX_FRAMES x 29
        DeviceArray<unsigned char> score_ws;       // xs_tsdf_score_poses_workspace_bytes(XS_SCORE_MAX_POSES)
        DeviceArray<double> score_sums;            // XS_SCORE_MAX_POSES x 2
        DeviceArray2D<float> score_depth;          // ScorePoses' scaled depth
        DeviceArray<unsigned char> align_ws;       // xs_tsdf_align_workspace_bytes(XS_ALIGN_MAX_TRANSFORMS)
        DeviceArray<double> align_sums;            // XS_ALIGN_MAX_TRANSFORMS x 29
        DeviceArray<unsigned char> ascore_ws;      // xs_tsdf_score_transforms_workspace_bytes(XS_ALIGN_SCORE_MAX_TRANSFORMS)
        DeviceArray<double> ascore_sums;           // XS_ALIGN_SCORE_MAX_TRANSFORMS x 2
        DeviceArray<unsigned char> register_ws;    // xs_tsdf_register_workspace_bytes(XS_REGISTER_MAX_TRANSFORMS)
        DeviceArray<double> register_sums;         // XS_REGISTER_MAX_TRANSFORMS x 29
        DeviceArray<unsigned char> rscore_ws;      // xs_tsdf_score_points_workspace_bytes(XS_REGISTER_SCORE_MAX_TRANSFORMS)
        DeviceArray<double> rscore_sums;           // XS_REGISTER_SCORE_MAX_TRANSFORMS x 2
    } reloc_;
    const float *GaussNewtonDenseView();       // the owned planes as the dense array the Gauss-Newton kernels index (packed into gn_dense when pitched)
    void BandIndexPrepare();                   // (re)builds the band index when the volume changed since it was built
    size_t BandBatchPrepare(const std::vector<DeviceArray2D<ushort>> &depths);   // index, workspace and scaled depths of a batch
    void GaussNewtonBandLaunch(const int *frames, int n, const Matrix4cf *camera2volume, size_t scaled_step, int rows, int cols, double *raw);
    void PoseHessianLaunch(const int *frames, int n, const Matrix4cf *camera2volume, size_t scaled_step, int rows, int cols, double *raw);
    void ensure_reduce_workspace(DeviceArray<unsigned char> &ws, size_t bytes, const char *what);   // grown when too small, its tickets zeroed only then
    void fetch_sums(double *device_sums, size_t count, double *host_sums);   // all-reduce when sharded, copy to the host, stream drain
    // View planning over the map (kf_planning.cpp): nothing the frame path touches.
    struct Planning {
        DeviceArray<unsigned char> view_grid;      // xs_view_grid_bytes(resolution): the observation grid + a launch's poses
        DeviceArray<unsigned> view_counts;         // XS_VIEW_MAX_POSES x 4
        GridKey grid_key;
        DeviceArray<unsigned char> clear_field;    // xs_clearance_bytes(resolution)
        DeviceArray<unsigned char> clear_ws;       // xs_clearance_workspace_bytes(resolution)
        ClearKey clear_key;
        DeviceArray<unsigned char> reach;          // xs_reach_bytes(resolution): reached and passable words
        DeviceArray<unsigned char> reach_io;       // a query's points and answers
        ReachKey reach_key;
        DeviceArray<unsigned char> travel;         // xs_travel_bytes(resolution): the travel field over the reached words
        DeviceArray<unsigned char> travel_ws;      // xs_travel_workspace_bytes()
        DeviceArray<unsigned char> travel_io;      // a cost query's voxels and answers
        DeviceArray<unsigned char> path_io;        // a path's target, length and voxels
        TravelKey travel_key;
        DeviceArray<unsigned char> frontier_mask;  // xs_frontier_mask_bytes(resolution)
        DeviceArray<unsigned char> frontier_labels;   // xs_frontier_label_bytes(resolution)
        DeviceArray<unsigned char> frontier_ws;    // xs_frontier_workspace_bytes(resolution, capacity of frontier_records_d)
        DeviceArray<unsigned long long> frontier_records_d;   // capacity x 8, and the count behind them
        std::vector<unsigned long long> frontier_records;     // the records of every cluster, on the host
        FrontierKey frontier_key;
        DeviceArray<unsigned char> render_ws;      // xs_render_workspace_bytes(resolution): header, a launch's poses, the brick mask
        GridKey render_key;                        // what the mask in it was built at
    } plan_;
    bool ViewGridPrepare(int min_weight);      // (re)builds the observation grid when the volume or min_weight changed since it was built
    bool ClearancePrepare(int R, int unknown_blocks, int min_weight);   // grid and clearance field in step with the volume and the arguments
    int ReachQuery(const float *points3xN, int n, int over_passable, int snap, unsigned char *reachable, unsigned short *clear2, int *voxel);
    int ReachPrepare(const Matrix4cf *start, float radius_m, int snap_vox, int unknown_blocks, int min_weight);   // plan_.reach in step with the arguments
    bool TravelPrepare(int limit);             // the travel field in step with plan_.reach and the limit
    bool FrontierPrepare(int cell, int min_weight);   // mask, labels and plan_.frontier_records in step with the volume and the arguments
    void reach_forget() { plan_.reach_key = ReachKey{}; plan_.travel_key = TravelKey{}; }   // the flood is not to be trusted, nor what was built over it
    // the volume object was replaced or released: whatever was derived from the old one is rebuilt on next use (the Gauss-Newton mailbox and
    // sequence numbers stay)
    bool takes_second_map(const xs_host::SecondMap &m, int min_axis, bool need_grad) const;   // second_map_ok against this volume
    void drain_device();   // what every call that takes a second map does before its first launch
    void invalidate_derived_maps() { reloc_.band_key = BandKey{}; plan_.grid_key = GridKey{}; plan_.clear_key = ClearKey{}; plan_.frontier_key = FrontierKey{}; plan_.render_key = GridKey{}; reach_forget(); }
    int OwnMap(bool with_grad, xs_host::SecondMap &out) const;   // this volume (it must exist) as a SecondMap, grad only with_grad: 1; -1 for unequal pitches
    // what MergeVolume, FusePoints and ReintegrateFrames do after their write: volume_generation, the sign map, the cached planning and
    // relocalisation maps, the previous frame's model maps at the current pose, and the stream drained (kf_second_map.cpp, beside RebuildSignMap)
    void volume_written_off_path();
    // the views of one volume through xs_render_views, in chunks; `ws` holds a mask built for (res, the options' min_weight) unless the cull is off
    int RenderVolume(const xs_host::SecondMap &vol, void *ws, const float *c2v, int stride, int P, const float *intr4, int rows, int cols, const xs_render_opts &opts,
                     const RenderOutputs &out, int on_device);
    // one xs_tsdf_sample_points launch over a volume described as a SecondMap (this map's included), with the staging of host points and outputs
    int SampleVolume(const xs_host::SecondMap &vol, const float *points, long long n, const double *T16, int min_weight, const SampleOutputs &out, int on_device);
    // the registration loop over a volume described as a SecondMap (this map's included), with the staging of host points
    int RegisterVolume(const xs_host::SecondMap &vol, const float *points, long long n, int on_device, const double *T16xN, int N, int iterations, double damping,
                       int min_weight, float max_residual, double *T16_out, double report[7], std::vector<double> *loss_history);
    // the map a point-cloud call asks: src, or this volume when src is null; -2 in shard mode, 0 without a volume, -1 for a map that is refused
    int register_map_of(const xs_host::SecondMap *src, xs_host::SecondMap &out) const;
    // P transforms (float xform12 each) scored over every stride-th of n device points, in launches of XS_REGISTER_SCORE_MAX_TRANSFORMS
    int ScorePointsVolume(const xs_host::SecondMap &vol, const float *points_dev, long long n, const float *xform12xP, int P, int stride, int min_weight,
                          float max_residual, double *out2xP, int *launches);
    DeviceArray<unsigned long long> fuse_acc_; // FusePoints' accumulator: one word per voxel, zero between calls
    DeviceArray2D<ushort> depth_ingest_d_;     // device copy of a host frame (ProcessFrameHost)
    ushort *ingest_pinned_[2] = {nullptr, nullptr};
    hipEvent_t ingest_done_[2] = {nullptr, nullptr};
    int ingest_seq_ = 0;
    DeviceArray<unsigned char> maps_prev0_block_;  // level-0 model vertex + normal maps, one allocation
    DeviceArray<float> ray_ws_;                // raycast: crossing time per pixel (march kernel -> crossing kernel)
    hipEvent_t tail_done_ = nullptr;           // completion of a frame's model-map pyramid (rides on its dispatch)
    bool tail_recorded_ = false;
    // the second set of per-frame buffers: the announced next frame's maps are built into it (HintNextFrame, SwapMapSets)
    std::vector<MapArr> depths_next_d, vmaps_next_d, nmaps_next_d;
    std::vector<DeviceArray2D<float>> vreal_next_d, nreal_next_d;
    DeviceArray2D<float> depthRawScaled_next_d;
    DeviceArray<float> depth_max_next_;
    // the model-map pyramid inside the raycast launch (YAML raycast_builds_pyramid, default true; single GPU, three levels, sign map on)
    bool raycast_builds_pyramid = true;
    int profile_integrate_every = 4;   // YAML profile_integrate_every: at profiling level 1 the integrate kernel's event pair rides on every n-th frame (IntegrateKernelTimedThisFrame)
    bool IntegrateKernelTimedThisFrame() const;
    bool pyramid_in_raycast_ = false;   // this frame's raycast launch built levels 1 and 2: ModelMapPyramid has nothing to do
    bool PreparePyramidLevels();
    // shard mode, raycast composite by owner-compacted exchange (YAML shard_composite_gather, default true; false = the int32 sum of the maps)
    bool shard_composite_gather = true;
    DeviceArray<unsigned char> gather_buf_, pack_buf_;   // the ranks' packed owned pixels (52 bytes each), all of them / this rank's
    DeviceArray<int> gather_counts_;                     // [rank] = owned pixels with a vertex
    int *gather_counts_host_ = nullptr;                  // pinned
    DeviceArray<unsigned char> depth_tiles_, depth_tiles_next_;   // per-tile depth range of the frame (xs_scale_depth_tiles -> the integrate call's brick classes)
    hipEvent_t surface_done_next_ = nullptr, scale_done_next_ = nullptr;
    bool real_maps_valid_next_ = false, scale_recorded_next_ = false;
    const void *next_hint_ptr_ = nullptr, *next_ready_ptr_ = nullptr;
    size_t next_hint_step_ = 0, next_ready_step_ = 0;
    bool next_ready_ = false;
    DeviceArray<unsigned char> sign_map_;      // raycast: bricks that may hold a negative voxel (single GPU)
    bool sign_map_on() const { return raycast_sign_map; }   // (every rank of a sharded volume keeps one for the planes it stores)
    unsigned char *sign_map_ptr() { return sign_map_on() ? sign_map_.ptr() : nullptr; }
    DeviceArray<int> ray_keys_, ray_min_keys_; // sharded raycast: first-event keys (own, agreed)
    // host-coherent: [0..54] sums + count, [56] completion sequence word, [64..80) pose state of the
    // device-side loop, [128 + 64*n ..) the 55 values of its iteration n
    enum { ICP_LOG_MAX = 62, PINNED_DOUBLES = 128 + 64 * ICP_LOG_MAX };
    double *pinned_sums_ = nullptr;
    unsigned long long *pinned_pairs_ = nullptr;   // XS_ICP_PAIRS_BYTES of host-coherent pinned memory (icp_publish_pairs)
    // the integrate call's header clear / count fold taken off the main stream (SurfaceMeasure, IntegrateFrame)
    bool integrate_split() const;
    void flush_pending_fold(hipStream_t st);
    bool integrate_header_clear_ = false;
    unsigned long long *pending_fold_ = nullptr;
    double *pinned_records_ = nullptr;   // xs_icp_records_bytes() of host-coherent pinned memory (icp_host_fold)
    void *icp_mailbox_ = nullptr;              // pose mailbox of the posted ICP launches (xs_icp_mailbox_alloc)
    long long counters_prepared_for_ = -1;     // the frame whose counter slot has been prepared (ring half cleared)
    unsigned long long *PrepareFrameCounters(hipStream_t st);
    int icp_mailbox_in_device_ = 0;
    unsigned long long icp_seq_ = 0;
public:
    // host wall clock of the ICP loop per pyramid level: from the completion of one iteration's sums to the completion of the next one's
    // (kernel + completion word over PCIe + solve + post) — SURVEY 8(d): "ICP: report us per iteration".  Always on: two clock reads.
    double icp_level_us[4] = {0, 0, 0, 0};          // [3]: the frame's first iteration, which also waits for the stream to drain the previous frame's tail
    long long icp_level_calls[4] = {0, 0, 0, 0};
    // host clock of the frame's tail (xs_kf_tail_host_times), microseconds summed since the last reset: [0] the last ICP sums seen ->
    // IntegrateFrame entered (solve, pose algebra), [1] entered -> the integrate launch call (transforms, cover test), [2] that call itself
    // (xs_integrate_scaled_ex2), [3] its return -> the raycast launch's return
    double tail_host_us[4] = {0, 0, 0, 0};
    long long tail_host_calls = 0;
    std::chrono::steady_clock::time_point t_last_sums_{};
    // test aids: start the launch sequence numbers at `v` (the mailbox is told); make the determinant gate fail at iteration n of the
    // next PoseEstimate (-1: off)
    void DebugSetIcpSequence(unsigned long long v);
    int debug_fail_icp_iteration_ = -1;
    int debug_post_delay_us_[2] = {0, 0};   // test aid: a random host sleep of [min, max] microseconds in front of every pose post (a slow host)
    unsigned debug_post_rng_ = 12345u;
private:
    void AbandonClassifiedList();
    hipStream_t aux_stream_ = nullptr;         // surface measure of frame k+1 runs here, under raycast / pyramid of frame k
    hipEvent_t surface_done_ = nullptr, integrate_done_ = nullptr, scale_done_ = nullptr;
    hipEvent_t integrate_done_now_ = nullptr;   // the event that marks the last integrate call's completion (integrate_done_, or its dispatch's stop event)
    bool integrate_recorded_ = false, scale_recorded_ = false;
    bool profiling_icp_sync = false;           // true: copy + stream synchronise instead of the spin (debug aid)
    int PoseEstimateOnDevice(Matrix3frm Rcurr, Vector3cf tcurr, const Matrix3frm &Rprev_inv, const Vector3cf &tprev, Matrix4cf c2w_curr,
                             int total_iters);
    enum class IcpSink { records, pairs, word };   // where an ICP launch wrote its sums (xs_icp_accumulate_records, XS_ICP_PUBLISH_PAIRS, done_flag)
    xs_wait_result wait_icp_sums(IcpSink sink, unsigned long long seq, int level);
    void icp_normal_equations(const MatS33 &Rcurr, const devComplex3 &tcurr, const MatS33 &Rprev_inv, const devComplex3 &tprev, int level,
                              hostComplexICP *A, hostComplexICP *b, long long *inliers);
    // deferred profiling: one slot of events + one pinned counter record per frame, folded into
    // stage_ms / cum_* only when somebody asks (no per-frame synchronisation)
    enum { PROF_RING = COUNTER_RING / 2 };
    struct ProfSlot { hipEvent_t ev[ST_COUNT][2]; bool used[ST_COUNT]; };
    std::vector<ProfSlot> prof_ring_;
    int prof_pending_ = 0;
    unsigned long long *pinned_counters_ = nullptr;  // [COUNTER_RING][2]: the ring, downloaded when the pending frames are folded
    void stage_begin(int st);
    void stage_end(int st);
    void end_profiled_frame();
public:
    void collect_stage_times();  // synchronises and folds the pending frames
    // level 0: off.  1: the integrate kernel's own event pair + the counters (what bench.py's timed region
    // needs; nothing extra on the stream between kernels).  2: an event pair around every stage as well —
    // each record is a packet the next kernel has to queue behind, so stage times come from their own pass.
    void set_profiling(int level);
    bool profiling_stages = false;
private:
};
