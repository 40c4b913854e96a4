// KinectFusionReconstruction.cpp — per-frame pipeline on one MI355X; follows the control flow
// of XKinectFusion/src/KinectFusionReconstruction.cpp:9-332 (cited per method) over the
// launcher shim.  One stream, no per-frame allocation, synchronisation only where the host
// needs a result (the 6x6 normal equations of each ICP iteration).
#include "KinectFusionReconstruction.h"
#include "newton_host.hpp"
#include "score_host.hpp"
#include "view_host.hpp"
#include <chrono>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

using namespace xs_host;

// The poll budget of every wait for a published result (xs_host_wait).  The wait also watches the stream, so the budget only ends a wait whose
// stream is still busy after this many polls (tens of seconds).
static constexpr long long kWaitPolls = 2000000000LL;
// A wait that ended without its result where none can be spared: one line naming the site and what happened, then exit(-1) (the hipSafeCall /
// check_rc convention).
[[noreturn]] static void wait_fatal(const char *site, const xs_wait_result &w) {
    std::cout << "error::KinectFusionReconstruction, " << site << ": " << xs_wait_str(w.status);
    if (w.status == xs_wait::failed) std::cout << " (" << hipGetErrorString(w.error) << ")";
    std::cout << std::endl;
    exit(-1);
}

KinectFusionReconstruction::KinectFusionReconstruction() {
    depth_width = 0;
    depth_height = 0;
    hipSafeCall(hipStreamCreateWithFlags(&aux_stream_, hipStreamNonBlocking));
    hipSafeCall(hipEventCreateWithFlags(&surface_done_, hipEventDisableTiming));
    hipSafeCall(hipEventCreateWithFlags(&integrate_done_, hipEventDisableTiming));
    hipSafeCall(hipEventCreateWithFlags(&scale_done_, hipEventDisableTiming));
    hipSafeCall(hipEventCreateWithFlags(&tail_done_, hipEventDisableTiming));
    hipSafeCall(hipEventCreateWithFlags(&surface_done_next_, hipEventDisableTiming));
    hipSafeCall(hipEventCreateWithFlags(&scale_done_next_, hipEventDisableTiming));
    hipSafeCall(hipHostMalloc((void **)&pinned_counters_, COUNTER_RING * 2 * sizeof(unsigned long long)));
    hipSafeCall(hipHostMalloc((void **)&pinned_sums_, PINNED_DOUBLES * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped));
    for (int i = 0; i < PINNED_DOUBLES; ++i) pinned_sums_[i] = 0.0;
    hipSafeCall(hipHostMalloc((void **)&pinned_pairs_, XS_ICP_PAIRS_BYTES, hipHostMallocCoherent | hipHostMallocMapped));
    std::memset(pinned_pairs_, 0, XS_ICP_PAIRS_BYTES);
    hipSafeCall(hipHostMalloc((void **)&pinned_records_, xs_icp_records_bytes(), hipHostMallocCoherent | hipHostMallocMapped));
    std::memset(pinned_records_, 0, xs_icp_records_bytes());
}

void KinectFusionReconstruction::SetSharding(int rank, int count, collective_fn fn, void *user) {
    shard_rank = rank; shard_count = count < 1 ? 1 : count; collective = fn; collective_user = user;
}

KinectFusionReconstruction::~KinectFusionReconstruction() {
    if (aux_stream_) { (void)hipStreamSynchronize(aux_stream_); (void)hipStreamDestroy(aux_stream_); }
    if (surface_done_) (void)hipEventDestroy(surface_done_);
    if (integrate_done_) (void)hipEventDestroy(integrate_done_);
    if (tail_done_) (void)hipEventDestroy(tail_done_);
    if (surface_done_next_) (void)hipEventDestroy(surface_done_next_);
    if (scale_done_next_) (void)hipEventDestroy(scale_done_next_);
    if (scale_done_) (void)hipEventDestroy(scale_done_);
    if (pinned_counters_) (void)hipHostFree(pinned_counters_);
    if (gather_counts_host_) (void)hipHostFree(gather_counts_host_);
    if (pinned_sums_) (void)hipHostFree(pinned_sums_);
    if (pinned_pairs_) (void)hipHostFree(pinned_pairs_);
    if (pinned_records_) (void)hipHostFree(pinned_records_);
    if (icp_mailbox_) (void)xs_icp_mailbox_free(icp_mailbox_, icp_mailbox_in_device_);
    if (gn_mailbox_) (void)xs_icp_mailbox_free(gn_mailbox_, gn_mailbox_in_device_);
    if (gn_publish_) (void)hipHostFree(gn_publish_);
    for (int i = 0; i < 2; ++i) {
        if (ingest_pinned_[i]) { (void)hipEventSynchronize(ingest_done_[i]); (void)hipHostFree(ingest_pinned_[i]); (void)hipEventDestroy(ingest_done_[i]); }
    }
    if (tsdf_volume_d_ptr) ReleaseBuffers();
    for (auto &slot : prof_ring_)
        for (int s = 0; s < ST_COUNT; ++s) { (void)hipEventDestroy(slot.ev[s][0]); (void)hipEventDestroy(slot.ev[s][1]); }
}

// reference :9-73
void KinectFusionReconstruction::SetYamlParameters(const FlatYaml &config_) {
    // schedules of the frame's tail that were measured, not adopted and removed: a configuration that asks for one
    // is refused before anything is allocated, not run as the default under another name
    for (const char *key : {"integrate_post_pose", "integrate_post_early", "integrate_classify_beside_icp", "integrate_classify_predicted"})
        if (config_.as<bool>(key, false)) throw std::runtime_error(std::string("retired YAML key (code removed): ") + key);
    if (config_.as<int>("integrate_classify_early", 0) != 0) throw std::runtime_error("retired YAML key (code removed): integrate_classify_early");
    this->config = config_;
    const int resolutionX = config.as<int>("tsdf_size_x");
    const int resolutionY = config.as<int>("tsdf_size_y");
    const int resolutionZ = config.as<int>("tsdf_size_z");
    volume_resolution = Vector3i(resolutionX, resolutionY, resolutionZ);
    voxel_size = config.as<float>("tsdf_voxel_size");
    max_integration_weight = config.as<int>("max_integration_weight");
    const float thres_range = config.as<float>("thres_range");

    csfd_seed_row = config.as<int>("csfd_seed_row", -1);
    csfd_seed_col = config.as<int>("csfd_seed_col", -1);
    csfd_seed_h = config.as<float>("csfd_seed_h", (float)H_);

    world2camera = Matrix4cf::Identity();
    if (csfd_seed_row >= 0 && csfd_seed_row < 4 && csfd_seed_col >= 0 && csfd_seed_col < 4)
        world2camera(csfd_seed_row, csfd_seed_col).imag(csfd_seed_h);  // the line the reference leaves commented (:22)
    world2camera_record.clear();
    world2camera_record.reserve(10000);
    world2camera_record.push_back(world2camera);
    world2volume = Matrix4cf::Identity();
    const float init_x = config.as<float>("init_x"), init_y = config.as<float>("init_y"), init_z = config.as<float>("init_z");
    const float r_x = config.as<float>("r_x") / 180.0f * float(M_PI);
    const float r_y = config.as<float>("r_y") / 180.0f * float(M_PI);
    const float r_z = config.as<float>("r_z") / 180.0f * float(M_PI);
    // Rx * Ry * Rz as rotation matrices (the reference multiplies real AngleAxisf objects, i.e.
    // quaternions; identical for the shipped r_x = r_y = r_z = 0)
    const Matrix3cf rotation = (angle_axis(hostComplex(r_x, 0.f), 0) * angle_axis(hostComplex(r_y, 0.f), 1)) * angle_axis(hostComplex(r_z, 0.f), 2);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) world2volume(i, j) = hostComplex(rotation(i, j).real(), 0.f);
    world2volume(0, 3) = hostComplex(init_x, 0.f);
    world2volume(1, 3) = hostComplex(init_y, 0.f);
    world2volume(2, 3) = hostComplex(init_z, 0.f);

    depth_width = config.as<int>("depth_width");
    depth_height = config.as<int>("depth_height");
    kinect_intrinsic.fx = config.as<float>("fx");
    kinect_intrinsic.fy = config.as<float>("fy");
    kinect_intrinsic.cx = config.as<float>("cx");
    kinect_intrinsic.cy = config.as<float>("cy");

    num_levels = config.as<int>("num_levels");
    if (num_levels > 3) {
        std::cout << "sorry, the max supported multi-level = 3" << "\n";
        num_levels = 3;
    }
    const int iters[] = {5, 4, 3};
    std::copy(iters, iters + num_levels, icp_iterations);

    distThres = config.as<float>("distThres");
    angleThres = float(sin(config.as<float>("angleThres") / 180.f * M_PI));

    biInterpolate_threshold = config.as<float>("biInterpolate_threshold");
    trunc_logistic_k = config.as<float>("trunc_logistic_k", 0.f);

    // planes owned / stored by this rank (whole volume when not sharded)
    zo0 = (int)((long long)resolutionZ * shard_rank / shard_count);
    zo1 = (int)((long long)resolutionZ * (shard_rank + 1) / shard_count);
    zs0 = shard_count > 1 ? std::max(0, zo0 - HALO) : 0;
    zs1 = shard_count > 1 ? std::min(resolutionZ, zo1 + HALO) : resolutionZ;
    icp_solve_on_device = config.as<bool>("icp_solve_on_device", false);
    icp_shard_rows = config.as<bool>("icp_shard_rows", false);
    icp_post_pose = config.as<bool>("icp_post_pose", true);
    icp_real_current_maps = config.as<bool>("icp_real_current_maps", true);
    integrate_classify_ahead = config.as<bool>("integrate_classify_ahead", true);
    integrate_classify_slack = std::max(1.0f, config.as<float>("integrate_classify_slack", 2.0f));
    raycast_sign_map = config.as<bool>("raycast_sign_map", true);
    raycast_sign_map_shift = std::min(6, std::max(0, config.as<int>("raycast_sign_map_shift", 0)));   // 0: the finest usable one
    icp_lookahead = config.as<int>("icp_lookahead", 1);
    icp_host_fold = config.as<bool>("icp_host_fold", false);
    icp_publish_pairs = config.as<bool>("icp_publish_pairs", true);
    force_shard_composite = config.as<bool>("force_shard_composite", false);
    shard_composite_gather = config.as<bool>("shard_composite_gather", true);
    raycast_builds_pyramid = config.as<bool>("raycast_builds_pyramid", true);
    gn_post_pose = config.as<bool>("gn_post_pose", true);
    gn_publish_sharded = config.as<bool>("gn_publish_sharded", true);
    profile_integrate_every = std::max(1, config.as<int>("profile_integrate_every", 4));
    AllocateBuffers();
    tsdf_volume_d_ptr = new TsdfVolume(Vector3i(resolutionX, resolutionY, zs1 - zs0), voxel_size, thres_range);
    if (sign_map_on()) {
        // the sign map of the ray march (include/xslam_amd.h), with the finest bricks the march can use for this camera and volume — or none
        const int finest = xs_raycast_signmap_shift(&kinect_intrinsic.fx, voxel_size, tsdf_volume_d_ptr->getTsdfTruncDist());
        raycast_sign_map_shift = finest ? std::max(raycast_sign_map_shift, finest) : 0;   // (a finer one than the march can use is coarsened)
        const int res[3] = {volume_resolution[0], volume_resolution[1], volume_resolution[2]};
        const size_t bytes = raycast_sign_map_shift ? xs_signmap_bytes(res, raycast_sign_map_shift) : 0;
        if (bytes) { sign_map_.create(bytes); RebuildSignMap(); }   // (from the volume as it is: empty)
        else raycast_sign_map = false;
    }

    use_gtPose = config.as<bool>("flag_use_gtPose", false);
    gt_poses.resize(0);
    frame_id = 0;
    frame_step = config.as<int>("frame_step", 1);
}

// reference :75-106 (the unused newTSDF_volume, jacobi and hessian buffers are not allocated)
void KinectFusionReconstruction::AllocateBuffers() {
    depths_curr_d.resize(num_levels);
    vmaps_curr_d.resize(num_levels);
    nmaps_curr_d.resize(num_levels);
    vmaps_g_prev_d.resize(num_levels);
    nmaps_g_prev_d.resize(num_levels);
    for (int i = 0; i < num_levels; ++i) {
        const int pyr_rows = depth_height >> i, pyr_cols = depth_width >> i;
        depths_curr_d[i].create(pyr_rows, pyr_cols);
        vmaps_curr_d[i].create(pyr_rows * 3, pyr_cols);
        nmaps_curr_d[i].create(pyr_rows * 3, pyr_cols);
        if (i == 0) {
            // the level-0 model maps share one allocation, vertex planes then normal planes: the sharded
            // raycast composite adds both with a single all-reduce
            const size_t step = ((size_t)pyr_cols * sizeof(devComplex) + 255) / 256 * 256;
            maps_prev0_block_.create(2 * (size_t)pyr_rows * 3 * step);
            vmaps_g_prev_d[0] = MapArr(pyr_rows * 3, pyr_cols, maps_prev0_block_.ptr(), step);
            nmaps_g_prev_d[0] = MapArr(pyr_rows * 3, pyr_cols, maps_prev0_block_.ptr() + (size_t)pyr_rows * 3 * step, step);
        } else {
            vmaps_g_prev_d[i].create(pyr_rows * 3, pyr_cols);
            nmaps_g_prev_d[i].create(pyr_rows * 3, pyr_cols);
        }
    }
    depthRawScaled_d.create(depth_height, depth_width);
    // the constant the raycast march divides by, checked once (all 2^32 operands, ~2 ms): it then takes floor(p / voxel_size) with the
    // short division; a constant that fails its check keeps the bracketed reciprocals + divide, same results
    xs_const_div_prepare(voxel_size);
    {
        const int res[3] = {volume_resolution[0], volume_resolution[1], volume_resolution[2]};
        integrate_ws_.create(xs_integrate_workspace_bytes(res, zs1 - zs0));
        icp_ws_.create(xs_icp_workspace_bytes());
        check_rc(xs_icp_workspace_init(icp_ws_.ptr(), current_stream()), "icp workspace");
        if (!icp_mailbox_) check_rc(xs_icp_mailbox_alloc(&icp_mailbox_, &icp_mailbox_in_device_), "icp mailbox");
        icp_sums_.create(64);
        icp_pose_.create(xs_icp_pose_state_bytes());
        ray_ws_.create((size_t)depth_width * depth_height);
        if (shard_count > 1 || force_shard_composite) {
            ray_keys_.create((size_t)depth_width * depth_height);
            ray_min_keys_.create((size_t)depth_width * depth_height);
        }
    }
    counters_.create(2 * COUNTER_RING);
    hipSafeCall(hipMemsetAsync(counters_.ptr(), 0, 2 * COUNTER_RING * sizeof(unsigned long long), current_stream()));
    depth_max_.create(4);
    depth_tiles_.create(xs_depth_tiles_bytes(depth_height, depth_width));
}

// reference :108-123
void KinectFusionReconstruction::ReleaseBuffers() {
    for (int i = 0; i < (int)depths_curr_d.size(); ++i) {
        depths_curr_d[i].release();
        vmaps_curr_d[i].release();
        nmaps_curr_d[i].release();
        vmaps_g_prev_d[i].release();
        nmaps_g_prev_d[i].release();
    }
    maps_prev0_block_.release();
    g_buf.release();
    sum_buf.release();
    depthRawScaled_d.release();
    for (auto &m : vreal_curr_d) m.release();
    for (auto &m : nreal_curr_d) m.release();
    real_maps_valid_ = false;
    delete tsdf_volume_d_ptr;
    tsdf_volume_d_ptr = nullptr;
}

// reference :125-145
int KinectFusionReconstruction::SmoothDepthFrame(MapArr &dst_d, const DeviceArray2D<ushort> &src_d) {
    if (src_d.rows() <= 0 || src_d.cols() <= 0) {
        std::cout << "error: KinectFusionReconstruction::SmoothDepthFrame, input map is empty" << std::endl;
        return 0;
    }
    if (dst_d.rows() != src_d.rows() || dst_d.cols() != src_d.cols()) {
        dst_d.release();
        dst_d.create(src_d.rows(), src_d.cols());
    }
    bilateralFilter(src_d, dst_d);
    return 1;
}

// reference :147-159.  On a failed alignment the reference returns without advancing frame_id,
// and its demo retries the same frame forever; the status is returned
// the same way here and the caller decides.
int KinectFusionReconstruction::ProcessFrame(const DeviceArray2D<ushort> &depth_frame_d) {
    const int align_return = AlignDepthToReconstruction(depth_frame_d, false);
    if (frame_id > 0 && !align_return) {
        std::cout << "Frame align failed!" << std::endl;
        return 0;
    }
    IntegrateFrame(depth_frame_d);
    frame_id += frame_step;
    if (profiling) end_profiled_frame();
    return 1;
}

// Depth ingest (main.cpp:50-58: imread -> upload -> ProcessFrame).  The frame goes through one of two
// host-pinned staging buffers and an asynchronous copy on the second stream — the stream the map
// preparation and the depth scaling run on, so they follow the copy with no host wait, and all of it
// runs under the previous frame's tail.  A caller that decodes straight into IngestBuffer() (or passes
// any pinned pointer) skips the staging copy.
ushort *KinectFusionReconstruction::IngestBuffer() {
    const int slot = ingest_seq_ & 1;
    const size_t bytes = (size_t)depth_width * depth_height * sizeof(ushort);
    if (!ingest_pinned_[slot]) {
        hipSafeCall(hipHostMalloc((void **)&ingest_pinned_[slot], bytes));
        hipSafeCall(hipEventCreateWithFlags(&ingest_done_[slot], hipEventDisableTiming));
    } else
        hipSafeCall(hipEventSynchronize(ingest_done_[slot]));  // the copy out of this slot two frames ago
    return ingest_pinned_[slot];
}
int KinectFusionReconstruction::ProcessFrameHost(const ushort *depth_host) {
    if (depth_width <= 0 || depth_height <= 0 || !depth_host) return 0;
    const size_t row = (size_t)depth_width * sizeof(ushort);
    const ushort *src = depth_host;
    int slot = -1;
    if (depth_host == ingest_pinned_[0] || depth_host == ingest_pinned_[1]) slot = depth_host == ingest_pinned_[0] ? 0 : 1;
    else {
        hipPointerAttribute_t attr;
        const bool pinned = hipPointerGetAttributes(&attr, depth_host) == hipSuccess && attr.type == hipMemoryTypeHost;
        if (!pinned) {
            (void)hipGetLastError();  // a pageable pointer is reported as an error: not one
            ushort *stage = IngestBuffer();
            slot = ingest_seq_ & 1;
            std::memcpy(stage, depth_host, row * depth_height);
            src = stage;
        }
    }
    depth_ingest_d_.create(depth_height, depth_width);
    hipSafeCall(hipMemcpy2DAsync(depth_ingest_d_.ptr(), depth_ingest_d_.step(), src, row, row, depth_height, hipMemcpyHostToDevice, aux_stream_));
    if (slot >= 0) {
        hipSafeCall(hipEventRecord(ingest_done_[slot], aux_stream_));
        if (slot == (ingest_seq_ & 1)) ++ingest_seq_;
    }
    return ProcessFrame(depth_ingest_d_);
}

// reference :161-175
int KinectFusionReconstruction::AlignDepthToReconstruction(const DeviceArray2D<ushort> &depth_frame_d, bool /*use_LM*/) {
    SurfaceMeasure(depth_frame_d);
    struct AtExit { KinectFusionReconstruction *k; ~AtExit() { k->EnqueueAnnouncedFrame(true); } } announced_at_exit{this};   // (whatever path is taken below)
    if (use_gtPose) return 1;
    Matrix4cf c2w_prev = inverse(world2camera_record.back());
    Matrix3frm Rprev = GetRotation(c2w_prev);
    Vector3cf tprev = GetTranslation(c2w_prev);
    Matrix3frm Rprev_inv = inverse(Rprev);
    Matrix3frm Rcurr = Rprev;
    Vector3cf tcurr = tprev;
    return PoseEstimate(Rcurr, tcurr, Rprev_inv, tprev);
}

// reference :177-235
int KinectFusionReconstruction::PoseEstimate(Matrix3frm Rcurr, Vector3cf tcurr, Matrix3frm Rprev_inv, Vector3cf tprev) {
    icp_log.clear();
    list_ready_ = false;
    if (frame_id == 0) return 0;
    Matrix4cf c2w_prev = inverse(world2camera_record.back());
    Matrix4cf c2w_curr = c2w_prev;
    auto &device_Rprev_inv = device_cast<MatS33>(Rprev_inv);
    auto &device_tprev = device_cast<devComplex3>(tprev);
    int total_iters = 0;
    for (int l = 0; l < num_levels; ++l) total_iters += icp_iterations[l];
    const bool icp_local = shard_count == 1 || !icp_shard_rows;  // this rank evaluates every pixel row itself
    if (icp_solve_on_device && icp_local && !profiling_icp_sync && total_iters >= 1 && total_iters <= ICP_LOG_MAX)
        return PoseEstimateOnDevice(Rcurr, tcurr, Rprev_inv, tprev, c2w_curr, total_iters);
    // posted mode: launch n + 1 is enqueued before the host waits for launch n, and gets its pose through
    // the mailbox after the solve (xs_icp_accumulate_posted)
    // (only with the mailbox in device memory behind a large BAR: 512 workgroups polling pinned host memory
    // over PCIe cost more than the launch latency they would save)
    const bool posted = icp_post_pose && icp_local && !profiling_icp_sync && total_iters >= 1 && icp_mailbox_ && icp_mailbox_in_device_;
    std::vector<int> level_of;
    for (int level_index = num_levels - 1; level_index >= 0; --level_index)
        for (int iter = 0; iter < icp_iterations[level_index]; ++iter) level_of.push_back(level_index);
    void *mailbox = icp_mailbox_;
    auto launch_local = [&](int level, const MatS33 *R, const devComplex3 *t, unsigned mail_seq) {
        MapArr &vc = vmaps_curr_d[level], &nc = nmaps_curr_d[level], &vp = vmaps_g_prev_d[level], &np_ = nmaps_g_prev_d[level];
        const Intr k = kinect_intrinsic(level);
        const int rows = vc.rows() / 3, cols = vc.cols();
        unsigned long long *flag = icp_publish_pairs ? XS_ICP_PUBLISH_PAIRS : reinterpret_cast<unsigned long long *>(pinned_sums_ + 56);
        double *sums_out = icp_publish_pairs ? reinterpret_cast<double *>(pinned_pairs_) : pinned_sums_;
        const unsigned long long seq = ++icp_seq_;
        if (icp_host_fold) {
            check_rc(xs_icp_accumulate_records(R ? &R->data[0].x.re : nullptr, R ? &t->x.re : nullptr, R ? nullptr : mailbox, mail_seq, &vc.ptr()->re,
                                               &nc.ptr()->re, &device_Rprev_inv.data[0].x.re, &device_tprev.x.re, &k.fx, &vp.ptr()->re, &np_.ptr()->re,
                                               vc.step(), rows, cols, distThres, angleThres, 0, rows, pinned_records_, seq, current_stream()),
                     "estimateCombined (records)");
            return seq;
        }
        const bool real = real_maps_valid_ && level < (int)vreal_curr_d.size();
        if (R && real)
            check_rc(xs_icp_accumulate_real(&R->data[0].x.re, &t->x.re, &vc.ptr()->re, &nc.ptr()->re, vreal_curr_d[level].ptr(), nreal_curr_d[level].ptr(),
                                            vreal_curr_d[level].step(), &device_Rprev_inv.data[0].x.re, &device_tprev.x.re, &k.fx, &vp.ptr()->re,
                                            &np_.ptr()->re, vc.step(), rows, cols, distThres, angleThres, 0, rows, icp_ws_.ptr(), sums_out, flag, seq,
                                            current_stream()), "estimateCombined");
        else if (R)
            check_rc(xs_icp_accumulate(&R->data[0].x.re, &t->x.re, &vc.ptr()->re, &nc.ptr()->re, &device_Rprev_inv.data[0].x.re,
                                       &device_tprev.x.re, &k.fx, &vp.ptr()->re, &np_.ptr()->re, vc.step(), rows, cols, distThres, angleThres,
                                       0, rows, icp_ws_.ptr(), sums_out, flag, seq, current_stream()), "estimateCombined");
        else if (real)
            check_rc(xs_icp_accumulate_posted_real(mailbox, mail_seq, &vc.ptr()->re, &nc.ptr()->re, vreal_curr_d[level].ptr(), nreal_curr_d[level].ptr(),
                                                   vreal_curr_d[level].step(), &device_Rprev_inv.data[0].x.re, &device_tprev.x.re, &k.fx,
                                                   &vp.ptr()->re, &np_.ptr()->re, vc.step(), rows, cols, distThres, angleThres, 0, rows, icp_ws_.ptr(),
                                                   sums_out, flag, seq, current_stream()), "estimateCombined (posted)");
        else
            check_rc(xs_icp_accumulate_posted(mailbox, mail_seq, &vc.ptr()->re, &nc.ptr()->re, &device_Rprev_inv.data[0].x.re,
                                              &device_tprev.x.re, &k.fx, &vp.ptr()->re, &np_.ptr()->re, vc.step(), rows, cols, distThres,
                                              angleThres, 0, rows, icp_ws_.ptr(), sums_out, flag, seq, current_stream()),
                     "estimateCombined (posted)");
        return seq;
    };
    stage_begin(ST_ICP);
    // posted mode: which launches are in the queue, their completion and mailbox sequence numbers
    std::vector<unsigned long long> seq_of(total_iters, 0);
    std::vector<unsigned> mail_of(total_iters, 0);
    int enqueued = 0;
    auto enqueue_through = [&](int last, MatS33 *R0, devComplex3 *t0) {
        for (; enqueued < total_iters && enqueued <= last; ++enqueued) {
            if (enqueued == 0) { seq_of[0] = launch_local(level_of[0], R0, t0, 0); continue; }
            // the mailbox sequence number is the low word of the launch's completion number; a poller accepts any post at or after its
            // own number in the modulo-2^32 order, so the numbers must stay monotone there: 0 (the mailbox's initial word) is skipped
            // by spending one completion number, not replaced by an out-of-order value
            if ((unsigned)(icp_seq_ + 1) == 0u) ++icp_seq_;
            const unsigned m = (unsigned)(icp_seq_ + 1);
            mail_of[enqueued] = m;
            seq_of[enqueued] = launch_local(level_of[enqueued], nullptr, nullptr, m);
        }
    };
    auto t_prev = std::chrono::steady_clock::now();
    for (int n = 0; n < total_iters; ++n) {
        {
            const int level_index = level_of[n];
            auto &device_Rcurr = device_cast<MatS33>(Rcurr);
            auto &device_tcurr = device_cast<devComplex3>(tcurr);
            hostComplexICP A[36], b[6];
            long long inliers = 0;
            bool next_enqueued = false;
            unsigned next_mail_seq = 0, last_mail_seq = 0;
            if (posted) {
                // launches n + 1 .. n + icp_lookahead are in the queue before the host waits for launch n: each becomes resident the
                // moment its predecessor retires and polls the mailbox for its own sequence number.  (Default 1.  A kernel trace
                // shows ~4 us between the 8 us launches of levels 2 and 1, but keeping 2, 3, 5 or all 11 launches ahead — the
                // frame's first ones are enqueued while the GPU still works on the previous frame's raycast — measured the same
                // 2 900-2 950 frames/s as one: those gaps are the profiler's.)
                enqueue_through(n + std::max(1, icp_lookahead), &device_Rcurr, &device_tcurr);
                EnqueueAnnouncedFrame(false);   // (one stage of the announced next frame's map preparation per iteration, behind this frame's ICP launches)
                // the last launch is in the queue: the integrate call's brick classification goes in behind it, for the pose that
                // launch starts from — the final one differs by the last level-0 update, which IntegrateFrame checks is covered
                if (n == total_iters - 1 && !list_ready_ && integrate_classify_ahead && integrate_split())
                    ClassifyAhead(Rcurr, tcurr);
                const unsigned long long seq = seq_of[n];
                if (n + 1 < total_iters) {
                    next_mail_seq = mail_of[n + 1];
                    last_mail_seq = mail_of[enqueued - 1];   // an abandon command with this number releases every launch in the queue
                    next_enqueued = true;
                }
                auto launch_gave_up = [&](xs_wait status) {   // never expected: the launch gave up on its pose, or never published
                    if (next_enqueued) xs_icp_post_pose(mailbox, nullptr, nullptr, last_mail_seq, 1);
                    hipSafeCall(hipStreamSynchronize(current_stream()));
                    check_rc(xs_icp_workspace_init(icp_ws_.ptr(), current_stream()), "icp workspace");
                    stage_end(ST_ICP);
                    AbandonClassifiedList();
                    std::cout << "error::KinectFusionReconstruction, ICP launch: " << xs_wait_str(status) << std::endl;
                    return 0;
                };
                const xs_wait_result w = wait_icp_sums(icp_host_fold ? IcpSink::records : icp_publish_pairs ? IcpSink::pairs : IcpSink::word, seq, level_index);
                if (w.status == xs_wait::failed) wait_fatal("ICP launch", w);
                if (w.status != xs_wait::published) return launch_gave_up(w.status);
                xs_icp_unpack(pinned_sums_, reinterpret_cast<double *>(A), reinterpret_cast<double *>(b));
                inliers = (long long)pinned_sums_[54];
            } else
                icp_normal_equations(device_Rcurr, device_tcurr, device_Rprev_inv, device_tprev, level_index, A, b, &inliers);
            if (level_index < 3) {   // this iteration's sums are in: the period since the previous iteration's were
                const auto t_now = std::chrono::steady_clock::now();
                const int slot = n == 0 ? 3 : level_index;   // (the frame's first iteration also waits for the previous frame's tail and the map preparation)
                icp_level_us[slot] += std::chrono::duration<double, std::micro>(t_now - t_prev).count();
                ++icp_level_calls[slot];
                t_prev = t_now;
                t_last_sums_ = t_now;
            }
            // The solve and the post come first: the enqueued launch is waiting for them.
            hostComplexICP sol[6];
            llt_solve6(A, b, sol);
            hostComplex result[6];
            for (int i = 0; i < 6; ++i) result[i] = hostComplex((float)sol[i].real(), (float)sol[i].imag());
            const hostComplex alpha = result[0], beta = result[1], gamma = result[2];
            const Matrix3cf Rinc = (angle_axis(gamma, 2) * angle_axis(beta, 1)) * angle_axis(alpha, 0);
            Vector3cf tinc; tinc[0] = result[3]; tinc[1] = result[4]; tinc[2] = result[5];
            const Vector3cf rt = Rinc * tcurr;
            Vector3cf tnext;
            for (int i = 0; i < 3; ++i) tnext[i] = rt[i] + tinc[i];
            const Matrix3frm Rnext = Rinc * Rcurr;
            // the reference's determinant gate (:203-210): a 6x6 LU in double, a fraction of a microsecond, so it is taken
            // before the post — the enqueued launch of a singular system is told to leave (cmd 1) instead of running
            // unobserved on maps the next frame's preparation may already be rewriting
            const double det = real_determinant6(A);
            bool singular = fabs(det) < 1e-15 || std::isnan(det);
            if (debug_fail_icp_iteration_ == n) { singular = true; debug_fail_icp_iteration_ = -1; }   // (test aid)
            if (debug_post_delay_us_[1] > 0) {   // (test aid: a slow host — the enqueued launch keeps polling)
                debug_post_rng_ = debug_post_rng_ * 1664525u + 1013904223u;
                const int span = debug_post_delay_us_[1] - debug_post_delay_us_[0] + 1;
                const int us = debug_post_delay_us_[0] + (int)((debug_post_rng_ >> 8) % (unsigned)(span > 0 ? span : 1));
                const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(us);
                while (std::chrono::steady_clock::now() < until) {}
            }
            if (next_enqueued) {
                if (singular) xs_icp_post_pose(mailbox, nullptr, nullptr, last_mail_seq, 1);
                else xs_icp_post_pose(mailbox, &device_cast<MatS33>(Rnext).data[0].x.re, &device_cast<devComplex3>(tnext).x.re, next_mail_seq, 0);
            }
            {   // diagnostics: re-pack the 27 sums in launch order
                int shift = 0;
                for (int i = 0; i < 6; ++i)
                    for (int j = i; j < 7; ++j, ++shift) {
                        const hostComplexICP v = (j == 6) ? b[i] : A[i * 6 + j];
                        icp_log.push_back(v.real());
                        icp_log.push_back(v.imag());
                    }
                icp_log.push_back((double)inliers);
            }
            if (singular) {
                if (std::isnan(det)) std::cout << "qnan det" << std::endl;
                else std::cout << "eps det: " << fabs(det) << std::endl;
                stage_end(ST_ICP);
                AbandonClassifiedList();
                return 0;
            }
            tcurr = tnext;
            Rcurr = Rnext;
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) c2w_curr(i, j) = Rcurr(i, j);
                c2w_curr(i, 3) = tcurr[i];
            }
            c2w_curr(3, 3) = hostComplex(1.f, 0.f);
        }
    }
    stage_end(ST_ICP);
    world2camera = inverse(c2w_curr);
    world2camera_record.push_back(world2camera);
    return 1;
}

// The same loop with the pose update on the device (xs_icp_iterate): the launches of all levels and
// iterations queue back to back, each leaving the pose for the next in device memory, and the host
// waits once per frame for the final pose instead of once per iteration for the 27 sums.
int KinectFusionReconstruction::PoseEstimateOnDevice(Matrix3frm Rcurr, Vector3cf tcurr, const Matrix3frm &Rprev_inv, const Vector3cf &tprev,
                                                     Matrix4cf c2w_curr, int total_iters) {
    struct PoseState { float R[18]; float t[6]; int status; int iters; double det; double pad[2]; };
    static_assert(sizeof(PoseState) == 128, "pose state layout (xs_icp_iterate)");
    PoseState *pose_host = reinterpret_cast<PoseState *>(pinned_sums_ + 64);
    double *log_host = pinned_sums_ + 128;
    const unsigned long long seq = ++icp_seq_;
    hipStream_t st = current_stream();
    stage_begin(ST_ICP);
    int n = 0;
    for (int level_index = num_levels - 1; level_index >= 0; --level_index) {
        MapArr &vc = vmaps_curr_d[level_index], &nc = nmaps_curr_d[level_index];
        MapArr &vp = vmaps_g_prev_d[level_index], &np_ = nmaps_g_prev_d[level_index];
        const Intr k = kinect_intrinsic(level_index);
        const int rows = vc.rows() / 3, cols = vc.cols();
        for (int iter = 0; iter < icp_iterations[level_index]; ++iter, ++n) {
            const bool first = (n == 0), last = (n == total_iters - 1);
            check_rc(xs_icp_iterate(first ? Rcurr.data() : nullptr, first ? tcurr.data() : nullptr, &vc.ptr()->re, &nc.ptr()->re,
                                    Rprev_inv.data(), tprev.data(), &k.fx, &vp.ptr()->re, &np_.ptr()->re, vc.step(), rows, cols, distThres,
                                    angleThres, icp_ws_.ptr(), icp_sums_.ptr(), log_host + 64 * n, icp_pose_.ptr(), pose_host,
                                    last ? reinterpret_cast<unsigned long long *>(pinned_sums_ + 56) : nullptr, seq, st),
                     "xs_icp_iterate");
        }
    }
    const xs_wait_result w = xs_host_wait([&] { return xs_poll_word(pinned_sums_ + 56, seq); }, kWaitPolls, st);
    if (w.status != xs_wait::published) wait_fatal("ICP loop on the device", w);
    stage_end(ST_ICP);
    const PoseState ps = *pose_host;
    for (int i = 0; i < ps.iters && i < total_iters; ++i)
        for (int j = 0; j < 55; ++j) icp_log.push_back(log_host[64 * i + j]);
    if (ps.status != 0) {
        if (ps.status == 2) std::cout << "qnan det" << std::endl;
        else std::cout << "eps det: " << fabs(ps.det) << std::endl;
        return 0;
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) c2w_curr(i, j) = hostComplex(ps.R[(i * 3 + j) * 2], ps.R[(i * 3 + j) * 2 + 1]);
        c2w_curr(i, 3) = hostComplex(ps.t[2 * i], ps.t[2 * i + 1]);
    }
    c2w_curr(3, 3) = hostComplex(1.f, 0.f);
    world2camera = inverse(c2w_curr);
    world2camera_record.push_back(world2camera);
    return 1;
}

// The 55 sums of ICP launch `seq` over all rows of `level`, from the sink the launch wrote (its records, added in index order; its 55 pairs; or
// the sums behind the completion word), into pinned_sums_[0..54].  One wait on the current stream.
xs_wait_result KinectFusionReconstruction::wait_icp_sums(IcpSink sink, unsigned long long seq, int level) {
    const hipStream_t st = current_stream();
    if (sink == IcpSink::records) {
        const int count = xs_icp_records_count(vmaps_curr_d[level].cols(), 0, vmaps_curr_d[level].rows() / 3);
        int next = 0;
        const xs_wait_result w = xs_host_wait([&] { return xs_poll_records(pinned_records_, count, seq, &next); }, kWaitPolls, st);
        if (w.status == xs_wait::published) xs_fold_records(pinned_records_, count, pinned_sums_);
        return w;
    }
    if (sink == IcpSink::pairs) {
        const xs_wait_result w = xs_host_wait([&] { return xs_poll_pairs(pinned_pairs_, seq); }, kWaitPolls, st);
        if (w.status == xs_wait::published) xs_read_pairs(pinned_pairs_, pinned_sums_);
        return w;
    }
    return xs_host_wait([&] { return xs_poll_word(pinned_sums_ + 56, seq); }, kWaitPolls, st);
}

// estimateCombined (ICP.cu:365-429) on this rank's pixel rows, summed over ranks, then unpacked
void KinectFusionReconstruction::icp_normal_equations(const MatS33 &Rcurr, const devComplex3 &tcurr, const MatS33 &Rprev_inv,
                                                      const devComplex3 &tprev, int level, hostComplexICP *A, hostComplexICP *b,
                                                      long long *inliers) {
    MapArr &vc = vmaps_curr_d[level], &nc = nmaps_curr_d[level], &vp = vmaps_g_prev_d[level], &np_ = nmaps_g_prev_d[level];
    const Intr k = kinect_intrinsic(level);
    const int rows = vc.rows() / 3, cols = vc.cols();
    const bool icp_local = shard_count == 1 || !icp_shard_rows;
    const int y0 = icp_local ? 0 : (int)((long long)rows * shard_rank / shard_count);
    const int y1 = icp_local ? rows : (int)((long long)rows * (shard_rank + 1) / shard_count);
    hipStream_t st = current_stream();
    if (icp_local && !profiling_icp_sync) {
        // single GPU: the kernel writes the sums straight into host-coherent pinned memory and then
        // publishes a sequence number; the host spins on it (no copy kernel, no stream synchronise)
        const unsigned long long seq = ++icp_seq_;
        if (icp_host_fold)
            check_rc(xs_icp_accumulate_records(&Rcurr.data[0].x.re, &tcurr.x.re, nullptr, 0, &vc.ptr()->re, &nc.ptr()->re, &Rprev_inv.data[0].x.re,
                                               &tprev.x.re, &k.fx, &vp.ptr()->re, &np_.ptr()->re, vc.step(), rows, cols, distThres, angleThres, y0, y1,
                                               pinned_records_, seq, st), "estimateCombined (records)");
        else
            check_rc(xs_icp_accumulate(&Rcurr.data[0].x.re, &tcurr.x.re, &vc.ptr()->re, &nc.ptr()->re, &Rprev_inv.data[0].x.re, &tprev.x.re,
                                       &k.fx, &vp.ptr()->re, &np_.ptr()->re, vc.step(), rows, cols, distThres, angleThres, y0, y1,
                                       icp_ws_.ptr(), pinned_sums_, reinterpret_cast<unsigned long long *>(pinned_sums_ + 56), seq, st),
                     "estimateCombined");
        const xs_wait_result w = wait_icp_sums(icp_host_fold ? IcpSink::records : IcpSink::word, seq, level);
        if (w.status != xs_wait::published) wait_fatal("estimateCombined", w);
    } else {
        check_rc(xs_icp_accumulate(&Rcurr.data[0].x.re, &tcurr.x.re, &vc.ptr()->re, &nc.ptr()->re, &Rprev_inv.data[0].x.re, &tprev.x.re,
                                   &k.fx, &vp.ptr()->re, &np_.ptr()->re, vc.step(), rows, cols, distThres, angleThres, y0, y1,
                                   icp_ws_.ptr(), icp_sums_.ptr(), nullptr, 0, st), "estimateCombined");
        if (!icp_local && collective) collective(collective_user, 0, icp_sums_.ptr(), 55);  // the 440-byte all-reduce
        hipSafeCall(hipMemcpyAsync(pinned_sums_, icp_sums_.ptr(), 55 * sizeof(double), hipMemcpyDeviceToHost, st));
        hipSafeCall(hipStreamSynchronize(st));
    }
    xs_icp_unpack(pinned_sums_, reinterpret_cast<double *>(A), reinterpret_cast<double *>(b));
    if (inliers) *inliers = (long long)pinned_sums_[54];
}

// Profiling level 1 attaches a start / stop event pair to the integrate kernel's dispatch (the roofline's kernel_ms).  The START event costs the
// launch call 4.8 us of host time (9.1 us against 4.2 with the completion event alone: bench.py's tail_host_us), on the critical path
// between the last ICP reduction and the raycast — 3 % of the frame rate it is there to annotate.  So the pair rides on every
// profile_integrate_every-th frame only (default 4; level 2, the per-stage pass, times every frame): the mean kernel time is that of the
// sampled launches.
bool KinectFusionReconstruction::IntegrateKernelTimedThisFrame() const {
    return profiling && (profiling_stages || profile_integrate_every <= 1 || counter_frame_ % profile_integrate_every == 0);
}
// one integrate call per frame (the volume is not sharded): its header clear and count fold can leave the main stream
bool KinectFusionReconstruction::integrate_split() const { return zs0 == zo0 && zs1 == zo1 && integrate_ws_.ptr() != nullptr; }
// the voxel count of the last integrate call still sits in the workspace header: fold it into its frame's counter slot
// (on `st`, which must be ordered behind that call: the main stream, or the auxiliary one after integrate_done_)
void KinectFusionReconstruction::flush_pending_fold(hipStream_t st) {
    if (!pending_fold_) return;
    check_rc(xs_integrate_fold_counts(integrate_ws_.ptr(), pending_fold_, st), "integrate count");
    pending_fold_ = nullptr;
}

// reference :237-278
// xs_integrate_classify for the camera pose (Rcurr, tcurr) = camera-to-world, on the main stream (behind the ICP launches)
void KinectFusionReconstruction::ClassifyAhead(const Matrix3frm &Rcurr, const Vector3cf &tcurr) {
    Matrix4cf c2w;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) c2w(i, j) = hostComplex(i == j ? 1.f : 0.f, 0.f);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) c2w(i, j) = Rcurr(i, j);
        c2w(i, 3) = tcurr[i];
    }
    // the volume-to-camera pose the list is classified for
    Matrix4cf v2c = inverse(world2volume * c2w);
    Matrix3frm Rv2c = GetRotation(v2c);
    Vector3cf tv2c = GetTranslation(v2c);
    std::memcpy(list_Rv2c_, &device_cast<MatS33>(Rv2c).data[0].x.re, sizeof(list_Rv2c_));
    std::memcpy(list_tv2c_, &device_cast<devComplex3>(tv2c).x.re, sizeof(list_tv2c_));
    hipStream_t st = current_stream();
    // the scaled depth's maximum and the cleared header come from the auxiliary stream
    if (scale_recorded_ && hipEventQuery(scale_done_) != hipSuccess) hipSafeCall(hipStreamWaitEvent(st, scale_done_, 0));
    const int res[3] = {volume_resolution.x(), volume_resolution.y(), volume_resolution.z()};
    xs_integrate_opts o = {};
    o.struct_bytes = sizeof(o);
    o.flags = integrate_header_clear_ ? XS_INTEGRATE_HEADER_IS_CLEAR : 0u;
    o.depth_tiles = depth_tiles_.ptr();   // the boxes' classes are decided here too, with the slack's pads (the integrate call checks its pose against them)
    check_rc(xs_integrate_classify_ex(depth_height, depth_width, &kinect_intrinsic.fx, res, voxel_size, list_Rv2c_, list_tv2c_,
                                      tsdf_volume_d_ptr->getTsdfTruncDist(), zo0, zo1, depth_max_.ptr(), integrate_ws_.ptr(), integrate_classify_slack,
                                      &o, st), "integrate classification");
    list_ready_ = true;
}

// this frame's counter slot; entering a half of the ring clears that half (its frames were folded or abandoned at least COUNTER_RING / 2
// frames ago) — once per frame, whichever of the two integrate paths comes first
unsigned long long *KinectFusionReconstruction::PrepareFrameCounters(hipStream_t st) {
    if (counters_prepared_for_ != counter_frame_) {
        counters_prepared_for_ = counter_frame_;
        if (counter_frame_ % (COUNTER_RING / 2) == 0 && counter_frame_ > 0)
            hipSafeCall(hipMemsetAsync(frame_counters(), 0, (COUNTER_RING / 2) * 2 * sizeof(unsigned long long), st));
    }
    return frame_counters();
}

// A frame whose alignment fails after ClassifyAhead has run never reaches IntegrateFrame: the classification kernel is still in the main
// stream, has filled the workspace header, and reads the frame's depth maximum — while the retried frame's SurfaceMeasure clears that header
// and rewrites the maximum on the auxiliary stream, ordered only behind the previous frame's integrate kernel.  So the failure path (rare: a
// singular system, a launch that timed out) drains the main stream, clears the header there and forgets the list.
void KinectFusionReconstruction::AbandonClassifiedList() {
    if (!list_ready_) return;
    list_ready_ = false;
    check_rc(xs_integrate_workspace_clear(integrate_ws_.ptr(), current_stream()), "integrate workspace");
    hipSafeCall(hipStreamSynchronize(current_stream()));
    integrate_header_clear_ = true;
}
void KinectFusionReconstruction::DebugSetIcpSequence(unsigned long long v) {
    synchronize();
    icp_seq_ = v;
    // the mailbox holds the number of the last post: bring it up to date, or a launch numbered just above v would take the stale, smaller
    // number for a later one after the 2^32 wrap (an abandon command nobody is waiting for)
    if (icp_mailbox_ && (unsigned)v != 0u) xs_icp_post_pose(icp_mailbox_, nullptr, nullptr, (unsigned)v, 1);
}

int KinectFusionReconstruction::IntegrateFrame(const DeviceArray2D<ushort> &depth_frame_d) {
    ++volume_generation;   // (the relocalisation index of this volume is stale from here on)
    if (use_gtPose) {
        Matrix4cf c2w = gt_poses[frame_id];
        world2camera = inverse(c2w);
        world2camera_record.back() = world2camera;
    }
    Matrix4cf c2w = inverse(world2camera_record.back());
    Matrix4cf c2v = world2volume * c2w;
    Matrix4cf v2c = inverse(c2v);
    Vector3cf tc2v = GetTranslation(c2v);
    auto &device_tc2v = device_cast<devComplex3>(tc2v);
    Matrix3frm Rv2c = GetRotation(v2c);
    auto &device_Rv2c = device_cast<MatS33>(Rv2c);
    Vector3cf tv2c = GetTranslation(v2c);
    auto &device_tv2c = device_cast<devComplex3>(tv2c);
    (void)device_tc2v;

    int3 volume_res;
    volume_res.x = volume_resolution.x();
    volume_res.y = volume_resolution.y();
    volume_res.z = volume_resolution.z();
    hipStream_t st = current_stream();
    const auto t_enter = std::chrono::steady_clock::now();
    auto t_call = t_enter, t_back = t_enter;
    unsigned long long *counters = PrepareFrameCounters(st);
    // the depth scaling ran on the auxiliary stream behind the map preparation
    // (a wait is a packet the next kernel queues behind: none is enqueued for an event that has already completed — the
    // scaling finished under the ICP loop long ago)
    if (scale_recorded_ && hipEventQuery(scale_done_) != hipSuccess) hipSafeCall(hipStreamWaitEvent(st, scale_done_, 0));
    float *depth_max_dev = depth_max_.ptr();  // filled with the scaled depth by SurfaceMeasure, on the auxiliary stream
    // integrateTsdfVolume (TsdfFusion.cu:173-201), its two launches timed separately
    const int res[3] = {volume_res.x, volume_res.y, volume_res.z};
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value(), grad = tsdf_volume_d_ptr->grad();
    DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    // ST_INTEGRATE brackets the integrate kernel proper of the owned planes (the events are recorded
    // inside xs_integrate_scaled, after the brick classification): the figure the roofline uses
    // The integrate kernel's completion is what the auxiliary stream waits for before it touches the scaled depth / the
    // workspace header again.  With one integrate call per frame that completion event rides on the kernel's own dispatch
    // (its stop event — the profiling pair's when profiling) instead of a marker packet behind it, which the raycast
    // launch would queue behind (~5 us of every frame).
    hipEvent_t integrate_stop = integrate_done_;
    xs_integrate_opts o = {};   // everything the integrate calls below take besides their arguments proper (no per-thread setters)
    o.struct_bytes = sizeof(o);
    if (IntegrateKernelTimedThisFrame()) {
        integrate_stop = prof_ring_[prof_pending_].ev[ST_INTEGRATE][1];
        o.start_event = prof_ring_[prof_pending_].ev[ST_INTEGRATE][0]; o.stop_event = integrate_stop;
        prof_ring_[prof_pending_].used[ST_INTEGRATE] = true;
    } else if (integrate_split())
        o.stop_event = integrate_stop;
    o.signmap = sign_map_ptr();   // (a rank of a sharded volume: the owned planes and both halo bands mark it)
    o.depth_tiles = depth_tiles_.ptr();
    // owned planes (counted), then the two halo bands every neighbour also integrates: the
    // update is per voxel and deterministic, so a halo voxel carries the owner's exact bits
    const int zr[3][2] = {{zo0, zo1}, {zs0, zo0}, {zo1, zs1}};
    for (int i = 0; i < 3; ++i) {
        const int za = zr[i][0], zb = zr[i][1];
        if (zb <= za) continue;
        const size_t off = (size_t)(za - zs0) * res[1];
        // header cleared and count folded on the auxiliary stream (SurfaceMeasure) when there is one call per frame
        const bool split = integrate_split() && integrate_header_clear_ && i == 0;
        unsigned list_flag = 0;
        if (i == 0 && list_ready_) {
            list_ready_ = false;
            const int covers = xs_integrate_list_covers(depth_frame_d.rows(), depth_frame_d.cols(), &kinect_intrinsic.fx, res, voxel_size, list_Rv2c_,
                                                        list_tv2c_, integrate_classify_slack, &device_Rv2c.data[0].x.re, &device_tv2c.x.re);
            ++list_cover_counts_[covers & 3];
            if (covers)   // (bit 1 clear: the list holds but the boxes' classes were padded for a nearer pose — they are decided again, the list stays)
                list_flag = XS_INTEGRATE_LIST_IS_READY | XS_INTEGRATE_HEADER_IS_CLEAR | ((covers & 2) ? 0u : XS_INTEGRATE_RECLASSIFY_BOXES);
            else   // the last update moved the frustum further than the widened list allows for (never seen): start over
                check_rc(xs_integrate_workspace_clear(integrate_ws_.ptr(), st), "integrate workspace");
        }
        o.flags = (split ? (XS_INTEGRATE_HEADER_IS_CLEAR | XS_INTEGRATE_NO_FOLD) : 0u) | list_flag;
        if (i == 0) t_call = std::chrono::steady_clock::now();
        check_rc(xs_integrate_scaled_ex2(depthRawScaled_d.ptr(), depthRawScaled_d.step(), depth_frame_d.rows(), depth_frame_d.cols(),
                                         &kinect_intrinsic.fx, max_integration_weight, res, voxel_size, &device_Rv2c.data[0].x.re,
                                         &device_tv2c.x.re, tsdf_volume_d_ptr->getTsdfTruncDist(), value.ptr((int)off), weight.ptr((int)off),
                                         grad.ptr((int)off), value.step(), biInterpolate_threshold, za, zb, i == 0 ? counters : nullptr,
                                         depth_max_dev, integrate_ws_.ptr(), &o, st),
                 "integrateTsdfVolume");
        if (split) { integrate_header_clear_ = false; pending_fold_ = counters; }
        if (i == 0) { t_back = std::chrono::steady_clock::now(); o.start_event = nullptr; o.stop_event = nullptr; }   // (the event pair rides on the owned planes' launch only)
    }

    if (integrate_split()) integrate_done_now_ = integrate_stop;          // attached to the dispatch above
    else { hipSafeCall(hipEventRecord(integrate_done_, st)); integrate_done_now_ = integrate_done_; }   // after the halo calls too
    integrate_recorded_ = true;
    stage_begin(ST_RAYCAST);
    hits_counter_ = counters + 1;
    CalculatePointCloud(vmaps_g_prev_d[0], nmaps_g_prev_d[0]);
    hits_counter_ = nullptr;
    if (frame_id > 0 && !use_gtPose) {
        const auto t_ray = std::chrono::steady_clock::now();
        auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        tail_host_us[0] += us(t_last_sums_, t_enter); tail_host_us[1] += us(t_enter, t_call); tail_host_us[2] += us(t_call, t_back); tail_host_us[3] += us(t_back, t_ray);
        ++tail_host_calls;
    }
    stage_end(ST_RAYCAST);
    stage_begin(ST_RESIZE);
    ModelMapPyramid();
    stage_end(ST_RESIZE);
    ++counter_frame_;
    return 1;
}

// reference :272-277: resizeVMap / resizeNMap per level.  With three levels both halvings of both maps
// are one launch (xs_resize_pyramid: same values).
// levels 1 and 2 of the model maps allocated, and all three levels' vertex / normal maps of equal pitch (what the one-launch pyramid — its
// own kernel or the raycast's epilogue — wants): false = the per-level launches
bool KinectFusionReconstruction::PreparePyramidLevels() {
    if (num_levels != 3) return false;
    const int rows0 = vmaps_g_prev_d[0].rows() / 3, cols0 = vmaps_g_prev_d[0].cols();
    for (int i = 1; i < 3; ++i) {
        vmaps_g_prev_d[i].create((rows0 >> i) * 3, cols0 >> i);
        nmaps_g_prev_d[i].create((rows0 >> i) * 3, cols0 >> i);
    }
    return vmaps_g_prev_d[0].step() == nmaps_g_prev_d[0].step() && vmaps_g_prev_d[1].step() == nmaps_g_prev_d[1].step() &&
           vmaps_g_prev_d[2].step() == nmaps_g_prev_d[2].step();
}
void KinectFusionReconstruction::ModelMapPyramid() {
    if (pyramid_in_raycast_) { pyramid_in_raycast_ = false; return; }   // built by the raycast launch (CalculatePointCloud)
    if (num_levels == 3) {
        const int rows0 = vmaps_g_prev_d[0].rows() / 3, cols0 = vmaps_g_prev_d[0].cols();
        if (PreparePyramidLevels()) {
            // (its completion = the end of the frame's tail: what the announced next frame's map preparation waits for, HintNextFrame)
            check_rc(xs_resize_pyramid_ex(&vmaps_g_prev_d[0].ptr()->re, &nmaps_g_prev_d[0].ptr()->re, vmaps_g_prev_d[0].step(), rows0, cols0,
                                          &vmaps_g_prev_d[1].ptr()->re, &nmaps_g_prev_d[1].ptr()->re, vmaps_g_prev_d[1].step(),
                                          &vmaps_g_prev_d[2].ptr()->re, &nmaps_g_prev_d[2].ptr()->re, vmaps_g_prev_d[2].step(), tail_done_, current_stream()),
                     "resizeMap");
            tail_recorded_ = true;
            return;
        }
    }
    for (int i = 1; i < num_levels; ++i) {
        resizeVMap(vmaps_g_prev_d[i - 1], vmaps_g_prev_d[i], false);
        resizeNMap(nmaps_g_prev_d[i - 1], nmaps_g_prev_d[i], false);
    }
}

// The announced next frame's map preparation (HintNextFrame), on the second stream, in stages: called from the ICP loop (PoseEstimate), one
// stage per iteration, and with `all` at the end of AlignDepthToReconstruction for whatever is left (or where there is no ICP loop).
void KinectFusionReconstruction::EnqueueAnnouncedFrame(bool all) {
    // One stage per call from the ICP loop (the host has ~8 us to spare per iteration: one more launch next to the ICP launch it enqueues while
    // the GPU runs the previous one — all six at once delayed the frame's second pose by 15 us), the rest at once when `all`.
    while (next_hint_ptr_) {
        hipStream_t main_stream = current_stream();
        current_stream() = aux_stream_;
        // The NEXT frame's map preparation — bilateral filter, depth pyramid, vertex / normal maps, scaled depth — goes into the second set of
        // buffers: it depends on that depth image alone and runs while this frame's ICP launches (45 to 256 workgroups each, waiting on one
        // another) leave most of the GPU idle, instead of next to this frame's integrate and raycast, which the next frame's first ICP launch
        // waits for.  The sets change places around each stage only: the ICP launches enqueued in between read this frame's maps.
        SwapMapSets();
        const DeviceArray2D<ushort> next(depth_height, depth_width, const_cast<void *>(next_hint_ptr_), next_hint_step_);   // borrowed
        if (next_stage_ == 0) {
            if (depths_curr_d.size() != depths_next_d.size()) depths_curr_d.resize(depths_next_d.size());
            for (size_t i = 0; i < depths_curr_d.size(); ++i)
                if (depths_curr_d[i].rows() != depths_next_d[i].rows() || depths_curr_d[i].cols() != depths_next_d[i].cols())
                    depths_curr_d[i].create(depths_next_d[i].rows(), depths_next_d[i].cols());
            if (vmaps_curr_d.size() != vmaps_next_d.size()) { vmaps_curr_d.resize(vmaps_next_d.size()); nmaps_curr_d.resize(nmaps_next_d.size()); }
            if (depthRawScaled_d.rows() != depth_height || depthRawScaled_d.cols() != depth_width) depthRawScaled_d.create(depth_height, depth_width);
            if (!depth_max_.ptr()) depth_max_.create(4);
            if (!depth_tiles_.ptr()) depth_tiles_.create(xs_depth_tiles_bytes(depth_height, depth_width));
            // ... not before the previous frame's raycast and pyramid are through (the main stream's ICP launches start there): the event rides
            // on that pyramid's dispatch, the wait is a packet of this stream only
            if (tail_recorded_ && hipEventQuery(tail_done_) != hipSuccess) hipSafeCall(hipStreamWaitEvent(aux_stream_, tail_done_, 0));
            // (this set's scaled depth was the previous frame's: that frame's integrate must be through with it — it is, wherever the pyramid's
            // event above exists; the explicit wait covers the configurations without one)
            if (integrate_recorded_ && hipEventQuery(integrate_done_now_) != hipSuccess) hipSafeCall(hipStreamWaitEvent(aux_stream_, integrate_done_now_, 0));
            SmoothDepthFrame(depths_curr_d[0], next);
        } else if (next_stage_ < num_levels) {
            pyrDown(depths_curr_d[next_stage_ - 1], depths_curr_d[next_stage_]);
        } else if (next_stage_ == num_levels) {
            EnqueueMapsFromPyramid();
            hipSafeCall(hipEventRecord(surface_done_, aux_stream_));
        } else {
            EnqueueScale(next);
        }
        SwapMapSets();
        current_stream() = main_stream;
        if (++next_stage_ > num_levels + 1) {
            next_ready_ptr_ = next_hint_ptr_; next_ready_step_ = next_hint_step_; next_ready_ = true;
            next_hint_ptr_ = nullptr;
            next_stage_ = 0;
        }
        if (!all) break;
    }
}

// createVMap + createNMap of the current set's depth pyramid, on current_stream()
void KinectFusionReconstruction::EnqueueMapsFromPyramid() {
    {   // createVMap + createNMap per level (camera frame, +z forward), all levels in one launch
        Intr ks[3];
        const float *dp[3]; size_t ds[3], ms[3];
        float *vp[3], *np_[3];
        bool uniform = num_levels <= 3;
        for (int i = 0; i < num_levels && uniform; ++i) {
            ks[i] = kinect_intrinsic(i);
            vmaps_curr_d[i].create(depths_curr_d[i].rows() * 3, depths_curr_d[i].cols());
            nmaps_curr_d[i].create(depths_curr_d[i].rows() * 3, depths_curr_d[i].cols());
            dp[i] = &depths_curr_d[i].ptr()->re; ds[i] = depths_curr_d[i].step();
            vp[i] = &vmaps_curr_d[i].ptr()->re; np_[i] = &nmaps_curr_d[i].ptr()->re; ms[i] = vmaps_curr_d[i].step();
            uniform = depths_curr_d[i].rows() == (depth_height >> i) && depths_curr_d[i].cols() == (depth_width >> i) &&
                      nmaps_curr_d[i].step() == ms[i];
        }
        real_maps_valid_ = false;
        if (uniform && icp_real_current_maps) {
            float *vr[3], *nr[3]; size_t rs[3];
            vreal_curr_d.resize(num_levels); nreal_curr_d.resize(num_levels);
            for (int i = 0; i < num_levels; ++i) {
                vreal_curr_d[i].create(depths_curr_d[i].rows() * 3, depths_curr_d[i].cols());
                nreal_curr_d[i].create(depths_curr_d[i].rows() * 3, depths_curr_d[i].cols());
                vr[i] = vreal_curr_d[i].ptr(); nr[i] = nreal_curr_d[i].ptr(); rs[i] = vreal_curr_d[i].step();
                uniform = uniform && nreal_curr_d[i].step() == rs[i];
            }
            if (uniform) {
                check_rc(xs_create_vnmaps_real(num_levels, &ks[0].fx, dp, ds, depth_height, depth_width, vp, np_, ms, vr, nr, rs, current_stream()), "createVMap");
                real_maps_valid_ = true;
            }
        }
        if (real_maps_valid_) {
        } else if (uniform)
            check_rc(xs_create_vnmaps(num_levels, &ks[0].fx, dp, ds, depth_height, depth_width, vp, np_, ms, current_stream()), "createVMap");
        else
            for (int i = 0; i < num_levels; ++i) {
                createVMap(kinect_intrinsic(i), depths_curr_d[i], vmaps_curr_d[i]);
                createNMap(vmaps_curr_d[i], nmaps_curr_d[i]);
            }
    }
}

// scaleDepthKernal of integrateTsdfVolume (TsdfFusion.cu:182-187) into the current set, on the auxiliary stream
void KinectFusionReconstruction::EnqueueScale(const DeviceArray2D<ushort> &depth_frame_d) {
    hipSafeCall(hipMemsetAsync(depth_max_.ptr(), 0, sizeof(float), aux_stream_));
    // (+ the per-tile depth range the integrate call classifies its bricks with: free space / nothing to write / per-voxel walk)
    check_rc(xs_scale_depth_tiles(depth_frame_d.ptr(), depth_frame_d.step(), depth_frame_d.rows(), depth_frame_d.cols(), depthRawScaled_d.ptr(),
                                  depthRawScaled_d.step(), depth_max_.ptr(), depth_tiles_.ptr(), aux_stream_), "scaleDepth");
    hipSafeCall(hipEventRecord(scale_done_, aux_stream_));
    scale_recorded_ = true;
}

// the two sets of per-frame buffers (filtered depth pyramid, vertex / normal maps and their real planes, scaled depth and its maximum,
// the events that say when they are ready) change places
void KinectFusionReconstruction::SwapMapSets() {
    std::swap(depths_curr_d, depths_next_d);
    std::swap(vmaps_curr_d, vmaps_next_d);
    std::swap(nmaps_curr_d, nmaps_next_d);
    std::swap(vreal_curr_d, vreal_next_d);
    std::swap(nreal_curr_d, nreal_next_d);
    std::swap(depthRawScaled_d, depthRawScaled_next_d);
    std::swap(depth_max_, depth_max_next_);
    std::swap(depth_tiles_, depth_tiles_next_);
    std::swap(surface_done_, surface_done_next_);
    std::swap(scale_done_, scale_done_next_);
    std::swap(real_maps_valid_, real_maps_valid_next_);
    std::swap(scale_recorded_, scale_recorded_next_);
}

// reference :280-299
void KinectFusionReconstruction::SurfaceMeasure(const DeviceArray2D<ushort> &depth_frame_d) {
    if (depth_width <= 0 || depth_height <= 0) {
        std::cout << "error::KinectFusionReconstruction, not created yet" << std::endl;
        return;
    }
    // The current-frame maps depend only on the new depth image, which must be complete when
    // ProcessFrame is called: they are built on a second stream, so they run under whatever the
    // main stream still has in flight from the previous frame (raycast, pyramid), and the main
    // stream picks them up through an event before the first ICP launch.
    hipStream_t main_stream = current_stream();
    current_stream() = aux_stream_;
    stage_begin(ST_SURFACE);
    const bool adopted = next_ready_ && next_ready_ptr_ == (const void *)depth_frame_d.ptr() && next_ready_step_ == depth_frame_d.step();
    next_ready_ = false;
    if (adopted) {
        // this frame was announced while the previous one was being tracked (HintNextFrame): its maps and its scaled depth were built then, on
        // this same stream, in the second set of buffers — the sets change places, and so do the events that say when they were ready
        SwapMapSets();
    } else {
        SmoothDepthFrame(depths_curr_d[0], depth_frame_d);
        for (int i = 1; i < num_levels; ++i) pyrDown(depths_curr_d[i - 1], depths_curr_d[i]);
        EnqueueMapsFromPyramid();
    }
    stage_end(ST_SURFACE);
    // the ICP needs the maps and nothing else of this stream: the main stream picks them up here, not
    // behind the depth scaling below (two more kernels and their packets in front of the first ICP launch)
    if (!adopted) hipSafeCall(hipEventRecord(surface_done_, aux_stream_));
    // scaleDepthKernal of integrateTsdfVolume (TsdfFusion.cu:182-187) also depends on the depth image
    // alone: metres + the frame's largest valid depth, ready long before integrate asks for them
    // (the previous frame's integrate, possibly still running on the main stream, reads the same
    // buffers: wait for it — it is the first thing in that frame's tail)
    if (integrate_recorded_ && hipEventQuery(integrate_done_now_) != hipSuccess) hipSafeCall(hipStreamWaitEvent(aux_stream_, integrate_done_now_, 0));
    // The two tiny launches that bracket an integrate call — the fold of the previous frame's voxel count and the clear of
    // the brick-list header — run here, off the main stream's dependent chain (each cost that chain a dispatch: ~14 us a
    // frame); the integrate call below is told so (IntegrateFrame).  One integrate call per frame only, i.e. not sharded.
    if (integrate_split()) {
        flush_pending_fold(aux_stream_);
        check_rc(xs_integrate_workspace_clear(integrate_ws_.ptr(), aux_stream_), "integrate workspace");
        integrate_header_clear_ = true;
    }
    if (!adopted) {
        stage_begin(ST_SCALE);
        EnqueueScale(depth_frame_d);
        stage_end(ST_SCALE);
    }
    list_ready_ = false;
    current_stream() = main_stream;
    // the main stream picks the maps up — without a wait packet when they are already there (the usual case once the
    // previous frame's tail is the longer of the two)
    if (hipEventQuery(surface_done_) != hipSuccess) hipSafeCall(hipStreamWaitEvent(main_stream, surface_done_, 0));
}

// reference :302-332
int KinectFusionReconstruction::CalculatePointCloud(MapArr &xyz_g_d, MapArr &normal_g_d) {
    Matrix4cf c2w = inverse(world2camera);
    Matrix4cf c2v = world2volume * c2w;
    Matrix4cf v2w = inverse(world2volume);
    Matrix3frm Rc2v = GetRotation(c2v);
    Vector3cf tc2v = GetTranslation(c2v);
    Matrix3frm Rv2w = GetRotation(v2w);
    Vector3cf tv2w = GetTranslation(v2w);
    auto &device_Rc2v = device_cast<MatS33>(Rc2v);
    auto &device_tc2v = device_cast<devComplex3>(tc2v);
    auto &device_Rv2w = device_cast<MatS33>(Rv2w);
    auto &device_tv2w = device_cast<devComplex3>(tv2w);
    int3 volume_res;
    volume_res.x = volume_resolution.x();
    volume_res.y = volume_resolution.y();
    volume_res.z = volume_resolution.z();
    if (sign_map_stale_) { RebuildSignMap(); sign_map_stale_ = false; }   // (xs_kf_volume_ptr handed the value array out since the last raycast)
    xs_raycast_opts ro = {};   // the sign map, the pyramid outputs and the completion event of the raycast calls below (no per-thread setters)
    ro.struct_bytes = sizeof(ro);
    ro.signmap = sign_map_ptr(); ro.signmap_shift = raycast_sign_map_shift; ro.signmap_tranc_dist = tsdf_volume_d_ptr->getTsdfTruncDist();
    if (shard_count == 1 && !force_shard_composite) {
        // the model-map pyramid rides in the raycast launch where it can (three levels, the level-0 model maps, one launch: the sign map's
        // form): ModelMapPyramid then has nothing to launch, and the tail's completion event rides on the raycast
        pyramid_in_raycast_ = false;
        const bool own_maps = &xyz_g_d == &vmaps_g_prev_d[0] && &normal_g_d == &nmaps_g_prev_d[0];
        if (raycast_builds_pyramid && own_maps && PreparePyramidLevels()) {
            ro.pyr_vmap1 = &vmaps_g_prev_d[1].ptr()->re; ro.pyr_nmap1 = &nmaps_g_prev_d[1].ptr()->re; ro.pyr_step1 = vmaps_g_prev_d[1].step();
            ro.pyr_vmap2 = &vmaps_g_prev_d[2].ptr()->re; ro.pyr_nmap2 = &nmaps_g_prev_d[2].ptr()->re; ro.pyr_step2 = vmaps_g_prev_d[2].step();
            ro.completion_event = tail_done_;
        }
        raycast(kinect_intrinsic, device_Rc2v, device_tc2v, device_Rv2w, device_tv2w, tsdf_volume_d_ptr->getTsdfTruncDist(), volume_res,
                voxel_size, tsdf_volume_d_ptr->value(), tsdf_volume_d_ptr->grad(), xyz_g_d, normal_g_d, hits_counter_, ray_ws_.ptr(), &ro);
        if (ro.pyramid_built) { pyramid_in_raycast_ = true; tail_recorded_ = true; }
        return 0;
    }
    // sharded: march this rank's planes, agree on the first event of every ray, add the winners
    const int res[3] = {volume_res.x, volume_res.y, volume_res.z};
    const int rows = xyz_g_d.rows() / 3, cols = xyz_g_d.cols();
    hipStream_t st = current_stream();
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value(), grad = tsdf_volume_d_ptr->grad();
    check_rc(xs_raycast_slab_ex(&kinect_intrinsic.fx, &device_Rc2v.data[0].x.re, &device_tc2v.x.re, &device_Rv2w.data[0].x.re, &device_tv2w.x.re,
                                tsdf_volume_d_ptr->getTsdfTruncDist(), res, voxel_size, value.ptr(), grad.ptr(), value.step(), zs0, zs1, zo0, zo1,
                                &xyz_g_d.ptr()->re, &normal_g_d.ptr()->re, xyz_g_d.step(), rows, cols, ray_keys_.ptr(), &ro, st), "raycast");
    hipSafeCall(hipMemcpyAsync(ray_min_keys_.ptr(), ray_keys_.ptr(), (size_t)rows * cols * sizeof(int), hipMemcpyDeviceToDevice, st));
    if (collective) collective(collective_user, 1, ray_min_keys_.ptr(), (long)rows * cols);
    // (what a rank receives: a ring all-reduce of S bytes over N ranks moves 2 (N - 1) / N x S through every rank, a gather the other ranks' parts)
    const double ring = shard_count > 1 ? 2.0 * (shard_count - 1) / shard_count : 0.0;
    composite_bytes_ += (long long)(ring * (double)rows * cols * sizeof(int));
    check_rc(xs_raycast_compose_mask(ray_keys_.ptr(), ray_min_keys_.ptr(), &xyz_g_d.ptr()->re, &normal_g_d.ptr()->re, xyz_g_d.step(), rows, cols, st), "raycast");
    if (collective && shard_composite_gather) {
        // Owner-compacted exchange: every rank packs the pixels it owns (52 bytes each), the counts travel as an int32 sum with one non-zero
        // entry per rank, the packs are gathered at the offsets every rank derives from the counts, and a scatter writes them into the maps.
        // One host wait per frame (the counts); half the bytes of adding the maps (a ring all-reduce moves every pixel's 48 bytes twice).
        const int n_ranks = shard_count;
        const size_t eb = xs_raycast_compose_entry_bytes();
        if (!gather_buf_.ptr()) {
            gather_buf_.create((size_t)rows * cols * eb);       // every pixel has at most one owner: the gathered packs fit
            pack_buf_.create((size_t)rows * cols * eb);
            gather_counts_.create((size_t)n_ranks);
            hipSafeCall(hipHostMalloc((void **)&gather_counts_host_, (size_t)n_ranks * sizeof(int)));
        }
        hipSafeCall(hipMemsetAsync(gather_counts_.ptr(), 0, (size_t)n_ranks * sizeof(int), st));
        check_rc(xs_raycast_compose_pack(ray_keys_.ptr(), ray_min_keys_.ptr(), &xyz_g_d.ptr()->re, &normal_g_d.ptr()->re, xyz_g_d.step(), rows, cols,
                                         pack_buf_.ptr(), gather_counts_.ptr() + shard_rank, st), "raycast");
        collective(collective_user, 2, gather_counts_.ptr(), n_ranks);
        hipSafeCall(hipMemcpyAsync(gather_counts_host_, gather_counts_.ptr(), (size_t)n_ranks * sizeof(int), hipMemcpyDeviceToHost, st));
        hipSafeCall(hipStreamSynchronize(st));
        std::vector<long long> desc((size_t)n_ranks + 2);
        desc[0] = (long long)(size_t)gather_buf_.ptr();
        desc[1] = 0;
        for (int r = 0; r < n_ranks; ++r) desc[(size_t)r + 2] = desc[(size_t)r + 1] + (long long)gather_counts_host_[r] * (long long)eb;
        const long long total = desc[(size_t)n_ranks + 1];
        if (total > (long long)rows * cols * (long long)eb) { std::cout << "error::KinectFusionReconstruction, composite: more owned pixels than pixels" << std::endl; exit(-1); }
        const long long mine = desc[(size_t)shard_rank + 2] - desc[(size_t)shard_rank + 1];
        if (mine > 0)
            hipSafeCall(hipMemcpyAsync(gather_buf_.ptr() + desc[(size_t)shard_rank + 1], pack_buf_.ptr(), (size_t)mine, hipMemcpyDeviceToDevice, st));
        collective(collective_user, 3, desc.data(), n_ranks);   // gather-v: afterwards every rank holds every rank's part
        composite_bytes_ += total - mine + (long long)(ring * n_ranks * sizeof(int));
        check_rc(xs_raycast_compose_scatter(gather_buf_.ptr(), (long)(total / (long long)eb), &xyz_g_d.ptr()->re, &normal_g_d.ptr()->re, xyz_g_d.step(), rows, cols, st), "raycast");
    } else if (collective) {
        const long words = (long)(xyz_g_d.step() / 4) * xyz_g_d.rows();
        const bool adjacent = normal_g_d.step() == xyz_g_d.step() && normal_g_d.rows() == xyz_g_d.rows() &&
                              (const char *)normal_g_d.ptr() == (const char *)xyz_g_d.ptr() + xyz_g_d.step() * (size_t)xyz_g_d.rows();
        if (adjacent) collective(collective_user, 2, xyz_g_d.ptr(), 2 * words);  // 14.7 MB, one collective
        else {
            collective(collective_user, 2, xyz_g_d.ptr(), words);
            collective(collective_user, 2, normal_g_d.ptr(), words);
        }
        composite_bytes_ += (long long)(ring * 2.0 * words * 4.0);
    }
    check_rc(xs_raycast_compose_finish(ray_min_keys_.ptr(), &xyz_g_d.ptr()->re, &normal_g_d.ptr()->re, xyz_g_d.step(), rows, cols,
                                       hits_counter_, st), "raycast");
    return 0;
}

// The six seeded volume-to-camera poses of one Gauss-Newton pass: v2c_k = inverse(se3Exp(i h e_k) * camera2volume), k = 0 .. 5.
// For a single seeded generator se3Exp takes its small-angle branch and is EXACTLY I + i h G_k (G_k: unit translation along axis k, or the hat matrix
// of axis k - 3), whose inverse is I - i h G_k up to a REAL term h^2 G_k^2 (1e-14: below the rounding of every entry it would touch).  So
//     v2c_k = v2c - i h (v2c G_k),        v2c = inverse(camera2volume) once,
// and v2c G_k is a column of v2c (translations) or two columns of its rotation swapped and signed (rotations): one 4x4 inverse and a few dozen products
// instead of six complex 4x4 products and six complex 4x4 cofactor inverses (4.9 -> 0.5 us on the build container's core; the host's side of a pass is
// what stands between two kernels).  The six poses share their real parts bit for bit by construction (the kernel counts a voxel only if every seeded
// evaluation keeps it); the imaginary parts equal those of the long form to rounding (tests/test_gauss_newton_gpu.py: the oracle twin, which inverts in
// double, and the analytic seeds of the per-pass test).
static void gn_seeded_poses(const xs_host::Matrix4cf &camera2volume, float R[6][18], float t[6][6]) {
    using namespace xs_host;
    const Matrix4cf v2c = inverse(camera2volume);
    const hostComplex ih(0.f, (float)H_);
    for (int k = 0; k < 6; ++k) {
        hostComplex Rk[3][3], tk[3];
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) Rk[i][j] = v2c.m[i][j]; tk[i] = v2c.m[i][3]; }
        if (k < 3) {
            for (int i = 0; i < 3; ++i) tk[i] = tk[i] - ih * v2c.m[i][k];                    // (v2c G_k): column 3 = column k of the rotation
        } else {
            const int a = k - 3, b = (a + 1) % 3, c = (a + 2) % 3;                           // hat(e_a): (c, b) = +1, (b, c) = -1
            for (int i = 0; i < 3; ++i) {
                Rk[i][b] = Rk[i][b] - ih * v2c.m[i][c];                                      // (R hat)(i, b) = R(i, c)
                Rk[i][c] = Rk[i][c] + ih * v2c.m[i][b];                                      // (R hat)(i, c) = -R(i, b)
            }
        }
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) { R[k][(i * 3 + j) * 2] = Rk[i][j].real(); R[k][(i * 3 + j) * 2 + 1] = Rk[i][j].imag(); }
            t[k][2 * i] = tk[i].real(); t[k][2 * i + 1] = tk[i].imag();
        }
    }
}
// What every pass of a frame shares: the scaled depth (once per frame, not per pass) and this rank's owned planes as the dense array the
// kernel indexes (a pitched volume is packed first); the pinned record and the mailbox of the loop protocol.
const float *KinectFusionReconstruction::GaussNewtonPrepare(const DeviceArray2D<ushort> &depth_frame_d) {
    hipStream_t st = current_stream();
    depthRawScaled_d.create(depth_frame_d.rows(), depth_frame_d.cols());
    check_rc(xs_scale_depth(depth_frame_d.ptr(), depth_frame_d.step(), depth_frame_d.rows(), depth_frame_d.cols(), depthRawScaled_d.ptr(),
                            depthRawScaled_d.step(), st), "scaleDepth");
    if (gn_sums_.size() < 32) gn_sums_.create(32);
    if (gn_ws_.size() < xs_tsdf_reduce_workspace_bytes()) {
        gn_ws_.create(xs_tsdf_reduce_workspace_bytes());
        check_rc(xs_tsdf_reduce_workspace_init(gn_ws_.ptr(), st), "reduce workspace");
    }
    if (!gn_publish_) {
        hipSafeCall(hipHostMalloc((void **)&gn_publish_, xs_gn_publish_bytes(), hipHostMallocCoherent | hipHostMallocMapped));
        std::memset(gn_publish_, 0, xs_gn_publish_bytes());
    }
    if (!gn_mailbox_ && gn_post_pose) check_rc(xs_icp_mailbox_alloc(&gn_mailbox_, &gn_mailbox_in_device_), "Gauss-Newton mailbox");
    return GaussNewtonDenseView();
}
const float *KinectFusionReconstruction::GaussNewtonDenseView() {
    hipStream_t st = current_stream();
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value();
    const size_t row_bytes = (size_t)volume_resolution[0] * sizeof(float), plane_rows = (size_t)volume_resolution[1];
    const float *gt = reinterpret_cast<const float *>(reinterpret_cast<const char *>(value.ptr()) + (size_t)(zo0 - zs0) * plane_rows * value.step());
    if (value.step() != row_bytes) {
        const size_t rows = (size_t)(zo1 - zo0) * plane_rows;
        if (gn_dense_.size() < rows * volume_resolution[0]) gn_dense_.create(rows * volume_resolution[0]);
        hipSafeCall(hipMemcpy2DAsync(gn_dense_.ptr(), row_bytes, gt, value.step(), row_bytes, rows, hipMemcpyDeviceToDevice, st));
        gt = gn_dense_.ptr();
    }
    return gt;
}
// One pass enqueued: the kernel over the owned planes (poses as arguments, or — R null — from the mailbox with number mail_seq), in shard
// mode the all-reduce of the 29 sums on the stream and then their publication; single GPU: the kernel's last workgroup publishes.  The host
// reads the record with GaussNewtonWait(seq).
void KinectFusionReconstruction::GaussNewtonEnqueue(const DeviceArray2D<ushort> &depth_frame_d, const float *gt, const float (*R)[18], const float (*t)[6],
                                                    unsigned mail_seq, unsigned long long seq) {
    hipStream_t st = current_stream();
    const int res[3] = {volume_resolution[0], volume_resolution[1], volume_resolution[2]};
    const bool sharded = shard_count > 1 && collective;
    xs_gn_opts o = {};
    o.struct_bytes = sizeof(o);
    o.pose_mailbox = R ? nullptr : gn_mailbox_; o.mailbox_seq = mail_seq;
    if (!sharded) { o.publish_host = gn_publish_; o.publish_seq = seq; }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (profiling && gn_events_.size() < 64) {   // (level 1 or 2: the kernel's own duration, for bench.py's host_us_per_pass)
        hipSafeCall(hipEventCreate(&e0)); hipSafeCall(hipEventCreate(&e1));
        gn_events_.push_back({e0, e1});
        hipSafeCall(hipEventRecord(e0, st));
    }
    check_rc(xs_tsdf_gauss_newton_terms_ex(depthRawScaled_d.ptr(), depthRawScaled_d.step(), depth_frame_d.rows(), depth_frame_d.cols(), &kinect_intrinsic.fx,
                                           res, voxel_size, R ? &R[0][0] : nullptr, t ? &t[0][0] : nullptr, tsdf_volume_d_ptr->getTsdfTruncDist(), gt, zo0,
                                           zo1, gn_ws_.ptr(), gn_sums_.ptr(), &o, st), "GaussNewtonTerms");
    if (e1) hipSafeCall(hipEventRecord(e1, st));
    if (sharded) {
        collective(collective_user, 0, gn_sums_.ptr(), 29);
        if (gn_publish_sharded) check_rc(xs_gn_publish_sums(gn_sums_.ptr(), 29, gn_publish_, seq, st), "GaussNewtonTerms");
        else {   // (YAML gn_publish_sharded: false — the round-5 way: copy + stream drain, then the record is filled by the host itself)
            hipSafeCall(hipMemcpyAsync(gn_publish_, gn_sums_.ptr(), 29 * sizeof(double), hipMemcpyDeviceToHost, st));
            hipSafeCall(hipStreamSynchronize(st));
            reinterpret_cast<volatile unsigned long long *>(gn_publish_)[32] = seq;
        }
    }
}
// the kernel's sums of the seeded imaginary parts -> derivative sums: divided by h^2 (J^T J) and h (J^T r)
static void gn_scale_sums(const double *raw, double out29[29]) {
    const double ih = 1.0 / (double)(float)H_;
    for (int i = 0; i < 21; ++i) out29[i] = raw[i] * ih * ih;
    for (int i = 21; i < 27; ++i) out29[i] = raw[i] * ih;
    out29[27] = raw[27]; out29[28] = raw[28];
}
// One host step of the Gauss-Newton loop on pass p's sums: the loss goes into the history; then 1 = the loop is finished (p was the final loss
// pass), -1 = it failed (nothing to align to, or the damped system is not positive definite), 0 = camera2volume took the step, go on.
static int gn_loop_step(const double s[29], int p, int iterations, float damping, xs_host::Matrix4cf &camera2volume, std::vector<double> *loss_history) {
    using namespace xs_host;
    if (loss_history) loss_history->push_back(s[28] > 0 ? s[27] / s[28] : 0.0);
    if (p == iterations) return 1;                        // the final loss pass
    if (s[28] < 6) return -1;                             // nothing to align to
    double A[36], b[6], x[6];
    int q = 0;
    for (int j = 0; j < 6; ++j)
        for (int k = j; k < 6; ++k, ++q) { A[j * 6 + k] = s[q]; A[k * 6 + j] = s[q]; }
    for (int k = 0; k < 6; ++k) { A[k * 6 + k] *= 1.0 + (double)damping; b[k] = -s[21 + k]; }
    if (!solve_spd6(A, b, x)) return -1;
    hostComplex xi[6];
    for (int k = 0; k < 6; ++k) xi[k] = hostComplex((float)x[k], 0.f);
    camera2volume = se3Exp(xi) * camera2volume;
    return 0;
}
// spins on the record's sequence word; false if the launch reported that it left without summing (abandoned, or its poses never came),
// fatal if the stream failed or drained without publishing
bool KinectFusionReconstruction::GaussNewtonWait(unsigned long long seq, double out29[29]) {
    const xs_wait_result w = xs_host_wait([&] { return xs_poll_word(gn_publish_ + 32, seq); }, kWaitPolls, current_stream());
    if (w.status == xs_wait::left) return false;
    if (w.status != xs_wait::published) wait_fatal("Gauss-Newton pass", w);
    gn_scale_sums(gn_publish_, out29);
    return true;
}
void KinectFusionReconstruction::GaussNewtonCollectEvents() {
    for (auto &e : gn_events_) {
        float ms = 0.f;
        if (hipEventSynchronize(e.second) == hipSuccess && hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) { gn_kernel_ms += ms; ++gn_kernel_calls; }
        (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second);
    }
    gn_events_.clear();
}

// BASELINE config 5 (see the header): one pass of xs_tsdf_gauss_newton_terms for the six seeded poses
int KinectFusionReconstruction::GaussNewtonTerms(const DeviceArray2D<ushort> &depth_frame_d, const Matrix4cf &camera2volume, double out29[29]) {
    if (!tsdf_volume_d_ptr) return 0;
    const float *gt = GaussNewtonPrepare(depth_frame_d);
    float R[6][18], t[6][6];
    gn_seeded_poses(camera2volume, R, t);
    const unsigned long long seq = ++gn_seq_;
    GaussNewtonEnqueue(depth_frame_d, gt, R, t, 0u, seq);
    const bool ok = GaussNewtonWait(seq, out29);
    GaussNewtonCollectEvents();
    return ok ? 1 : 0;
}

// The Gauss-Newton loop with the ICP loop's protocol (round 6): the depth is scaled once per frame; a pass's sums reach the host through a
// pinned record the kernel's last workgroup writes (no copy, no stream drain); and pass n + 1 is in the queue BEFORE the host waits for pass
// n — its kernel resident, polling a mailbox for the six poses the host posts after the solve — so what stands between two kernels is the
// record's way to the host, the 6x6 solve, six pose inversions and one posted write (YAML gn_post_pose, default true; single GPU with a mailbox
// in device memory — a sharded rank enqueues pass n + 1 after the solve, its all-reduce on the stream in front of the publication).
int KinectFusionReconstruction::RelocalizeGaussNewton(const DeviceArray2D<ushort> &depth_frame_d, Matrix4cf &camera2volume, int iterations,
                                                      float damping, std::vector<double> *loss_history) {
    if (!tsdf_volume_d_ptr) return 0;
    const int passes = iterations + (loss_history ? 1 : 0);   // (the last one only reports the loss the loop ended at)
    if (passes <= 0) return 1;
    const float *gt = GaussNewtonPrepare(depth_frame_d);
    const bool ahead = gn_post_pose && shard_count == 1 && gn_mailbox_ && gn_mailbox_in_device_;
    float R[6][18], t[6][6];
    gn_seeded_poses(camera2volume, R, t);
    unsigned long long seq = ++gn_seq_;
    GaussNewtonEnqueue(depth_frame_d, gt, R, t, 0u, seq);
    int rc = 1;
    const auto t_begin = std::chrono::steady_clock::now();
    int done = 0;
    for (int p = 0; p < passes; ++p) {
        unsigned long long next_seq = 0;
        unsigned next_mail = 0;
        if (ahead && p + 1 < passes) {
            next_seq = ++gn_seq_; next_mail = ++gn_mail_seq_;
            if (next_mail == 0) next_mail = ++gn_mail_seq_;   // (0 is the mailbox's initial content)
            GaussNewtonEnqueue(depth_frame_d, gt, nullptr, nullptr, next_mail, next_seq);
        }
        auto leave = [&](int code) {   // the loop ends here: a launch that is waiting for its poses is told to leave, and has left before its buffers are reused
            if (next_seq) {
                xs_gn_post_poses(gn_mailbox_, nullptr, nullptr, next_mail, 1);
                double ignore[29];
                (void)GaussNewtonWait(next_seq, ignore);
            }
            rc = code;
        };
        double s[29];
        if (!GaussNewtonWait(seq, s)) { leave(0); break; }
        ++done;
        if (p > 0 && ahead) { gn_poll_us += gn_publish_[30] * 0.01; ++gn_poll_passes; }   // (this pass was enqueued ahead: what its kernel waited for its poses, 100 MHz ticks)
        const int step = gn_loop_step(s, p, iterations, damping, camera2volume, loss_history);
        if (step > 0) break;
        if (step < 0) { leave(0); break; }
        if (p + 1 < passes) {
            gn_seeded_poses(camera2volume, R, t);
            if (next_seq) { xs_gn_post_poses(gn_mailbox_, &R[0][0], &t[0][0], next_mail, 0); seq = next_seq; }
            else { seq = ++gn_seq_; GaussNewtonEnqueue(depth_frame_d, gt, R, t, 0u, seq); }
        }
    }
    gn_pass_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_begin).count();
    gn_passes += done;
    GaussNewtonCollectEvents();
    return rc;
}

// The band index of the owned planes, rebuilt when anything wrote the volume since it was built (volume_generation).  Count, then fill: the
// arrays grow to the count when they are too small.
void KinectFusionReconstruction::BandIndexPrepare() {
    if (band_generation_ == volume_generation && band_.nblocks > 0) return;
    hipStream_t st = current_stream();
    const int res[3] = {volume_resolution[0], volume_resolution[1], volume_resolution[2]};
    const float *gt = GaussNewtonDenseView();
    const size_t segs_bytes = xs_tsdf_band_segs_bytes(res, zo0, zo1);
    if (segs_bytes == 0) { std::cout << "error::KinectFusionReconstruction, relocalisation index: bad slab" << std::endl; exit(-1); }
    if (band_segs_.size() < segs_bytes / sizeof(long long)) band_segs_.create(segs_bytes / sizeof(long long));
    for (int attempt = 0;; ++attempt) {
        band_.keys = band_keys_.ptr(); band_.values = band_values_.ptr(); band_.segs = band_segs_.ptr();
        band_.capacity = (long long)std::min(band_keys_.size(), band_values_.size());
        const int rc = xs_tsdf_band_build(gt, res, zo0, zo1, &band_, st);
        if (rc == 0) break;
        if (rc != XS_BAND_OVER_CAPACITY || attempt > 0) check_rc(rc, "relocalisation index");
        band_keys_.create((size_t)band_.count);
        band_values_.create((size_t)band_.count);
    }
    band_generation_ = volume_generation;
}

// What the batched loops share: the band index, the Gauss-Newton band workspace and sums, and every frame's depth scaled once (not per
// pass) into band_depth_.  Returns the scaled depths' common step.
size_t KinectFusionReconstruction::BandBatchPrepare(const std::vector<DeviceArray2D<ushort>> &depths) {
    const int F = (int)depths.size();
    hipStream_t st = current_stream();
    BandIndexPrepare();
    const size_t ws_bytes = xs_tsdf_band_workspace_bytes(XS_BAND_MAX_FRAMES);
    if (band_ws_.size() < ws_bytes) {
        band_ws_.create(ws_bytes);
        check_rc(xs_tsdf_reduce_workspace_init(band_ws_.ptr(), st), "band workspace");   // (zeroes the tickets: once)
    }
    if (band_sums_.size() < (size_t)XS_BAND_MAX_FRAMES * 29) band_sums_.create((size_t)XS_BAND_MAX_FRAMES * 29);
    if ((int)band_depth_.size() < F) band_depth_.resize((size_t)F);
    const int rows = depths[0].rows(), cols = depths[0].cols();
    for (int f = 0; f < F; ++f) {   // the depth is scaled once per frame, not per pass
        band_depth_[(size_t)f].create(rows, cols);
        check_rc(xs_scale_depth(depths[(size_t)f].ptr(), depths[(size_t)f].step(), rows, cols, band_depth_[(size_t)f].ptr(), band_depth_[(size_t)f].step(), st),
                 "scaleDepth");
    }
    const size_t scaled_step = band_depth_[0].step();
    for (int f = 1; f < F; ++f)
        if (band_depth_[(size_t)f].step() != scaled_step) { std::cout << "error::KinectFusionReconstruction, batch: depth steps differ" << std::endl; exit(-1); }
    return scaled_step;
}

int KinectFusionReconstruction::RelocalizeGaussNewtonBatch(const std::vector<DeviceArray2D<ushort>> &depths, Matrix4cf *camera2volume, int iterations,
                                                           float damping, int *ok, std::vector<double> *loss_history) {
    const int F = (int)depths.size();
    for (int f = 0; f < F; ++f) ok[f] = 0;
    if (!tsdf_volume_d_ptr || F == 0) return 0;
    const int passes = iterations + (loss_history ? 1 : 0);
    if (passes <= 0) { for (int f = 0; f < F; ++f) ok[f] = 1; return F; }
    hipStream_t st = current_stream();
    const int rows = depths[0].rows(), cols = depths[0].cols();
    const size_t scaled_step = BandBatchPrepare(depths);
    const bool sharded = shard_count > 1 && collective;
    std::vector<int> active(F);
    for (int f = 0; f < F; ++f) active[(size_t)f] = f;
    std::vector<float> R((size_t)XS_BAND_MAX_FRAMES * 108), t((size_t)XS_BAND_MAX_FRAMES * 36);
    std::vector<const float *> dptr(XS_BAND_MAX_FRAMES);
    std::vector<double> raw((size_t)XS_BAND_MAX_FRAMES * 29);
    int succeeded = 0;
    for (int p = 0; p < passes && !active.empty(); ++p) {
        std::vector<int> next;
        for (size_t c0 = 0; c0 < active.size(); c0 += XS_BAND_MAX_FRAMES) {   // one launch per chunk of the frames still active
            const int n = (int)std::min(active.size() - c0, (size_t)XS_BAND_MAX_FRAMES);
            for (int i = 0; i < n; ++i) {
                const int f = active[c0 + (size_t)i];
                gn_seeded_poses(camera2volume[f], reinterpret_cast<float (*)[18]>(&R[(size_t)i * 108]), reinterpret_cast<float (*)[6]>(&t[(size_t)i * 36]));
                dptr[(size_t)i] = band_depth_[(size_t)f].ptr();
            }
            check_rc(xs_tsdf_gauss_newton_terms_band(n, dptr.data(), scaled_step, rows, cols, &kinect_intrinsic.fx, voxel_size, R.data(), t.data(),
                                                     tsdf_volume_d_ptr->getTsdfTruncDist(), &band_, band_ws_.ptr(), band_sums_.ptr(), st), "GaussNewtonTermsBand");
            if (sharded) collective(collective_user, 0, band_sums_.ptr(), (long)n * 29);   // the per-pass all-reduce of GaussNewtonEnqueue, F x 29 wide
            hipSafeCall(hipMemcpyAsync(raw.data(), band_sums_.ptr(), (size_t)n * 29 * sizeof(double), hipMemcpyDeviceToHost, st));
            hipSafeCall(hipStreamSynchronize(st));
            for (int i = 0; i < n; ++i) {
                const int f = active[c0 + (size_t)i];
                double s[29];
                gn_scale_sums(&raw[(size_t)i * 29], s);
                const int step = gn_loop_step(s, p, iterations, damping, camera2volume[f], loss_history ? &loss_history[f] : nullptr);
                if (step == 0 && p + 1 == passes) ok[f] = 1;   // (no loss pass: the last step ends the loop, as in RelocalizeGaussNewton)
                if (step > 0) ok[f] = 1;
                if (step == 0 && p + 1 < passes) next.push_back(f);
            }
        }
        active.swap(next);
    }
    for (int f = 0; f < F; ++f) succeeded += ok[f];
    return succeeded;
}


// ---- exact-Hessian (Newton) relocalisation over the band index ----
// One launch of xs_tsdf_pose_hessian_band for the n frames `frames` of the prepared batch (band_depth_), at most XS_BAND_MAX_FRAMES: the
// seeded poses, in shard mode the all-reduce of the n x 29 sums, the copy and the stream drain; raw: the kernel's sums.
void KinectFusionReconstruction::PoseHessianLaunch(const int *frames, int n, const Matrix4cf *camera2volume, size_t scaled_step, int rows, int cols, double *raw) {
    hipStream_t st = current_stream();
    const size_t ws_bytes = xs_tsdf_pose_hessian_workspace_bytes(XS_BAND_MAX_FRAMES);
    if (newton_ws_.size() < ws_bytes) {
        newton_ws_.create(ws_bytes);
        check_rc(xs_tsdf_reduce_workspace_init(newton_ws_.ptr(), st), "pose Hessian workspace");   // (zeroes the tickets: once)
    }
    if (newton_sums_.size() < (size_t)XS_BAND_MAX_FRAMES * 29) newton_sums_.create((size_t)XS_BAND_MAX_FRAMES * 29);
    std::vector<float> R((size_t)n * 21 * 36), t((size_t)n * 21 * 12);
    std::vector<const float *> dptr((size_t)n);
    for (int i = 0; i < n; ++i) {
        newton_seeded_poses(camera2volume[frames[i]], reinterpret_cast<float (*)[36]>(&R[(size_t)i * 21 * 36]), reinterpret_cast<float (*)[12]>(&t[(size_t)i * 21 * 12]));
        dptr[(size_t)i] = band_depth_[(size_t)frames[i]].ptr();
    }
    check_rc(xs_tsdf_pose_hessian_band(n, dptr.data(), scaled_step, rows, cols, &kinect_intrinsic.fx, voxel_size, R.data(), t.data(),
                                       tsdf_volume_d_ptr->getTsdfTruncDist(), &band_, newton_ws_.ptr(), newton_sums_.ptr(), st), "PoseHessianBand");
    if (shard_count > 1 && collective) collective(collective_user, 0, newton_sums_.ptr(), (long)n * 29);
    hipSafeCall(hipMemcpyAsync(raw, newton_sums_.ptr(), (size_t)n * 29 * sizeof(double), hipMemcpyDeviceToHost, st));
    hipSafeCall(hipStreamSynchronize(st));
}

int KinectFusionReconstruction::PoseHessianTerms(const DeviceArray2D<ushort> &depth_frame_d, const Matrix4cf &camera2volume, double out29[29]) {
    if (!tsdf_volume_d_ptr) return 0;
    const std::vector<DeviceArray2D<ushort>> depths(1, depth_frame_d);
    const size_t scaled_step = BandBatchPrepare(depths);
    const int frame = 0;
    double raw[29];
    PoseHessianLaunch(&frame, 1, &camera2volume, scaled_step, depth_frame_d.rows(), depth_frame_d.cols(), raw);
    newton_scale_sums(raw, out29);
    return 1;
}

// RelocalizeGaussNewtonBatch's loop with the Newton step: a pass is one pose-Hessian launch per chunk of the frames still active; a frame
// whose damped Hessian is not positive definite takes, for that iteration, the Gauss-Newton step of gn_loop_step on the six-pose band sums of
// its pose (one more launch, F = 1), and fallbacks[f] counts it.
int KinectFusionReconstruction::RelocalizeNewtonBatch(const std::vector<DeviceArray2D<ushort>> &depths, Matrix4cf *camera2volume, int iterations,
                                                      float damping, int *ok, std::vector<double> *loss_history, int *fallbacks) {
    const int F = (int)depths.size();
    for (int f = 0; f < F; ++f) { ok[f] = 0; if (fallbacks) fallbacks[f] = 0; }
    if (!tsdf_volume_d_ptr || F == 0) return 0;
    const int passes = iterations + (loss_history ? 1 : 0);
    if (passes <= 0) { for (int f = 0; f < F; ++f) ok[f] = 1; return F; }
    hipStream_t st = current_stream();
    const int rows = depths[0].rows(), cols = depths[0].cols();
    const size_t scaled_step = BandBatchPrepare(depths);
    const bool sharded = shard_count > 1 && collective;
    std::vector<int> active(F);
    for (int f = 0; f < F; ++f) active[(size_t)f] = f;
    std::vector<double> raw((size_t)XS_BAND_MAX_FRAMES * 29);
    for (int p = 0; p < passes && !active.empty(); ++p) {
        std::vector<int> next;
        for (size_t c0 = 0; c0 < active.size(); c0 += XS_BAND_MAX_FRAMES) {   // one launch per chunk of the frames still active
            const int n = (int)std::min(active.size() - c0, (size_t)XS_BAND_MAX_FRAMES);
            PoseHessianLaunch(&active[c0], n, camera2volume, scaled_step, rows, cols, raw.data());
            for (int i = 0; i < n; ++i) {
                const int f = active[c0 + (size_t)i];
                double s[29];
                newton_scale_sums(&raw[(size_t)i * 29], s);
                if (loss_history) loss_history[f].push_back(s[28] > 0 ? s[27] / s[28] : 0.0);
                if (p == iterations) { ok[f] = 1; continue; }   // the final loss pass
                if (s[28] < 6) continue;                        // nothing to align to: the frame fails
                if (!newton_step(s, (double)damping, camera2volume[f])) {
                    // not positive definite: this iteration's step is Gauss-Newton's, from the six-pose sums at the same pose
                    float R6[6][18], t6[6][6];
                    gn_seeded_poses(camera2volume[f], R6, t6);
                    const float *d = band_depth_[(size_t)f].ptr();
                    check_rc(xs_tsdf_gauss_newton_terms_band(1, &d, scaled_step, rows, cols, &kinect_intrinsic.fx, voxel_size, &R6[0][0], &t6[0][0],
                                                             tsdf_volume_d_ptr->getTsdfTruncDist(), &band_, band_ws_.ptr(), band_sums_.ptr(), st), "GaussNewtonTermsBand");
                    if (sharded) collective(collective_user, 0, band_sums_.ptr(), 29);
                    double gn_raw[29], gn[29];
                    hipSafeCall(hipMemcpyAsync(gn_raw, band_sums_.ptr(), 29 * sizeof(double), hipMemcpyDeviceToHost, st));
                    hipSafeCall(hipStreamSynchronize(st));
                    gn_scale_sums(gn_raw, gn);
                    if (fallbacks) ++fallbacks[f];
                    if (gn_loop_step(gn, p, iterations, damping, camera2volume[f], nullptr) != 0) continue;   // that failed too
                }
                if (p + 1 == passes) ok[f] = 1;   // (no loss pass: the last step ends the loop)
                else next.push_back(f);
            }
        }
        active.swap(next);
    }
    int succeeded = 0;
    for (int f = 0; f < F; ++f) succeeded += ok[f];
    return succeeded;
}

// ---- many pose hypotheses against the map in one band pass, and global relocalisation ----
int KinectFusionReconstruction::ScorePoses(const DeviceArray2D<ushort> &depth_frame_d, const Matrix4cf *camera2volume, int P, double *out2xP) {
    if (!tsdf_volume_d_ptr || P < 0) return 0;
    if (P == 0) return 1;
    hipStream_t st = current_stream();
    BandIndexPrepare();
    const size_t ws_bytes = xs_tsdf_score_poses_workspace_bytes(XS_SCORE_MAX_POSES);
    if (score_ws_.size() < ws_bytes) {
        score_ws_.create(ws_bytes);
        check_rc(xs_tsdf_reduce_workspace_init(score_ws_.ptr(), st), "score workspace");   // (zeroes the tickets: once)
    }
    if (score_sums_.size() < (size_t)XS_SCORE_MAX_POSES * 2) score_sums_.create((size_t)XS_SCORE_MAX_POSES * 2);
    const int rows = depth_frame_d.rows(), cols = depth_frame_d.cols();
    score_depth_.create(rows, cols);   // the depth is scaled once, not per chunk
    check_rc(xs_scale_depth(depth_frame_d.ptr(), depth_frame_d.step(), rows, cols, score_depth_.ptr(), score_depth_.step(), st), "scaleDepth");
    const bool sharded = shard_count > 1 && collective;
    std::vector<float> R, t;
    for (int p0 = 0; p0 < P; p0 += XS_SCORE_MAX_POSES) {
        const int n = std::min(P - p0, (int)XS_SCORE_MAX_POSES);
        R.resize((size_t)n * 9); t.resize((size_t)n * 3);
        for (int i = 0; i < n; ++i) {
            const Matrix4cf inv = inverse(camera2volume[p0 + i]);   // (newton_seeded_poses' real parts: the same inverse, its real part as float)
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) R[(size_t)i * 9 + (size_t)r * 3 + c] = inv.m[r][c].real();
                t[(size_t)i * 3 + r] = inv.m[r][3].real();
            }
        }
        check_rc(xs_tsdf_score_poses_band(n, score_depth_.ptr(), score_depth_.step(), rows, cols, &kinect_intrinsic.fx, voxel_size, R.data(), t.data(),
                                          tsdf_volume_d_ptr->getTsdfTruncDist(), &band_, score_ws_.ptr(), score_sums_.ptr(), st), "ScorePosesBand");
        if (sharded) collective(collective_user, 0, score_sums_.ptr(), (long)n * 2);
        hipSafeCall(hipMemcpyAsync(out2xP + 2 * (size_t)p0, score_sums_.ptr(), (size_t)n * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        hipSafeCall(hipStreamSynchronize(st));   // (the chunk's host arrays and the workspace are free again)
    }
    return 1;
}

int KinectFusionReconstruction::RelocalizeGlobal(const DeviceArray2D<ushort> &depth_frame_d, const Matrix4cf *candidates, int P, int keep, int iterations,
                                                 float damping, Matrix4cf &best, double report[8]) {
    for (int i = 0; i < 8; ++i) report[i] = 0.0;
    report[0] = -1.0;
    if (!tsdf_volume_d_ptr || P <= 0 || keep <= 0) return 0;
    std::vector<double> before((size_t)P * 2);
    if (!ScorePoses(depth_frame_d, candidates, P, before.data())) return 0;
    report[6] = (double)band_.count;
    const std::vector<int> top = score_top_k(before.data(), P, keep);
    const int K = (int)top.size();
    std::vector<Matrix4cf> refined((size_t)K);
    for (int k = 0; k < K; ++k) refined[(size_t)k] = candidates[top[(size_t)k]];
    const std::vector<DeviceArray2D<ushort>> depths((size_t)K, depth_frame_d);   // the same image in every slot
    std::vector<int> ok((size_t)K, 0);
    report[5] = (double)RelocalizeGaussNewtonBatch(depths, refined.data(), iterations, damping, ok.data(), nullptr);
    std::vector<double> after((size_t)K * 2);
    ScorePoses(depth_frame_d, refined.data(), K, after.data());
    const int w = score_winner(after.data(), ok.data(), K);
    if (w < 0) return 0;
    best = refined[(size_t)w];
    report[0] = (double)top[(size_t)w];
    report[1] = score_S(&before[2 * (size_t)top[(size_t)w]]);
    report[2] = score_S(&after[2 * (size_t)w]);
    report[3] = after[2 * (size_t)w];
    report[4] = after[2 * (size_t)w + 1];
    return 1;
}

// ---- candidate views against the map in one launch, and the next best view ----
// The observation grid follows the volume the way BandIndexPrepare's index does.  False when the resolution has no grid.
bool KinectFusionReconstruction::ViewGridPrepare(int min_weight) {
    const int mw = min_weight < 1 ? 1 : min_weight;
    const int res[3] = {volume_resolution[0], volume_resolution[1], volume_resolution[2]};
    const size_t bytes = xs_view_grid_bytes(res);
    if (bytes == 0) return false;
    if (view_grid_.size() < bytes) { view_grid_.create(bytes); view_generation_ = -1; }
    if (view_generation_ == volume_generation && view_min_weight_ == mw) return true;
    const DeviceArray2D<float> value = tsdf_volume_d_ptr->value();
    const DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    if (value.step() != weight.step()) { std::cout << "error::KinectFusionReconstruction, observation grid: value and weight pitches differ" << std::endl; exit(-1); }
    check_rc(xs_view_grid_build(value.ptr(), weight.ptr(), value.step(), res, mw, view_grid_.ptr(), current_stream()), "ViewGridBuild");
    view_generation_ = volume_generation;
    view_min_weight_ = mw;
    return true;
}

int KinectFusionReconstruction::ScoreViews(const Matrix4cf *camera2volume, int P, const xs_view_opts *opts, int min_weight, unsigned *out4xP) {
    if (shard_count > 1) return -2;   // a ray's occlusion is not additive over the ranks' z-slabs
    if (P < 0 || (P > 0 && (!camera2volume || !out4xP))) return -1;
    if (!tsdf_volume_d_ptr) return 0;
    if (P == 0) return 1;
    hipStream_t st = current_stream();
    if (!ViewGridPrepare(min_weight)) return -1;
    if (view_counts_.size() < (size_t)XS_VIEW_MAX_POSES * 4) view_counts_.create((size_t)XS_VIEW_MAX_POSES * 4);
    const int res[3] = {volume_resolution[0], volume_resolution[1], volume_resolution[2]};
    std::vector<float> R, t;
    for (int p0 = 0; p0 < P; p0 += XS_VIEW_MAX_POSES) {
        const int n = std::min(P - p0, (int)XS_VIEW_MAX_POSES);
        R.resize((size_t)n * 9); t.resize((size_t)n * 3);
        for (int i = 0; i < n; ++i)
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) R[(size_t)i * 9 + (size_t)r * 3 + c] = camera2volume[p0 + i].m[r][c].real();
                t[(size_t)i * 3 + r] = camera2volume[p0 + i].m[r][3].real();
            }
        const int rc = xs_score_views(n, R.data(), t.data(), &kinect_intrinsic.fx, depth_height, depth_width, res, voxel_size, view_grid_.ptr(), opts,
                                      view_counts_.ptr(), st);
        if (rc == (int)hipErrorInvalidValue) return -1;   // the options: nothing was launched
        check_rc(rc, "ScoreViews");
        hipSafeCall(hipMemcpyAsync(out4xP + 4 * (size_t)p0, view_counts_.ptr(), (size_t)n * 4 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        hipSafeCall(hipStreamSynchronize(st));   // (the grid's pose staging area and the counts are free again)
    }
    return 1;
}

int KinectFusionReconstruction::NextBestView(const Matrix4cf *camera2volume, int P, const xs_view_opts *opts, int min_weight, unsigned min_hits,
                                             unsigned *out4xP) {
    std::vector<unsigned> own;
    if (!out4xP && P > 0) { own.resize((size_t)P * 4); out4xP = own.data(); }
    const int rc = ScoreViews(camera2volume, P, opts, min_weight, out4xP);
    if (rc == -1) return -3;   // (-1 is "no pose qualifies" here)
    if (rc < 0) return rc;
    if (rc == 0) return -1;
    return next_best_view(out4xP, P, min_hits);
}

// ---- clearance and reachability of candidate views ----
// The field follows the grid, the grid the volume.  False when the resolution has no field.
bool KinectFusionReconstruction::ClearancePrepare(int R, int unknown_blocks, int min_weight) {
    const int mw = min_weight < 1 ? 1 : min_weight;
    const int res[3] = {volume_resolution[0], volume_resolution[1], volume_resolution[2]};
    const size_t bytes = xs_clearance_bytes(res), ws = xs_clearance_workspace_bytes(res);
    if (bytes == 0 || !ViewGridPrepare(mw)) return false;
    if (clear_field_.size() < bytes) { clear_field_.create(bytes); clear_generation_ = -1; }
    if (clear_ws_.size() < ws) clear_ws_.create(ws);
    if (clear_generation_ == volume_generation && clear_min_weight_ == mw && clear_R_ == R && clear_unknown_ == unknown_blocks) return true;
    check_rc(xs_clearance_build(view_grid_.ptr(), res, R, unknown_blocks, clear_ws_.ptr(), reinterpret_cast<unsigned short *>(clear_field_.ptr()),
                                current_stream()), "ClearanceBuild");
    clear_generation_ = volume_generation;
    clear_min_weight_ = mw; clear_R_ = R; clear_unknown_ = unknown_blocks;
    reach_generation_ = -1;   // (the flood was over another field)
    return true;
}

int KinectFusionReconstruction::ClearanceField(int max_radius_vox, int unknown_blocks, int min_weight, unsigned short *host_out) {
    if (shard_count > 1) return -2;   // a distance is not additive over the ranks' z-slabs
    if (!host_out || max_radius_vox < 1 || max_radius_vox > XS_CLEARANCE_MAX_RADIUS || (unknown_blocks != 0 && unknown_blocks != 1)) return -1;
    if (!tsdf_volume_d_ptr) return 0;
    if (!ClearancePrepare(max_radius_vox, unknown_blocks, min_weight)) return -1;
    hipStream_t st = current_stream();
    const int res[3] = {volume_resolution[0], volume_resolution[1], volume_resolution[2]};
    hipSafeCall(hipMemcpyAsync(host_out, clear_field_.ptr(), xs_clearance_bytes(res), hipMemcpyDeviceToHost, st));
    hipSafeCall(hipStreamSynchronize(st));
    return 1;
}

// n points through xs_reach_query against reach_ and clear_field_, in chunks of 4096; the answers on the host when the call returns
int KinectFusionReconstruction::ReachQuery(const float *points3xN, int n, int over_passable, int snap, unsigned char *reachable, unsigned short *clear2,
                                           int *voxel) {
    enum { CHUNK = 4096, POINTS = 0, VOXEL = CHUNK * 12, CLEAR2 = VOXEL + CHUNK * 12, FLAGS = CLEAR2 + CHUNK * 2, BYTES = FLAGS + CHUNK };
    if (reach_io_.size() < (size_t)BYTES) reach_io_.create(BYTES);
    hipStream_t st = current_stream();
    const int res[3] = {volume_resolution[0], volume_resolution[1], volume_resolution[2]};
    unsigned char *io = reach_io_.ptr();
    for (int p0 = 0; p0 < n; p0 += CHUNK) {
        const int m = std::min(n - p0, (int)CHUNK);
        hipSafeCall(hipMemcpyAsync(io + POINTS, points3xN + 3 * (size_t)p0, (size_t)m * 12, hipMemcpyHostToDevice, st));
        const int rc = xs_reach_query(m, reinterpret_cast<const float *>(io + POINTS), res, voxel_size, reach_.ptr(), over_passable,
                                      reinterpret_cast<const unsigned short *>(clear_field_.ptr()), snap, io + FLAGS, reinterpret_cast<unsigned short *>(io + CLEAR2),
                                      reinterpret_cast<int *>(io + VOXEL), st);
        if (rc == (int)hipErrorInvalidValue) return -1;
        check_rc(rc, "ReachQuery");
        if (reachable) hipSafeCall(hipMemcpyAsync(reachable + p0, io + FLAGS, (size_t)m, hipMemcpyDeviceToHost, st));
        if (clear2) hipSafeCall(hipMemcpyAsync(clear2 + p0, io + CLEAR2, (size_t)m * 2, hipMemcpyDeviceToHost, st));
        if (voxel) hipSafeCall(hipMemcpyAsync(voxel + 3 * (size_t)p0, io + VOXEL, (size_t)m * 12, hipMemcpyDeviceToHost, st));
        hipSafeCall(hipStreamSynchronize(st));   // (the staging area is free again)
    }
    return 1;
}

int KinectFusionReconstruction::Reachable(const Matrix4cf *start, float radius_m, int snap_vox, int unknown_blocks, int min_weight, int P,
                                          const Matrix4cf *camera2volume, unsigned char *reachable, unsigned short *clear2) {
    if (shard_count > 1) return -2;   // connectivity is not additive over the ranks' z-slabs
    int r2 = 0, R = 0;
    if (P < 0 || (P > 0 && (!camera2volume || !reachable || !clear2)) || snap_vox < 0 || snap_vox > XS_REACH_MAX_SNAP ||
        (unknown_blocks != 0 && unknown_blocks != 1) || !reach_radius(radius_m, voxel_size, r2, R))
        return -1;
    if (!tsdf_volume_d_ptr) return 0;
    const int mw = min_weight < 1 ? 1 : min_weight;
    if (!ClearancePrepare(R, unknown_blocks, mw)) return -1;
    hipStream_t st = current_stream();
    const int res[3] = {volume_resolution[0], volume_resolution[1], volume_resolution[2]};
    const size_t bytes = xs_reach_bytes(res);
    if (bytes == 0) return -1;
    if (reach_.size() < bytes) { reach_.create(bytes); reach_generation_ = -1; }
    const unsigned short *field = reinterpret_cast<const unsigned short *>(clear_field_.ptr());
    const bool same_field = reach_generation_ == volume_generation && reach_min_weight_ == mw && reach_R_ == R && reach_unknown_ == unknown_blocks && reach_r2_ == r2;
    // the passable words (those of the last flood, if it was over this field at this r2), and the start snapped over them
    if (!same_field) check_rc(xs_reach_passable(view_grid_.ptr(), field, res, r2, reach_.ptr(), st), "ReachPassable");
    const Matrix4cf from = start ? *start : getCamera2Volume();
    const float p[3] = {from.m[0][3].real(), from.m[1][3].real(), from.m[2][3].real()};
    int seed[3] = {-1, -1, -1};
    unsigned char found = 0;
    if (ReachQuery(p, 1, 1, snap_vox, &found, nullptr, seed) < 0) return -1;
    if (!found) seed[0] = seed[1] = seed[2] = -1;   // (outside the volume as a seed: contributes nothing, and nothing is reached)
    if (!same_field || seed[0] != reach_seed_[0] || seed[1] != reach_seed_[1] || seed[2] != reach_seed_[2]) {
        reach_generation_ = -1;
        check_rc(xs_reach_flood(view_grid_.ptr(), field, res, r2, seed, 1, reach_.ptr(), nullptr, st), "ReachFlood");
        reach_generation_ = volume_generation;
        reach_min_weight_ = mw; reach_R_ = R; reach_unknown_ = unknown_blocks; reach_r2_ = r2;
        reach_seed_[0] = seed[0]; reach_seed_[1] = seed[1]; reach_seed_[2] = seed[2];
    }
    if (P == 0) return 1;
    std::vector<float> pts((size_t)P * 3);
    for (int i = 0; i < P; ++i)
        for (int c = 0; c < 3; ++c) pts[(size_t)i * 3 + c] = camera2volume[i].m[c][3].real();
    return ReachQuery(pts.data(), P, 0, 0, reachable, clear2, nullptr);
}

int KinectFusionReconstruction::NextReachableView(const Matrix4cf *camera2volume, int P, const xs_view_opts *opts, int min_weight, unsigned min_hits,
                                                  unsigned *out4xP, float radius_m, int snap_vox, int unknown_blocks, unsigned char *reachable) {
    std::vector<unsigned> own;
    std::vector<unsigned char> own_flags;
    std::vector<unsigned short> clear2((size_t)(P > 0 ? P : 0));
    if (!out4xP && P > 0) { own.resize((size_t)P * 4); out4xP = own.data(); }
    if (!reachable && P > 0) { own_flags.resize((size_t)P); reachable = own_flags.data(); }
    int rc = Reachable(nullptr, radius_m, snap_vox, unknown_blocks, min_weight, P, camera2volume, reachable, clear2.data());
    if (rc == 1) rc = ScoreViews(camera2volume, P, opts, min_weight, out4xP);
    if (rc == -1) return -3;   // (-1 is "no pose qualifies" here)
    if (rc < 0) return rc;
    if (rc == 0) return -1;
    return next_reachable_view(out4xP, reachable, P, min_hits);
}

// reference :334-372
KinectFusionReconstruction::CPointCloud KinectFusionReconstruction::ExportPointCloud(int max_buffer) {
    CPointCloud res;
    if (max_buffer <= 0 || !tsdf_volume_d_ptr) return res;
    DeviceArray<float3> cloud_buffer, normal_buffer;
    cloud_buffer.create(max_buffer);
    normal_buffer.create(max_buffer);
    int3 volume_res;
    volume_res.x = volume_resolution.x();
    volume_res.y = volume_resolution.y();
    volume_res.z = volume_resolution.z();
    // a rank of a sharded run reports the crossings of the planes it owns (the +z neighbour of its last
    // plane is in its halo); the single-GPU case is the whole volume
    const int z1 = std::min(zo1, volume_res.z - 1);
    PtrSz<float3> cloud; cloud.data = cloud_buffer.ptr(); cloud.size = (size_t)max_buffer;
    const size_t num_points = extractPoints(tsdf_volume_d_ptr->value(), tsdf_volume_d_ptr->weight(), tsdf_volume_d_ptr->grad(), volume_res,
                                            voxel_size, cloud, zs0, zo0, std::max(z1, zo0));
    if (num_points == 0) return res;
    cloud.size = num_points;
    PtrSz<float3> normal; normal.data = normal_buffer.ptr(); normal.size = num_points;
    extractNormals(tsdf_volume_d_ptr->value(), tsdf_volume_d_ptr->weight(), tsdf_volume_d_ptr->grad(), volume_res, voxel_size, cloud, normal,
                   zs0, zs1);
    res.positions.resize(3 * num_points);
    res.normals.resize(3 * num_points);
    hipSafeCall(hipMemcpy(res.positions.data(), cloud_buffer.ptr(), num_points * sizeof(float3), hipMemcpyDeviceToHost));
    hipSafeCall(hipMemcpy(res.normals.data(), normal_buffer.ptr(), num_points * sizeof(float3), hipMemcpyDeviceToHost));
    return res;
}
bool KinectFusionReconstruction::CPointCloud::exportPly(const std::string &filename) const {
    std::ofstream file_out{filename};
    if (!file_out.is_open()) return false;
    file_out << "ply\nformat ascii 1.0\ncomment Created by myself\nelement vertex " << size() << "\n";
    file_out << "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\nend_header\n";
    for (size_t i = 0; i < size(); ++i)
        file_out << positions[3 * i] << " " << positions[3 * i + 1] << " " << positions[3 * i + 2] << " " << normals[3 * i] << " "
                 << normals[3 * i + 1] << " " << normals[3 * i + 2] << "\n";
    return true;
}

KinectFusionReconstruction::CMesh KinectFusionReconstruction::ExportMesh(int min_weight) {
    CMesh m;
    if (!tsdf_volume_d_ptr) return m;
    if (sign_map_stale_) { RebuildSignMap(); sign_map_stale_ = false; }   // (the map must be a superset of the negative voxels)
    const int res[3] = {volume_resolution.x(), volume_resolution.y(), volume_resolution.z()};
    const bool seeded = csfd_seed_row >= 0 && csfd_seed_row < 4 && csfd_seed_col >= 0 && csfd_seed_col < 4;
    m.has_im = seeded;   // (also for an empty mesh: a rank without surface still says whether its vertices would carry derivatives)
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value(), grad = tsdf_volume_d_ptr->grad();
    DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    // (TsdfVolume allocates the three arrays alike: one pitch)
    xs_mesh_opts o{};
    o.struct_bytes = sizeof(o);
    o.zs0 = zs0; o.zs1 = zs1;
    o.z0 = zo0; o.z1 = std::max(std::min(zo1, res[2] - 1), zo0);   // (as ExportPointCloud)
    o.min_weight = min_weight; o.want_normals = 1;
    o.signmap = sign_map_ptr(); o.signmap_shift = raycast_sign_map_shift;
    DeviceArray<unsigned char> ws;
    ws.create(xs_mesh_workspace_bytes(res, &o));
    const float *g = seeded ? grad.ptr(0) : nullptr;
    size_t nv = 0, nt = 0;
    int rc = xs_extract_mesh(value.ptr(0), weight.ptr(0), g, value.step(), res, voxel_size, &o, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0,
                             ws.ptr(), &nv, &nt, current_stream());
    if (rc == 0) return m;   // (nothing fits in no room only when there is nothing)
    if (rc != XS_MESH_OVER_CAPACITY) check_rc(rc, "mesh count");
    DeviceArray<float> verts, vim, normals;
    DeviceArray<unsigned long long> keys;
    DeviceArray<int> tris;
    verts.create(3 * nv); normals.create(3 * nv); keys.create(nv); tris.create(3 * std::max<size_t>(nt, 1));
    if (seeded) vim.create(3 * nv);
    size_t nv2 = 0, nt2 = 0;
    check_rc(xs_extract_mesh(value.ptr(0), weight.ptr(0), g, value.step(), res, voxel_size, &o, verts.ptr(), seeded ? vim.ptr() : nullptr,
                             normals.ptr(), keys.ptr(), nv, tris.ptr(), nt, ws.ptr(), &nv2, &nt2, current_stream()), "mesh");
    m.positions.resize(3 * nv); m.normals.resize(3 * nv); m.edge_keys.resize(nv); m.triangles.resize(3 * nt);
    hipSafeCall(hipMemcpy(m.positions.data(), verts.ptr(), 3 * nv * sizeof(float), hipMemcpyDeviceToHost));
    hipSafeCall(hipMemcpy(m.normals.data(), normals.ptr(), 3 * nv * sizeof(float), hipMemcpyDeviceToHost));
    hipSafeCall(hipMemcpy(m.edge_keys.data(), keys.ptr(), nv * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (nt) hipSafeCall(hipMemcpy(m.triangles.data(), tris.ptr(), 3 * nt * sizeof(int), hipMemcpyDeviceToHost));
    if (seeded) {
        m.vertex_im.resize(3 * nv);
        hipSafeCall(hipMemcpy(m.vertex_im.data(), vim.ptr(), 3 * nv * sizeof(float), hipMemcpyDeviceToHost));
    }
    return m;
}
bool KinectFusionReconstruction::CMesh::exportPly(const std::string &filename) const {
    std::ofstream f(filename, std::ios::binary);
    if (!f.is_open()) return false;
    const bool d = has_im;
    f << "ply\nformat binary_little_endian 1.0\nelement vertex " << vertices() << "\n";
    f << "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n";
    if (d) f << "property float dx\nproperty float dy\nproperty float dz\n";
    f << "element face " << faces() << "\nproperty list uchar int vertex_indices\nend_header\n";
    std::vector<float> row(d ? 9 : 6);   // (x86 / the hosts this builds for are little-endian: the floats go out as they are)
    for (size_t i = 0; i < vertices(); ++i) {
        for (int k = 0; k < 3; ++k) { row[k] = positions[3 * i + k]; row[3 + k] = normals[3 * i + k]; if (d) row[6 + k] = vertex_im[3 * i + k]; }
        f.write(reinterpret_cast<const char *>(row.data()), (std::streamsize)(row.size() * sizeof(float)));
    }
    char face[13];
    face[0] = 3;
    for (size_t t = 0; t < faces(); ++t) {
        std::memcpy(face + 1, &triangles[3 * t], 12);
        f.write(face, 13);
    }
    return (bool)f;
}

void KinectFusionReconstruction::synchronize() { hipSafeCall(hipStreamSynchronize(current_stream())); }

long long KinectFusionReconstruction::lastUpdatedVoxels() { return last_frame_counter(0); }
long long KinectFusionReconstruction::lastRaycastHits() { return last_frame_counter(1); }
long long KinectFusionReconstruction::last_frame_counter(int which) {
    if (counter_frame_ == 0) return 0;
    unsigned long long h[2] = {0, 0};
    synchronize();
    flush_pending_fold(current_stream());
    hipSafeCall(hipStreamSynchronize(current_stream()));
    hipSafeCall(hipMemcpy(h, counters_.ptr() + 2 * (size_t)((counter_frame_ - 1) % COUNTER_RING), sizeof(h), hipMemcpyDeviceToHost));
    return (long long)h[which];
}

// ---- volume checkpoint --------------------------------------------------------------------
// reference :438-447 writes raw float32 values; here X*Y*Z of them (the reference's count uses
// res[2] twice)
void KinectFusionReconstruction::saveTSDFVolume(const std::string &tsdf_filename) {
    std::vector<float> tsdf;
    tsdf_volume_d_ptr->downloadTSDFWithoutGrad(tsdf);
    std::ofstream f(tsdf_filename, std::ios::binary);
    f.write(reinterpret_cast<const char *>(tsdf.data()), (std::streamsize)(tsdf.size() * sizeof(float)));
}
namespace {
// Volume checkpoint, version 2.  Layout: header, n_poses x Matrix4cf, then value / grad / weight of the stored planes
// [zs0, zs1) as dense rows of X elements (a rank of a sharded run saves and restores its own planes).
struct CkptHeader {
    char magic[8];
    int res[3];
    float voxel_size, tranc_dist;
    int frame_id, n_poses;
    int zs0, zs1;        // planes held in this file
    int shard_rank, shard_count;
};
const int CKPT_MAX_POSES = 1 << 24;   // a sanity bound on the pose record (16 M frames), not a format limit
// one device <- host copy of a dense array into the EXISTING pitched buffer (no reallocation, no temporaries)
template <class T>
void restore_rows(DeviceArray2D<T> dst, const std::vector<T> &src, int cols, size_t rows) {
    hipSafeCall(hipMemcpy2D(dst.ptr(), dst.step(), src.data(), (size_t)cols * sizeof(T), (size_t)cols * sizeof(T), rows, hipMemcpyHostToDevice));
}
}  // namespace
void KinectFusionReconstruction::saveCheckpoint(const std::string &filename) {
    std::vector<float> v, g;
    std::vector<int> w;
    tsdf_volume_d_ptr->downloadTSDFWithGrad(v, g);
    tsdf_volume_d_ptr->downloadWeight(w);
    CkptHeader h{};
    std::snprintf(h.magic, sizeof(h.magic), "XSTSDF2");
    for (int i = 0; i < 3; ++i) h.res[i] = volume_resolution[i];
    h.voxel_size = voxel_size; h.tranc_dist = tsdf_volume_d_ptr->getTsdfTruncDist(); h.frame_id = frame_id;
    h.n_poses = (int)world2camera_record.size();
    h.zs0 = zs0; h.zs1 = zs1; h.shard_rank = shard_rank; h.shard_count = shard_count;
    std::ofstream f(filename, std::ios::binary);
    f.write(reinterpret_cast<const char *>(&h), sizeof(h));
    f.write(reinterpret_cast<const char *>(world2camera_record.data()), (std::streamsize)(h.n_poses * sizeof(Matrix4cf)));
    f.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * 4));
    f.write(reinterpret_cast<const char *>(g.data()), (std::streamsize)(g.size() * 4));
    f.write(reinterpret_cast<const char *>(w.data()), (std::streamsize)(w.size() * 4));
}
// Nothing of *this is touched until the whole file has been read and validated: magic, volume geometry (resolution,
// voxel size, truncation distance), the planes it holds against the planes this instance stores, a sane pose count and
// the exact file length.  Returns false (state unchanged) on any mismatch.
// The sign map from the volume alone (allocation, checkpoint, anything that wrote the value array without the integrate kernels).
void KinectFusionReconstruction::RebuildSignMap() {
    ++volume_generation;   // the documented "the volume was written" call: the relocalisation index is rebuilt too
    if (!sign_map_on() || !sign_map_.ptr() || !tsdf_volume_d_ptr) return;
    const int res[3] = {volume_resolution.x(), volume_resolution.y(), volume_resolution.z()};
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value();
    check_rc(xs_signmap_rebuild_slab(sign_map_.ptr(), res, raycast_sign_map_shift, tsdf_volume_d_ptr->getTsdfTruncDist(), value.ptr(0), value.step(),
                                     zs0, zs1, current_stream()), "sign map");
}

bool KinectFusionReconstruction::loadCheckpoint(const std::string &filename) {
    std::ifstream f(filename, std::ios::binary);
    if (!f || !tsdf_volume_d_ptr) return false;
    f.seekg(0, std::ios::end);
    const long long file_bytes = (long long)f.tellg();
    f.seekg(0, std::ios::beg);
    CkptHeader h{};
    if (file_bytes < (long long)sizeof(h)) return false;
    f.read(reinterpret_cast<char *>(&h), sizeof(h));
    if (!f || std::memcmp(h.magic, "XSTSDF2", 8) != 0) return false;
    for (int i = 0; i < 3; ++i) if (h.res[i] != volume_resolution[i]) return false;
    if (h.voxel_size != voxel_size || h.tranc_dist != tsdf_volume_d_ptr->getTsdfTruncDist()) return false;
    if (h.zs0 != zs0 || h.zs1 != zs1 || h.shard_rank != shard_rank || h.shard_count != shard_count) return false;
    if (h.n_poses < 1 || h.n_poses > CKPT_MAX_POSES || h.frame_id < 0) return false;
    const int X = h.res[0];
    const size_t rows = (size_t)h.res[1] * (size_t)(h.zs1 - h.zs0), n = rows * (size_t)X;
    const long long expect = (long long)sizeof(h) + (long long)h.n_poses * (long long)sizeof(Matrix4cf) + 3LL * (long long)n * 4LL;
    if (file_bytes != expect) return false;            // truncated or trailing bytes
    std::vector<Matrix4cf> poses((size_t)h.n_poses);
    f.read(reinterpret_cast<char *>(poses.data()), (std::streamsize)(poses.size() * sizeof(Matrix4cf)));
    std::vector<float> v(n), g(n);
    std::vector<int> w(n);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(n * 4));
    f.read(reinterpret_cast<char *>(g.data()), (std::streamsize)(n * 4));
    f.read(reinterpret_cast<char *>(w.data()), (std::streamsize)(n * 4));
    if (!f) return false;
    DeviceArray2D<float> dv = tsdf_volume_d_ptr->value(), dg = tsdf_volume_d_ptr->grad();
    DeviceArray2D<int> dw = tsdf_volume_d_ptr->weight();
    if ((size_t)dv.rows() != rows || dv.cols() != X || (size_t)dg.rows() != rows || (size_t)dw.rows() != rows) return false;
    // validated: commit
    synchronize();
    restore_rows(dv, v, X, rows);
    restore_rows(dg, g, X, rows);
    restore_rows(dw, w, X, rows);
    ++volume_generation;
    RebuildSignMap();    // the volume was written behind the integrate kernels' back
    world2camera_record.swap(poses);
    world2camera = world2camera_record.back();
    frame_id = h.frame_id;
    // previous-frame maps are derived state: regenerate them from the restored volume and pose (in a sharded run every
    // rank must load its own file before the next frame: the raycast composite is a collective)
    CalculatePointCloud(vmaps_g_prev_d[0], nmaps_g_prev_d[0]);
    ModelMapPyramid();
    synchronize();
    return true;
}

// ---- per-stage HIP event timing (on the stream the kernels are launched on) -----------------
void KinectFusionReconstruction::set_profiling(int level) {
    const bool on = level > 0;
    if (on && prof_ring_.empty()) {
        prof_ring_.resize(PROF_RING);
        for (auto &slot : prof_ring_)
            for (int s = 0; s < ST_COUNT; ++s) {
                hipSafeCall(hipEventCreate(&slot.ev[s][0]));
                hipSafeCall(hipEventCreate(&slot.ev[s][1]));
                slot.used[s] = false;
            }
    }
    if (profiling) collect_stage_times();
    profiling = on;
    profiling_stages = level > 1;
}
void KinectFusionReconstruction::stage_begin(int st) {
    if (!profiling_stages) return;
    hipSafeCall(hipEventRecord(prof_ring_[prof_pending_].ev[st][0], current_stream()));
}
void KinectFusionReconstruction::stage_end(int st) {
    if (!profiling_stages) return;
    hipSafeCall(hipEventRecord(prof_ring_[prof_pending_].ev[st][1], current_stream()));
    prof_ring_[prof_pending_].used[st] = true;
}
void KinectFusionReconstruction::end_profiled_frame() {
    // nothing is enqueued here: the frame's counters stay in their ring slot until the pending frames are folded
    if (++prof_pending_ == PROF_RING) collect_stage_times();
}
void KinectFusionReconstruction::collect_stage_times() {
    flush_pending_fold(current_stream());
    synchronize();
    if (prof_pending_ > 0)
        hipSafeCall(hipMemcpy(pinned_counters_, counters_.ptr(), COUNTER_RING * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int f = 0; f < prof_pending_; ++f) {
        // pending frame f is the (prof_pending_ - f)-th most recent integrated frame
        const long long fr = counter_frame_ - prof_pending_ + f;
        if (fr >= 0) {
            cum_updated += (long long)pinned_counters_[2 * (fr % COUNTER_RING)];
            cum_hits += (long long)pinned_counters_[2 * (fr % COUNTER_RING) + 1];
        }
        for (int s = 0; s < ST_COUNT; ++s) {
            if (!prof_ring_[f].used[s]) continue;
            float ms = 0.f;
            hipSafeCall(hipEventElapsedTime(&ms, prof_ring_[f].ev[s][0], prof_ring_[f].ev[s][1]));
            stage_ms[s] += ms;
            stage_calls[s] += 1;
            prof_ring_[f].used[s] = false;
        }
    }
    prof_pending_ = 0;
}
