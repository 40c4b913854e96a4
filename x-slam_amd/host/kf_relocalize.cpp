// kf_relocalize.cpp — the pose of a lost camera against the map as it stands: the dense Gauss-Newton pass and loop, the band index and both
// batched loops over it, pose scoring and global relocalisation (DESIGN.md sections 4.9, 4.15 - 4.17).  None of it runs during tracking.
#include "kf_internal.hpp"
#include "newton_host.hpp"
#include "score_host.hpp"

using namespace xs_host;
static_assert(GN_H == H_, "gn_host.hpp restates the seed step of xs_types.hpp");

// (the tickets are zeroed once per allocation: the kernels leave them zero)
void KinectFusionReconstruction::ensure_reduce_workspace(DeviceArray<unsigned char> &ws, size_t bytes, const char *what) {
    if (ws.size() >= bytes) return;
    ws.create(bytes);
    check_rc(xs_tsdf_reduce_workspace_init(ws.ptr(), current_stream()), what);
}
// (after the drain the launch's host arrays and its workspace are free again)
void KinectFusionReconstruction::fetch_sums(double *device_sums, size_t count, double *host_sums) {
    hipStream_t st = current_stream();
    if (shard_count > 1 && collective) collective(collective_user, 0, device_sums, (long)count);
    hipSafeCall(hipMemcpyAsync(host_sums, device_sums, count * sizeof(double), hipMemcpyDeviceToHost, st));
    hipSafeCall(hipStreamSynchronize(st));
}

// What every pass of a frame shares: the scaled depth (once per frame, not per pass) and this rank's owned planes as the dense array the
// kernel indexes (a pitched volume is packed first); the pinned record and the mailbox of the loop protocol.
const float *KinectFusionReconstruction::GaussNewtonPrepare(const DeviceArray2D<ushort> &depth_frame_d) {
    hipStream_t st = current_stream();
    depthRawScaled_d.create(depth_frame_d.rows(), depth_frame_d.cols());
    check_rc(xs_scale_depth(depth_frame_d.ptr(), depth_frame_d.step(), depth_frame_d.rows(), depth_frame_d.cols(), depthRawScaled_d.ptr(),
                            depthRawScaled_d.step(), st), "scaleDepth");
    if (reloc_.gn_sums.size() < 32) reloc_.gn_sums.create(32);
    ensure_reduce_workspace(reloc_.gn_ws, xs_tsdf_reduce_workspace_bytes(), "reduce workspace");
    if (!reloc_.gn_publish) {
        hipSafeCall(hipHostMalloc((void **)&reloc_.gn_publish, xs_gn_publish_bytes(), hipHostMallocCoherent | hipHostMallocMapped));
        std::memset(reloc_.gn_publish, 0, xs_gn_publish_bytes());
    }
    if (!reloc_.gn_mailbox && gn_post_pose) check_rc(xs_icp_mailbox_alloc(&reloc_.gn_mailbox, &reloc_.gn_mailbox_in_device), "Gauss-Newton mailbox");
    return GaussNewtonDenseView();
}
const float *KinectFusionReconstruction::GaussNewtonDenseView() {
    hipStream_t st = current_stream();
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value();
    const size_t row_bytes = (size_t)volume_resolution[0] * sizeof(float), plane_rows = (size_t)volume_resolution[1];
    const float *gt = reinterpret_cast<const float *>(reinterpret_cast<const char *>(value.ptr()) + (size_t)(zo0 - zs0) * plane_rows * value.step());
    if (value.step() != row_bytes) {
        const size_t rows = (size_t)(zo1 - zo0) * plane_rows;
        if (reloc_.gn_dense.size() < rows * volume_resolution[0]) reloc_.gn_dense.create(rows * volume_resolution[0]);
        hipSafeCall(hipMemcpy2DAsync(reloc_.gn_dense.ptr(), row_bytes, gt, value.step(), row_bytes, rows, hipMemcpyDeviceToDevice, st));
        gt = reloc_.gn_dense.ptr();
    }
    return gt;
}
// One pass enqueued: the kernel over the owned planes (poses as arguments, or — R null — from the mailbox with number mail_seq), in shard
// mode the all-reduce of the 29 sums on the stream and then their publication; single GPU: the kernel's last workgroup publishes.  The host
// reads the record with GaussNewtonWait(seq).
void KinectFusionReconstruction::GaussNewtonEnqueue(const DeviceArray2D<ushort> &depth_frame_d, const float *gt, const float (*R)[18], const float (*t)[6],
                                                    unsigned mail_seq, unsigned long long seq) {
    hipStream_t st = current_stream();
    const bool sharded = shard_count > 1 && collective;
    xs_gn_opts o = {};
    o.struct_bytes = sizeof(o);
    o.pose_mailbox = R ? nullptr : reloc_.gn_mailbox; o.mailbox_seq = mail_seq;
    if (!sharded) { o.publish_host = reloc_.gn_publish; o.publish_seq = seq; }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (profiling && reloc_.gn_events.size() < 64) {   // (level 1 or 2: the kernel's own duration, for bench.py's host_us_per_pass)
        hipSafeCall(hipEventCreate(&e0)); hipSafeCall(hipEventCreate(&e1));
        reloc_.gn_events.push_back({e0, e1});
        hipSafeCall(hipEventRecord(e0, st));
    }
    check_rc(xs_tsdf_gauss_newton_terms_ex(depthRawScaled_d.ptr(), depthRawScaled_d.step(), depth_frame_d.rows(), depth_frame_d.cols(), &kinect_intrinsic.fx,
                                           res3(), voxel_size, R ? &R[0][0] : nullptr, t ? &t[0][0] : nullptr, tsdf_volume_d_ptr->getTsdfTruncDist(), gt, zo0,
                                           zo1, reloc_.gn_ws.ptr(), reloc_.gn_sums.ptr(), &o, st), "GaussNewtonTerms");
    if (e1) hipSafeCall(hipEventRecord(e1, st));
    if (sharded && gn_publish_sharded) {
        collective(collective_user, 0, reloc_.gn_sums.ptr(), 29);
        check_rc(xs_gn_publish_sums(reloc_.gn_sums.ptr(), 29, reloc_.gn_publish, seq, st), "GaussNewtonTerms");
    } else if (sharded) {   // (YAML gn_publish_sharded: false — the round-5 way: copy + stream drain, then the record is filled by the host itself)
        fetch_sums(reloc_.gn_sums.ptr(), 29, reloc_.gn_publish);
        reinterpret_cast<volatile unsigned long long *>(reloc_.gn_publish)[32] = seq;
    }
}
// spins on the record's sequence word; false if the launch reported that it left without summing (abandoned, or its poses never came),
// fatal if the stream failed or drained without publishing
bool KinectFusionReconstruction::GaussNewtonWait(unsigned long long seq, double out29[29]) {
    const xs_wait_result w = xs_host_wait([&] { return xs_poll_word(reloc_.gn_publish + 32, seq); }, kWaitPolls, current_stream());
    if (w.status == xs_wait::left) return false;
    if (w.status != xs_wait::published) wait_fatal("Gauss-Newton pass", w);
    gn_scale_sums(reloc_.gn_publish, out29);
    return true;
}
void KinectFusionReconstruction::GaussNewtonCollectEvents() {
    for (auto &e : reloc_.gn_events) {
        float ms = 0.f;
        if (hipEventSynchronize(e.second) == hipSuccess && hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) { gn_kernel_ms += ms; ++gn_kernel_calls; }
        (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second);
    }
    reloc_.gn_events.clear();
}

// BASELINE config 5 (see the header): one pass of xs_tsdf_gauss_newton_terms for the six seeded poses
int KinectFusionReconstruction::GaussNewtonTerms(const DeviceArray2D<ushort> &depth_frame_d, const Matrix4cf &camera2volume, double out29[29]) {
    if (!tsdf_volume_d_ptr) return 0;
    const float *gt = GaussNewtonPrepare(depth_frame_d);
    float R[6][18], t[6][6];
    gn_seeded_poses(camera2volume, R, t);
    const unsigned long long seq = ++reloc_.gn_seq;
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
    const bool ahead = gn_post_pose && shard_count == 1 && reloc_.gn_mailbox && reloc_.gn_mailbox_in_device;
    float R[6][18], t[6][6];
    gn_seeded_poses(camera2volume, R, t);
    unsigned long long seq = ++reloc_.gn_seq;
    GaussNewtonEnqueue(depth_frame_d, gt, R, t, 0u, seq);
    int rc = 1;
    const auto t_begin = std::chrono::steady_clock::now();
    int done = 0;
    for (int p = 0; p < passes; ++p) {
        unsigned long long next_seq = 0;
        unsigned next_mail = 0;
        if (ahead && p + 1 < passes) {
            next_seq = ++reloc_.gn_seq; next_mail = ++reloc_.gn_mail_seq;
            if (next_mail == 0) next_mail = ++reloc_.gn_mail_seq;   // (0 is the mailbox's initial content)
            GaussNewtonEnqueue(depth_frame_d, gt, nullptr, nullptr, next_mail, next_seq);
        }
        auto leave = [&](int code) {   // the loop ends here: a launch that is waiting for its poses is told to leave, and has left before its buffers are reused
            if (next_seq) {
                xs_gn_post_poses(reloc_.gn_mailbox, nullptr, nullptr, next_mail, 1);
                double ignore[29];
                (void)GaussNewtonWait(next_seq, ignore);
            }
            rc = code;
        };
        double s[29];
        if (!GaussNewtonWait(seq, s)) { leave(0); break; }
        ++done;
        if (p > 0 && ahead) { gn_poll_us += reloc_.gn_publish[30] * 0.01; ++gn_poll_passes; }   // (this pass was enqueued ahead: what its kernel waited for its poses, 100 MHz ticks)
        const int step = gn_loop_step(s, p, iterations, damping, camera2volume, loss_history);
        if (step > 0) break;
        if (step < 0) { leave(0); break; }
        if (p + 1 < passes) {
            gn_seeded_poses(camera2volume, R, t);
            if (next_seq) { xs_gn_post_poses(reloc_.gn_mailbox, &R[0][0], &t[0][0], next_mail, 0); seq = next_seq; }
            else { seq = ++reloc_.gn_seq; GaussNewtonEnqueue(depth_frame_d, gt, R, t, 0u, seq); }
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
    if (reloc_.band_key == BandKey{volume_generation} && reloc_.band.nblocks > 0) return;
    hipStream_t st = current_stream();
    const int *res = res3();
    const float *gt = GaussNewtonDenseView();
    const size_t segs_bytes = xs_tsdf_band_segs_bytes(res, zo0, zo1);
    if (segs_bytes == 0) { std::cout << "error::KinectFusionReconstruction, relocalisation index: bad slab" << std::endl; exit(-1); }
    if (reloc_.band_segs.size() < segs_bytes / sizeof(long long)) reloc_.band_segs.create(segs_bytes / sizeof(long long));
    for (int attempt = 0;; ++attempt) {
        reloc_.band.keys = reloc_.band_keys.ptr(); reloc_.band.values = reloc_.band_values.ptr(); reloc_.band.segs = reloc_.band_segs.ptr();
        reloc_.band.capacity = (long long)std::min(reloc_.band_keys.size(), reloc_.band_values.size());
        const int rc = xs_tsdf_band_build(gt, res, zo0, zo1, &reloc_.band, st);
        if (rc == 0) break;
        if (rc != XS_BAND_OVER_CAPACITY || attempt > 0) check_rc(rc, "relocalisation index");
        reloc_.band_keys.create((size_t)reloc_.band.count);
        reloc_.band_values.create((size_t)reloc_.band.count);
    }
    reloc_.band_key = BandKey{volume_generation};
}

// What the batched loops share: the band index, the Gauss-Newton band workspace and sums, and every frame's depth scaled once (not per
// pass) into reloc_.band_depth.  Returns the scaled depths' common step.
size_t KinectFusionReconstruction::BandBatchPrepare(const std::vector<DeviceArray2D<ushort>> &depths) {
    const int F = (int)depths.size();
    hipStream_t st = current_stream();
    BandIndexPrepare();
    ensure_reduce_workspace(reloc_.band_ws, xs_tsdf_band_workspace_bytes(XS_BAND_MAX_FRAMES), "band workspace");
    if (reloc_.band_sums.size() < (size_t)XS_BAND_MAX_FRAMES * 29) reloc_.band_sums.create((size_t)XS_BAND_MAX_FRAMES * 29);
    if ((int)reloc_.band_depth.size() < F) reloc_.band_depth.resize((size_t)F);
    const int rows = depths[0].rows(), cols = depths[0].cols();
    for (int f = 0; f < F; ++f) {   // the depth is scaled once per frame, not per pass
        reloc_.band_depth[(size_t)f].create(rows, cols);
        check_rc(xs_scale_depth(depths[(size_t)f].ptr(), depths[(size_t)f].step(), rows, cols, reloc_.band_depth[(size_t)f].ptr(), reloc_.band_depth[(size_t)f].step(), st),
                 "scaleDepth");
    }
    const size_t scaled_step = reloc_.band_depth[0].step();
    for (int f = 1; f < F; ++f)
        if (reloc_.band_depth[(size_t)f].step() != scaled_step) { std::cout << "error::KinectFusionReconstruction, batch: depth steps differ" << std::endl; exit(-1); }
    return scaled_step;
}

// One launch of xs_tsdf_gauss_newton_terms_band for the n frames `frames` of the prepared batch (reloc_.band_depth), at most XS_BAND_MAX_FRAMES:
// the six seeded poses of each, the launch, and its n x 29 sums fetched into raw.
void KinectFusionReconstruction::GaussNewtonBandLaunch(const int *frames, int n, const Matrix4cf *camera2volume, size_t scaled_step, int rows, int cols, double *raw) {
    std::vector<float> R((size_t)n * 108), t((size_t)n * 36);
    std::vector<const float *> dptr((size_t)n);
    for (int i = 0; i < n; ++i) {
        gn_seeded_poses(camera2volume[frames[i]], reinterpret_cast<float (*)[18]>(&R[(size_t)i * 108]), reinterpret_cast<float (*)[6]>(&t[(size_t)i * 36]));
        dptr[(size_t)i] = reloc_.band_depth[(size_t)frames[i]].ptr();
    }
    check_rc(xs_tsdf_gauss_newton_terms_band(n, dptr.data(), scaled_step, rows, cols, &kinect_intrinsic.fx, voxel_size, R.data(), t.data(),
                                             tsdf_volume_d_ptr->getTsdfTruncDist(), &reloc_.band, reloc_.band_ws.ptr(), reloc_.band_sums.ptr(), current_stream()),
             "GaussNewtonTermsBand");
    fetch_sums(reloc_.band_sums.ptr(), (size_t)n * 29, raw);   // (shard mode: the per-pass all-reduce of GaussNewtonEnqueue, n x 29 wide)
}

// gn_batch_loop (gn_host.hpp) over the band index: a pass is one six-pose launch per chunk of the frames still active, the step RelocalizeGaussNewton's own.
int KinectFusionReconstruction::RelocalizeGaussNewtonBatch(const std::vector<DeviceArray2D<ushort>> &depths, Matrix4cf *camera2volume, int iterations,
                                                           float damping, int *ok, std::vector<double> *loss_history) {
    const int F = (int)depths.size();
    if (!tsdf_volume_d_ptr) { std::fill(ok, ok + F, 0); return 0; }
    const size_t scaled_step = F > 0 && iterations + (loss_history ? 1 : 0) > 0 ? BandBatchPrepare(depths) : 0;   // (a loop that launches nothing prepares nothing)
    return gn_batch_loop(F, iterations, loss_history, ok, XS_BAND_MAX_FRAMES,
        [&](const int *frames, int n, double *sums) {
            GaussNewtonBandLaunch(frames, n, camera2volume, scaled_step, depths[0].rows(), depths[0].cols(), sums);
            for (int i = 0; i < n; ++i) gn_scale_sums(sums + 29 * i, sums + 29 * i);
        },
        [&](int f, const double *s, int) { return damped_spd6_step(s, (double)damping, camera2volume[f]); });
}

// ---- exact-Hessian (Newton) relocalisation over the band index ----
// One launch of xs_tsdf_pose_hessian_band for the n frames `frames` of the prepared batch (reloc_.band_depth), at most XS_BAND_MAX_FRAMES: the
// seeded poses, the launch, and its n x 29 sums fetched into raw.
void KinectFusionReconstruction::PoseHessianLaunch(const int *frames, int n, const Matrix4cf *camera2volume, size_t scaled_step, int rows, int cols, double *raw) {
    ensure_reduce_workspace(reloc_.newton_ws, xs_tsdf_pose_hessian_workspace_bytes(XS_BAND_MAX_FRAMES), "pose Hessian workspace");
    if (reloc_.newton_sums.size() < (size_t)XS_BAND_MAX_FRAMES * 29) reloc_.newton_sums.create((size_t)XS_BAND_MAX_FRAMES * 29);
    std::vector<float> R((size_t)n * 21 * 36), t((size_t)n * 21 * 12);
    std::vector<const float *> dptr((size_t)n);
    for (int i = 0; i < n; ++i) {
        newton_seeded_poses(camera2volume[frames[i]], reinterpret_cast<float (*)[36]>(&R[(size_t)i * 21 * 36]), reinterpret_cast<float (*)[12]>(&t[(size_t)i * 21 * 12]));
        dptr[(size_t)i] = reloc_.band_depth[(size_t)frames[i]].ptr();
    }
    check_rc(xs_tsdf_pose_hessian_band(n, dptr.data(), scaled_step, rows, cols, &kinect_intrinsic.fx, voxel_size, R.data(), t.data(),
                                       tsdf_volume_d_ptr->getTsdfTruncDist(), &reloc_.band, reloc_.newton_ws.ptr(), reloc_.newton_sums.ptr(), current_stream()),
             "PoseHessianBand");
    fetch_sums(reloc_.newton_sums.ptr(), (size_t)n * 29, raw);
}

int KinectFusionReconstruction::PoseHessianTerms(const DeviceArray2D<ushort> &depth_frame_d, const Matrix4cf &camera2volume, double out29[29]) {
    if (!tsdf_volume_d_ptr) return 0;
    const std::vector<DeviceArray2D<ushort>> depths(1, depth_frame_d);
    const size_t scaled_step = BandBatchPrepare(depths);
    const int frame = 0;
    PoseHessianLaunch(&frame, 1, &camera2volume, scaled_step, depth_frame_d.rows(), depth_frame_d.cols(), out29);
    newton_scale_sums(out29, out29);
    return 1;
}

// gn_batch_loop with the Newton step: a pass is one pose-Hessian launch per chunk of the frames still active; a frame whose damped Hessian is not
// positive definite takes, for that iteration, the Gauss-Newton step on the six-pose band sums of its pose (one more launch, n = 1): fallbacks[f].
int KinectFusionReconstruction::RelocalizeNewtonBatch(const std::vector<DeviceArray2D<ushort>> &depths, Matrix4cf *camera2volume, int iterations,
                                                      float damping, int *ok, std::vector<double> *loss_history, int *fallbacks) {
    const int F = (int)depths.size();
    if (fallbacks) std::fill(fallbacks, fallbacks + F, 0);
    if (!tsdf_volume_d_ptr) { std::fill(ok, ok + F, 0); return 0; }
    const size_t scaled_step = F > 0 && iterations + (loss_history ? 1 : 0) > 0 ? BandBatchPrepare(depths) : 0;   // (a loop that launches nothing prepares nothing)
    return gn_batch_loop(F, iterations, loss_history, ok, XS_BAND_MAX_FRAMES,
        [&](const int *frames, int n, double *sums) {
            PoseHessianLaunch(frames, n, camera2volume, scaled_step, depths[0].rows(), depths[0].cols(), sums);
            for (int i = 0; i < n; ++i) newton_scale_sums(sums + 29 * i, sums + 29 * i);
        },
        [&](int f, const double *s, int) {
            if (newton_step(s, (double)damping, camera2volume[f])) return true;
            // not positive definite: this iteration's step is Gauss-Newton's, from the six-pose sums at the same pose
            double gn[29];
            GaussNewtonBandLaunch(&f, 1, camera2volume, scaled_step, depths[0].rows(), depths[0].cols(), gn);
            gn_scale_sums(gn, gn);
            if (fallbacks) ++fallbacks[f];
            return damped_spd6_step(gn, (double)damping, camera2volume[f]);   // (false: that failed too)
        });
}

// ---- many pose hypotheses against the map in one band pass, and global relocalisation ----
int KinectFusionReconstruction::ScorePoses(const DeviceArray2D<ushort> &depth_frame_d, const Matrix4cf *camera2volume, int P, double *out2xP) {
    if (!tsdf_volume_d_ptr || P < 0) return 0;
    if (P == 0) return 1;
    hipStream_t st = current_stream();
    BandIndexPrepare();
    ensure_reduce_workspace(reloc_.score_ws, xs_tsdf_score_poses_workspace_bytes(XS_SCORE_MAX_POSES), "score workspace");
    if (reloc_.score_sums.size() < (size_t)XS_SCORE_MAX_POSES * 2) reloc_.score_sums.create((size_t)XS_SCORE_MAX_POSES * 2);
    const int rows = depth_frame_d.rows(), cols = depth_frame_d.cols();
    reloc_.score_depth.create(rows, cols);   // the depth is scaled once, not per chunk
    check_rc(xs_scale_depth(depth_frame_d.ptr(), depth_frame_d.step(), rows, cols, reloc_.score_depth.ptr(), reloc_.score_depth.step(), st), "scaleDepth");
    std::vector<float> R((size_t)std::min(P, (int)XS_SCORE_MAX_POSES) * 9), t(R.size() / 3);
    for (int p0 = 0; p0 < P; p0 += XS_SCORE_MAX_POSES) {
        const int n = std::min(P - p0, (int)XS_SCORE_MAX_POSES);
        for (int i = 0; i < n; ++i) pack_real_pose(inverse(camera2volume[p0 + i]), &R[(size_t)i * 9], &t[(size_t)i * 3]);   // (newton_seeded_poses' real parts)
        check_rc(xs_tsdf_score_poses_band(n, reloc_.score_depth.ptr(), reloc_.score_depth.step(), rows, cols, &kinect_intrinsic.fx, voxel_size, R.data(), t.data(),
                                          tsdf_volume_d_ptr->getTsdfTruncDist(), &reloc_.band, reloc_.score_ws.ptr(), reloc_.score_sums.ptr(), st), "ScorePosesBand");
        fetch_sums(reloc_.score_sums.ptr(), (size_t)n * 2, out2xP + 2 * (size_t)p0);
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
    report[6] = (double)reloc_.band.count;
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
