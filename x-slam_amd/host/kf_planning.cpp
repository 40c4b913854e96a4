// kf_planning.cpp — where could the camera go, and what would it see there: the observation grid and the view scores, the clearance field
// and reachability (DESIGN.md sections 4.18, 4.19).  Each derived map is cached under the key it was built with.  None of it runs during tracking.
#include "kf_internal.hpp"
#include "view_host.hpp"

using namespace xs_host;

// ---- candidate views against the map in one launch, and the next best view ----
// The observation grid follows the volume the way BandIndexPrepare's index does.  False when the resolution has no grid.
bool KinectFusionReconstruction::ViewGridPrepare(int min_weight) {
    const int mw = min_weight < 1 ? 1 : min_weight;
    const GridKey key{volume_generation, mw};
    const size_t bytes = xs_view_grid_bytes(res3());
    if (bytes == 0) return false;
    if (plan_.view_grid.size() < bytes) { plan_.view_grid.create(bytes); plan_.grid_key = GridKey{}; }
    if (plan_.grid_key == key) return true;
    const DeviceArray2D<float> value = tsdf_volume_d_ptr->value();
    const DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    if (value.step() != weight.step()) { std::cout << "error::KinectFusionReconstruction, observation grid: value and weight pitches differ" << std::endl; exit(-1); }
    check_rc(xs_view_grid_build(value.ptr(), weight.ptr(), value.step(), res3(), mw, plan_.view_grid.ptr(), current_stream()), "ViewGridBuild");
    plan_.grid_key = key;
    return true;
}

int KinectFusionReconstruction::ScoreViews(const Matrix4cf *camera2volume, int P, const xs_view_opts *opts, int min_weight, unsigned *out4xP) {
    if (shard_count > 1) return -2;   // a ray's occlusion is not additive over the ranks' z-slabs
    if (P < 0 || (P > 0 && (!camera2volume || !out4xP))) return -1;
    if (!tsdf_volume_d_ptr) return 0;
    if (P == 0) return 1;
    hipStream_t st = current_stream();
    if (!ViewGridPrepare(min_weight)) return -1;
    if (plan_.view_counts.size() < (size_t)XS_VIEW_MAX_POSES * 4) plan_.view_counts.create((size_t)XS_VIEW_MAX_POSES * 4);
    std::vector<float> R((size_t)std::min(P, (int)XS_VIEW_MAX_POSES) * 9), t(R.size() / 3);
    for (int p0 = 0; p0 < P; p0 += XS_VIEW_MAX_POSES) {
        const int n = std::min(P - p0, (int)XS_VIEW_MAX_POSES);
        for (int i = 0; i < n; ++i) pack_real_pose(camera2volume[p0 + i], &R[(size_t)i * 9], &t[(size_t)i * 3]);
        const int rc = xs_score_views(n, R.data(), t.data(), &kinect_intrinsic.fx, depth_height, depth_width, res3(), voxel_size, plan_.view_grid.ptr(), opts,
                                      plan_.view_counts.ptr(), st);
        if (rc == (int)hipErrorInvalidValue) return -1;   // the options: nothing was launched
        check_rc(rc, "ScoreViews");
        hipSafeCall(hipMemcpyAsync(out4xP + 4 * (size_t)p0, plan_.view_counts.ptr(), (size_t)n * 4 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
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
    const ClearKey key{GridKey{volume_generation, mw}, R, unknown_blocks};
    const size_t bytes = xs_clearance_bytes(res3()), ws = xs_clearance_workspace_bytes(res3());
    if (bytes == 0 || !ViewGridPrepare(mw)) return false;
    if (plan_.clear_field.size() < bytes) { plan_.clear_field.create(bytes); plan_.clear_key = ClearKey{}; }
    if (plan_.clear_ws.size() < ws) plan_.clear_ws.create(ws);
    if (plan_.clear_key == key) return true;
    check_rc(xs_clearance_build(plan_.view_grid.ptr(), res3(), R, unknown_blocks, plan_.clear_ws.ptr(), reinterpret_cast<unsigned short *>(plan_.clear_field.ptr()),
                                current_stream()), "ClearanceBuild");
    plan_.clear_key = key;
    plan_.reach_key = ReachKey{};   // (the flood was over another field)
    return true;
}

int KinectFusionReconstruction::ClearanceField(int max_radius_vox, int unknown_blocks, int min_weight, unsigned short *host_out) {
    if (shard_count > 1) return -2;   // a distance is not additive over the ranks' z-slabs
    if (!host_out || max_radius_vox < 1 || max_radius_vox > XS_CLEARANCE_MAX_RADIUS || (unknown_blocks != 0 && unknown_blocks != 1)) return -1;
    if (!tsdf_volume_d_ptr) return 0;
    if (!ClearancePrepare(max_radius_vox, unknown_blocks, min_weight)) return -1;
    hipStream_t st = current_stream();
    hipSafeCall(hipMemcpyAsync(host_out, plan_.clear_field.ptr(), xs_clearance_bytes(res3()), hipMemcpyDeviceToHost, st));
    hipSafeCall(hipStreamSynchronize(st));
    return 1;
}

// n points through xs_reach_query against plan_.reach and plan_.clear_field, in chunks of 4096; the answers on the host when the call returns
int KinectFusionReconstruction::ReachQuery(const float *points3xN, int n, int over_passable, int snap, unsigned char *reachable, unsigned short *clear2,
                                           int *voxel) {
    enum { CHUNK = 4096, POINTS = 0, VOXEL = CHUNK * 12, CLEAR2 = VOXEL + CHUNK * 12, FLAGS = CLEAR2 + CHUNK * 2, BYTES = FLAGS + CHUNK };
    if (plan_.reach_io.size() < (size_t)BYTES) plan_.reach_io.create(BYTES);
    hipStream_t st = current_stream();
    unsigned char *io = plan_.reach_io.ptr();
    for (int p0 = 0; p0 < n; p0 += CHUNK) {
        const int m = std::min(n - p0, (int)CHUNK);
        hipSafeCall(hipMemcpyAsync(io + POINTS, points3xN + 3 * (size_t)p0, (size_t)m * 12, hipMemcpyHostToDevice, st));
        const int rc = xs_reach_query(m, reinterpret_cast<const float *>(io + POINTS), res3(), voxel_size, plan_.reach.ptr(), over_passable,
                                      reinterpret_cast<const unsigned short *>(plan_.clear_field.ptr()), snap, io + FLAGS, reinterpret_cast<unsigned short *>(io + CLEAR2),
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
    const int *res = res3();
    const size_t bytes = xs_reach_bytes(res);
    if (bytes == 0) return -1;
    if (plan_.reach.size() < bytes) { plan_.reach.create(bytes); plan_.reach_key = ReachKey{}; }
    const unsigned short *field = reinterpret_cast<const unsigned short *>(plan_.clear_field.ptr());
    ReachKey key{plan_.clear_key, r2, {-1, -1, -1}};
    // the passable words (those of the last flood, if it was over this field at this r2), and the start snapped over them
    if (!(plan_.reach_key.field == key.field) || plan_.reach_key.r2 != r2) {
        plan_.reach_key = ReachKey{};
        check_rc(xs_reach_passable(plan_.view_grid.ptr(), field, res, r2, plan_.reach.ptr(), st), "ReachPassable");
    }
    float p[3];
    pack_real_pose(start ? *start : getCamera2Volume(), nullptr, p);
    unsigned char found = 0;
    if (ReachQuery(p, 1, 1, snap_vox, &found, nullptr, key.seed) < 0) return -1;
    if (!found) key.seed[0] = key.seed[1] = key.seed[2] = -1;   // (outside the volume as a seed: contributes nothing, and nothing is reached)
    if (!(plan_.reach_key == key)) {
        plan_.reach_key = ReachKey{};
        check_rc(xs_reach_flood(plan_.view_grid.ptr(), field, res, r2, key.seed, 1, plan_.reach.ptr(), nullptr, st), "ReachFlood");
        plan_.reach_key = key;
    }
    if (P == 0) return 1;
    std::vector<float> pts((size_t)P * 3);
    for (int i = 0; i < P; ++i) pack_real_pose(camera2volume[i], nullptr, &pts[(size_t)i * 3]);
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
