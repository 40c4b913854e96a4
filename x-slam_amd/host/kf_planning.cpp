// kf_planning.cpp — where could the camera go, and what would it see there: the observation grid and the view scores, the clearance field
// and reachability, travel cost and paths, frontier clusters and the views proposed from them (DESIGN.md sections 4.18 to 4.21).  Each derived map is cached under the key it was built with.  None of it runs during tracking.
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

// What a Next... call returns when the calls it is made of did not return 1.  Its own -1 is "no pose qualifies", so their -1 (bad arguments)
// becomes -3 and their 0 (no volume) -1; -2 (sharded) stays.
static int next_view_error(int rc) { return rc == -1 ? -3 : (rc == 0 ? -1 : rc); }

int KinectFusionReconstruction::NextBestView(const Matrix4cf *camera2volume, int P, const xs_view_opts *opts, int min_weight, unsigned min_hits,
                                             unsigned *out4xP) {
    std::vector<unsigned> own;
    if (!out4xP && P > 0) { own.resize((size_t)P * 4); out4xP = own.data(); }
    const int rc = ScoreViews(camera2volume, P, opts, min_weight, out4xP);
    if (rc <= 0) return next_view_error(rc);
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
    reach_forget();   // (the flood was over another field)
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

// The checks of Reachable's start and body, then the field, the passable words, the snapped seed and the flood, each from its cache when its
// key holds.  1 when plan_.reach is in step with the arguments, otherwise what Reachable returns.
int KinectFusionReconstruction::ReachPrepare(const Matrix4cf *start, float radius_m, int snap_vox, int unknown_blocks, int min_weight) {
    if (shard_count > 1) return -2;   // connectivity is not additive over the ranks' z-slabs
    int r2 = 0, R = 0;
    if (snap_vox < 0 || snap_vox > XS_REACH_MAX_SNAP || (unknown_blocks != 0 && unknown_blocks != 1) || !reach_radius(radius_m, voxel_size, r2, R)) return -1;
    if (!tsdf_volume_d_ptr) return 0;
    const int mw = min_weight < 1 ? 1 : min_weight;
    if (!ClearancePrepare(R, unknown_blocks, mw)) return -1;
    hipStream_t st = current_stream();
    const int *res = res3();
    const size_t bytes = xs_reach_bytes(res);
    if (bytes == 0) return -1;
    if (plan_.reach.size() < bytes) { plan_.reach.create(bytes); reach_forget(); }
    const unsigned short *field = reinterpret_cast<const unsigned short *>(plan_.clear_field.ptr());
    ReachKey key{plan_.clear_key, r2, {-1, -1, -1}};
    // the passable words (those of the last flood, if it was over this field at this r2), and the start snapped over them
    if (!(plan_.reach_key.field == key.field) || plan_.reach_key.r2 != r2) {
        reach_forget();
        check_rc(xs_reach_passable(plan_.view_grid.ptr(), field, res, r2, plan_.reach.ptr(), st), "ReachPassable");
    }
    float p[3];
    pack_real_pose(start ? *start : getCamera2Volume(), nullptr, p);
    unsigned char found = 0;
    if (ReachQuery(p, 1, 1, snap_vox, &found, nullptr, key.seed) < 0) return -1;
    if (!found) key.seed[0] = key.seed[1] = key.seed[2] = -1;   // (outside the volume as a seed: contributes nothing, and nothing is reached)
    if (!(plan_.reach_key == key)) {
        reach_forget();
        check_rc(xs_reach_flood(plan_.view_grid.ptr(), field, res, r2, key.seed, 1, plan_.reach.ptr(), nullptr, st), "ReachFlood");
        plan_.reach_key = key;
    }
    return 1;
}

int KinectFusionReconstruction::Reachable(const Matrix4cf *start, float radius_m, int snap_vox, int unknown_blocks, int min_weight, int P,
                                          const Matrix4cf *camera2volume, unsigned char *reachable, unsigned short *clear2) {
    if (shard_count > 1) return -2;
    if (P < 0 || (P > 0 && (!camera2volume || !reachable || !clear2))) return -1;
    const int rc = ReachPrepare(start, radius_m, snap_vox, unknown_blocks, min_weight);
    if (rc != 1 || P == 0) return rc;
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
    if (rc <= 0) return next_view_error(rc);
    return next_reachable_view(out4xP, reachable, P, min_hits);
}

// ---- travel cost and shortest collision-free path to a candidate view ----
// The travel field follows the flood: built over plan_.reach from the flood's own seed, rebuilt when the flood's key or the limit differ.
bool KinectFusionReconstruction::TravelPrepare(int limit) {
    const TravelKey key{plan_.reach_key, limit};
    const size_t bytes = xs_travel_bytes(res3());
    if (bytes == 0) return false;
    if (plan_.travel.size() < bytes) { plan_.travel.create(bytes); plan_.travel_key = TravelKey{}; }
    if (plan_.travel_ws.size() < xs_travel_workspace_bytes()) plan_.travel_ws.create(xs_travel_workspace_bytes());
    if (plan_.travel_key == key) return true;
    plan_.travel_key = TravelKey{};
    check_rc(xs_travel_build(plan_.reach.ptr(), res3(), key.reach.seed, 1, limit, reinterpret_cast<unsigned short *>(plan_.travel.ptr()), plan_.travel_ws.ptr(),
                             nullptr, current_stream()), "TravelBuild");
    plan_.travel_key = key;
    return true;
}

int KinectFusionReconstruction::Travel(const Matrix4cf *start, float radius_m, int snap_vox, int unknown_blocks, int min_weight, float max_travel_m, int P,
                                       const Matrix4cf *camera2volume, unsigned char *reachable, unsigned short *clear2, unsigned short *travel3) {
    if (shard_count > 1) return -2;   // a path is not additive over the ranks' z-slabs
    if (P < 0 || (P > 0 && (!camera2volume || !reachable || !clear2 || !travel3)) || std::isnan(max_travel_m)) return -1;
    const int rc = ReachPrepare(start, radius_m, snap_vox, unknown_blocks, min_weight);
    if (rc != 1) return rc;
    if (!TravelPrepare(travel_limit(max_travel_m, voxel_size))) return -1;
    if (P == 0) return 1;
    std::vector<float> pts((size_t)P * 3);
    std::vector<int> voxel((size_t)P * 3);
    for (int i = 0; i < P; ++i) pack_real_pose(camera2volume[i], nullptr, &pts[(size_t)i * 3]);
    if (ReachQuery(pts.data(), P, 0, 0, reachable, clear2, voxel.data()) < 0) return -1;
    // the answering voxels ((-1, -1, -1) where not reached: NONE) through xs_travel_query, in chunks of 4096
    enum { CHUNK = 4096, VOXEL = 0, COST = CHUNK * 12, BYTES = COST + CHUNK * 2 };
    if (plan_.travel_io.size() < (size_t)BYTES) plan_.travel_io.create(BYTES);
    hipStream_t st = current_stream();
    unsigned char *io = plan_.travel_io.ptr();
    for (int p0 = 0; p0 < P; p0 += CHUNK) {
        const int m = std::min(P - p0, (int)CHUNK);
        hipSafeCall(hipMemcpyAsync(io + VOXEL, voxel.data() + 3 * (size_t)p0, (size_t)m * 12, hipMemcpyHostToDevice, st));
        check_rc(xs_travel_query(m, reinterpret_cast<const int *>(io + VOXEL), res3(), reinterpret_cast<const unsigned short *>(plan_.travel.ptr()),
                                 reinterpret_cast<unsigned short *>(io + COST), st), "TravelQuery");
        hipSafeCall(hipMemcpyAsync(travel3 + p0, io + COST, (size_t)m * 2, hipMemcpyDeviceToHost, st));
        hipSafeCall(hipStreamSynchronize(st));   // (the staging area is free again)
    }
    return 1;
}

int KinectFusionReconstruction::PathTo(const Matrix4cf *start, float radius_m, int snap_vox, int unknown_blocks, int min_weight, float max_travel_m,
                                       const Matrix4cf &target, int capacity, int *voxels3, float *points3, int *needed_out) {
    if (shard_count > 1) return -2;
    if (capacity < 1 || std::isnan(max_travel_m)) return -1;
    const int rc = ReachPrepare(start, radius_m, snap_vox, unknown_blocks, min_weight);
    if (rc != 1) return rc;
    const int limit = travel_limit(max_travel_m, voxel_size);
    if (!TravelPrepare(limit)) return -1;
    float p[3];
    int voxel[3];
    unsigned char found = 0;
    pack_real_pose(target, nullptr, p);
    if (ReachQuery(p, 1, 0, 0, &found, nullptr, voxel) < 0) return -1;
    if (!found) return 0;
    // the target, then the length, then the path's voxels in the kernel's order (target first)
    const size_t bytes = 16 + (size_t)capacity * 12;
    if (plan_.path_io.size() < bytes) plan_.path_io.create(bytes);
    hipStream_t st = current_stream();
    int *io = reinterpret_cast<int *>(plan_.path_io.ptr());
    hipSafeCall(hipMemcpyAsync(io, voxel, 12, hipMemcpyHostToDevice, st));
    check_rc(xs_travel_path(1, io, res3(), plan_.reach.ptr(), reinterpret_cast<const unsigned short *>(plan_.travel.ptr()), limit, capacity, io + 4, io + 3, st),
             "TravelPath");
    int len = 0;
    hipSafeCall(hipMemcpyAsync(&len, io + 3, sizeof(int), hipMemcpyDeviceToHost, st));
    hipSafeCall(hipStreamSynchronize(st));
    if (needed_out) *needed_out = len;
    if (len > capacity) return -4;
    if (len < 1) return 0;   // (beyond the limit)
    std::vector<int> path((size_t)len * 3);
    hipSafeCall(hipMemcpyAsync(path.data(), io + 4, (size_t)len * 12, hipMemcpyDeviceToHost, st));
    hipSafeCall(hipStreamSynchronize(st));
    for (int s = 0; s < len; ++s)   // start first, target last
        for (int c = 0; c < 3; ++c) {
            const int v = path[3 * (size_t)(len - 1 - s) + (size_t)c];
            if (voxels3) voxels3[3 * (size_t)s + (size_t)c] = v;
            if (points3) points3[3 * (size_t)s + (size_t)c] = ((float)v + 0.5f) * voxel_size;
        }
    return len;
}

int KinectFusionReconstruction::NextViewByTravel(const Matrix4cf *camera2volume, int P, const xs_view_opts *opts, int min_weight, unsigned min_hits,
                                                 unsigned *out4xP, float radius_m, int snap_vox, int unknown_blocks, float max_travel_m, float bias_m,
                                                 unsigned short *travel3_out) {
    if (!(bias_m >= 0.f) || !std::isfinite(bias_m)) return shard_count > 1 ? -2 : -3;
    std::vector<unsigned> own;
    std::vector<unsigned short> own_travel, clear2((size_t)(P > 0 ? P : 0));
    std::vector<unsigned char> flags((size_t)(P > 0 ? P : 0));
    if (!out4xP && P > 0) { own.resize((size_t)P * 4); out4xP = own.data(); }
    if (!travel3_out && P > 0) { own_travel.resize((size_t)P); travel3_out = own_travel.data(); }
    int rc = Travel(nullptr, radius_m, snap_vox, unknown_blocks, min_weight, max_travel_m, P, camera2volume, flags.data(), clear2.data(), travel3_out);
    if (rc == 1) rc = ScoreViews(camera2volume, P, opts, min_weight, out4xP);
    if (rc <= 0) return next_view_error(rc);
    return next_view_by_travel(out4xP, travel3_out, P, min_hits, travel_bias(bias_m, voxel_size));
}

// ---- frontier clusters and the views proposed from them ----
// Mask, labels and the records of every cluster (on the host) follow the grid, the grid the volume.  False when the resolution has no labels.
bool KinectFusionReconstruction::FrontierPrepare(int cell, int min_weight) {
    const int mw = min_weight < 1 ? 1 : min_weight;
    const int *res = res3();
    const size_t mask_bytes = xs_frontier_mask_bytes(res), label_bytes = xs_frontier_label_bytes(res);
    if (mask_bytes == 0 || label_bytes == 0 || !ViewGridPrepare(mw)) return false;
    const FrontierKey key{plan_.grid_key, cell};
    if (plan_.frontier_mask.size() < mask_bytes) { plan_.frontier_mask.create(mask_bytes); plan_.frontier_key = FrontierKey{}; }
    if (plan_.frontier_labels.size() < label_bytes) { plan_.frontier_labels.create(label_bytes); plan_.frontier_key = FrontierKey{}; }
    if (plan_.frontier_key == key) return true;
    plan_.frontier_key = FrontierKey{};
    hipStream_t st = current_stream();
    unsigned *labels = reinterpret_cast<unsigned *>(plan_.frontier_labels.ptr());
    int capacity = plan_.frontier_records_d.size() > 1 ? (int)((plan_.frontier_records_d.size() - 1) / FRONTIER_RECORD_WORDS) : 4096;
    auto room_for = [&](int cap) {   // the records with the count behind them, and the workspace that goes with that capacity
        if (plan_.frontier_records_d.size() < (size_t)cap * FRONTIER_RECORD_WORDS + 1) plan_.frontier_records_d.create((size_t)cap * FRONTIER_RECORD_WORDS + 1);
        const size_t ws = xs_frontier_workspace_bytes(res, cap);
        if (plan_.frontier_ws.size() < ws) plan_.frontier_ws.create(ws);
    };
    room_for(capacity);
    check_rc(xs_frontier_mask(plan_.view_grid.ptr(), res, plan_.frontier_mask.ptr(), st), "FrontierMask");
    check_rc(xs_frontier_label(plan_.frontier_mask.ptr(), res, cell, labels, plan_.frontier_ws.ptr(), nullptr, st), "FrontierLabel");
    unsigned count = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {   // (the second with room for the count the first returned)
        unsigned long long *rec = plan_.frontier_records_d.ptr();
        check_rc(xs_frontier_clusters(plan_.frontier_mask.ptr(), labels, res, capacity, rec, reinterpret_cast<unsigned *>(rec + (size_t)capacity * FRONTIER_RECORD_WORDS),
                                      &count, plan_.frontier_ws.ptr(), st), "FrontierClusters");
        if (count <= (unsigned)capacity) break;
        if (count > 0x7fffffffu / 2u) return false;
        capacity = (int)count;
        room_for(capacity);
    }
    plan_.frontier_records.assign((size_t)count * FRONTIER_RECORD_WORDS, 0ull);
    if (count) {
        hipSafeCall(hipMemcpyAsync(plan_.frontier_records.data(), plan_.frontier_records_d.ptr(), plan_.frontier_records.size() * sizeof(unsigned long long),
                                   hipMemcpyDeviceToHost, st));
        hipSafeCall(hipStreamSynchronize(st));
    }
    plan_.frontier_key = key;
    return true;
}

int KinectFusionReconstruction::Frontiers(int cell, unsigned long long min_size, int min_weight, int capacity, unsigned long long *records8, int *count_out) {
    if (shard_count > 1) return -2;   // a cluster is not additive over the ranks' z-slabs
    if (!count_out || capacity < 0 || (capacity > 0 && !records8) || !frontier_cell_valid(cell)) return -1;
    if (!tsdf_volume_d_ptr) return 0;
    if (!FrontierPrepare(cell, min_weight)) return -1;
    const int n = (int)(plan_.frontier_records.size() / FRONTIER_RECORD_WORDS);
    std::vector<int> keep((size_t)n);
    const int m = frontier_select(plan_.frontier_records.data(), n, min_size, keep.data());
    *count_out = m;
    if (m > capacity) return -4;
    for (int i = 0; i < m; ++i)
        std::memcpy(records8 + (size_t)i * FRONTIER_RECORD_WORDS, plan_.frontier_records.data() + (size_t)keep[(size_t)i] * FRONTIER_RECORD_WORDS,
                    FRONTIER_RECORD_WORDS * sizeof(unsigned long long));
    return 1;
}

int KinectFusionReconstruction::ProposeViews(float radius_m, int start_snap_vox, int unknown_blocks, int min_weight, int cell, unsigned long long min_size,
                                             int views_per_cluster, float standoff_m, int snap_vox, int capacity, Matrix4cf *c2v_out, int *cluster_out,
                                             int *count_out) {
    if (shard_count > 1) return -2;   // neither connectivity nor a cluster is additive over the ranks' z-slabs
    if (!count_out || capacity < 0 || (capacity > 0 && (!c2v_out || !cluster_out)) || !frontier_cell_valid(cell) || views_per_cluster < 1 ||
        views_per_cluster > 4096 || !(standoff_m >= 0.f) || !std::isfinite(standoff_m) || snap_vox < 0 || snap_vox > XS_REACH_MAX_SNAP)
        return -1;
    const int rc = ReachPrepare(nullptr, radius_m, start_snap_vox, unknown_blocks, min_weight);
    if (rc != 1) return rc;
    if (!FrontierPrepare(cell, min_weight)) return -1;
    const int n = (int)(plan_.frontier_records.size() / FRONTIER_RECORD_WORDS), V = views_per_cluster;
    std::vector<int> keep((size_t)n);
    const int m = frontier_select(plan_.frontier_records.data(), n, min_size, keep.data());
    *count_out = 0;
    if (m == 0) return 1;
    // the standpoints of every kept cluster through one query over the reached words
    std::vector<float> centroid((size_t)m * 3), pts((size_t)m * (size_t)V * 3);
    for (int i = 0; i < m; ++i) {
        frontier_centroid(plan_.frontier_records.data() + (size_t)keep[(size_t)i] * FRONTIER_RECORD_WORDS, voxel_size, &centroid[(size_t)i * 3]);
        for (int j = 0; j < V; ++j) frontier_standpoint(&centroid[(size_t)i * 3], standoff_m, j, &pts[((size_t)i * (size_t)V + (size_t)j) * 3]);
    }
    std::vector<unsigned char> found((size_t)m * (size_t)V);
    std::vector<int> voxel((size_t)m * (size_t)V * 3);
    if (ReachQuery(pts.data(), m * V, 0, snap_vox, found.data(), nullptr, voxel.data()) < 0) return -1;
    // the image-down hint: the current camera's y axis; its x axis where that is along the view
    const Matrix4cf cam = getCamera2Volume();
    const float down[3] = {cam.m[0][1].real(), cam.m[1][1].real(), cam.m[2][1].real()}, side[3] = {cam.m[0][0].real(), cam.m[1][0].real(), cam.m[2][0].real()};
    std::vector<Matrix4cf> poses;
    std::vector<int> cluster;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < V; ++j) {
            const size_t q = (size_t)i * (size_t)V + (size_t)j;
            if (!found[q]) continue;
            bool seen = false;   // (the same answering voxel for the same cluster)
            for (int k = 0; k < j && !seen; ++k) {
                const size_t e = (size_t)i * (size_t)V + (size_t)k;
                seen = found[e] && voxel[3 * e] == voxel[3 * q] && voxel[3 * e + 1] == voxel[3 * q + 1] && voxel[3 * e + 2] == voxel[3 * q + 2];
            }
            if (seen) continue;
            const float pos[3] = {voxel_centre(voxel[3 * q], voxel_size), voxel_centre(voxel[3 * q + 1], voxel_size), voxel_centre(voxel[3 * q + 2], voxel_size)};
            float R[9];
            if (!look_at(pos, &centroid[(size_t)i * 3], down, side, R)) continue;   // (the centroid itself: no direction to look in)
            Matrix4cf pose;
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c) pose.m[r][c] = hostComplex(r == c ? 1.f : 0.f, 0.f);
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) pose.m[r][c] = hostComplex(R[3 * r + c], 0.f);
                pose.m[r][3] = hostComplex(pos[r], 0.f);
            }
            poses.push_back(pose);
            cluster.push_back(i);
        }
    *count_out = (int)poses.size();
    if ((int)poses.size() > capacity) return -4;
    for (size_t p = 0; p < poses.size(); ++p) { c2v_out[p] = poses[p]; cluster_out[p] = cluster[p]; }
    return 1;
}
