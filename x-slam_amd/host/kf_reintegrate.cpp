// kf_reintegrate.cpp — taking fused frames out of the volume and fusing them again at corrected poses: the orchestrator's
// side of xs_tsdf_reintegrate.  What IntegrateFrame does for the frame in hand, this does for frames of the past, with a sign; afterwards everything
// derived from the volume follows it, as after MergeVolume.  None of it runs during tracking.
#include "kf_internal.hpp"
#include <cmath>
#include <map>

using namespace xs_host;

static bool finite_pose(const Matrix4cf &m) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            if (!std::isfinite(m.m[r][c].real()) || !std::isfinite(m.m[r][c].imag())) return false;
    return true;
}

int KinectFusionReconstruction::ReintegrateFrames(int n, const DeviceArray2D<ushort> *depths, const Matrix4cf *c2v_old, const Matrix4cf *c2v_new, const int *mode,
                                                  const int *frame_index, unsigned long long counts4[4]) {
    if (shard_count > 1) return -2;   // (the kernel takes a plane range; the halo planes and the collective of the counts are not built)
    if (!tsdf_volume_d_ptr) return 0;
    if (n < 1 || !depths || !mode) return -1;
    for (int i = 0; i < n; ++i) {
        if (mode[i] < 1 || mode[i] > 3 || !depths[i].ptr()) return -1;
        if ((mode[i] & 1) && (!c2v_old || !finite_pose(c2v_old[i]))) return -1;
        if ((mode[i] & 2) && (!c2v_new || !finite_pose(c2v_new[i]))) return -1;
        if (frame_index && frame_index[i] >= 0 && (frame_index[i] >= (int)world2camera_record.size() || !(mode[i] & 2))) return -1;
    }
    drain_device();
    hipStream_t st = current_stream();
    const int rows = depth_height, cols = depth_width;
    // each distinct image scaled once, into buffers of the call's own (depthRawScaled_d belongs to the frame path)
    std::map<const void *, int> slot_of;
    std::vector<DeviceArray2D<float>> scaled;
    std::vector<int> slot((size_t)n);
    for (int i = 0; i < n; ++i) {
        auto it = slot_of.find(depths[i].ptr());
        if (it == slot_of.end()) {
            it = slot_of.emplace(depths[i].ptr(), (int)scaled.size()).first;
            scaled.emplace_back();
            scaled.back().create(rows, cols);
            check_rc(xs_scale_depth(depths[i].ptr(), depths[i].step(), rows, cols, scaled.back().ptr(), scaled.back().step(), st), "scaleDepth");
        }
        slot[(size_t)i] = it->second;
    }
    const size_t scaled_step = scaled[0].step();
    for (auto &s : scaled)
        if (s.step() != scaled_step) return -1;   // (one pitch per launch; the allocator gives equal images equal pitches)
    // the op list: the pose algebra of IntegrateFrame
    std::vector<xs_reintegrate_op> ops;
    auto push = [&](int sign, const Matrix4cf &c2v, int i) {
        Matrix4cf v2c = inverse(c2v);
        Matrix3frm Rv2c = GetRotation(v2c);
        Vector3cf tv2c = GetTranslation(v2c);
        xs_reintegrate_op o;
        o.sign = sign;
        o.depth_scaled = scaled[(size_t)slot[(size_t)i]].ptr();
        std::memcpy(o.Rv2c18, &device_cast<MatS33>(Rv2c).data[0].x.re, sizeof(o.Rv2c18));
        std::memcpy(o.tv2c6, &device_cast<devComplex3>(tv2c).x.re, sizeof(o.tv2c6));
        ops.push_back(o);
    };
    for (int i = 0; i < n; ++i) {
        if (mode[i] & 1) push(-1, c2v_old[i], i);
        if (mode[i] & 2) push(+1, c2v_new[i], i);
    }
    DeviceArray<unsigned long long> count;
    count.create(4);
    hipSafeCall(hipMemsetAsync(count.ptr(), 0, 4 * sizeof(unsigned long long), st));
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value(), grad = tsdf_volume_d_ptr->grad();
    DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    for (size_t at = 0; at < ops.size(); at += XS_REINTEGRATE_MAX_OPS) {
        const int m = (int)std::min<size_t>(XS_REINTEGRATE_MAX_OPS, ops.size() - at);
        check_rc(xs_tsdf_reintegrate(m, ops.data() + at, scaled_step, rows, cols, &kinect_intrinsic.fx, max_integration_weight, res3(), voxel_size,
                                     tsdf_volume_d_ptr->getTsdfTruncDist(), biInterpolate_threshold, value.ptr(0), weight.ptr(0), grad.ptr(0), value.step(), 0,
                                     res3()[2], count.ptr(), 0u, st), "reintegrate");
    }
    // the record, where asked for: c2v = world2volume * c2w
    if (frame_index) {
        const Matrix4cf volume2world = inverse(world2volume);
        for (int i = 0; i < n; ++i) {
            if (frame_index[i] < 0) continue;
            world2camera_record[(size_t)frame_index[i]] = inverse(volume2world * c2v_new[i]);
            if (frame_index[i] + 1 == (int)world2camera_record.size()) world2camera = world2camera_record.back();
        }
    }
    volume_written_off_path();
    if (counts4) hipSafeCall(hipMemcpy(counts4, count.ptr(), 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 1;
}
