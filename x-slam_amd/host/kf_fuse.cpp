// kf_fuse.cpp — a registered point cloud fused into the map (xs_tsdf_fuse_points_accumulate and xs_tsdf_fuse_points_fold
// in include/xslam_amd.h: the contract; fuse_host.hpp: the host's side of it).  What IntegrateFrame does with a pinhole depth image, this does
// with points and a sensor origin; afterwards everything derived from the volume follows it, as after ReintegrateFrames.  None of it runs
// during tracking.
#include "kf_internal.hpp"
#include "fuse_host.hpp"

using namespace xs_host;

int KinectFusionReconstruction::FusePoints(const float *points, long long n, int on_device, const double *T16, const float *origin3, float min_range,
                                           float max_range, int carve, int weight, unsigned long long counts5[5]) {
    if (shard_count > 1) return -2;   // a ray crosses the ranks' z-slabs, and each rank would need the whole cloud: not built
    if (!tsdf_volume_d_ptr) return 0;
    if (n < 1 || !points || !origin3) return -1;
    float xform[12];
    if (T16 && !fuse_xform12(T16, xform)) return -1;
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value(), grad = tsdf_volume_d_ptr->grad();
    DeviceArray2D<int> weights = tsdf_volume_d_ptr->weight();
    if (value.step() != weights.step() || value.step() != grad.step()) return -1;
    const float tranc = tsdf_volume_d_ptr->getTsdfTruncDist();
    xs_fuse_opts o;
    o.struct_bytes = sizeof(o);
    o.min_range = min_range; o.max_range = max_range; o.carve = carve ? 1 : 0;
    // everything the two calls would refuse, before anything is allocated or launched (the pointers that are not there yet stand in as `this`)
    long long first = 0, count = 0;
    fuse_run(n, 0, &first, &count);
    if (fuse_validate_accumulate(count, points, T16 ? xform : nullptr, origin3, res3(), voxel_size, tranc, true, o.struct_bytes, (unsigned)sizeof(o), min_range,
                                 max_range, this, this) != FUSE_ACCEPTED)
        return -1;
    if (fuse_validate_fold(true, value.step(), res3(), 0, res3()[2], this, weight, max_integration_weight) != FUSE_ACCEPTED) return -1;
    const size_t words = fuse_accumulator_bytes(res3()) / sizeof(unsigned long long);
    hipStream_t st = current_stream();
    drain_device();
    if (fuse_acc_.size() != words) {   // first use, after ReleaseFuseScratch, or another volume: zeroed once; every fold leaves it zero
        fuse_acc_.create(words);
        hipSafeCall(hipMemsetAsync(fuse_acc_.ptr(), 0, words * sizeof(unsigned long long), st));
    }
    DeviceArray<unsigned long long> counts;
    counts.create(5);
    hipSafeCall(hipMemsetAsync(counts.ptr(), 0, 5 * sizeof(unsigned long long), st));
    DeviceArray<float> points_d;   // a run of host points at a time
    if (!(on_device & 1)) points_d.create(3 * (size_t)count);
    for (long long r = 0; fuse_run(n, r, &first, &count); ++r) {
        const float *run = points + 3 * (size_t)first;
        if (!(on_device & 1)) {
            hipSafeCall(hipMemcpyAsync(points_d.ptr(), run, 3 * (size_t)count * sizeof(float), hipMemcpyHostToDevice, st));
            run = points_d.ptr();
        }
        check_rc(xs_tsdf_fuse_points_accumulate(count, run, T16 ? xform : nullptr, origin3, res3(), voxel_size, tranc, &o, fuse_acc_.ptr(), counts.ptr(), st),
                 "fuse accumulate");
        check_rc(xs_tsdf_fuse_points_fold(value.ptr(0), weights.ptr(0), grad.ptr(0), value.step(), res3(), 0, res3()[2], fuse_acc_.ptr(), weight,
                                          max_integration_weight, counts.ptr() + 4, st), "fuse fold");
    }
    volume_written_off_path();
    if (counts5) hipSafeCall(hipMemcpy(counts5, counts.ptr(), 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 1;
}
