// kf_sample.cpp — asking a map: the signed distance, its gradient and whether the place was seen, at points the caller supplies or at the pixels of
// a depth frame, of this map or of a second one (xs_tsdf_sample_points and xs_tsdf_sample_depth in include/xslam_amd.h:
// the contract; sample_host.hpp: the host's side of it).  Nothing of any map or cache is modified, and none of it runs during tracking.
#include "kf_internal.hpp"
#include "sample_host.hpp"

using namespace xs_host;

namespace {
using Out = KinectFusionReconstruction::SampleOutputs;
bool any_output(const Out &o) { return o.status || o.value || o.dvalue || o.gradient || o.counts; }

// The outputs of one launch over `count` points: the caller's own pointers when they are device memory, otherwise device buffers of the call's
// own that fetch() copies to the caller's host arrays.
struct Staged {
    DeviceArray<unsigned char> status;
    DeviceArray<float> value, dvalue, gradient;
    DeviceArray<unsigned long long> counts;
    Out dev;
    Staged(const Out &out, size_t count, bool on_device) : dev(out) {
        if (on_device) return;
        if (out.status) { status.create(count); dev.status = status.ptr(); }
        if (out.value) { value.create(count); dev.value = value.ptr(); }
        if (out.dvalue) { dvalue.create(count); dev.dvalue = dvalue.ptr(); }
        if (out.gradient) { gradient.create(3 * count); dev.gradient = gradient.ptr(); }
        if (out.counts) { counts.create(4); dev.counts = counts.ptr(); }
    }
    void fetch(const Out &out, size_t count, bool on_device, hipStream_t st) const {
        if (on_device) return;
        if (out.status) hipSafeCall(hipMemcpyAsync(out.status, dev.status, count, hipMemcpyDeviceToHost, st));
        if (out.value) hipSafeCall(hipMemcpyAsync(out.value, dev.value, count * sizeof(float), hipMemcpyDeviceToHost, st));
        if (out.dvalue) hipSafeCall(hipMemcpyAsync(out.dvalue, dev.dvalue, count * sizeof(float), hipMemcpyDeviceToHost, st));
        if (out.gradient) hipSafeCall(hipMemcpyAsync(out.gradient, dev.gradient, 3 * count * sizeof(float), hipMemcpyDeviceToHost, st));
        if (out.counts) hipSafeCall(hipMemcpyAsync(out.counts, dev.counts, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    }
};
xs_sample_opts opts_of(int min_weight) {
    xs_sample_opts o;
    o.struct_bytes = sizeof(o);
    o.min_weight = min_weight;
    return o;
}
}  // namespace

int KinectFusionReconstruction::SampleVolume(const SecondMap &vol, const float *points, long long n, const double *T16, int min_weight, const SampleOutputs &out,
                                             int on_device) {
    if (n < 1 || n > SAMPLE_MAX_POINTS || !points || !any_output(out) || (out.dvalue && !vol.grad)) return -1;
    float xform[12];
    if (T16 && !sample_xform12(T16, xform)) return -1;
    const bool points_dev = on_device & 1, out_dev = on_device & 2;
    hipStream_t st = current_stream();
    drain_device();
    DeviceArray<float> points_d;
    if (!points_dev) {
        points_d.create(3 * (size_t)n);
        hipSafeCall(hipMemcpyAsync(points_d.ptr(), points, 3 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    }
    const Staged staged(out, (size_t)n, out_dev);
    const xs_sample_opts o = opts_of(min_weight);
    const int rc = xs_tsdf_sample_points(n, points_dev ? points : points_d.ptr(), T16 ? xform : nullptr, vol.value, vol.weight, vol.grad, vol.step, vol.res,
                                         vol.voxel_size, &o, staged.dev.status, staged.dev.value, staged.dev.dvalue, staged.dev.gradient, staged.dev.counts, st);
    if (rc == (int)hipErrorInvalidValue) return -1;   // the arguments: nothing was launched
    check_rc(rc, "SamplePoints");
    staged.fetch(out, (size_t)n, out_dev, st);
    hipSafeCall(hipStreamSynchronize(st));
    return 1;
}

int KinectFusionReconstruction::SamplePoints(const float *points, long long n, const double *T16, int min_weight, const SampleOutputs &out, int on_device) {
    if (shard_count > 1) return -2;   // a point's eight corners may straddle two ranks' z-slabs
    if (!tsdf_volume_d_ptr) return 0;
    const DeviceArray2D<float> value = tsdf_volume_d_ptr->value(), grad = tsdf_volume_d_ptr->grad();
    const DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    if (value.step() != weight.step() || (out.dvalue && value.step() != grad.step())) return -1;
    const SecondMap self{value.ptr(), weight.ptr(), out.dvalue ? grad.ptr() : nullptr, value.step(), {res3()[0], res3()[1], res3()[2]}, voxel_size,
                         tsdf_volume_d_ptr->getTsdfTruncDist()};
    return SampleVolume(self, points, n, T16, min_weight, out, on_device);
}

int KinectFusionReconstruction::SampleSecondMap(const SecondMap &src, const float *points, long long n, const double *T16, int min_weight, const SampleOutputs &out,
                                                int on_device) {
    if (shard_count > 1) return -2;
    if (!tsdf_volume_d_ptr) return 0;
    if (!takes_second_map(src, 1, out.dvalue != nullptr)) return -1;
    return SampleVolume(src, points, n, T16, min_weight, out, on_device);
}

int KinectFusionReconstruction::FrameResiduals(const unsigned short *depth, size_t depth_step, const float *c2v, int stride, const float *intr4, int rows, int cols,
                                               int min_weight, const SampleOutputs &out, int on_device) {
    if (shard_count > 1) return -2;
    if (!tsdf_volume_d_ptr) return 0;
    if (!depth || !c2v || (stride != 1 && stride != 2) || !any_output(out)) return -1;
    if (rows == 0 && cols == 0) { rows = depth_height; cols = depth_width; }
    if (rows < 1 || cols < 1 || rows > RENDER_MAX_IMAGE || cols > RENDER_MAX_IMAGE) return -1;
    const bool depth_dev = on_device & 1, out_dev = on_device & 2;
    if (depth_step == 0) depth_step = (size_t)cols * 2;
    if (depth_step % 2 != 0 || depth_step < (size_t)cols * 2) return -1;
    const DeviceArray2D<float> value = tsdf_volume_d_ptr->value(), grad = tsdf_volume_d_ptr->grad();
    const DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    if (value.step() != weight.step() || (out.dvalue && value.step() != grad.step())) return -1;
    float R[9], t[3];
    render_pose(c2v, stride, R, t);
    hipStream_t st = current_stream();
    drain_device();
    DeviceArray<unsigned short> depth_d;
    if (!depth_dev) {   // the host image's rows, packed
        depth_d.create((size_t)rows * (size_t)cols);
        hipSafeCall(hipMemcpy2DAsync(depth_d.ptr(), (size_t)cols * 2, depth, depth_step, (size_t)cols * 2, (size_t)rows, hipMemcpyHostToDevice, st));
    }
    const size_t count = (size_t)rows * (size_t)cols;
    const Staged staged(out, count, out_dev);
    const xs_sample_opts o = opts_of(min_weight);
    const int rc = xs_tsdf_sample_depth(depth_dev ? depth : depth_d.ptr(), depth_dev ? depth_step : (size_t)cols * 2, rows, cols, intr4 ? intr4 : &kinect_intrinsic.fx, R, t,
                                        value.ptr(), weight.ptr(), out.dvalue ? grad.ptr() : nullptr, value.step(), res3(), voxel_size, &o, staged.dev.status,
                                        staged.dev.value, staged.dev.dvalue, staged.dev.gradient, staged.dev.counts, st);
    if (rc == (int)hipErrorInvalidValue) return -1;
    check_rc(rc, "FrameResiduals");
    staged.fetch(out, count, out_dev, st);
    hipSafeCall(hipStreamSynchronize(st));
    return 1;
}
