// kf_sample.cpp — asking a map: the signed distance, its gradient and whether the place was seen, at points the caller supplies or at the pixels of
// a depth frame, of this map or of a second one (xs_tsdf_sample_points and xs_tsdf_sample_depth in include/xslam_amd.h:
// the contract; sample_host.hpp: the host's side of it).  Nothing of any map or cache is modified, and none of it runs during tracking.
#include "kf_internal.hpp"
#include "sample_host.hpp"

using namespace xs_host;

namespace {
using Out = KinectFusionReconstruction::SampleOutputs;
bool any_output(const Out &o) { return o.status || o.value || o.dvalue || o.gradient || o.counts; }

// The outputs of one launch over `count` points, each where the launch writes it (StagedOutput); fetch() brings the staged ones to the caller.
struct Staged {
    StagedOutput<unsigned char> status;
    StagedOutput<float> value, dvalue, gradient;
    StagedOutput<unsigned long long> counts;
    Staged(const Out &out, size_t count, bool on_device)
        : status(out.status, count, on_device), value(out.value, count, on_device), dvalue(out.dvalue, count, on_device),
          gradient(out.gradient, 3 * count, on_device), counts(out.counts, 4, on_device) {}
    void fetch(size_t count, hipStream_t st) {
        status.fetch(0, count, st); value.fetch(0, count, st); dvalue.fetch(0, count, st); gradient.fetch(0, 3 * count, st); counts.fetch(0, 4, st);
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
    const DeviceInput<float> points_d(points, 3 * (size_t)n, points_dev, st);
    Staged staged(out, (size_t)n, out_dev);
    const xs_sample_opts o = opts_of(min_weight);
    const int rc = xs_tsdf_sample_points(n, points_d.ptr, T16 ? xform : nullptr, vol.value, vol.weight, vol.grad, vol.step, vol.res, vol.voxel_size, &o,
                                         staged.status.at(0), staged.value.at(0), staged.dvalue.at(0), staged.gradient.at(0), staged.counts.at(0), st);
    if (rc == (int)hipErrorInvalidValue) return -1;   // the arguments: nothing was launched
    check_rc(rc, "SamplePoints");
    staged.fetch((size_t)n, st);
    hipSafeCall(hipStreamSynchronize(st));
    return 1;
}

int KinectFusionReconstruction::SamplePoints(const float *points, long long n, const double *T16, int min_weight, const SampleOutputs &out, int on_device) {
    if (shard_count > 1) return -2;   // a point's eight corners may straddle two ranks' z-slabs
    if (!tsdf_volume_d_ptr) return 0;
    SecondMap self;
    if (OwnMap(out.dvalue != nullptr, self) != 1) return -1;
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
    SecondMap self;
    if (OwnMap(out.dvalue != nullptr, self) != 1) return -1;
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
    Staged staged(out, count, out_dev);
    const xs_sample_opts o = opts_of(min_weight);
    const int rc = xs_tsdf_sample_depth(depth_dev ? depth : depth_d.ptr(), depth_dev ? depth_step : (size_t)cols * 2, rows, cols, intr4 ? intr4 : &kinect_intrinsic.fx, R, t,
                                        self.value, self.weight, self.grad, self.step, self.res, self.voxel_size, &o, staged.status.at(0), staged.value.at(0),
                                        staged.dvalue.at(0), staged.gradient.at(0), staged.counts.at(0), st);
    if (rc == (int)hipErrorInvalidValue) return -1;
    check_rc(rc, "FrameResiduals");
    staged.fetch(count, st);
    hipSafeCall(hipStreamSynchronize(st));
    return 1;
}
