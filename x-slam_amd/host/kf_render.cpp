// kf_render.cpp — showing a map: depth, normal and shaded views from poses the caller picks, of this map or of a second one (DESIGN.md section
// 4.28; xs_render_views in include/xslam_amd.h: the contract; render_host.hpp: the host's side of it).  None of it runs during tracking.
#include "kf_internal.hpp"
#include "render_host.hpp"

using namespace xs_host;

namespace {
// null opts: every default, with the cull
xs_render_opts render_opts_of(const xs_render_opts *opts) {
    xs_render_opts o;
    std::memset(&o, 0, sizeof(o));
    o.struct_bytes = sizeof(o);
    o.cull = 1;
    return opts ? *opts : o;
}
bool any_output(const KinectFusionReconstruction::RenderOutputs &o) { return o.depth || o.depth_u16 || o.normal || o.shade || o.counts; }
}  // namespace

int KinectFusionReconstruction::RenderVolume(const float *value, const int *weight, size_t step, const int *res, float vs, void *ws, const float *c2v, int stride, int P,
                                             const float *intr4, int rows, int cols, const xs_render_opts &opts, const RenderOutputs &out, int on_device) {
    hipStream_t st = current_stream();
    const size_t plane = (size_t)rows * (size_t)cols;
    const int chunk = std::min(P, (int)XS_RENDER_MAX_VIEWS);
    // host outputs: one chunk's images in device buffers of the call's own
    DeviceArray<float> depth_d, normal_d;
    DeviceArray<uint16_t> depth16_d;
    DeviceArray<unsigned char> shade_d;
    DeviceArray<unsigned> counts_d;
    if (!on_device) {
        if (out.depth) depth_d.create((size_t)chunk * plane);
        if (out.depth_u16) depth16_d.create((size_t)chunk * plane);
        if (out.normal) normal_d.create((size_t)chunk * 3 * plane);
        if (out.shade) shade_d.create((size_t)chunk * plane);
        if (out.counts) counts_d.create((size_t)chunk * 4);
    }
    std::vector<float> R((size_t)chunk * 9), t((size_t)chunk * 3);
    for (int p0 = 0; p0 < P; p0 += XS_RENDER_MAX_VIEWS) {
        const int n = std::min(P - p0, (int)XS_RENDER_MAX_VIEWS);
        for (int i = 0; i < n; ++i) render_pose(c2v + (size_t)(p0 + i) * 16 * stride, stride, &R[(size_t)i * 9], &t[(size_t)i * 3]);
        RenderOutputs o;   // where this chunk is written
        if (on_device) {
            o.depth = out.depth ? out.depth + (size_t)p0 * plane : nullptr;
            o.depth_u16 = out.depth_u16 ? out.depth_u16 + (size_t)p0 * plane : nullptr;
            o.normal = out.normal ? out.normal + (size_t)p0 * 3 * plane : nullptr;
            o.shade = out.shade ? out.shade + (size_t)p0 * plane : nullptr;
            o.counts = out.counts ? out.counts + (size_t)p0 * 4 : nullptr;
        } else {
            o.depth = out.depth ? depth_d.ptr() : nullptr; o.depth_u16 = out.depth_u16 ? depth16_d.ptr() : nullptr;
            o.normal = out.normal ? normal_d.ptr() : nullptr; o.shade = out.shade ? shade_d.ptr() : nullptr; o.counts = out.counts ? counts_d.ptr() : nullptr;
        }
        const int rc = xs_render_views(n, R.data(), t.data(), intr4, rows, cols, value, weight, step, res, vs, &opts, ws, o.depth, o.depth_u16, o.normal, o.shade,
                                       o.counts, st);
        if (rc == (int)hipErrorInvalidValue) return -1;   // the arguments: nothing was launched
        check_rc(rc, "RenderViews");
        if (!on_device) {
            if (out.depth) hipSafeCall(hipMemcpyAsync(out.depth + (size_t)p0 * plane, o.depth, (size_t)n * plane * sizeof(float), hipMemcpyDeviceToHost, st));
            if (out.depth_u16) hipSafeCall(hipMemcpyAsync(out.depth_u16 + (size_t)p0 * plane, o.depth_u16, (size_t)n * plane * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
            if (out.normal) hipSafeCall(hipMemcpyAsync(out.normal + (size_t)p0 * 3 * plane, o.normal, (size_t)n * 3 * plane * sizeof(float), hipMemcpyDeviceToHost, st));
            if (out.shade) hipSafeCall(hipMemcpyAsync(out.shade + (size_t)p0 * plane, o.shade, (size_t)n * plane, hipMemcpyDeviceToHost, st));
            if (out.counts) hipSafeCall(hipMemcpyAsync(out.counts + (size_t)p0 * 4, o.counts, (size_t)n * 4 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        }
        hipSafeCall(hipStreamSynchronize(st));   // (the workspace's pose staging area and the chunk's buffers are free again)
    }
    return 1;
}

int KinectFusionReconstruction::RenderViews(const float *c2v, int stride, int P, const float *intr4, int rows, int cols, const xs_render_opts *opts,
                                            const RenderOutputs &out, int on_device) {
    if (shard_count > 1) return -2;   // a ray's first crossing is not additive over the ranks' z-slabs
    if (!tsdf_volume_d_ptr) return 0;
    if (P < 1 || !c2v || (stride != 1 && stride != 2) || !any_output(out)) return -1;
    const xs_render_opts o = render_opts_of(opts);
    if (rows == 0 && cols == 0) { rows = depth_height; cols = depth_width; }
    if (rows < 1 || cols < 1 || rows > RENDER_MAX_IMAGE || cols > RENDER_MAX_IMAGE) return -1;
    const DeviceArray2D<float> value = tsdf_volume_d_ptr->value();
    const DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    if (value.step() != weight.step()) return -1;
    const size_t bytes = xs_render_workspace_bytes(res3());
    if (bytes == 0) return -1;
    drain_device();
    if (plan_.render_ws.size() < bytes) { plan_.render_ws.create(bytes); plan_.render_key = GridKey{}; }
    if (o.cull) {   // the mask follows the volume the way ViewGridPrepare's grid does
        const GridKey key{volume_generation, o.min_weight < 1 ? 1 : o.min_weight};
        if (!(plan_.render_key == key)) {
            check_rc(xs_render_mask_build(value.ptr(), weight.ptr(), value.step(), res3(), key.min_weight, plan_.render_ws.ptr(), current_stream()), "RenderMaskBuild");
            plan_.render_key = key;
        }
    }
    return RenderVolume(value.ptr(), weight.ptr(), value.step(), res3(), voxel_size, plan_.render_ws.ptr(), c2v, stride, P, intr4 ? intr4 : &kinect_intrinsic.fx, rows,
                        cols, o, out, on_device);
}

int KinectFusionReconstruction::RenderSecondMap(const SecondMap &src, const float *c2v, int stride, int P, const float *intr4, int rows, int cols,
                                                const xs_render_opts *opts, const RenderOutputs &out, int on_device) {
    if (shard_count > 1) return -2;
    if (!tsdf_volume_d_ptr) return 0;
    if (P < 1 || !c2v || (stride != 1 && stride != 2) || !any_output(out) || !takes_second_map(src, 1, false)) return -1;
    const xs_render_opts o = render_opts_of(opts);
    if (rows == 0 && cols == 0) { rows = depth_height; cols = depth_width; }
    if (rows < 1 || cols < 1 || rows > RENDER_MAX_IMAGE || cols > RENDER_MAX_IMAGE) return -1;
    const size_t bytes = xs_render_workspace_bytes(src.res);
    if (bytes == 0) return -1;
    drain_device();
    DeviceArray<unsigned char> ws;   // of the call's own: this instance's cached mask stays
    ws.create(bytes);
    if (o.cull) check_rc(xs_render_mask_build(src.value, src.weight, src.step, src.res, o.min_weight, ws.ptr(), current_stream()), "RenderMaskBuild");
    return RenderVolume(src.value, src.weight, src.step, src.res, src.voxel_size, ws.ptr(), c2v, stride, P, intr4 ? intr4 : &kinect_intrinsic.fx, rows, cols, o, out,
                        on_device);
}
