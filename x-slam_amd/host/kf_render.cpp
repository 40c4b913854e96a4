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

int KinectFusionReconstruction::RenderVolume(const SecondMap &vol, void *ws, const float *c2v, int stride, int P, const float *intr4, int rows, int cols,
                                             const xs_render_opts &opts, const RenderOutputs &out, int on_device) {
    hipStream_t st = current_stream();
    const size_t plane = (size_t)rows * (size_t)cols, chunk = (size_t)std::min(P, (int)XS_RENDER_MAX_VIEWS);
    // where a chunk's images are written: host outputs go through device buffers of the call's own, one chunk long
    StagedOutput<float> depth(out.depth, chunk * plane, on_device), normal(out.normal, chunk * 3 * plane, on_device);
    StagedOutput<uint16_t> depth_u16(out.depth_u16, chunk * plane, on_device);
    StagedOutput<unsigned char> shade(out.shade, chunk * plane, on_device);
    StagedOutput<unsigned> counts(out.counts, chunk * 4, on_device);
    std::vector<float> R(chunk * 9), t(chunk * 3);
    for (int p0 = 0; p0 < P; p0 += XS_RENDER_MAX_VIEWS) {
        const int n = std::min(P - p0, (int)XS_RENDER_MAX_VIEWS);
        for (int i = 0; i < n; ++i) render_pose(c2v + (size_t)(p0 + i) * 16 * stride, stride, &R[(size_t)i * 9], &t[(size_t)i * 3]);
        const size_t at = (size_t)p0 * plane, len = (size_t)n * plane;
        const int rc = xs_render_views(n, R.data(), t.data(), intr4, rows, cols, vol.value, vol.weight, vol.step, vol.res, vol.voxel_size, &opts, ws, depth.at(at),
                                       depth_u16.at(at), normal.at(3 * at), shade.at(at), counts.at((size_t)p0 * 4), st);
        if (rc == (int)hipErrorInvalidValue) return -1;   // the arguments: nothing was launched
        check_rc(rc, "RenderViews");
        depth.fetch(at, len, st); depth_u16.fetch(at, len, st); normal.fetch(3 * at, 3 * len, st); shade.fetch(at, len, st);
        counts.fetch((size_t)p0 * 4, (size_t)n * 4, st);
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
    SecondMap self;
    if (OwnMap(false, self) != 1) return -1;
    const size_t bytes = xs_render_workspace_bytes(res3());
    if (bytes == 0) return -1;
    drain_device();
    if (plan_.render_ws.size() < bytes) { plan_.render_ws.create(bytes); plan_.render_key = GridKey{}; }
    if (o.cull) {   // the mask follows the volume the way ViewGridPrepare's grid does
        const GridKey key{volume_generation, o.min_weight < 1 ? 1 : o.min_weight};
        if (!(plan_.render_key == key)) {
            check_rc(xs_render_mask_build(self.value, self.weight, self.step, self.res, key.min_weight, plan_.render_ws.ptr(), current_stream()), "RenderMaskBuild");
            plan_.render_key = key;
        }
    }
    return RenderVolume(self, plan_.render_ws.ptr(), c2v, stride, P, intr4 ? intr4 : &kinect_intrinsic.fx, rows, cols, o, out, on_device);
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
    return RenderVolume(src, ws.ptr(), c2v, stride, P, intr4 ? intr4 : &kinect_intrinsic.fx, rows, cols, o, out, on_device);
}
