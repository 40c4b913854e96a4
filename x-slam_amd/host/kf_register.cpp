// kf_register.cpp — a point cloud registered to a map: the rigid transform that puts the caller's points on the surface of this map or of a
// second one, by damped Gauss-Newton from one or many starts (xs_tsdf_register_terms in include/xslam_amd.h: the
// contract; register_host.hpp: the host's side of it).  Nothing of any map or cache is modified, and none of it runs during tracking.
#include "kf_internal.hpp"
#include "register_host.hpp"
#include <cmath>

using namespace xs_host;

int KinectFusionReconstruction::RegisterVolume(const SecondMap &vol, const float *points, long long n, int on_device, const double *T16xN, int N, int iterations,
                                               double damping, int min_weight, float max_residual, double *T16_out, double report[7],
                                               std::vector<double> *loss_history) {
    if (n < 1 || n > SAMPLE_MAX_POINTS || !points || !T16xN || !T16_out || N < 1 || iterations < 0 || min_weight < 1) return -1;
    if (!(max_residual > 0.f) || !std::isfinite(max_residual) || !(damping >= 0.0) || !std::isfinite(damping)) return -1;
    std::vector<double> T((size_t)N * 16);
    float probe[12];
    for (int s = 0; s < N; ++s) {
        for (int i = 0; i < 16; ++i) T[(size_t)s * 16 + i] = T16xN[(size_t)s * 16 + i];
        if (!register_xform12(&T[(size_t)s * 16], probe)) return -1;
    }
    const bool points_dev = on_device & 1;
    hipStream_t st = current_stream();
    drain_device();
    const DeviceInput<float> points_d(points, 3 * (size_t)n, points_dev, st);
    ensure_reduce_workspace(reloc_.register_ws, xs_tsdf_register_workspace_bytes(XS_REGISTER_MAX_TRANSFORMS), "register workspace");
    if (reloc_.register_sums.size() < (size_t)XS_REGISTER_MAX_TRANSFORMS * 29) reloc_.register_sums.create((size_t)XS_REGISTER_MAX_TRANSFORMS * 29);
    std::vector<float> xforms((size_t)XS_REGISTER_MAX_TRANSFORMS * 12);
    bool refused = false;
    const GnMultistart r = gn_multistart(N, iterations, XS_REGISTER_MAX_TRANSFORMS, true,   // (the loss pass always: its sums pick the winner)
        [&](const int *starts, int count, double *sums) {
            for (int i = 0; i < count; ++i) {
                float *m = &xforms[(size_t)i * 12];
                if (register_xform12(&T[(size_t)starts[i] * 16], m)) continue;
                // a step took T out of float32's range: a transform that sends every point to (-1, -1, -1), outside any volume, so the start
                // ends with count 0 and fails
                std::fill(m, m + 9, 0.f);
                m[9] = m[10] = m[11] = -1.f;
            }
            const int rc = refused ? (int)hipErrorInvalidValue
                                   : xs_tsdf_register_terms(count, n, points_d.ptr, xforms.data(), vol.value, vol.weight, vol.step, vol.res, vol.voxel_size,
                                                            min_weight, max_residual, reloc_.register_ws.ptr(), reloc_.register_sums.ptr(), st);
            if (rc == (int)hipErrorInvalidValue) {   // the arguments: nothing was launched, and every start fails with count 0
                refused = true;
                std::fill(sums, sums + (size_t)count * 29, 0.0);
                return;
            }
            check_rc(rc, "RegisterTerms");
            fetch_sums(reloc_.register_sums.ptr(), (size_t)count * 29, sums);
        },
        [&](int s, const double *sums, int) { return register_step(sums, damping, &T[(size_t)s * 16]); });
    hipSafeCall(hipStreamSynchronize(st));
    if (refused) return -1;
    gn_multistart_report(r, report);
    if (report) report[6] = (double)n;
    if (r.win < 0) return 0;
    for (int i = 0; i < 16; ++i) T16_out[i] = T[(size_t)r.win * 16 + i];
    if (loss_history) *loss_history = r.history;
    return 1;
}

int KinectFusionReconstruction::RegisterPoints(const float *points, long long n, int on_device, const double *T16xN, int N, int iterations, double damping,
                                               int min_weight, float max_residual, double *T16_out, double report[7], std::vector<double> *loss_history) {
    register_report_clear(report);
    if (shard_count > 1) return -2;   // a point's eight corners may straddle two ranks' z-slabs, and the sums would need the all-reduce: not built
    if (!tsdf_volume_d_ptr) return 0;
    SecondMap self;
    if (OwnMap(false, self) != 1) return -1;
    return RegisterVolume(self, points, n, on_device, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report, loss_history);
}

int KinectFusionReconstruction::RegisterSecondMap(const SecondMap &src, const float *points, long long n, int on_device, const double *T16xN, int N, int iterations,
                                                  double damping, int min_weight, float max_residual, double *T16_out, double report[7],
                                                  std::vector<double> *loss_history) {
    register_report_clear(report);
    if (shard_count > 1) return -2;
    if (!tsdf_volume_d_ptr) return 0;
    if (!takes_second_map(src, 1, false)) return -1;
    return RegisterVolume(src, points, n, on_device, T16xN, N, iterations, damping, min_weight, max_residual, T16_out, report, loss_history);
}
