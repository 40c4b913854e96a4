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
    DeviceArray<float> points_d;
    if (!points_dev) {
        points_d.create(3 * (size_t)n);
        hipSafeCall(hipMemcpyAsync(points_d.ptr(), points, 3 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    }
    ensure_reduce_workspace(reloc_.register_ws, xs_tsdf_register_workspace_bytes(XS_REGISTER_MAX_TRANSFORMS), "register workspace");
    if (reloc_.register_sums.size() < (size_t)XS_REGISTER_MAX_TRANSFORMS * 29) reloc_.register_sums.create((size_t)XS_REGISTER_MAX_TRANSFORMS * 29);
    std::vector<std::vector<double>> history((size_t)N);   // (always kept: the last pass's sums pick the winner)
    std::vector<double> last((size_t)N * 29, 0.0);
    std::vector<int> ok((size_t)N, 0);
    std::vector<float> xforms((size_t)XS_REGISTER_MAX_TRANSFORMS * 12);
    int passes = 0;
    bool refused = false;
    gn_batch_loop(N, iterations, history.data(), ok.data(), XS_REGISTER_MAX_TRANSFORMS,
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
                                   : xs_tsdf_register_terms(count, n, points_dev ? points : points_d.ptr(), xforms.data(), vol.value, vol.weight, vol.step, vol.res,
                                                            vol.voxel_size, min_weight, max_residual, reloc_.register_ws.ptr(), reloc_.register_sums.ptr(), st);
            if (rc == (int)hipErrorInvalidValue) {   // the arguments: nothing was launched, and every start fails with count 0
                refused = true;
                std::fill(sums, sums + (size_t)count * 29, 0.0);
                return;
            }
            check_rc(rc, "RegisterTerms");
            fetch_sums(reloc_.register_sums.ptr(), (size_t)count * 29, sums);
            ++passes;
            for (int i = 0; i < count; ++i) std::copy(sums + 29 * i, sums + 29 * i + 29, last.begin() + (size_t)starts[i] * 29);
        },
        [&](int s, const double *sums, int) { return register_step(sums, damping, &T[(size_t)s * 16]); });
    hipSafeCall(hipStreamSynchronize(st));
    if (refused) return -1;
    // the winner: AlignVolume's rule
    auto S = [&](int s) { return last[(size_t)s * 29 + 28] - last[(size_t)s * 29 + 27]; };
    int win = -1, ended_ok = 0;
    for (int s = 0; s < N; ++s) {
        if (!ok[(size_t)s] || last[(size_t)s * 29 + 28] < 6) continue;
        ++ended_ok;
        if (win < 0 || S(s) > S(win)) win = s;
    }
    if (report) { report[4] = (double)passes; report[5] = (double)ended_ok; report[6] = (double)n; }
    if (win < 0) return 0;
    const double *s = &last[(size_t)win * 29];
    for (int i = 0; i < 16; ++i) T16_out[i] = T[(size_t)win * 16 + i];
    if (report) { report[0] = (double)win; report[1] = s[28]; report[2] = s[27]; report[3] = s[28] > 0 ? s[27] / s[28] : 0.0; }
    if (loss_history) *loss_history = history[(size_t)win];
    return 1;
}

int KinectFusionReconstruction::RegisterPoints(const float *points, long long n, int on_device, const double *T16xN, int N, int iterations, double damping,
                                               int min_weight, float max_residual, double *T16_out, double report[7], std::vector<double> *loss_history) {
    register_report_clear(report);
    if (shard_count > 1) return -2;   // a point's eight corners may straddle two ranks' z-slabs, and the sums would need the all-reduce: not built
    if (!tsdf_volume_d_ptr) return 0;
    const DeviceArray2D<float> value = tsdf_volume_d_ptr->value();
    const DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    if (value.step() != weight.step()) return -1;
    const SecondMap self{value.ptr(), weight.ptr(), nullptr, value.step(), {res3()[0], res3()[1], res3()[2]}, voxel_size, tsdf_volume_d_ptr->getTsdfTruncDist()};
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
