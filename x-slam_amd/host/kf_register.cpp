// kf_register.cpp — a point cloud registered to a map: the rigid transform that puts the caller's points on the surface of this map or of a
// second one, by damped Gauss-Newton from one or many starts (xs_tsdf_register_terms in include/xslam_amd.h: the
// contract; register_host.hpp: the host's side of it), and, when there is no start, the search that finds some: many transforms scored in one
// launch, the best refined in shrinking boxes, and the survivors handed to that loop (section 4.32; xs_tsdf_score_points: the contract;
// register_search_host.hpp: the host's side).  Nothing of any map or cache is modified, and none of it runs during tracking.
#include "kf_internal.hpp"
#include "register_host.hpp"
#include "register_search_host.hpp"   // points_centroid, the options' defaults and refusals; align_search_host.hpp's candidates and ranking
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

// ---- many transforms of a cloud against a map, and registration with no starting guess ---------------------------
int KinectFusionReconstruction::register_map_of(const SecondMap *src, SecondMap &out) const {
    if (shard_count > 1) return -2;   // as RegisterPoints: a point's corners may straddle two ranks' z-slabs
    if (!tsdf_volume_d_ptr) return 0;
    if (!src) return OwnMap(false, out) == 1 ? 1 : -1;
    if (!takes_second_map(*src, 1, false)) return -1;
    out = *src;
    return 1;
}

int KinectFusionReconstruction::ScorePointsVolume(const SecondMap &vol, const float *points_dev, long long n, const float *xform12xP, int P, int stride,
                                                  int min_weight, float max_residual, double *out2xP, int *launches) {
    ensure_reduce_workspace(reloc_.rscore_ws, xs_tsdf_score_points_workspace_bytes(XS_REGISTER_SCORE_MAX_TRANSFORMS), "point score workspace");
    if (reloc_.rscore_sums.size() < (size_t)XS_REGISTER_SCORE_MAX_TRANSFORMS * 2) reloc_.rscore_sums.create((size_t)XS_REGISTER_SCORE_MAX_TRANSFORMS * 2);
    for (int p0 = 0; p0 < P; p0 += XS_REGISTER_SCORE_MAX_TRANSFORMS) {
        const int count = std::min(P - p0, (int)XS_REGISTER_SCORE_MAX_TRANSFORMS);
        const int rc = xs_tsdf_score_points(count, n, stride, points_dev, xform12xP + 12 * (size_t)p0, vol.value, vol.weight, vol.step, vol.res, vol.voxel_size,
                                            min_weight, max_residual, reloc_.rscore_ws.ptr(), reloc_.rscore_sums.ptr(), current_stream());
        if (rc == (int)hipErrorInvalidValue) return -1;   // the arguments: nothing was launched
        check_rc(rc, "ScorePoints");
        fetch_sums(reloc_.rscore_sums.ptr(), (size_t)count * 2, out2xP + 2 * (size_t)p0);
        if (launches) ++*launches;
    }
    return 1;
}

namespace {
// the float xform12 of every T16xP + 16 p by register_xform12's rule; false for one that is not finite in float32
bool xforms_of(const double *T16xP, int P, std::vector<float> &xforms) {
    xforms.resize((size_t)P * 12);
    for (int p = 0; p < P; ++p)
        if (!register_xform12(T16xP + 16 * (size_t)p, &xforms[(size_t)p * 12])) return false;
    return true;
}
}  // namespace

int KinectFusionReconstruction::ScorePointTransforms(const SecondMap *src, const float *points, long long n, int on_device, const double *T16xP, int P, int stride,
                                                     int min_weight, float max_residual, double *out2xP) {
    SecondMap vol;
    const int have = register_map_of(src, vol);
    if (have != 1) return have;
    if (n < 1 || n > SAMPLE_MAX_POINTS || !points || !T16xP || !out2xP || P < 1 || stride < 1 || min_weight < 1) return -1;
    if (!(max_residual > 0.f) || !std::isfinite(max_residual)) return -1;
    std::vector<float> xforms;
    if (!xforms_of(T16xP, P, xforms)) return -1;
    hipStream_t st = current_stream();
    drain_device();
    const DeviceInput<float> points_d(points, 3 * (size_t)n, on_device & 1, st);
    const int rc = ScorePointsVolume(vol, points_d.ptr, n, xforms.data(), P, stride, min_weight, max_residual, out2xP, nullptr);
    hipSafeCall(hipStreamSynchronize(st));
    return rc;
}

void KinectFusionReconstruction::RegisterSearchDefaults(xs_register_search_opts *o) const {
    register_search_defaults(tsdf_volume_d_ptr ? (double)tsdf_volume_d_ptr->getTsdfTruncDist() : 0.0, o);
}

int KinectFusionReconstruction::RegisterPointsGlobal(const SecondMap *src, const float *points, long long n, int on_device, const xs_register_search_opts *opts,
                                                     double *T16_out, double report[12]) {
    align_report_clear(report, 12);
    SecondMap vol;
    const int have = register_map_of(src, vol);
    if (have != 1) return have;
    xs_register_search_opts o;
    if (opts) o = *opts; else RegisterSearchDefaults(&o);
    if (!points || !T16_out || register_search_validate(o, n) != RSEARCH_ACCEPTED) return -1;
    const float max_residual = (float)o.max_residual;
    const long long scored = register_scored_points(n, o.stride);
    hipStream_t st = current_stream();
    drain_device();
    const DeviceInput<float> points_d(points, 3 * (size_t)n, on_device & 1, st);
    if (report) { report[8] = (double)n; report[9] = (double)scored; }
    // the cloud's centroid over the scored points; a device cloud's through a strided copy of exactly those, so both give the same bits
    double c_cloud[3], c_map[3];
    if (on_device & 1) {
        std::vector<float> strided((size_t)scored * 3);
        hipSafeCall(hipMemcpy2D(strided.data(), 3 * sizeof(float), points, (size_t)o.stride * 3 * sizeof(float), 3 * sizeof(float), (size_t)scored, hipMemcpyDeviceToHost));
        if (!points_centroid(strided.data(), scored, 1, c_cloud)) return -1;
    } else if (!points_centroid(points, n, o.stride, c_cloud)) return -1;
    int rc = second_map_centroid(vol, c_map);
    if (rc != 1) return rc;
    std::vector<double> cand, out2;
    std::vector<float> xforms;
    int launches = 0;
    auto score = [&]() {
        const int P = (int)(cand.size() / 16);
        out2.resize((size_t)P * 2);
        if (!xforms_of(cand.data(), P, xforms)) return -1;
        return ScorePointsVolume(vol, points_d.ptr, n, xforms.data(), P, o.stride, o.min_weight, max_residual, out2.data(), &launches);
    };
    if (o.user_n > 0) cand.assign(o.user_T16xN, o.user_T16xN + 16 * (size_t)o.user_n);
    else {
        cand.resize((size_t)o.candidates * 16);
        if (!align_search_free(o.candidates, c_cloud, c_map, o.box_t, cand.data())) return -1;
    }
    std::vector<double> kept, kept_S;
    auto rank = [&]() {
        int idx[32];
        const int K = align_search_rank(out2.data(), (int)(out2.size() / 2), o.keep, idx);
        kept.resize((size_t)K * 16);
        kept_S.resize((size_t)K);
        for (int k = 0; k < K; ++k) {
            std::copy(&cand[(size_t)idx[k] * 16], &cand[(size_t)idx[k] * 16] + 16, &kept[(size_t)k * 16]);
            kept_S[(size_t)k] = score_S(&out2[2 * (size_t)idx[k]]);
        }
    };
    rc = score();
    if (rc != 1) return rc;
    rank();
    const int per = std::max(1, o.candidates / o.keep);
    double bt = o.refine_t, br = o.refine_r;
    for (int r = 1; r <= o.rounds; ++r, bt *= 0.5, br *= 0.5) {
        const int K = (int)kept_S.size();
        cand.resize((size_t)K * per * 16);
        for (int k = 0; k < K; ++k)
            if (!align_search_around(&kept[(size_t)k * 16], c_cloud, bt, br, per, &cand[(size_t)k * per * 16])) return -1;
        rc = score();
        if (rc != 1) return rc;
        rank();
    }
    if (report) report[5] = (double)launches;
    double r7[7], T[16];
    register_report_clear(r7);
    rc = RegisterVolume(vol, points_d.ptr, n, 1, kept.data(), (int)kept_S.size(), o.iterations, o.damping, o.min_weight, max_residual, T, r7, nullptr);
    if (report) { report[6] = r7[4]; report[7] = r7[5]; }
    if (rc != 1) return rc;
    for (int i = 0; i < 16; ++i) T16_out[i] = T[i];
    if (report) {
        report[0] = r7[0]; report[1] = kept_S[(size_t)r7[0]];
        report[2] = r7[1]; report[3] = r7[2]; report[4] = r7[3];
        double d2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double q = ((T[4 * a] * c_cloud[0] + T[4 * a + 1] * c_cloud[1]) + T[4 * a + 2] * c_cloud[2]) + T[4 * a + 3];
            d2 += (q - c_map[a]) * (q - c_map[a]);
        }
        report[10] = std::sqrt(d2);
    }
    return 1;
}
