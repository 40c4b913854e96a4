// kf_second_map.cpp — what enters the orchestrator as a whole map (merge_host.hpp: SecondMap): the two ways to obtain one, from another instance and
// from a checkpoint file, and the five operations that take one: merged into this volume, aligned to it beforehand, from a guess or from none, many
// transforms scored against it, or compared with it voxel by voxel into clusters of change; and what follows a write to the volume off the frame path.  Except for RebuildSignMap
// after a write through xs_kf_volume_ptr, none of it runs during tracking.
#include "kf_internal.hpp"
#include "align_host.hpp"
#include "align_search_host.hpp"
#include "merge_host.hpp"
#include "view_host.hpp"   // the frontier's record format, cell rule and frontier_select
#include "../../include/xslam_amd_pipeline.h"   // xs_align_search_opts
#include <cmath>

using namespace xs_host;

// ---- obtaining the second map ------------------------------------------------------------------------------------------------------
int KinectFusionReconstruction::OtherInstanceMap(KinectFusionReconstruction *other, bool with_grad, SecondMap &out) const {
    if (!other || other == this) return -1;
    if (other->shard_count > 1) return -2;
    if (!other->tsdf_volume_d_ptr) return -1;
    other->synchronize();
    return other->OwnMap(with_grad, out);
}

int KinectFusionReconstruction::OwnMap(bool with_grad, SecondMap &out) const {
    auto v = tsdf_volume_d_ptr->value(), g = tsdf_volume_d_ptr->grad();
    auto w = tsdf_volume_d_ptr->weight();
    if (v.step() != w.step() || (with_grad && v.step() != g.step())) return -1;
    out = SecondMap{v.ptr(), w.ptr(), with_grad ? g.ptr() : nullptr, v.step(), {res3()[0], res3()[1], res3()[2]}, voxel_size, tsdf_volume_d_ptr->getTsdfTruncDist()};
    return 1;
}

int KinectFusionReconstruction::OpenCheckpointMap(const std::string &filename, CheckpointMap &out) {
    if (shard_count > 1) return -2;
    if (!tsdf_volume_d_ptr) return 0;
    CheckpointFile c;
    if (!c.read(filename)) return -1;
    const CkptPrefix &p = c.prefix();
    for (int i = 0; i < 3; ++i)
        if (p.res[i] < 1 || p.res[i] > 65535) return -1;
    if (p.shard_count != 1 || p.shard_rank != 0 || p.zs0 != 0 || p.zs1 != p.res[2]) return -1;   // a whole volume
    if (!(p.voxel_size > 0.f) || !std::isfinite(p.voxel_size) || p.tranc_dist != tsdf_volume_d_ptr->getTsdfTruncDist()) return -1;
    const size_t rows = (size_t)p.res[1] * (size_t)p.res[2];
    if (rows >= (size_t)1 << 31) return -1;
    out.dv.create((int)rows, p.res[0]); out.dg.create((int)rows, p.res[0]); out.dw.create((int)rows, p.res[0]);
    if (out.dv.step() != out.dg.step() || out.dv.step() != out.dw.step()) return -1;
    c.write_to(out.dv.ptr(0), out.dw.ptr(0), out.dg.ptr(0), out.dv.step(), checkpoint_staging_words);
    out.map = SecondMap{out.dv.ptr(0), out.dw.ptr(0), out.dg.ptr(0), out.dv.step(), {p.res[0], p.res[1], p.res[2]}, p.voxel_size, p.tranc_dist};
    return 1;
}

bool KinectFusionReconstruction::takes_second_map(const SecondMap &m, int min_axis, bool need_grad) const {
    return second_map_ok(m, min_axis, need_grad, tsdf_volume_d_ptr->getTsdfTruncDist(), tsdf_volume_d_ptr->value().ptr(0), tsdf_volume_d_ptr->weight().ptr(0),
                         tsdf_volume_d_ptr->grad().ptr(0));
}
// the source may belong to another instance with streams of its own: drain the device, not just this instance's stream
void KinectFusionReconstruction::drain_device() {
    synchronize();
    hipSafeCall(hipDeviceSynchronize());
}
// The sign map from the volume alone (allocation, checkpoint, anything that wrote the value array without the integrate kernels).
void KinectFusionReconstruction::RebuildSignMap() {
    ++volume_generation;   // the documented "the volume was written" call: the relocalisation index is rebuilt too
    if (!sign_map_on() || !sign_map_.ptr() || !tsdf_volume_d_ptr) return;
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value();
    check_rc(xs_signmap_rebuild_slab(sign_map_.ptr(), res3(), raycast_sign_map_shift, tsdf_volume_d_ptr->getTsdfTruncDist(), value.ptr(0), value.step(),
                                     zs0, zs1, current_stream()), "sign map");
}
// A merge, fused points or reintegrated frames wrote the volume: everything derived from it follows (volume_generation moves here and in RebuildSignMap).
void KinectFusionReconstruction::volume_written_off_path() {
    ++volume_generation;
    RebuildSignMap();
    sign_map_stale_ = false;
    invalidate_derived_maps();
    CalculatePointCloud(vmaps_g_prev_d[0], nmaps_g_prev_d[0]);
    ModelMapPyramid();
    synchronize();
}

// ---- merging a second map ----------------------------------------------------------------------------------
int KinectFusionReconstruction::MergeVolume(const SecondMap &src, const double *T16, int min_weight, unsigned long long *written) {
    if (shard_count > 1) return -2;   // the source's image in a rank's z-slab needs the whole source on every rank: not built
    if (!tsdf_volume_d_ptr) return 0;
    if (!T16 || min_weight < 1 || !takes_second_map(src, 1, true)) return -1;
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value(), grad = tsdf_volume_d_ptr->grad();
    DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    float xform[12];
    if (!merge_affine(T16, (double)voxel_size, (double)src.voxel_size, xform)) return -1;
    const size_t ws_bytes = xs_tsdf_merge_workspace_bytes(res3(), src.res);
    if (ws_bytes == 0) return -1;
    drain_device();
    DeviceArray<unsigned char> ws;
    ws.create(ws_bytes);
    DeviceArray<unsigned long long> count;
    count.create(1);
    hipSafeCall(hipMemsetAsync(count.ptr(), 0, sizeof(unsigned long long), current_stream()));
    check_rc(xs_tsdf_merge(value.ptr(0), weight.ptr(0), grad.ptr(0), value.step(), res3(), 0, res3()[2], src.value, src.weight, src.grad, src.step, src.res,
                           xform, min_weight, max_integration_weight, 0u, count.ptr(), ws.ptr(), current_stream()), "merge");
    volume_written_off_path();
    if (written) hipSafeCall(hipMemcpy(written, count.ptr(), sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 1;
}

// ---- aligning a second map -----------------------------------------------------------------------------------
int KinectFusionReconstruction::AlignVolume(const SecondMap &src, const double *T16xN, int N, int iterations, double damping, int min_weight, float max_residual,
                                            double *T16_out, double report[8], std::vector<double> *loss_history) {
    align_report_clear(report, 8);
    if (shard_count > 1) return -2;   // the band index of a rank holds its own planes, the sums would need the all-reduce: not built
    if (!tsdf_volume_d_ptr) return 0;
    if (!T16xN || !T16_out || N < 1 || iterations < 0 || min_weight < 1) return -1;
    if (!(max_residual > 0.f) || !std::isfinite(max_residual) || !(damping >= 0.0) || !std::isfinite(damping)) return -1;
    if (!takes_second_map(src, 2, false)) return -1;
    std::vector<double> T((size_t)N * 16);
    float probe[6][24];
    for (int n = 0; n < N; ++n) {
        for (int i = 0; i < 16; ++i) T[(size_t)n * 16 + i] = T16xN[(size_t)n * 16 + i];
        if (!align_seeded_maps(&T[(size_t)n * 16], (double)voxel_size, (double)src.voxel_size, probe)) return -1;
    }
    drain_device();
    BandIndexPrepare();
    ensure_reduce_workspace(reloc_.align_ws, xs_tsdf_align_workspace_bytes(XS_ALIGN_MAX_TRANSFORMS), "align workspace");
    if (reloc_.align_sums.size() < (size_t)XS_ALIGN_MAX_TRANSFORMS * 29) reloc_.align_sums.create((size_t)XS_ALIGN_MAX_TRANSFORMS * 29);
    std::vector<float> maps((size_t)XS_ALIGN_MAX_TRANSFORMS * 144);
    const GnMultistart r = gn_multistart(N, iterations, XS_ALIGN_MAX_TRANSFORMS, true,   // (the loss pass always: its sums pick the winner)
        [&](const int *starts, int n, double *sums) {
            for (int i = 0; i < n; ++i) {
                float *m = &maps[(size_t)i * 144];
                if (align_seeded_maps(&T[(size_t)starts[i] * 16], (double)voxel_size, (double)src.voxel_size, reinterpret_cast<float (*)[24]>(m))) continue;
                // a step took T out of float32's range: a map that misses the source (every index is -1), so the start ends with count 0 and fails
                std::fill(m, m + 144, 0.f);
                for (int k = 0; k < 6; ++k)
                    for (int a = 0; a < 3; ++a) m[24 * k + 2 * (9 + a)] = -1.f;
            }
            check_rc(xs_tsdf_align_terms(n, &reloc_.band, src.value, src.weight, src.step, src.res, maps.data(), min_weight, max_residual, reloc_.align_ws.ptr(),
                                         reloc_.align_sums.ptr(), current_stream()), "AlignTerms");
            fetch_sums(reloc_.align_sums.ptr(), (size_t)n * 29, sums);
            for (int i = 0; i < n; ++i) gn_scale_sums(sums + 29 * i, sums + 29 * i);
        },
        [&](int n, const double *s, int) { return align_step(s, damping, &T[(size_t)n * 16]); });
    gn_multistart_report(r, report);
    if (report) report[6] = (double)reloc_.band.count;
    if (r.win < 0) return 0;
    for (int i = 0; i < 16; ++i) T16_out[i] = T[(size_t)r.win * 16 + i];
    if (loss_history) *loss_history = r.history;
    return 1;
}

// ---- many transforms against the other map, and alignment with no initial guess --------------------------------
int KinectFusionReconstruction::ScoreTransformsVolume(const SecondMap &src, const double *T16xP, int P, int stride, int min_weight, float max_residual, double *out2xP,
                                                      int *launches) {
    if (shard_count > 1) return -2;   // as AlignVolume: a rank's band index holds its own planes
    if (!tsdf_volume_d_ptr) return 0;
    if (!T16xP || !out2xP || P < 1 || stride < 1 || min_weight < 1 || !(max_residual > 0.f) || !std::isfinite(max_residual)) return -1;
    if (!takes_second_map(src, 2, false)) return -1;
    std::vector<float> xforms((size_t)P * 12);
    for (int p = 0; p < P; ++p)
        if (!merge_affine(T16xP + 16 * (size_t)p, (double)voxel_size, (double)src.voxel_size, &xforms[(size_t)p * 12])) return -1;
    drain_device();
    BandIndexPrepare();
    ensure_reduce_workspace(reloc_.ascore_ws, xs_tsdf_score_transforms_workspace_bytes(XS_ALIGN_SCORE_MAX_TRANSFORMS), "transform score workspace");
    if (reloc_.ascore_sums.size() < (size_t)XS_ALIGN_SCORE_MAX_TRANSFORMS * 2) reloc_.ascore_sums.create((size_t)XS_ALIGN_SCORE_MAX_TRANSFORMS * 2);
    for (int p0 = 0; p0 < P; p0 += XS_ALIGN_SCORE_MAX_TRANSFORMS) {
        const int n = std::min(P - p0, (int)XS_ALIGN_SCORE_MAX_TRANSFORMS);
        check_rc(xs_tsdf_score_transforms(n, &reloc_.band, stride, src.value, src.weight, src.step, src.res, &xforms[(size_t)p0 * 12], min_weight, max_residual,
                                          reloc_.ascore_ws.ptr(), reloc_.ascore_sums.ptr(), current_stream()), "ScoreTransforms");
        fetch_sums(reloc_.ascore_sums.ptr(), (size_t)n * 2, out2xP + 2 * (size_t)p0);
        if (launches) ++*launches;
    }
    return 1;
}

void KinectFusionReconstruction::AlignSearchDefaults(xs_align_search_opts *o) const {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->struct_bytes = sizeof(*o);
    o->candidates = 2048; o->keep = 8; o->rounds = 2; o->stride = 4; o->iterations = 10; o->min_weight = 1;
    o->box_t = o->refine_t = tsdf_volume_d_ptr ? (double)tsdf_volume_d_ptr->getTsdfTruncDist() : 0.0;
    o->refine_r = 0.25; o->damping = 1e-3; o->max_residual = 1.0;
}

namespace {
// what the search itself refuses (AlignVolume and ScoreTransformsVolume refuse the rest)
bool search_opts_ok(const xs_align_search_opts &o) {
    if (o.struct_bytes != sizeof(xs_align_search_opts)) return false;
    if (o.candidates < 1 || o.keep < 1 || o.keep > 32 || o.rounds < 0 || o.stride < 1 || o.iterations < 0 || o.min_weight < 1) return false;
    for (double b : {o.box_t, o.refine_t, o.refine_r})
        if (!(b >= 0.0) || !std::isfinite(b)) return false;
    if (!(o.damping >= 0.0) || !std::isfinite(o.damping) || !(o.max_residual > 0.0) || !std::isfinite((double)(float)o.max_residual)) return false;
    if (o.user_n < 0 || (o.user_n > 0 && !o.user_T16xN)) return false;
    return true;
}
}  // namespace
// The centroid of a map's band from one band build over it (count, then fill) into temporary buffers: the map's owner keeps its caches.
// 1; 0 for an empty band; -1 for a resolution the band build does not take.  (Declared in kf_internal.hpp: RegisterPointsGlobal uses it too.)
int second_map_centroid(const SecondMap &src, double c_other[3]) {
    hipStream_t st = current_stream();
    const int X = src.res[0];
    const size_t rows = (size_t)src.res[1] * (size_t)src.res[2];
    DeviceArray<float> packed;
    const float *dense = src.value;
    if (src.step != (size_t)X * 4) {   // the band walk indexes a dense array
        packed.create(rows * (size_t)X);
        hipSafeCall(hipMemcpy2DAsync(packed.ptr(), (size_t)X * 4, src.value, src.step, (size_t)X * 4, rows, hipMemcpyDeviceToDevice, st));
        dense = packed.ptr();
    }
    const size_t segs_bytes = xs_tsdf_band_segs_bytes(src.res, 0, src.res[2]);
    if (segs_bytes == 0) return -1;
    DeviceArray<long long> segs;
    segs.create(segs_bytes / sizeof(long long));
    DeviceArray<unsigned long long> keys_d;
    DeviceArray<float> values_d;
    xs_band_index idx = {};
    idx.segs = segs.ptr();
    int rc = xs_tsdf_band_build(dense, src.res, 0, src.res[2], &idx, st);
    if (rc == XS_BAND_OVER_CAPACITY) {
        keys_d.create((size_t)idx.count);
        values_d.create((size_t)idx.count);
        idx.keys = keys_d.ptr(); idx.values = values_d.ptr(); idx.capacity = idx.count;
        rc = xs_tsdf_band_build(dense, src.res, 0, src.res[2], &idx, st);
    }
    check_rc(rc, "the other map's band");
    std::vector<unsigned long long> keys((size_t)idx.count);
    if (idx.count > 0) hipSafeCall(hipMemcpy(keys.data(), idx.keys, (size_t)idx.count * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return band_centroid(keys.data(), idx.count, (double)src.voxel_size, c_other) ? 1 : 0;
}

int KinectFusionReconstruction::AlignVolumeGlobal(const SecondMap &src, const xs_align_search_opts *opts, double *T16_out, double report[12]) {
    align_report_clear(report, 12);
    if (shard_count > 1) return -2;
    if (!tsdf_volume_d_ptr) return 0;
    xs_align_search_opts o;
    if (opts) o = *opts; else AlignSearchDefaults(&o);
    if (!T16_out || !search_opts_ok(o) || !takes_second_map(src, 2, false)) return -1;
    const float max_residual = (float)o.max_residual;
    drain_device();
    BandIndexPrepare();
    std::vector<double> cand, out2;
    int launches = 0;
    auto score = [&]() {
        out2.resize(cand.size() / 16 * 2);
        return ScoreTransformsVolume(src, cand.data(), (int)(cand.size() / 16), o.stride, o.min_weight, max_residual, out2.data(), &launches);
    };
    const long long band_n = reloc_.band.count;
    if (report) { report[8] = (double)band_n; report[9] = (double)((band_n + o.stride - 1) / o.stride); }
    // this map's centroid from its band index, the keys downloaded once
    double c_this[3], c_other[3];
    {
        std::vector<unsigned long long> keys((size_t)band_n);
        if (band_n > 0) hipSafeCall(hipMemcpy(keys.data(), reloc_.band.keys, (size_t)band_n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (!band_centroid(keys.data(), band_n, (double)voxel_size, c_this)) return 0;
    }
    int rc = second_map_centroid(src, c_other);
    if (rc != 1) return rc;
    if (o.user_n > 0) cand.assign(o.user_T16xN, o.user_T16xN + 16 * (size_t)o.user_n);
    else {
        cand.resize((size_t)o.candidates * 16);
        if (!align_search_free(o.candidates, c_this, c_other, o.box_t, cand.data())) return -1;
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
            if (!align_search_around(&kept[(size_t)k * 16], c_this, bt, br, per, &cand[(size_t)k * per * 16])) return -1;
        rc = score();
        if (rc != 1) return rc;
        rank();
    }
    if (report) report[5] = (double)launches;
    double r8[8];
    double T[16];
    rc = AlignVolume(src, kept.data(), (int)kept_S.size(), o.iterations, o.damping, o.min_weight, max_residual, T, r8, nullptr);
    if (report) { report[6] = r8[4]; report[7] = r8[5]; }
    if (rc != 1) return rc;
    for (int i = 0; i < 16; ++i) T16_out[i] = T[i];
    if (report) {
        report[0] = r8[0]; report[1] = kept_S[(size_t)r8[0]];
        report[2] = r8[1]; report[3] = r8[2]; report[4] = r8[3];
        double d2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double q = ((T[4 * a] * c_this[0] + T[4 * a + 1] * c_this[1]) + T[4 * a + 2] * c_this[2]) + T[4 * a + 3];
            d2 += (q - c_other[a]) * (q - c_other[a]);
        }
        report[10] = std::sqrt(d2);
    }
    return 1;
}

// ---- what differs between this map and a second map ------------------------------------------------------------
int KinectFusionReconstruction::DiffVolume(const SecondMap &src, const double *T16, int min_weight, float lo, float hi, int cell, unsigned long long min_size,
                                           int capacity, unsigned long long *this_records8, int *this_count, unsigned long long *other_records8,
                                           int *other_count, unsigned long long counts3[3], unsigned char *this_dense, unsigned char *other_dense) {
    if (shard_count > 1) return -2;   // the source's image in a rank's z-slab needs the whole source on every rank, and a cluster is not additive over slabs
    if (!this_count || !other_count || capacity < 0 || (capacity > 0 && (!this_records8 || !other_records8)) || !frontier_cell_valid(cell)) return -1;
    if (!tsdf_volume_d_ptr) return 0;
    if (!T16 || min_weight < 1 || !std::isfinite(lo) || !std::isfinite(hi) || lo > hi || !takes_second_map(src, 1, false)) return -1;
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value();
    DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    float xform[12];
    if (!merge_affine(T16, (double)voxel_size, (double)src.voxel_size, xform)) return -1;
    const int *res = res3();
    const size_t ws_bytes = xs_tsdf_diff_workspace_bytes(res, src.res), mask_bytes = xs_frontier_mask_bytes(res), label_bytes = xs_frontier_label_bytes(res);
    if (ws_bytes == 0 || mask_bytes == 0 || label_bytes == 0 || res[0] > 65535) return -1;
    drain_device();
    // buffers of the call's own: the frontier cache, and everything else derived from the volume, stays as it is
    hipStream_t st = current_stream();
    DeviceArray<unsigned char> ws, masks, labels, frontier_ws, dense;
    DeviceArray<unsigned long long> counts, records_d;
    ws.create(ws_bytes);
    masks.create(2 * mask_bytes);
    labels.create(label_bytes);
    counts.create(3);
    void *mask[2] = {masks.ptr(), masks.ptr() + mask_bytes};
    hipSafeCall(hipMemsetAsync(counts.ptr(), 0, 3 * sizeof(unsigned long long), st));
    check_rc(xs_tsdf_diff(value.ptr(0), weight.ptr(0), value.step(), res, src.value, src.weight, src.step, src.res, xform, min_weight, lo, hi, 0u, mask[0], mask[1],
                          counts.ptr(), ws.ptr(), st), "diff");
    std::vector<unsigned long long> records[2];
    std::vector<int> keep[2];
    int kept[2] = {0, 0};
    int cap = 4096;
    auto room_for = [&](int c) {   // the records with the count behind them, and the workspace that goes with that capacity
        records_d.create((size_t)c * FRONTIER_RECORD_WORDS + 1);
        frontier_ws.create(xs_frontier_workspace_bytes(res, c));
    };
    room_for(cap);
    for (int k = 0; k < 2; ++k) {
        unsigned *lab = reinterpret_cast<unsigned *>(labels.ptr());
        check_rc(xs_frontier_label(mask[k], res, cell, lab, frontier_ws.ptr(), nullptr, st), "DiffLabel");
        unsigned count = 0;
        for (int attempt = 0; attempt < 2; ++attempt) {   // (the second with room for the count the first returned)
            unsigned long long *rec = records_d.ptr();
            check_rc(xs_frontier_clusters(mask[k], lab, res, cap, rec, reinterpret_cast<unsigned *>(rec + (size_t)cap * FRONTIER_RECORD_WORDS), &count,
                                          frontier_ws.ptr(), st), "DiffClusters");
            if (count <= (unsigned)cap) break;
            if (count > 0x7fffffffu / 2u) return -1;
            cap = (int)count;
            room_for(cap);
        }
        records[k].assign((size_t)count * FRONTIER_RECORD_WORDS, 0ull);
        if (count) {
            hipSafeCall(hipMemcpyAsync(records[k].data(), records_d.ptr(), records[k].size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            hipSafeCall(hipStreamSynchronize(st));
        }
        keep[k].resize((size_t)count);
        kept[k] = frontier_select(records[k].data(), (int)count, min_size, keep[k].data());
    }
    *this_count = kept[0];
    *other_count = kept[1];
    if (kept[0] > capacity || kept[1] > capacity) return -4;
    unsigned long long *out[2] = {this_records8, other_records8};
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < kept[k]; ++i)
            std::memcpy(out[k] + (size_t)i * FRONTIER_RECORD_WORDS, records[k].data() + (size_t)keep[k][(size_t)i] * FRONTIER_RECORD_WORDS,
                        FRONTIER_RECORD_WORDS * sizeof(unsigned long long));
    if (counts3) hipSafeCall(hipMemcpy(counts3, counts.ptr(), 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned char *host_dense[2] = {this_dense, other_dense};
    for (int k = 0; k < 2; ++k) {
        if (!host_dense[k]) continue;
        const size_t voxels = (size_t)res[0] * (size_t)res[1] * (size_t)res[2];
        dense.create(voxels);
        check_rc(xs_frontier_expand(mask[k], res, dense.ptr(), st), "DiffExpand");
        hipSafeCall(hipMemcpyAsync(host_dense[k], dense.ptr(), voxels, hipMemcpyDeviceToHost, st));
        hipSafeCall(hipStreamSynchronize(st));
    }
    return 1;
}

