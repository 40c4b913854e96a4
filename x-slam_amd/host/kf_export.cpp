// kf_export.cpp — what leaves the orchestrator: point cloud and mesh with their PLY writers, the last frame's counters, the raw volume
// and the checkpoint; and what enters it as a whole map: a second volume or checkpoint merged into this one, and aligned to it beforehand, from a guess or from none,
// or compared with it voxel by voxel into clusters of change.
// None of it runs during tracking.
#include "kf_internal.hpp"
#include "align_host.hpp"
#include "align_search_host.hpp"
#include "merge_host.hpp"
#include "pack_host.hpp"
#include "view_host.hpp"   // the frontier's record format, cell rule and frontier_select
#include "../../include/xslam_amd_pipeline.h"   // xs_align_search_opts
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

using namespace xs_host;

// reference :334-372
KinectFusionReconstruction::CPointCloud KinectFusionReconstruction::ExportPointCloud(int max_buffer) {
    CPointCloud res;
    if (max_buffer <= 0 || !tsdf_volume_d_ptr) return res;
    DeviceArray<float3> cloud_buffer, normal_buffer;
    cloud_buffer.create(max_buffer);
    normal_buffer.create(max_buffer);
    const int3 volume_res = make_int3(res3()[0], res3()[1], res3()[2]);
    // a rank of a sharded run reports the crossings of the planes it owns (the +z neighbour of its last
    // plane is in its halo); the single-GPU case is the whole volume
    const int z1 = std::min(zo1, volume_res.z - 1);
    PtrSz<float3> cloud; cloud.data = cloud_buffer.ptr(); cloud.size = (size_t)max_buffer;
    const size_t num_points = extractPoints(tsdf_volume_d_ptr->value(), tsdf_volume_d_ptr->weight(), tsdf_volume_d_ptr->grad(), volume_res,
                                            voxel_size, cloud, zs0, zo0, std::max(z1, zo0));
    if (num_points == 0) return res;
    cloud.size = num_points;
    PtrSz<float3> normal; normal.data = normal_buffer.ptr(); normal.size = num_points;
    extractNormals(tsdf_volume_d_ptr->value(), tsdf_volume_d_ptr->weight(), tsdf_volume_d_ptr->grad(), volume_res, voxel_size, cloud, normal,
                   zs0, zs1);
    res.positions.resize(3 * num_points);
    res.normals.resize(3 * num_points);
    hipSafeCall(hipMemcpy(res.positions.data(), cloud_buffer.ptr(), num_points * sizeof(float3), hipMemcpyDeviceToHost));
    hipSafeCall(hipMemcpy(res.normals.data(), normal_buffer.ptr(), num_points * sizeof(float3), hipMemcpyDeviceToHost));
    return res;
}
bool KinectFusionReconstruction::CPointCloud::exportPly(const std::string &filename) const {
    std::ofstream file_out{filename};
    if (!file_out.is_open()) return false;
    file_out << "ply\nformat ascii 1.0\ncomment Created by myself\nelement vertex " << size() << "\n";
    file_out << "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\nend_header\n";
    for (size_t i = 0; i < size(); ++i)
        file_out << positions[3 * i] << " " << positions[3 * i + 1] << " " << positions[3 * i + 2] << " " << normals[3 * i] << " "
                 << normals[3 * i + 1] << " " << normals[3 * i + 2] << "\n";
    return true;
}

KinectFusionReconstruction::CMesh KinectFusionReconstruction::ExportMesh(int min_weight) {
    CMesh m;
    if (!tsdf_volume_d_ptr) return m;
    if (sign_map_stale_) { RebuildSignMap(); sign_map_stale_ = false; }   // (the map must be a superset of the negative voxels)
    const int *res = res3();
    const bool seeded = csfd_seed_row >= 0 && csfd_seed_row < 4 && csfd_seed_col >= 0 && csfd_seed_col < 4;
    m.has_im = seeded;   // (also for an empty mesh: a rank without surface still says whether its vertices would carry derivatives)
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value(), grad = tsdf_volume_d_ptr->grad();
    DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    // (TsdfVolume allocates the three arrays alike: one pitch)
    xs_mesh_opts o{};
    o.struct_bytes = sizeof(o);
    o.zs0 = zs0; o.zs1 = zs1;
    o.z0 = zo0; o.z1 = std::max(std::min(zo1, res[2] - 1), zo0);   // (as ExportPointCloud)
    o.min_weight = min_weight; o.want_normals = 1;
    o.signmap = sign_map_ptr(); o.signmap_shift = raycast_sign_map_shift;
    DeviceArray<unsigned char> ws;
    ws.create(xs_mesh_workspace_bytes(res, &o));
    const float *g = seeded ? grad.ptr(0) : nullptr;
    size_t nv = 0, nt = 0;
    int rc = xs_extract_mesh(value.ptr(0), weight.ptr(0), g, value.step(), res, voxel_size, &o, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0,
                             ws.ptr(), &nv, &nt, current_stream());
    if (rc == 0) return m;   // (nothing fits in no room only when there is nothing)
    if (rc != XS_MESH_OVER_CAPACITY) check_rc(rc, "mesh count");
    DeviceArray<float> verts, vim, normals;
    DeviceArray<unsigned long long> keys;
    DeviceArray<int> tris;
    verts.create(3 * nv); normals.create(3 * nv); keys.create(nv); tris.create(3 * std::max<size_t>(nt, 1));
    if (seeded) vim.create(3 * nv);
    size_t nv2 = 0, nt2 = 0;
    check_rc(xs_extract_mesh(value.ptr(0), weight.ptr(0), g, value.step(), res, voxel_size, &o, verts.ptr(), seeded ? vim.ptr() : nullptr,
                             normals.ptr(), keys.ptr(), nv, tris.ptr(), nt, ws.ptr(), &nv2, &nt2, current_stream()), "mesh");
    m.positions.resize(3 * nv); m.normals.resize(3 * nv); m.edge_keys.resize(nv); m.triangles.resize(3 * nt);
    hipSafeCall(hipMemcpy(m.positions.data(), verts.ptr(), 3 * nv * sizeof(float), hipMemcpyDeviceToHost));
    hipSafeCall(hipMemcpy(m.normals.data(), normals.ptr(), 3 * nv * sizeof(float), hipMemcpyDeviceToHost));
    hipSafeCall(hipMemcpy(m.edge_keys.data(), keys.ptr(), nv * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (nt) hipSafeCall(hipMemcpy(m.triangles.data(), tris.ptr(), 3 * nt * sizeof(int), hipMemcpyDeviceToHost));
    if (seeded) {
        m.vertex_im.resize(3 * nv);
        hipSafeCall(hipMemcpy(m.vertex_im.data(), vim.ptr(), 3 * nv * sizeof(float), hipMemcpyDeviceToHost));
    }
    return m;
}
bool KinectFusionReconstruction::CMesh::exportPly(const std::string &filename) const {
    std::ofstream f(filename, std::ios::binary);
    if (!f.is_open()) return false;
    const bool d = has_im;
    f << "ply\nformat binary_little_endian 1.0\nelement vertex " << vertices() << "\n";
    f << "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n";
    if (d) f << "property float dx\nproperty float dy\nproperty float dz\n";
    f << "element face " << faces() << "\nproperty list uchar int vertex_indices\nend_header\n";
    std::vector<float> row(d ? 9 : 6);   // (x86 / the hosts this builds for are little-endian: the floats go out as they are)
    for (size_t i = 0; i < vertices(); ++i) {
        for (int k = 0; k < 3; ++k) { row[k] = positions[3 * i + k]; row[3 + k] = normals[3 * i + k]; if (d) row[6 + k] = vertex_im[3 * i + k]; }
        f.write(reinterpret_cast<const char *>(row.data()), (std::streamsize)(row.size() * sizeof(float)));
    }
    char face[13];
    face[0] = 3;
    for (size_t t = 0; t < faces(); ++t) {
        std::memcpy(face + 1, &triangles[3 * t], 12);
        f.write(face, 13);
    }
    return (bool)f;
}

long long KinectFusionReconstruction::lastUpdatedVoxels() { return last_frame_counter(0); }
long long KinectFusionReconstruction::lastRaycastHits() { return last_frame_counter(1); }
long long KinectFusionReconstruction::last_frame_counter(int which) {
    if (counter_frame_ == 0) return 0;
    unsigned long long h[2] = {0, 0};
    synchronize();
    flush_pending_fold(current_stream());
    hipSafeCall(hipStreamSynchronize(current_stream()));
    hipSafeCall(hipMemcpy(h, counters_.ptr() + 2 * (size_t)((counter_frame_ - 1) % COUNTER_RING), sizeof(h), hipMemcpyDeviceToHost));
    return (long long)h[which];
}

// ---- volume checkpoint --------------------------------------------------------------------
// reference :438-447 writes raw float32 values; here X*Y*Z of them (the reference's count uses
// res[2] twice)
void KinectFusionReconstruction::saveTSDFVolume(const std::string &tsdf_filename) {
    std::vector<float> tsdf;
    tsdf_volume_d_ptr->downloadTSDFWithoutGrad(tsdf);
    std::ofstream f(tsdf_filename, std::ios::binary);
    f.write(reinterpret_cast<const char *>(tsdf.data()), (std::streamsize)(tsdf.size() * sizeof(float)));
}
namespace {
// Volume checkpoint, version 2.  Layout: header, n_poses x Matrix4cf, then value / grad / weight of the stored planes
// [zs0, zs1) as dense rows of X elements (a rank of a sharded run saves and restores its own planes).
struct CkptHeader {
    char magic[8];
    int res[3];
    float voxel_size, tranc_dist;
    int frame_id, n_poses;
    int zs0, zs1;        // planes held in this file
    int shard_rank, shard_count;
};
const int CKPT_MAX_POSES = 1 << 24;   // a sanity bound on the pose record (16 M frames), not a format limit
// one device <- host copy of a dense array into the EXISTING pitched buffer (no reallocation, no temporaries)
template <class T>
void restore_rows(DeviceArray2D<T> dst, const std::vector<T> &src, int cols, size_t rows) {
    hipSafeCall(hipMemcpy2D(dst.ptr(), dst.step(), src.data(), (size_t)cols * sizeof(T), (size_t)cols * sizeof(T), rows, hipMemcpyHostToDevice));
}

// ---- the brick-sparse checkpoint, version 3 (pack_host.hpp: the format and its validation) ----
static_assert(sizeof(CkptHeader) == sizeof(CkptPrefix) && sizeof(Matrix4cf) == PACK_POSE_BYTES, "XSTSDF3 shares XSTSDF2's header fields and pose record");
// the one staging buffer of a sparse save or load, pinned so that the copies run at the link's rate
struct PinnedWords {
    unsigned *p = nullptr;
    explicit PinnedWords(size_t words) { hipSafeCall(hipHostMalloc((void **)&p, words * sizeof(unsigned), hipHostMallocDefault)); }
    ~PinnedWords() { if (p) (void)hipHostFree(p); }
    PinnedWords(const PinnedWords &) = delete;
    PinnedWords &operator=(const PinnedWords &) = delete;
};
// a chunk holds at most the staging buffer's words, at least one brick's, and no more than there is
uint64_t chunk_words_for(unsigned long long staging_words, uint64_t payload_words) {
    return std::max<uint64_t>(PACK_MAX_BRICK_WORDS, std::min<uint64_t>(staging_words, payload_words));
}
// An XSTSDF3 file read whole into host memory and validated in full; nothing on the device is touched or allocated.
struct SparseFile {
    PackHeader h{};
    std::vector<char> bytes;           // the file
    std::vector<uint64_t> offsets;     // nbricks + 1
    const char *poses() const { return bytes.data() + sizeof(PackHeader); }
    const unsigned char *cls() const { return reinterpret_cast<const unsigned char *>(poses() + (size_t)h.p.n_poses * PACK_POSE_BYTES); }
    const char *payload() const { return reinterpret_cast<const char *>(cls()) + pack_class_bytes_padded(h.nbricks); }
};
bool read_sparse_file(std::ifstream &f, long long file_bytes, SparseFile &s) {
    if (file_bytes < (long long)sizeof(PackHeader)) return false;
    f.seekg(0, std::ios::beg);
    f.read(reinterpret_cast<char *>(&s.h), sizeof(s.h));
    uint64_t head = 0;
    if (!f || pack_validate_header(s.h, &head) != PACK_OK) return false;
    if ((uint64_t)file_bytes != head + 4 * s.h.payload_words) return false;   // (before the file's size is allocated: the size is then what the header says)
    s.bytes.resize((size_t)file_bytes);
    f.seekg(0, std::ios::beg);
    f.read(s.bytes.data(), (std::streamsize)file_bytes);
    if (!f || pack_validate(s.h, s.cls(), (uint64_t)file_bytes, nullptr) != PACK_OK) return false;
    s.offsets.resize((size_t)s.h.nbricks + 1);
    pack_offsets(s.cls(), s.h.nbricks, s.offsets.data());
    return true;
}
// The validated file's volume into three device arrays of one pitch, at their first stored plane: class bytes up, offsets by the device's scan,
// then chunk by chunk through the pinned buffer and the unpack kernel.  Every in-volume voxel is written; the stream is drained on return.
void unpack_sparse(const SparseFile &s, float *value, int *weight, float *grad, size_t step, unsigned long long staging_words) {
    hipStream_t st = current_stream();
    const int *res = s.h.p.res, planes = s.h.p.zs1 - s.h.p.zs0;
    const uint64_t nbricks = s.h.nbricks, padded = pack_class_bytes_padded(nbricks);
    DeviceArray<unsigned char> cls_d, ws;
    DeviceArray<unsigned long long> off_d;
    DeviceArray<unsigned> pay_d;
    cls_d.create(padded);
    off_d.create(nbricks + 1);
    ws.create(xs_tsdf_pack_workspace_bytes(res, planes));
    const uint64_t chunk_words = chunk_words_for(staging_words, s.h.payload_words);
    pay_d.create(chunk_words);
    PinnedWords pin(chunk_words);
    hipSafeCall(hipMemcpyAsync(cls_d.ptr(), s.cls(), padded, hipMemcpyHostToDevice, st));
    check_rc(xs_tsdf_pack_offsets(cls_d.ptr(), nbricks, off_d.ptr(), ws.ptr(), st), "pack offsets");
    for (uint64_t b0 = 0, b1; b0 < nbricks; b0 = b1) {
        b1 = pack_chunk_end(s.offsets.data(), nbricks, b0, chunk_words);
        const size_t n = (size_t)(s.offsets[b1] - s.offsets[b0]);
        std::memcpy(pin.p, s.payload() + 4 * s.offsets[b0], 4 * n);
        hipSafeCall(hipMemcpyAsync(pay_d.ptr(), pin.p, 4 * n, hipMemcpyHostToDevice, st));
        check_rc(xs_tsdf_unpack(value, weight, grad, step, res, planes, cls_d.ptr(), off_d.ptr(), b0, b1, pay_d.ptr(), st), "unpack");
        hipSafeCall(hipStreamSynchronize(st));   // (the pinned buffer is filled again)
    }
}
}  // namespace

bool KinectFusionReconstruction::saveCheckpointSparse(const std::string &filename, unsigned long long *stats12) {
    if (stats12) std::fill(stats12, stats12 + 12, 0ull);
    if (!tsdf_volume_d_ptr) return false;
    DeviceArray2D<float> dv = tsdf_volume_d_ptr->value(), dg = tsdf_volume_d_ptr->grad();
    DeviceArray2D<int> dw = tsdf_volume_d_ptr->weight();
    if (dv.step() != dg.step() || dv.step() != dw.step()) return false;   // (TsdfVolume allocates the three arrays alike)
    const int *res = res3(), planes = zs1 - zs0;
    PackHeader h{};
    int nb[3];
    const uint64_t nbricks = pack_brick_grid(res[0], res[1], planes, nb);
    if (nbricks == 0 || xs_tsdf_pack_bricks(res, planes) != nbricks) return false;
    const uint64_t padded = pack_class_bytes_padded(nbricks);
    synchronize();
    hipStream_t st = current_stream();
    DeviceArray<unsigned char> cls_d, ws;
    DeviceArray<unsigned long long> off_d;
    cls_d.create(padded);
    off_d.create(nbricks + 1);
    ws.create(xs_tsdf_pack_workspace_bytes(res, planes));
    hipSafeCall(hipMemsetAsync(cls_d.ptr(), 0, padded, st));   // (the padding)
    check_rc(xs_tsdf_pack_classify(dv.ptr(0), dw.ptr(0), dg.ptr(0), dv.step(), res, planes, cls_d.ptr(), off_d.ptr(), ws.ptr(), st), "pack classify");
    std::vector<unsigned char> cls(padded);
    unsigned long long payload_words = 0;
    hipSafeCall(hipMemcpyAsync(cls.data(), cls_d.ptr(), padded, hipMemcpyDeviceToHost, st));
    hipSafeCall(hipMemcpyAsync(&payload_words, off_d.ptr() + nbricks, sizeof(payload_words), hipMemcpyDeviceToHost, st));
    hipSafeCall(hipStreamSynchronize(st));
    std::vector<uint64_t> offsets(nbricks + 1);
    pack_offsets(cls.data(), nbricks, offsets.data());
    if (offsets[nbricks] != payload_words) check_rc(-1, "pack classify: the device's offsets disagree with its class bytes");
    std::snprintf(h.p.magic, sizeof(h.p.magic), "XSTSDF3");
    for (int i = 0; i < 3; ++i) h.p.res[i] = volume_resolution[i];
    h.p.voxel_size = voxel_size; h.p.tranc_dist = tsdf_volume_d_ptr->getTsdfTruncDist(); h.p.frame_id = frame_id;
    h.p.n_poses = (int)world2camera_record.size();
    h.p.zs0 = zs0; h.p.zs1 = zs1; h.p.shard_rank = shard_rank; h.p.shard_count = shard_count;
    h.brick_edge = PACK_BRICK_EDGE; h.nbx = nb[0]; h.nby = nb[1]; h.nbz = nb[2]; h.reserved = 0;
    h.nbricks = nbricks; h.payload_words = payload_words;
    std::ofstream f(filename, std::ios::binary);
    if (!f) return false;
    f.write(reinterpret_cast<const char *>(&h), sizeof(h));
    f.write(reinterpret_cast<const char *>(world2camera_record.data()), (std::streamsize)((size_t)h.p.n_poses * sizeof(Matrix4cf)));
    f.write(reinterpret_cast<const char *>(cls.data()), (std::streamsize)padded);
    const uint64_t chunk_words = chunk_words_for(checkpoint_staging_words, payload_words);
    DeviceArray<unsigned> pay_d;
    pay_d.create(chunk_words);
    PinnedWords pin(chunk_words);
    unsigned long long chunks = 0;
    for (uint64_t b0 = 0, b1; b0 < nbricks; b0 = b1, ++chunks) {
        b1 = pack_chunk_end(offsets.data(), nbricks, b0, chunk_words);
        const size_t n = (size_t)(offsets[b1] - offsets[b0]);
        check_rc(xs_tsdf_pack_gather(dv.ptr(0), dw.ptr(0), dg.ptr(0), dv.step(), res, planes, cls_d.ptr(), off_d.ptr(), b0, b1, pay_d.ptr(), st), "pack gather");
        hipSafeCall(hipMemcpyAsync(pin.p, pay_d.ptr(), 4 * n, hipMemcpyDeviceToHost, st));
        hipSafeCall(hipStreamSynchronize(st));
        f.write(reinterpret_cast<const char *>(pin.p), (std::streamsize)(4 * n));
    }
    f.flush();
    if (!f) return false;
    if (stats12) {
        stats12[0] = nbricks;
        for (uint64_t b = 0; b < nbricks; ++b) ++stats12[1 + cls[b]];
        stats12[9] = payload_words;
        stats12[10] = sizeof(h) + (uint64_t)h.p.n_poses * sizeof(Matrix4cf) + padded + 4 * payload_words;
        stats12[11] = chunks;
    }
    return true;
}
void KinectFusionReconstruction::saveCheckpoint(const std::string &filename) {
    std::vector<float> v, g;
    std::vector<int> w;
    tsdf_volume_d_ptr->downloadTSDFWithGrad(v, g);
    tsdf_volume_d_ptr->downloadWeight(w);
    CkptHeader h{};
    std::snprintf(h.magic, sizeof(h.magic), "XSTSDF2");
    for (int i = 0; i < 3; ++i) h.res[i] = volume_resolution[i];
    h.voxel_size = voxel_size; h.tranc_dist = tsdf_volume_d_ptr->getTsdfTruncDist(); h.frame_id = frame_id;
    h.n_poses = (int)world2camera_record.size();
    h.zs0 = zs0; h.zs1 = zs1; h.shard_rank = shard_rank; h.shard_count = shard_count;
    std::ofstream f(filename, std::ios::binary);
    f.write(reinterpret_cast<const char *>(&h), sizeof(h));
    f.write(reinterpret_cast<const char *>(world2camera_record.data()), (std::streamsize)(h.n_poses * sizeof(Matrix4cf)));
    f.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * 4));
    f.write(reinterpret_cast<const char *>(g.data()), (std::streamsize)(g.size() * 4));
    f.write(reinterpret_cast<const char *>(w.data()), (std::streamsize)(w.size() * 4));
}
// Nothing of *this is touched until the whole file has been read and validated: magic, volume geometry (resolution,
// voxel size, truncation distance), the planes it holds against the planes this instance stores, a sane pose count and
// the exact file length.  Returns false (state unchanged) on any mismatch.
bool KinectFusionReconstruction::loadCheckpoint(const std::string &filename) {
    std::ifstream f(filename, std::ios::binary);
    if (!f || !tsdf_volume_d_ptr) return false;
    f.seekg(0, std::ios::end);
    const long long file_bytes = (long long)f.tellg();
    f.seekg(0, std::ios::beg);
    CkptHeader h{};
    if (file_bytes < (long long)sizeof(h)) return false;
    f.read(reinterpret_cast<char *>(&h), sizeof(h));
    if (!f) return false;
    // what follows the restored volume, whichever format it came in
    auto commit = [&](std::vector<Matrix4cf> &poses, int file_frame_id) {
        ++volume_generation;
        RebuildSignMap();    // the volume was written behind the integrate kernels' back
        world2camera_record.swap(poses);
        world2camera = world2camera_record.back();
        frame_id = file_frame_id;
        // previous-frame maps are derived state: regenerate them from the restored volume and pose (in a sharded run every
        // rank must load its own file before the next frame: the raycast composite is a collective)
        CalculatePointCloud(vmaps_g_prev_d[0], nmaps_g_prev_d[0]);
        ModelMapPyramid();
        synchronize();
    };
    if (std::memcmp(h.magic, "XSTSDF3", 8) == 0) {
        // the brick-sparse format: the same geometry and shard checks against this instance, and pack_validate's on the file itself, which is read
        // whole into host memory before anything is touched
        SparseFile s;
        if (!read_sparse_file(f, file_bytes, s)) return false;
        const CkptPrefix &p = s.h.p;
        for (int i = 0; i < 3; ++i) if (p.res[i] != volume_resolution[i]) return false;
        if (p.voxel_size != voxel_size || p.tranc_dist != tsdf_volume_d_ptr->getTsdfTruncDist()) return false;
        if (p.zs0 != zs0 || p.zs1 != zs1 || p.shard_rank != shard_rank || p.shard_count != shard_count || p.frame_id < 0) return false;
        DeviceArray2D<float> dv = tsdf_volume_d_ptr->value(), dg = tsdf_volume_d_ptr->grad();
        DeviceArray2D<int> dw = tsdf_volume_d_ptr->weight();
        const size_t rows = (size_t)p.res[1] * (size_t)(p.zs1 - p.zs0);
        if ((size_t)dv.rows() != rows || dv.cols() != p.res[0] || (size_t)dg.rows() != rows || (size_t)dw.rows() != rows) return false;
        if (dv.step() != dg.step() || dv.step() != dw.step()) return false;
        std::vector<Matrix4cf> poses((size_t)p.n_poses);
        std::memcpy(static_cast<void *>(poses.data()), s.poses(), poses.size() * sizeof(Matrix4cf));
        // validated: commit
        synchronize();
        unpack_sparse(s, dv.ptr(0), dw.ptr(0), dg.ptr(0), dv.step(), checkpoint_staging_words);
        commit(poses, p.frame_id);
        return true;
    }
    if (std::memcmp(h.magic, "XSTSDF2", 8) != 0) return false;
    for (int i = 0; i < 3; ++i) if (h.res[i] != volume_resolution[i]) return false;
    if (h.voxel_size != voxel_size || h.tranc_dist != tsdf_volume_d_ptr->getTsdfTruncDist()) return false;
    if (h.zs0 != zs0 || h.zs1 != zs1 || h.shard_rank != shard_rank || h.shard_count != shard_count) return false;
    if (h.n_poses < 1 || h.n_poses > CKPT_MAX_POSES || h.frame_id < 0) return false;
    const int X = h.res[0];
    const size_t rows = (size_t)h.res[1] * (size_t)(h.zs1 - h.zs0), n = rows * (size_t)X;
    const long long expect = (long long)sizeof(h) + (long long)h.n_poses * (long long)sizeof(Matrix4cf) + 3LL * (long long)n * 4LL;
    if (file_bytes != expect) return false;            // truncated or trailing bytes
    std::vector<Matrix4cf> poses((size_t)h.n_poses);
    f.read(reinterpret_cast<char *>(poses.data()), (std::streamsize)(poses.size() * sizeof(Matrix4cf)));
    std::vector<float> v(n), g(n);
    std::vector<int> w(n);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(n * 4));
    f.read(reinterpret_cast<char *>(g.data()), (std::streamsize)(n * 4));
    f.read(reinterpret_cast<char *>(w.data()), (std::streamsize)(n * 4));
    if (!f) return false;
    DeviceArray2D<float> dv = tsdf_volume_d_ptr->value(), dg = tsdf_volume_d_ptr->grad();
    DeviceArray2D<int> dw = tsdf_volume_d_ptr->weight();
    if ((size_t)dv.rows() != rows || dv.cols() != X || (size_t)dg.rows() != rows || (size_t)dw.rows() != rows) return false;
    // validated: commit
    synchronize();
    restore_rows(dv, v, X, rows);
    restore_rows(dg, g, X, rows);
    restore_rows(dw, w, X, rows);
    commit(poses, h.frame_id);
    return true;
}

// ---- merging a second map ----------------------------------------------------------------------------------
int KinectFusionReconstruction::MergeVolume(const float *src_value, const int *src_weight, const float *src_grad, size_t src_step, const int *src_res,
                                            float src_voxel_size, float src_tranc_dist, const double *T16, int min_weight, unsigned long long *written) {
    if (shard_count > 1) return -2;   // the source's image in a rank's z-slab needs the whole source on every rank: not built
    if (!tsdf_volume_d_ptr) return 0;
    if (!src_value || !src_weight || !src_grad || !src_res || !T16 || min_weight < 1) return -1;
    for (int k = 0; k < 3; ++k)
        if (src_res[k] < 1) return -1;
    if (!(src_voxel_size > 0.f) || !std::isfinite(src_voxel_size) || src_tranc_dist != tsdf_volume_d_ptr->getTsdfTruncDist()) return -1;
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value(), grad = tsdf_volume_d_ptr->grad();
    DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    if (src_value == value.ptr(0) || src_weight == weight.ptr(0) || src_grad == grad.ptr(0)) return -1;
    float xform[12];
    if (!merge_affine(T16, (double)voxel_size, (double)src_voxel_size, xform)) return -1;
    const size_t ws_bytes = xs_tsdf_merge_workspace_bytes(res3(), src_res);
    if (ws_bytes == 0 || src_step % 4 != 0 || src_step < (size_t)src_res[0] * 4) return -1;
    // the source may belong to another instance with streams of its own: drain the device, not just this instance's stream
    synchronize();
    hipSafeCall(hipDeviceSynchronize());
    DeviceArray<unsigned char> ws;
    ws.create(ws_bytes);
    DeviceArray<unsigned long long> count;
    count.create(1);
    hipSafeCall(hipMemsetAsync(count.ptr(), 0, sizeof(unsigned long long), current_stream()));
    check_rc(xs_tsdf_merge(value.ptr(0), weight.ptr(0), grad.ptr(0), value.step(), res3(), 0, res3()[2], src_value, src_weight, src_grad, src_step, src_res,
                           xform, min_weight, max_integration_weight, 0u, count.ptr(), ws.ptr(), current_stream()), "merge");
    ++volume_generation;
    RebuildSignMap();    // the volume was written behind the integrate kernels' back
    sign_map_stale_ = false;
    invalidate_derived_maps();
    CalculatePointCloud(vmaps_g_prev_d[0], nmaps_g_prev_d[0]);
    ModelMapPyramid();
    synchronize();
    if (written) hipSafeCall(hipMemcpy(written, count.ptr(), sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 1;
}

namespace {
// A checkpoint file of a whole volume in either format (XSTSDF2: dense; XSTSDF3: brick-sparse, pack_validate on top), validated in full (magic, exact length,
// shard_count 1, the truncation distance `tranc_dist`) and uploaded, the dense file as it is, the sparse one compact and expanded by the unpack kernel,
// to a temporary device volume with one pitch for the three arrays.  False on any mismatch, with nothing allocated.
struct CkptVolume {
    CkptHeader h{};
    DeviceArray2D<float> dv, dg;
    DeviceArray2D<int> dw;
};
bool upload_whole_checkpoint(const std::string &filename, float tranc_dist, unsigned long long staging_words, CkptVolume &out) {
    CkptHeader &h = out.h;
    std::ifstream f(filename, std::ios::binary);
    if (!f) return false;
    f.seekg(0, std::ios::end);
    const long long file_bytes = (long long)f.tellg();
    f.seekg(0, std::ios::beg);
    if (file_bytes < (long long)sizeof(h)) return false;
    f.read(reinterpret_cast<char *>(&h), sizeof(h));
    if (!f) return false;
    const bool sparse = std::memcmp(h.magic, "XSTSDF3", 8) == 0;
    if (!sparse && std::memcmp(h.magic, "XSTSDF2", 8) != 0) return false;
    for (int i = 0; i < 3; ++i)
        if (h.res[i] < 1 || h.res[i] > 65535) return false;
    if (h.shard_count != 1 || h.shard_rank != 0 || h.zs0 != 0 || h.zs1 != h.res[2]) return false;   // a whole volume
    if (!(h.voxel_size > 0.f) || !std::isfinite(h.voxel_size) || h.tranc_dist != tranc_dist) return false;
    if (h.n_poses < 1 || h.n_poses > CKPT_MAX_POSES) return false;
    const int X = h.res[0];
    const size_t rows = (size_t)h.res[1] * (size_t)h.res[2], n = rows * (size_t)X;
    if (rows >= (size_t)1 << 31) return false;
    if (sparse) {   // the compact file up, the temporary volume filled by the unpack kernel (the header's first 52 bytes are the fields checked above)
        SparseFile s;
        if (!read_sparse_file(f, file_bytes, s)) return false;
        out.dv.create((int)rows, X); out.dg.create((int)rows, X); out.dw.create((int)rows, X);
        if (out.dv.step() != out.dg.step() || out.dv.step() != out.dw.step()) return false;
        unpack_sparse(s, out.dv.ptr(0), out.dw.ptr(0), out.dg.ptr(0), out.dv.step(), staging_words);
        return true;
    }
    const long long expect = (long long)sizeof(h) + (long long)h.n_poses * (long long)sizeof(Matrix4cf) + 3LL * (long long)n * 4LL;
    if (file_bytes != expect) return false;            // truncated or trailing bytes
    f.seekg((std::streamoff)((long long)sizeof(h) + (long long)h.n_poses * (long long)sizeof(Matrix4cf)), std::ios::beg);
    std::vector<float> v(n), g(n);
    std::vector<int> w(n);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(n * 4));
    f.read(reinterpret_cast<char *>(g.data()), (std::streamsize)(n * 4));
    f.read(reinterpret_cast<char *>(w.data()), (std::streamsize)(n * 4));
    if (!f) return false;
    out.dv.create((int)rows, X); out.dg.create((int)rows, X); out.dw.create((int)rows, X);
    if (out.dv.step() != out.dg.step() || out.dv.step() != out.dw.step()) return false;
    restore_rows(out.dv, v, X, rows);
    restore_rows(out.dg, g, X, rows);
    restore_rows(out.dw, w, X, rows);
    return true;
}
}  // namespace

int KinectFusionReconstruction::MergeCheckpoint(const std::string &filename, const double *T16, int min_weight, unsigned long long *written) {
    if (shard_count > 1) return -2;
    if (!tsdf_volume_d_ptr) return 0;
    if (!T16 || min_weight < 1) return -1;
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(T16[i])) return -1;
    CkptVolume c;
    if (!upload_whole_checkpoint(filename, tsdf_volume_d_ptr->getTsdfTruncDist(), checkpoint_staging_words, c)) return -1;
    return MergeVolume(c.dv.ptr(0), c.dw.ptr(0), c.dg.ptr(0), c.dv.step(), c.h.res, c.h.voxel_size, c.h.tranc_dist, T16, min_weight, written);
}

// ---- aligning a second map -----------------------------------------------------------------------------------
int KinectFusionReconstruction::AlignVolume(const float *src_value, const int *src_weight, size_t src_step, const int *src_res, float src_voxel_size,
                                            float src_tranc_dist, const double *T16xN, int N, int iterations, double damping, int min_weight,
                                            float max_residual, double *T16_out, double report[8], std::vector<double> *loss_history) {
    if (report) { for (int i = 0; i < 8; ++i) report[i] = 0.0; report[0] = -1.0; }
    if (shard_count > 1) return -2;   // the band index of a rank holds its own planes, the sums would need the all-reduce: not built
    if (!tsdf_volume_d_ptr) return 0;
    if (!src_value || !src_weight || !src_res || !T16xN || !T16_out || N < 1 || iterations < 0 || min_weight < 1) return -1;
    if (!(max_residual > 0.f) || !std::isfinite(max_residual) || !(damping >= 0.0) || !std::isfinite(damping)) return -1;
    for (int k = 0; k < 3; ++k)
        if (src_res[k] < 2) return -1;
    if (!(src_voxel_size > 0.f) || !std::isfinite(src_voxel_size) || src_tranc_dist != tsdf_volume_d_ptr->getTsdfTruncDist()) return -1;
    if (src_value == tsdf_volume_d_ptr->value().ptr(0) || src_weight == tsdf_volume_d_ptr->weight().ptr(0)) return -1;
    if (src_step % 4 != 0 || src_step < (size_t)src_res[0] * 4) return -1;
    std::vector<double> T((size_t)N * 16);
    float probe[6][24];
    for (int n = 0; n < N; ++n) {
        for (int i = 0; i < 16; ++i) T[(size_t)n * 16 + i] = T16xN[(size_t)n * 16 + i];
        if (!align_seeded_maps(&T[(size_t)n * 16], (double)voxel_size, (double)src_voxel_size, probe)) return -1;
    }
    // the source may belong to another instance with streams of its own: drain the device, not just this instance's stream
    synchronize();
    hipSafeCall(hipDeviceSynchronize());
    BandIndexPrepare();
    ensure_reduce_workspace(reloc_.align_ws, xs_tsdf_align_workspace_bytes(XS_ALIGN_MAX_TRANSFORMS), "align workspace");
    if (reloc_.align_sums.size() < (size_t)XS_ALIGN_MAX_TRANSFORMS * 29) reloc_.align_sums.create((size_t)XS_ALIGN_MAX_TRANSFORMS * 29);
    std::vector<std::vector<double>> history((size_t)N);   // (always kept: the last pass's sums pick the winner)
    std::vector<double> last((size_t)N * 29, 0.0);
    std::vector<int> ok((size_t)N, 0);
    std::vector<float> maps((size_t)XS_ALIGN_MAX_TRANSFORMS * 144);
    int passes = 0;
    gn_batch_loop(N, iterations, history.data(), ok.data(), XS_ALIGN_MAX_TRANSFORMS,
        [&](const int *starts, int n, double *sums) {
            for (int i = 0; i < n; ++i) {
                float *m = &maps[(size_t)i * 144];
                if (align_seeded_maps(&T[(size_t)starts[i] * 16], (double)voxel_size, (double)src_voxel_size, reinterpret_cast<float (*)[24]>(m))) continue;
                // a step took T out of float32's range: a map that misses the source (every index is -1), so the start ends with count 0 and fails
                std::fill(m, m + 144, 0.f);
                for (int k = 0; k < 6; ++k)
                    for (int a = 0; a < 3; ++a) m[24 * k + 2 * (9 + a)] = -1.f;
            }
            check_rc(xs_tsdf_align_terms(n, &reloc_.band, src_value, src_weight, src_step, src_res, maps.data(), min_weight, max_residual, reloc_.align_ws.ptr(),
                                         reloc_.align_sums.ptr(), current_stream()), "AlignTerms");
            fetch_sums(reloc_.align_sums.ptr(), (size_t)n * 29, sums);
            ++passes;
            for (int i = 0; i < n; ++i) {
                gn_scale_sums(sums + 29 * i, sums + 29 * i);
                std::copy(sums + 29 * i, sums + 29 * i + 29, last.begin() + (size_t)starts[i] * 29);
            }
        },
        [&](int n, const double *s, int) { return align_step(s, damping, &T[(size_t)n * 16]); });
    // the winner: the start that ended ok, with at least six voxels in its last pass too (gn_batch_loop lets the loss pass end ok whatever it
    // counts: a start that its last step, or no step at all, left off the other map is no result), with the highest S = count - sum r^2
    // (relocalize_global's score; ties: the lower index)
    auto S = [&](int n) { return last[(size_t)n * 29 + 28] - last[(size_t)n * 29 + 27]; };
    int win = -1, ended_ok = 0;
    for (int n = 0; n < N; ++n) {
        if (!ok[(size_t)n] || last[(size_t)n * 29 + 28] < 6) continue;
        ++ended_ok;
        if (win < 0 || S(n) > S(win)) win = n;
    }
    if (report) { report[4] = (double)passes; report[5] = (double)ended_ok; report[6] = (double)reloc_.band.count; }
    if (win < 0) return 0;
    const double *s = &last[(size_t)win * 29];
    for (int i = 0; i < 16; ++i) T16_out[i] = T[(size_t)win * 16 + i];
    if (report) { report[0] = (double)win; report[1] = s[28]; report[2] = s[27]; report[3] = s[28] > 0 ? s[27] / s[28] : 0.0; }
    if (loss_history) *loss_history = history[(size_t)win];
    return 1;
}

int KinectFusionReconstruction::AlignCheckpoint(const std::string &filename, const double *T16xN, int N, int iterations, double damping, int min_weight,
                                                float max_residual, double *T16_out, double report[8], std::vector<double> *loss_history) {
    if (report) { for (int i = 0; i < 8; ++i) report[i] = 0.0; report[0] = -1.0; }
    if (shard_count > 1) return -2;
    if (!tsdf_volume_d_ptr) return 0;
    if (!T16xN || !T16_out || N < 1) return -1;
    for (int i = 0; i < 16 * N; ++i)
        if (i % 16 < 12 && !std::isfinite(T16xN[i])) return -1;
    CkptVolume c;
    if (!upload_whole_checkpoint(filename, tsdf_volume_d_ptr->getTsdfTruncDist(), checkpoint_staging_words, c)) return -1;
    return AlignVolume(c.dv.ptr(0), c.dw.ptr(0), c.dv.step(), c.h.res, c.h.voxel_size, c.h.tranc_dist, T16xN, N, iterations, damping, min_weight, max_residual,
                       T16_out, report, loss_history);
}

// ---- many transforms against the other map, and alignment with no initial guess --------------------------------
namespace {
// the other map of a scoring call or a search, as AlignVolume checks its own
bool other_map_ok(const KinectFusionReconstruction &k, const float *src_value, const int *src_weight, size_t src_step, const int *src_res, float src_voxel_size,
                  float src_tranc_dist) {
    if (!src_value || !src_weight || !src_res) return false;
    for (int a = 0; a < 3; ++a)
        if (src_res[a] < 2) return false;
    if (!(src_voxel_size > 0.f) || !std::isfinite(src_voxel_size) || src_tranc_dist != k.tsdf_volume_d_ptr->getTsdfTruncDist()) return false;
    if (src_value == k.tsdf_volume_d_ptr->value().ptr(0) || src_weight == k.tsdf_volume_d_ptr->weight().ptr(0)) return false;
    return src_step % 4 == 0 && src_step >= (size_t)src_res[0] * 4;
}
}  // namespace
int KinectFusionReconstruction::ScoreTransformsVolume(const float *src_value, const int *src_weight, size_t src_step, const int *src_res, float src_voxel_size,
                                                      float src_tranc_dist, const double *T16xP, int P, int stride, int min_weight, float max_residual,
                                                      double *out2xP, int *launches) {
    if (shard_count > 1) return -2;   // as AlignVolume: a rank's band index holds its own planes
    if (!tsdf_volume_d_ptr) return 0;
    if (!T16xP || !out2xP || P < 1 || stride < 1 || min_weight < 1 || !(max_residual > 0.f) || !std::isfinite(max_residual)) return -1;
    if (!other_map_ok(*this, src_value, src_weight, src_step, src_res, src_voxel_size, src_tranc_dist)) return -1;
    std::vector<float> xforms((size_t)P * 12);
    for (int p = 0; p < P; ++p)
        if (!merge_affine(T16xP + 16 * (size_t)p, (double)voxel_size, (double)src_voxel_size, &xforms[(size_t)p * 12])) return -1;
    // the source may belong to another instance with streams of its own: drain the device, not just this instance's stream
    synchronize();
    hipSafeCall(hipDeviceSynchronize());
    BandIndexPrepare();
    ensure_reduce_workspace(reloc_.ascore_ws, xs_tsdf_score_transforms_workspace_bytes(XS_ALIGN_SCORE_MAX_TRANSFORMS), "transform score workspace");
    if (reloc_.ascore_sums.size() < (size_t)XS_ALIGN_SCORE_MAX_TRANSFORMS * 2) reloc_.ascore_sums.create((size_t)XS_ALIGN_SCORE_MAX_TRANSFORMS * 2);
    for (int p0 = 0; p0 < P; p0 += XS_ALIGN_SCORE_MAX_TRANSFORMS) {
        const int n = std::min(P - p0, (int)XS_ALIGN_SCORE_MAX_TRANSFORMS);
        check_rc(xs_tsdf_score_transforms(n, &reloc_.band, stride, src_value, src_weight, src_step, src_res, &xforms[(size_t)p0 * 12], min_weight, max_residual,
                                          reloc_.ascore_ws.ptr(), reloc_.ascore_sums.ptr(), current_stream()), "ScoreTransforms");
        fetch_sums(reloc_.ascore_sums.ptr(), (size_t)n * 2, out2xP + 2 * (size_t)p0);
        if (launches) ++*launches;
    }
    return 1;
}

int KinectFusionReconstruction::ScoreTransformsCheckpoint(const std::string &filename, const double *T16xP, int P, int stride, int min_weight, float max_residual,
                                                          double *out2xP) {
    if (shard_count > 1) return -2;
    if (!tsdf_volume_d_ptr) return 0;
    if (!T16xP || !out2xP || P < 1) return -1;
    CkptVolume c;
    if (!upload_whole_checkpoint(filename, tsdf_volume_d_ptr->getTsdfTruncDist(), checkpoint_staging_words, c)) return -1;
    return ScoreTransformsVolume(c.dv.ptr(0), c.dw.ptr(0), c.dv.step(), c.h.res, c.h.voxel_size, c.h.tranc_dist, T16xP, P, stride, min_weight, max_residual, out2xP);
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

int KinectFusionReconstruction::AlignVolumeGlobal(const float *src_value, const int *src_weight, size_t src_step, const int *src_res, float src_voxel_size,
                                                  float src_tranc_dist, const xs_align_search_opts *opts, double *T16_out, double report[12]) {
    if (report) { for (int i = 0; i < 12; ++i) report[i] = 0.0; report[0] = -1.0; }
    if (shard_count > 1) return -2;
    if (!tsdf_volume_d_ptr) return 0;
    xs_align_search_opts o;
    if (opts) o = *opts; else AlignSearchDefaults(&o);
    if (!T16_out || !search_opts_ok(o) || !other_map_ok(*this, src_value, src_weight, src_step, src_res, src_voxel_size, src_tranc_dist)) return -1;
    const float max_residual = (float)o.max_residual;
    // the source may belong to another instance with streams of its own: drain the device, not just this instance's stream
    synchronize();
    hipSafeCall(hipDeviceSynchronize());
    BandIndexPrepare();
    std::vector<double> cand, out2;
    int launches = 0;
    auto score = [&]() {
        out2.resize(cand.size() / 16 * 2);
        return ScoreTransformsVolume(src_value, src_weight, src_step, src_res, src_voxel_size, src_tranc_dist, cand.data(), (int)(cand.size() / 16), o.stride,
                                     o.min_weight, max_residual, out2.data(), &launches);
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
    // the other map's from one band build over the source (count, then fill) into temporary buffers: the other instance's caches stay
    {
        hipStream_t st = current_stream();
        const int X = src_res[0];
        const size_t rows = (size_t)src_res[1] * (size_t)src_res[2];
        DeviceArray<float> packed;
        const float *dense = src_value;
        if (src_step != (size_t)X * 4) {   // the band walk indexes a dense array
            packed.create(rows * (size_t)X);
            hipSafeCall(hipMemcpy2DAsync(packed.ptr(), (size_t)X * 4, src_value, src_step, (size_t)X * 4, rows, hipMemcpyDeviceToDevice, st));
            dense = packed.ptr();
        }
        const size_t segs_bytes = xs_tsdf_band_segs_bytes(src_res, 0, src_res[2]);
        if (segs_bytes == 0) return -1;
        DeviceArray<long long> segs;
        segs.create(segs_bytes / sizeof(long long));
        DeviceArray<unsigned long long> keys_d;
        DeviceArray<float> values_d;
        xs_band_index idx = {};
        idx.segs = segs.ptr();
        int rc = xs_tsdf_band_build(dense, src_res, 0, src_res[2], &idx, st);
        if (rc == XS_BAND_OVER_CAPACITY) {
            keys_d.create((size_t)idx.count);
            values_d.create((size_t)idx.count);
            idx.keys = keys_d.ptr(); idx.values = values_d.ptr(); idx.capacity = idx.count;
            rc = xs_tsdf_band_build(dense, src_res, 0, src_res[2], &idx, st);
        }
        check_rc(rc, "the other map's band");
        std::vector<unsigned long long> keys((size_t)idx.count);
        if (idx.count > 0) hipSafeCall(hipMemcpy(keys.data(), idx.keys, (size_t)idx.count * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (!band_centroid(keys.data(), idx.count, (double)src_voxel_size, c_other)) return 0;
    }
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
    int rc = score();
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
    rc = AlignVolume(src_value, src_weight, src_step, src_res, src_voxel_size, src_tranc_dist, kept.data(), (int)kept_S.size(), o.iterations, o.damping, o.min_weight,
                     max_residual, T, r8, nullptr);
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

int KinectFusionReconstruction::AlignCheckpointGlobal(const std::string &filename, const xs_align_search_opts *opts, double *T16_out, double report[12]) {
    if (report) { for (int i = 0; i < 12; ++i) report[i] = 0.0; report[0] = -1.0; }
    if (shard_count > 1) return -2;
    if (!tsdf_volume_d_ptr) return 0;
    if (!T16_out || (opts && !search_opts_ok(*opts))) return -1;
    CkptVolume c;
    if (!upload_whole_checkpoint(filename, tsdf_volume_d_ptr->getTsdfTruncDist(), checkpoint_staging_words, c)) return -1;
    return AlignVolumeGlobal(c.dv.ptr(0), c.dw.ptr(0), c.dv.step(), c.h.res, c.h.voxel_size, c.h.tranc_dist, opts, T16_out, report);
}

// ---- what differs between this map and a second map ------------------------------------------------------------
int KinectFusionReconstruction::DiffVolume(const float *src_value, const int *src_weight, size_t src_step, const int *src_res, float src_voxel_size,
                                           float src_tranc_dist, const double *T16, int min_weight, float lo, float hi, int cell, unsigned long long min_size,
                                           int capacity, unsigned long long *this_records8, int *this_count, unsigned long long *other_records8,
                                           int *other_count, unsigned long long counts3[3], unsigned char *this_dense, unsigned char *other_dense) {
    if (shard_count > 1) return -2;   // the source's image in a rank's z-slab needs the whole source on every rank, and a cluster is not additive over slabs
    if (!this_count || !other_count || capacity < 0 || (capacity > 0 && (!this_records8 || !other_records8)) || !frontier_cell_valid(cell)) return -1;
    if (!tsdf_volume_d_ptr) return 0;
    if (!src_value || !src_weight || !src_res || !T16 || min_weight < 1) return -1;
    if (!std::isfinite(lo) || !std::isfinite(hi) || lo > hi) return -1;
    for (int k = 0; k < 3; ++k)
        if (src_res[k] < 1) return -1;
    if (!(src_voxel_size > 0.f) || !std::isfinite(src_voxel_size) || src_tranc_dist != tsdf_volume_d_ptr->getTsdfTruncDist()) return -1;
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value();
    DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    if (src_value == value.ptr(0) || src_weight == weight.ptr(0)) return -1;
    float xform[12];
    if (!merge_affine(T16, (double)voxel_size, (double)src_voxel_size, xform)) return -1;
    const int *res = res3();
    const size_t ws_bytes = xs_tsdf_diff_workspace_bytes(res, src_res), mask_bytes = xs_frontier_mask_bytes(res), label_bytes = xs_frontier_label_bytes(res);
    if (ws_bytes == 0 || mask_bytes == 0 || label_bytes == 0 || res[0] > 65535 || src_step % 4 != 0 || src_step < (size_t)src_res[0] * 4) return -1;
    // the source may belong to another instance with streams of its own: drain the device, not just this instance's stream
    synchronize();
    hipSafeCall(hipDeviceSynchronize());
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
    check_rc(xs_tsdf_diff(value.ptr(0), weight.ptr(0), value.step(), res, src_value, src_weight, src_step, src_res, xform, min_weight, lo, hi, 0u, mask[0], mask[1],
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

int KinectFusionReconstruction::DiffCheckpoint(const std::string &filename, const double *T16, int min_weight, float lo, float hi, int cell,
                                               unsigned long long min_size, int capacity, unsigned long long *this_records8, int *this_count,
                                               unsigned long long *other_records8, int *other_count, unsigned long long counts3[3], unsigned char *this_dense,
                                               unsigned char *other_dense) {
    if (shard_count > 1) return -2;
    if (!tsdf_volume_d_ptr) return 0;
    if (!T16 || min_weight < 1) return -1;
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(T16[i])) return -1;
    CkptVolume c;
    if (!upload_whole_checkpoint(filename, tsdf_volume_d_ptr->getTsdfTruncDist(), checkpoint_staging_words, c)) return -1;
    return DiffVolume(c.dv.ptr(0), c.dw.ptr(0), c.dv.step(), c.h.res, c.h.voxel_size, c.h.tranc_dist, T16, min_weight, lo, hi, cell, min_size, capacity,
                      this_records8, this_count, other_records8, other_count, counts3, this_dense, other_dense);
}
