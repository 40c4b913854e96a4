// kf_checkpoint.cpp — the volume checkpoint in its two formats: the dense XSTSDF2 and the brick-sparse XSTSDF3 (pack_host.hpp: the
// formats' rules).  Both save routines, the one host-side reader of either format (CheckpointFile) with its one write into device arrays, and
// loadCheckpoint.  None of it runs during tracking.
#include "kf_internal.hpp"
#include <cstdio>
#include <fstream>

using namespace xs_host;

namespace {
static_assert(sizeof(Matrix4cf) == PACK_POSE_BYTES, "the pose record of both formats");
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
// the 52 bytes both formats begin with, as a save of `k` writes them
CkptPrefix prefix_of(const KinectFusionReconstruction &k, const char *magic) {
    CkptPrefix p{};
    std::snprintf(p.magic, sizeof(p.magic), "%s", magic);
    for (int i = 0; i < 3; ++i) p.res[i] = k.volume_resolution[i];
    p.voxel_size = k.voxel_size; p.tranc_dist = k.tsdf_volume_d_ptr->getTsdfTruncDist(); p.frame_id = k.frame_id;
    p.n_poses = (int)k.world2camera_record.size();
    p.zs0 = k.zs0; p.zs1 = k.zs1; p.shard_rank = k.shard_rank; p.shard_count = k.shard_count;
    return p;
}
bool read_sparse_file(std::ifstream &f, uint64_t file_bytes, SparseFile &s) {
    if (file_bytes < sizeof(PackHeader)) return false;
    f.seekg(0, std::ios::beg);
    f.read(reinterpret_cast<char *>(&s.h), sizeof(s.h));
    uint64_t head = 0;
    if (!f || pack_validate_header(s.h, &head) != PACK_OK) return false;
    if (file_bytes != head + 4 * s.h.payload_words) return false;   // (before the file's size is allocated: the size is then what the header says)
    s.bytes.resize((size_t)file_bytes);
    f.seekg(0, std::ios::beg);
    f.read(s.bytes.data(), (std::streamsize)file_bytes);
    if (!f || pack_validate(s.h, s.cls(), file_bytes, nullptr) != PACK_OK) return false;
    s.offsets.resize((size_t)s.h.nbricks + 1);
    pack_offsets(s.cls(), s.h.nbricks, s.offsets.data());
    return true;
}
// one device <- host copy of a dense array into an EXISTING pitched buffer (no reallocation, no temporaries)
template <class T>
void restore_rows(T *dst, size_t step, const std::vector<T> &src, int cols, size_t rows) {
    hipSafeCall(hipMemcpy2D(dst, step, src.data(), (size_t)cols * sizeof(T), (size_t)cols * sizeof(T), rows, hipMemcpyHostToDevice));
}
// The sparse file's volume: class bytes up, offsets by the device's scan, then chunk by chunk through the pinned buffer and the unpack kernel.
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

bool CheckpointFile::read(const std::string &filename) {
    std::ifstream f(filename, std::ios::binary);
    if (!f) return false;
    f.seekg(0, std::ios::end);
    const long long end = (long long)f.tellg();
    f.seekg(0, std::ios::beg);
    CkptPrefix &p = sparse.h.p;
    if (end < (long long)sizeof(p)) return false;
    const uint64_t file_bytes = (uint64_t)end;
    f.read(reinterpret_cast<char *>(&p), sizeof(p));
    if (!f) return false;
    is_sparse = pack_magic_is(p.magic, "XSTSDF3");
    if (is_sparse) {
        if (!read_sparse_file(f, file_bytes, sparse)) return false;
        poses.resize((size_t)p.n_poses);
        std::memcpy(static_cast<void *>(poses.data()), sparse.poses(), poses.size() * sizeof(Matrix4cf));
        return true;
    }
    uint64_t words = 0;
    if (pack_validate_dense(p, file_bytes, &words) != PACK_OK) return false;
    const size_t n = (size_t)(words / 3);
    poses.resize((size_t)p.n_poses);
    value.resize(n); grad.resize(n); weight.resize(n);
    f.read(reinterpret_cast<char *>(poses.data()), (std::streamsize)(poses.size() * sizeof(Matrix4cf)));
    f.read(reinterpret_cast<char *>(value.data()), (std::streamsize)(n * 4));
    f.read(reinterpret_cast<char *>(grad.data()), (std::streamsize)(n * 4));
    f.read(reinterpret_cast<char *>(weight.data()), (std::streamsize)(n * 4));
    return (bool)f;
}
void CheckpointFile::write_to(float *dv, int *dw, float *dg, size_t step, unsigned long long staging_words) const {
    if (is_sparse) return unpack_sparse(sparse, dv, dw, dg, step, staging_words);
    const CkptPrefix &p = prefix();
    const size_t rows = (size_t)p.res[1] * (size_t)(p.zs1 - p.zs0);
    restore_rows(dv, step, value, p.res[0], rows);
    restore_rows(dg, step, grad, p.res[0], rows);
    restore_rows(dw, step, weight, p.res[0], rows);
}

// xs_host_checkpoint_info (include/xslam_amd_pipeline.h: the layout of out32): a file's header and what its format's validation says.  No device call.
int xs_host::checkpoint_info(const char *path, double *out32) {
    if (!path || !out32) return -1;
    for (int i = 0; i < 32; ++i) out32[i] = 0.0;
    std::ifstream f(path, std::ios::binary);
    if (!f) return -1;
    f.seekg(0, std::ios::end);
    const long long file_bytes = (long long)f.tellg();
    f.seekg(0, std::ios::beg);
    PackHeader h{};
    if (file_bytes < (long long)sizeof(CkptPrefix)) return -1;
    f.read(reinterpret_cast<char *>(&h.p), sizeof(h.p));
    if (!f) return -1;
    const bool v3 = pack_magic_is(h.p.magic, "XSTSDF3"), v2 = pack_magic_is(h.p.magic, "XSTSDF2");
    if (!v2 && !v3) return -1;
    const CkptPrefix &p = h.p;
    out32[0] = v3 ? 3.0 : 2.0;
    for (int i = 0; i < 3; ++i) out32[2 + i] = p.res[i];
    out32[5] = p.voxel_size; out32[6] = p.tranc_dist; out32[7] = p.frame_id; out32[8] = p.n_poses; out32[9] = p.zs0; out32[10] = p.zs1;
    out32[11] = p.shard_rank; out32[12] = p.shard_count;
    out32[27] = (double)file_bytes;
    PackError e = PACK_OK;
    if (v2) {
        uint64_t words = 0;
        e = pack_validate_dense(p, (uint64_t)file_bytes, &words);
        out32[26] = (double)words;
    } else {
        if (file_bytes < (long long)sizeof(PackHeader)) e = PACK_BAD_LENGTH;
        else {
            f.read(reinterpret_cast<char *>(&h) + sizeof(h.p), sizeof(h) - sizeof(h.p));
            out32[13] = h.brick_edge; out32[14] = h.nbx; out32[15] = h.nby; out32[16] = h.nbz;
            out32[17] = (double)h.nbricks; out32[26] = (double)h.payload_words;
            uint64_t head = 0;
            e = f ? pack_validate_header(h, &head) : PACK_BAD_LENGTH;
            if (e == PACK_OK) {
                if ((uint64_t)file_bytes < head) e = PACK_BAD_LENGTH;
                else {
                    std::vector<unsigned char> cls((size_t)pack_class_bytes_padded(h.nbricks));
                    f.seekg((std::streamoff)(sizeof(PackHeader) + (uint64_t)p.n_poses * PACK_POSE_BYTES), std::ios::beg);
                    f.read(reinterpret_cast<char *>(cls.data()), (std::streamsize)cls.size());
                    uint64_t hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    e = f ? pack_validate(h, cls.data(), (uint64_t)file_bytes, hist) : PACK_BAD_LENGTH;
                    for (int c = 0; c < 8; ++c) out32[18 + c] = (double)hist[c];
                }
            }
        }
    }
    out32[1] = e == PACK_OK ? 1.0 : 0.0;
    out32[28] = (double)e;
    return 0;
}

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
    h.p = prefix_of(*this, "XSTSDF3");
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
// Volume checkpoint, version 2.  Layout: the prefix, n_poses x Matrix4cf, then value / grad / weight of the stored planes [zs0, zs1) as dense rows of
// X elements (a rank of a sharded run saves and restores its own planes).
void KinectFusionReconstruction::saveCheckpoint(const std::string &filename) {
    std::vector<float> v, g;
    std::vector<int> w;
    tsdf_volume_d_ptr->downloadTSDFWithGrad(v, g);
    tsdf_volume_d_ptr->downloadWeight(w);
    const CkptPrefix h = prefix_of(*this, "XSTSDF2");
    std::ofstream f(filename, std::ios::binary);
    f.write(reinterpret_cast<const char *>(&h), sizeof(h));
    f.write(reinterpret_cast<const char *>(world2camera_record.data()), (std::streamsize)(h.n_poses * sizeof(Matrix4cf)));
    f.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * 4));
    f.write(reinterpret_cast<const char *>(g.data()), (std::streamsize)(g.size() * 4));
    f.write(reinterpret_cast<const char *>(w.data()), (std::streamsize)(w.size() * 4));
}
// Nothing of *this is touched until the whole file has been read and validated: its format's rules (CheckpointFile::read), then against this
// instance the volume geometry (resolution, voxel size, truncation distance), the planes and the rank, and the arrays it goes into.  Returns false
// (state unchanged) on any mismatch.
bool KinectFusionReconstruction::loadCheckpoint(const std::string &filename) {
    CheckpointFile c;
    if (!tsdf_volume_d_ptr || !c.read(filename)) return false;
    const CkptPrefix &p = c.prefix();
    for (int i = 0; i < 3; ++i) if (p.res[i] != volume_resolution[i]) return false;
    if (p.voxel_size != voxel_size || p.tranc_dist != tsdf_volume_d_ptr->getTsdfTruncDist()) return false;
    if (p.zs0 != zs0 || p.zs1 != zs1 || p.shard_rank != shard_rank || p.shard_count != shard_count || p.frame_id < 0) return false;
    DeviceArray2D<float> dv = tsdf_volume_d_ptr->value(), dg = tsdf_volume_d_ptr->grad();
    DeviceArray2D<int> dw = tsdf_volume_d_ptr->weight();
    const size_t rows = (size_t)p.res[1] * (size_t)(p.zs1 - p.zs0);
    if ((size_t)dv.rows() != rows || dv.cols() != p.res[0] || (size_t)dg.rows() != rows || (size_t)dw.rows() != rows) return false;
    if (dv.step() != dg.step() || dv.step() != dw.step()) return false;
    // validated: commit
    synchronize();
    c.write_to(dv.ptr(0), dw.ptr(0), dg.ptr(0), dv.step(), checkpoint_staging_words);
    // Not volume_written_off_path(): the poses are restored between the sign map and the model maps, which are rendered at the restored pose;
    // the derived maps are not invalidated (their keys hold volume_generation, which moves) and sign_map_stale_ stays as it is.
    ++volume_generation;
    RebuildSignMap();    // the volume was written behind the integrate kernels' back
    world2camera_record.swap(c.poses);
    world2camera = world2camera_record.back();
    frame_id = p.frame_id;
    // previous-frame maps are derived state: regenerate them from the restored volume and pose (in a sharded run every
    // rank must load its own file before the next frame: the raycast composite is a collective)
    CalculatePointCloud(vmaps_g_prev_d[0], nmaps_g_prev_d[0]);
    ModelMapPyramid();
    synchronize();
    return true;
}
