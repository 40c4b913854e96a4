// kf_internal.hpp — what more than one translation unit of the orchestrator needs and no caller of the class does
// (KinectFusionReconstruction.cpp: lifecycle and frame path; kf_relocalize.cpp; kf_planning.cpp; kf_export.cpp: point cloud, mesh, counters, raw
// volume; kf_checkpoint.cpp: saving, reading and restoring checkpoints; kf_second_map.cpp: the calls that take a second map; kf_reintegrate.cpp:
// frames taken out and fused again; kf_render.cpp: views of a map; kf_sample.cpp: the map asked at the caller's points; kf_register.cpp: a point
// cloud registered to a map; kf_fuse.cpp: a point cloud fused into the map; and the C ABI over them, xs_host_capi.cpp: the calls that take no
// instance, xs_pipeline_capi.cpp: lifecycle, frame path, relocalisation, planning, export, statistics, xs_pipeline_maps_capi.cpp: the calls
// that take a second map or edit or query a map).
#pragma once
#include "KinectFusionReconstruction.h"
#include "pack_host.hpp"
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>

// The poll budget of every wait for a published result (xs_host_wait).  The wait also watches the stream, so the budget only ends a wait whose
// stream is still busy after this many polls (tens of seconds).
static constexpr long long kWaitPolls = 2000000000LL;
// A wait that ended without its result where none can be spared: one line naming the site and what happened, then exit(-1) (the hipSafeCall /
// check_rc convention).
[[noreturn]] inline void wait_fatal(const char *site, const xs_wait_result &w) {
    std::cout << "error::KinectFusionReconstruction, " << site << ": " << xs_wait_str(w.status);
    if (w.status == xs_wait::failed) std::cout << " (" << hipGetErrorString(w.error) << ")";
    std::cout << std::endl;
    exit(-1);
}

// the real part of a pose as the kernels that take real poses want it: row-major rotation, translation (R9 null: the translation alone)
inline void pack_real_pose(const xs_host::Matrix4cf &pose, float R9[9], float t3[3]) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; R9 && c < 3; ++c) R9[r * 3 + c] = pose.m[r][c].real();
        t3[r] = pose.m[r][3].real();
    }
}

// A pose as the C ABI passes it (32 floats: 4 x 4 (re, im) pairs, row-major) as a Matrix4cf, an array of them, and the way back.
inline xs_host::Matrix4cf pose_of(const float *c2v32) {
    xs_host::Matrix4cf m;
    std::memcpy(static_cast<void *>(&m), c2v32, 32 * sizeof(float));
    return m;
}
inline std::vector<xs_host::Matrix4cf> poses_of(const float *c2v32xP, int poses) {
    std::vector<xs_host::Matrix4cf> m((size_t)(poses > 0 ? poses : 0));
    for (int p = 0; p < poses; ++p) m[(size_t)p] = pose_of(c2v32xP + 32 * (size_t)p);
    return m;
}
inline void pose_to(const xs_host::Matrix4cf &m, float *c2v32) { std::memcpy(c2v32, &m, 32 * sizeof(float)); }

namespace xs_host { int checkpoint_info(const char *path, double *out32); }   // kf_checkpoint.cpp: what xs_host_checkpoint_info returns
// kf_second_map.cpp: the centroid of a map's band from a band build into temporary buffers (no cache of any instance is touched): 1; 0 for an
// empty band; -1 for a resolution the band build does not take.  AlignVolumeGlobal asks it for the other map, RegisterPointsGlobal for the map.
int second_map_centroid(const xs_host::SecondMap &src, double centroid3[3]);

// An input array of a launch: the caller's pointer when that is device memory, otherwise a buffer of the call's own the array is copied to on `st`.
template <class T>
struct DeviceInput {
    DeviceArray<T> own;
    const T *ptr;
    DeviceInput(const T *src, size_t count, bool on_device, hipStream_t st) : ptr(src) {
        if (on_device) return;
        own.create(count);
        hipSafeCall(hipMemcpyAsync(own.ptr(), src, count * sizeof(T), hipMemcpyHostToDevice, st));
        ptr = own.ptr();
    }
};
// An optional output array of a launch (null: not wanted) that is written in chunks of at most `chunk` elements: the caller's pointer when that
// is device memory, otherwise a buffer of the call's own, one chunk long, that fetch() copies to its place in the caller's host array.
template <class T>
struct StagedOutput {
    DeviceArray<T> own;
    T *out;
    bool staged;
    StagedOutput(T *out, size_t chunk, bool on_device) : out(out), staged(out && !on_device) { if (staged) own.create(chunk); }
    T *at(size_t offset) { return staged ? own.ptr() : out ? out + offset : nullptr; }   // where a launch writes the chunk that begins at `offset`
    void fetch(size_t offset, size_t count, hipStream_t st) {
        if (staged) hipSafeCall(hipMemcpyAsync(out + offset, own.ptr(), count * sizeof(T), hipMemcpyDeviceToHost, st));
    }
};

// An XSTSDF3 file read whole into host memory and validated in full (pack_validate).
struct SparseFile {
    xs_host::PackHeader h{};
    std::vector<char> bytes;           // the file
    std::vector<uint64_t> offsets;     // nbricks + 1
    const char *poses() const { return bytes.data() + sizeof(xs_host::PackHeader); }
    const unsigned char *cls() const { return reinterpret_cast<const unsigned char *>(poses() + (size_t)h.p.n_poses * xs_host::PACK_POSE_BYTES); }
    const char *payload() const { return reinterpret_cast<const char *>(cls()) + xs_host::pack_class_bytes_padded(h.nbricks); }
};
// A checkpoint file of either format (the magic decides) in host memory, validated at the format's level: pack_validate_dense or pack_validate
// (pack_host.hpp).  Nothing on the device is touched or allocated by read; what the file must be for its reader (this instance's geometry for
// loadCheckpoint, a whole volume for OpenCheckpointMap) is the reader's to check, on prefix().
struct CheckpointFile {
    bool read(const std::string &filename);   // false for a file that cannot be read or breaks its format's rules
    const xs_host::CkptPrefix &prefix() const { return sparse.h.p; }
    std::vector<xs_host::Matrix4cf> poses;
    // The file's volume into three device arrays of one pitch of `step` bytes, at their first stored plane: every in-volume voxel is written and the
    // copies have completed on return.  staging_words: the pinned buffer of a sparse file's chunks.
    void write_to(float *value, int *weight, float *grad, size_t step, unsigned long long staging_words) const;

private:
    bool is_sparse = false;
    SparseFile sparse;                 // (a dense file uses its prefix alone)
    std::vector<float> value, grad;    // a dense file's arrays
    std::vector<int> weight;
};
