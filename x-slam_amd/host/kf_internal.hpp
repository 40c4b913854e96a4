// kf_internal.hpp — what more than one translation unit of the orchestrator needs and no caller of the class does
// (KinectFusionReconstruction.cpp: lifecycle and frame path; kf_relocalize.cpp; kf_planning.cpp; kf_export.cpp: point cloud, mesh, counters, raw
// volume; kf_checkpoint.cpp: saving, reading and restoring checkpoints; kf_second_map.cpp: the calls that take a second map; kf_reintegrate.cpp: frames taken out and fused again; kf_render.cpp: views of a map; kf_sample.cpp: the map asked at the caller's points; kf_register.cpp: a point cloud registered to a map).
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
