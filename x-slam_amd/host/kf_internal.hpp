// kf_internal.hpp — what more than one translation unit of the orchestrator needs and no caller of the class does
// (KinectFusionReconstruction.cpp: lifecycle and frame path; kf_relocalize.cpp; kf_planning.cpp; kf_export.cpp).
#pragma once
#include "KinectFusionReconstruction.h"
#include <algorithm>
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
