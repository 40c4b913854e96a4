// xs_icp_args.h — what an ICP launch receives: the argument blocks of k_icp and k_icp_solve, the size of a workgroup record and the
// constants that kernel, launcher and self-test share.  The kernels are in xs_icp.hip, the search in xs_icp_search.h, the folds in xs_icp_fold.h.
#pragma once
#include "xs_device.h"
#include "xs_icp_solve.h"
#include "xs_host_wait.h"

using namespace xs;   // (IcpArgs and IcpSolveArgs stay at global scope: they are part of the kernels' mangled names)

struct IcpArgs {
    MatS33 Rcurr; cfloat3 tcurr;
    const cfloat *vmap_curr; const cfloat *nmap_curr;
    // optional: the same two maps' real parts as float planes (their imaginary parts are zeros when the depth image is real:
    // xs_create_vnmaps_real) — read instead of the complex maps, half the bytes
    const float *vreal; const float *nreal; size_t rstep;
    MatS33 Rprev_inv; cfloat3 tprev;
    Intr intr;
    const cfloat *vmap_g_prev; const cfloat *nmap_g_prev;
    size_t mstep;
    float distThres, angleThres;
    int cols, rows;
    int y0, y1;             // pixel rows this launch covers (row sharding across GPUs)
    double *partials;       // [gridDim.x][56]
    unsigned *ticket;       // zeroed before the launch
    double *out;            // 54 sums (27 x re,im) + [54] = inlier count
    unsigned long long *done_flag; unsigned long long done_seq;  // optional: host-visible completion word
    int pairs;              // out is host-coherent pinned memory taking 55 x {u64 done_seq, double sum}: every sum carries its own sequence word (XS_ICP_PUBLISH_PAIRS)
    // optional device-side pose update (xs_icp_iterate): the last workgroup solves for the increment and
    // composes it into *pose, which the next launch reads instead of Rcurr / tcurr above
    IcpPoseState *pose; IcpPoseState *pose_host; int load_pose;
    // optional posted pose (xs_icp_accumulate_posted): the launch was enqueued before its pose was known and
    // picks it up from a 128-byte mailbox in host-coherent pinned memory once the host has posted mailbox_seq
    const unsigned *mailbox; unsigned mailbox_seq;
    // optional host fold (xs_icp_accumulate_records): every workgroup stores its record straight into host-coherent
    // pinned memory, sequence number last, and leaves; the host adds the records (xs_icp_sum_records)
    double *host_records; unsigned long long record_seq;
};

struct IcpSolveArgs {
    const double *sums;     // the 55 values the reduction just wrote
    double *sums_host;      // optional host-visible copy of them (per-iteration log)
    MatS33 Rcurr; cfloat3 tcurr; int load_pose;  // load_pose: start from these instead of *pose
    IcpPoseState *pose, *pose_host;
    unsigned long long *done_flag; unsigned long long done_seq;
};

constexpr int NS = 54;      // 27 complex sums
constexpr int NP = 56;      // partial record: 54 sums + count + pad
static_assert(NP == XS_ICP_RECORD_DOUBLES && NS + 1 == XS_ICP_PAIRS, "the host's wire formats (xs_host_wait.h)");

// POSE_ARGS: Rcurr / tcurr are kernel arguments (xs_icp_accumulate, first iteration of xs_icp_iterate).
// POSE_DEVICE: they are what k_icp_solve left in device memory after the previous iteration.
// POSE_POSTED: the host posts them while this launch is already resident — the launch latency of an
// iteration (~4 us) overlaps the previous iteration's epilogue and the host's solve.
enum { POSE_ARGS = 0, POSE_DEVICE = 1, POSE_POSTED = 2 };
constexpr unsigned long long kIcpTimeoutBit = 1ull << 63;   // in a completion / sequence word: the launch gave up waiting for its posted pose

enum { XS_ICP_MAX_BLOCKS = 768 };  // records a launch may write = eight-wave workgroups resident at once (three per CU: 51 KB of LDS, 79 VGPRs)
