// xs_icp_launch.h — the host's side of an ICP launch before anything touches the device: which instance of k_icp a launch runs and with how
// many workgroups (icp_blocks), what an entry point of the C ABI asks for (IcpLaunch), and the validation that turns such a request into
// kernel arguments (icp_plan).  xs_icp.hip enqueues the plan.
#pragma once
#include <algorithm>
#include <string.h>
#include "xs_env.h"
#include "xs_icp_args.h"
#include "../../include/xslam_amd.h"

// The six instances of k_icp<POSE, WAVES, PASSES, BAL>, and which of them a launch over pixel rows [y0, y1) runs with how many workgroups
// (= records): eight waves with one 64-pixel tile each while all of them are resident at once (two or three such workgroups per CU, see
// PASSES: up to 768, i.e. 6 144 tiles — every level of a 640 x 480 frame), else four waves striding over the tiles with the sums in registers
// (any size).
// More tiles than the 4 096 waves a launch can keep resident at this kernel's register / LDS budget, by up to a quarter (level 0 of a
// 640 x 480 frame: 4 800): one sixteen-wave workgroup per CU, 18 or 19 tiles each (W16_BAL) — 256 records for the last workgroup to add
// instead of 512 or 600.  XS_ICP_BALANCED (measurement aid): 1 = 512 eight-wave workgroups of nine or ten tiles (W8_BAL), 0 = the
// one-tile-per-wave launch.
enum class IcpInstance { W4_P2, W8_P1, W8_P2, W8_P3, W8_BAL, W16_BAL };
struct IcpGrid { IcpInstance instance; int blocks; };
static IcpGrid icp_blocks(int cols, int y0, int y1) {
    const int tiles = div_up(cols, 64) * (y1 - y0);
    static const int mode = product_env_int("XS_ICP_BALANCED", 2);   // (a documented switch: INTEGRATION.md "Environment"; tests/test_publish_stress_gpu.py runs both balanced instances)
    if (mode != 0 && tiles > 8 * 512 && tiles <= 10 * 512) return mode == 1 ? IcpGrid{IcpInstance::W8_BAL, 512} : IcpGrid{IcpInstance::W16_BAL, 256};
    int blocks = div_up(tiles, 8);
    if (blocks > XS_ICP_MAX_BLOCKS) return {IcpInstance::W4_P2, std::min(div_up(tiles, 4), 512)};
    if (blocks < 1) blocks = 1;
    return {blocks <= 256 ? IcpInstance::W8_P1 : (blocks <= 512 ? IcpInstance::W8_P2 : IcpInstance::W8_P3), blocks};
}

// What an ABI entry point asks for: each fills the fields it has, by name; the rest stay zero.
struct IcpLaunch {
    const char *who = nullptr;   // the caller's "null pointer" message
    // the pose: as arguments, or posted to a mailbox after the launch, or (xs_icp_iterate) left on the device by the previous solve
    const float *Rcurr18 = nullptr, *tcurr6 = nullptr;
    const void *mailbox = nullptr; unsigned mailbox_seq = 0;
    IcpPoseState *pose = nullptr, *pose_host = nullptr; double *sums_host = nullptr;
    // the current frame's maps (vreal / nreal: optionally their real parts as float planes) and the model's
    const float *vmap_curr = nullptr, *nmap_curr = nullptr, *vreal = nullptr, *nreal = nullptr; size_t rstep = 0;
    const float *Rprev_inv18 = nullptr, *tprev6 = nullptr, *intr4 = nullptr, *vmap_g_prev = nullptr, *nmap_g_prev = nullptr; size_t map_step = 0;
    int rows = 0, cols = 0; float distThres = 0.0f, angleThres = 0.0f; int y0 = 0, y1 = 0;
    // where the sums go: a workspace + 55 doubles (+ completion word), or records for the host to add
    void *workspace = nullptr; double *sums_dev = nullptr; unsigned long long *done_flag = nullptr; unsigned long long done_seq = 0;
    double *host_records = nullptr; unsigned long long record_seq = 0;
    void *stream = nullptr;
};
// the real planes of xs_icp_accumulate_real / _posted_real: both given, wide enough; the complex maps may then be NULL (they are only tested for null)
static int icp_real_planes(IcpLaunch &l, const float *vreal, const float *nreal, size_t real_step, const char *what) {
    if (!vreal || !nreal || real_step < (size_t)l.cols * 4) return xs_set_error(hipErrorInvalidValue, what);
    l.vreal = vreal; l.nreal = nreal; l.rstep = real_step;
    if (!l.vmap_curr) l.vmap_curr = vreal;
    if (!l.nmap_curr) l.nmap_curr = nreal;
    return 0;
}

// What goes to the device: the reduction's arguments, its shape, where its pose comes from, and the solve behind it if there is one.
struct IcpPlan { IcpArgs a; IcpGrid grid; int pose_src; bool solve; IcpSolveArgs sa; };
// Validate a request and build its plan.  Nothing here touches the device.
static int icp_plan(const IcpLaunch &l, IcpPlan &p) {
    if ((!l.pose && !l.mailbox && (!l.Rcurr18 || !l.tcurr6)) || !l.vmap_curr || !l.nmap_curr || !l.Rprev_inv18 || !l.tprev6 || !l.intr4 || !l.vmap_g_prev ||
        !l.nmap_g_prev || (!l.host_records && (!l.workspace || !l.sums_dev)))
        return xs_set_error(hipErrorInvalidValue, l.who);
    int y0 = l.y0, y1 = l.y1;
    if (y0 < 0 || y1 > l.rows || y1 < y0) return xs_set_error(hipErrorInvalidValue, "xs_icp: bad row range");
    // an empty range at the end of the image: the one-tile-per-wave instances request the vertex of pixel (0, y0) for every lane
    // without a tile, and row y0 == rows lies one row past the maps — the same empty launch over the last row instead
    if (y0 == y1 && y0 == l.rows && l.rows > 0) y0 = y1 = l.rows - 1;
    IcpArgs &a = p.a;
    if (l.Rcurr18) { load_mat(l.Rcurr18, a.Rcurr); load_vec(l.tcurr6, a.tcurr); }
    else { memset(&a.Rcurr, 0, sizeof(a.Rcurr)); memset(&a.tcurr, 0, sizeof(a.tcurr)); }
    load_mat(l.Rprev_inv18, a.Rprev_inv); load_vec(l.tprev6, a.tprev);
    a.vmap_curr = (const cfloat *)l.vmap_curr; a.nmap_curr = (const cfloat *)l.nmap_curr;
    a.vmap_g_prev = (const cfloat *)l.vmap_g_prev; a.nmap_g_prev = (const cfloat *)l.nmap_g_prev;
    a.mstep = l.map_step; a.intr = Intr{l.intr4[0], l.intr4[1], l.intr4[2], l.intr4[3]};
    a.vreal = l.vreal; a.nreal = l.nreal; a.rstep = l.rstep;
    a.distThres = l.distThres; a.angleThres = l.angleThres; a.cols = l.cols; a.rows = l.rows; a.y0 = y0; a.y1 = y1;
    a.ticket = (unsigned *)l.workspace;   // must be zero on first use (xs_icp_workspace_init); every launch leaves it zero
    a.partials = l.workspace ? (double *)((char *)l.workspace + 256) : nullptr;
    a.host_records = l.host_records; a.record_seq = l.record_seq;
    a.out = l.sums_dev; a.done_flag = l.done_flag; a.done_seq = l.done_seq;
    a.pairs = 0;
    if (l.done_flag == XS_ICP_PUBLISH_PAIRS) {
        if (l.pose || l.host_records) return xs_set_error(hipErrorInvalidValue, "xs_icp: XS_ICP_PUBLISH_PAIRS goes with the plain and posted accumulate calls only");
        a.pairs = 1; a.done_flag = nullptr;
    }
    a.pose = l.pose; a.pose_host = l.pose_host; a.load_pose = (l.pose && l.Rcurr18) ? 1 : 0;
    a.mailbox = nullptr; a.mailbox_seq = 0;
    p.grid = icp_blocks(l.cols, y0, y1);
    p.solve = l.pose != nullptr;
    p.pose_src = POSE_ARGS;
    if (l.pose) {
        // the reduction, then the pose update it feeds; the completion word belongs to the second kernel
        IcpSolveArgs &sa = p.sa;
        sa.sums = l.sums_dev; sa.sums_host = l.sums_host; sa.Rcurr = a.Rcurr; sa.tcurr = a.tcurr; sa.load_pose = a.load_pose;
        sa.pose = l.pose; sa.pose_host = l.pose_host; sa.done_flag = l.done_flag; sa.done_seq = l.done_seq;
        a.done_flag = nullptr;
        if (!a.load_pose) p.pose_src = POSE_DEVICE;
    } else if (l.mailbox) {
        a.mailbox = (const unsigned *)l.mailbox; a.mailbox_seq = l.mailbox_seq;
        p.pose_src = POSE_POSTED;
    }
    return 0;
}
