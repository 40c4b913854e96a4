// xs_icp_host.hip — what the ICP reduction (xs_icp.hip) leaves to the CPU: the host halves of its three publish protocols — the pose
// mailbox, the {sequence number, sum} pairs, the per-workgroup records — the unpacking of the 55 sums into A and b, and estimateCombined
// as one blocking call.  No kernel here; the wire formats are in xs_host_wait.h and xs_mailbox.h.
#include <algorithm>
#include <climits>
#include <string.h>
#include "xs_device.h"
#include "xs_mailbox.h"
#include "xs_host_wait.h"
#include "../../include/xslam_amd.h"

using namespace xs;

/* Host half of xs_icp_accumulate_records: waits (spinning) until records 0 .. count - 1 carry `seq`, then adds them in that order — one
 * fixed order, so the 55 results are the same bits for the same records whatever order the workgroups finished in.  sums55: 54 sums +
 * inlier count.  Returns 0; 1 if a record reports that its launch gave up waiting for a posted pose; -1 after max_spins polls (<= 0: no limit). */
extern "C" int xs_icp_sum_records(const double *records_host, int count, unsigned long long seq, double *sums55, long long max_spins) {
    if (!records_host || !sums55 || count < 1) return -1;
    int next = 0;
    const xs_wait_result w = xs_host_wait([&] { return xs_poll_records(records_host, count, seq, &next); }, max_spins <= 0 ? LLONG_MAX : max_spins);
    if (w.status == xs_wait::left) return 1;
    if (w.status != xs_wait::published) return -1;
    xs_fold_records(records_host, count, sums55);
    return 0;
}

/* host half of XS_ICP_PUBLISH_PAIRS: every pair {sequence number, sum} arrives as one 16-byte write; done when all 55 carry `seq` */
extern "C" int xs_icp_wait_pairs(const void *pairs_host, unsigned long long seq, double *sums55, long long max_spins) {
    const xs_wait_result w = xs_host_wait([&] { return xs_poll_pairs(pairs_host, seq); }, std::max(max_spins, 1LL));
    if (w.status == xs_wait::left) return 1;
    if (w.status != xs_wait::published) return 2;
    xs_read_pairs(pairs_host, sums55);
    return 0;
}

extern "C" size_t xs_icp_mailbox_bytes(void) { return MAILBOX_WORDS * sizeof(unsigned); }
/* Host side of the mailbox: one box (xs_mailbox.h has the layout, the order of stores and fences, and the reasons). */
extern "C" void xs_icp_post_pose(void *mailbox_host, const float *Rcurr18, const float *tcurr6, unsigned mailbox_seq, int cmd) {
    alignas(64) unsigned img[1][MAILBOX_WORDS];
    mailbox_image(img[0], Rcurr18, tcurr6, mailbox_seq, cmd);
    mailbox_post(mailbox_host, img, 1);
}
/* A mailbox where polling is cheapest: fine-grained device memory the CPU writes through the large
 * BAR (512 workgroups then poll local memory, not the PCIe link), or — without a large BAR —
 * host-coherent pinned memory.  Zeroed.  *in_device_memory (optional) says which one it is. */
extern "C" int xs_icp_mailbox_alloc(void **mailbox, int *in_device_memory) {
    if (!mailbox) return xs_set_error(hipErrorInvalidValue, "xs_icp_mailbox_alloc: null pointer");
    int dev = 0, large_bar = 0;
    XS_CHECK(hipGetDevice(&dev));
    if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, dev) != hipSuccess) { large_bar = 0; (void)hipGetLastError(); }
    const char *force_host = getenv("XS_ICP_MAILBOX_HOST");   // (a documented switch: INTEGRATION.md "Environment")
    void *p = nullptr;
    if (large_bar && !(force_host && force_host[0] == '1') &&
        hipExtMallocWithFlags(&p, 4096, hipDeviceMallocFinegrained) == hipSuccess) {
        XS_CHECK(hipMemset(p, 0, 4096));
        XS_CHECK(hipDeviceSynchronize());
        if (in_device_memory) *in_device_memory = 1;
    } else {
        (void)hipGetLastError();
        XS_CHECK(hipHostMalloc(&p, 4096, hipHostMallocCoherent | hipHostMallocMapped));
        memset(p, 0, 4096);
        if (in_device_memory) *in_device_memory = 0;
    }
    *mailbox = p;
    return 0;
}
extern "C" int xs_icp_mailbox_free(void *mailbox, int in_device_memory) {
    if (!mailbox) return 0;
    if (in_device_memory) XS_CHECK(hipFree(mailbox));
    else XS_CHECK(hipHostFree(mailbox));
    return 0;
}

/* estimateCombined whole (ICP.cu:365-429): the reduction, then — where the reference synchronises the device and downloads (:414-417) —
 * the kernel's last workgroup has written the 27 sums and the inlier count straight into host-coherent pinned memory, each with the launch's
 * number in the same 16-byte store (XS_ICP_PUBLISH_PAIRS), and the host spins until all of them carry it: the call returns when the launch, and
 * with it everything before it on the stream, has completed, without a copy or a stream drain (round 6: ~10 us less per iteration for a caller
 * that changes nothing).  Unpacks
 * into the symmetric 6x6 A (A[i*6+j] = A[j*6+i]) and b, both complex<double> (re, im) pairs.  sums_dev (optional): also receives the 55
 * doubles, by an asynchronous copy the call does not wait for.  inliers may be NULL.  One call at a time per host thread. */
extern "C" int xs_estimate_combined(const float *Rcurr18, const float *tcurr6, const float *vmap_curr, const float *nmap_curr,
                                    const float *Rprev_inv18, const float *tprev6, const float *intr4, const float *vmap_g_prev,
                                    const float *nmap_g_prev, size_t map_step, int rows, int cols, float distThres, float angleThres,
                                    void *workspace, double *sums_dev, double *A72_host, double *b12_host, long long *inliers,
                                    void *stream) {
    static thread_local double *host = nullptr;            // the 55 sums as doubles (what xs_icp_unpack and the optional copy read)
    static thread_local void *pairs = nullptr;             // XS_ICP_PUBLISH_PAIRS: 55 x {sequence number, sum} written by the launch
    static thread_local unsigned long long seq = 0;
    if (!host) {   // both buffers or neither: a failed allocation is retried by the next call
        double *h = nullptr;
        void *p = nullptr;
        hipError_t e = hipHostMalloc((void **)&h, 64 * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostMalloc(&p, XS_ICP_PAIRS_BYTES, hipHostMallocCoherent | hipHostMallocMapped);
        if (e != hipSuccess) {
            if (h) (void)hipHostFree(h);
            return xs_set_error(e, "xs_estimate_combined: hipHostMalloc");
        }
        memset(h, 0, 64 * sizeof(double));
        memset(p, 0, XS_ICP_PAIRS_BYTES);
        host = h;
        pairs = p;
    }
    ++seq;
    int rc = xs_icp_accumulate(Rcurr18, tcurr6, vmap_curr, nmap_curr, Rprev_inv18, tprev6, intr4, vmap_g_prev, nmap_g_prev, map_step,
                               rows, cols, distThres, angleThres, 0, rows, workspace, static_cast<double *>(pairs), XS_ICP_PUBLISH_PAIRS, seq, stream);
    if (rc) return rc;
    if (rows <= 0 || cols <= 0) { XS_CHECK(hipStreamSynchronize((hipStream_t)stream)); memset(host, 0, 55 * sizeof(double)); }   // (nothing was launched: nothing publishes)
    else {
        const xs_wait_result w = xs_host_wait([&] { return xs_poll_pairs(pairs, seq); }, 4000000000LL, (hipStream_t)stream);
        if (w.status == xs_wait::failed) return xs_set_error(w.error, "xs_estimate_combined");
        if (w.status != xs_wait::published)   // (drained: the workspace's ticket was not zero — xs_icp_workspace_init)
            return xs_set_error(hipErrorLaunchTimeOut, w.status == xs_wait::drained ? "xs_estimate_combined: the stream drained and the launch published nothing"
                                                                                     : "xs_estimate_combined: the launch published nothing within the poll budget");
        xs_read_pairs(pairs, host);
    }
    xs_icp_unpack(host, A72_host, b12_host);
    if (inliers) *inliers = (long long)host[54];
    if (sums_dev) XS_CHECK(hipMemcpyAsync(sums_dev, host, 55 * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream));
    return 0;
}

/* ICP.cu:419-428 on the host: 27 (re, im) sums -> symmetric A[36] and b[6], complex<double> */
extern "C" void xs_icp_unpack(const double *sums54, double *A72, double *b12) {
    int shift = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 7; ++j) {
            const double re = sums54[2 * shift], im = sums54[2 * shift + 1];
            ++shift;
            if (j == 6) { b12[2 * i] = re; b12[2 * i + 1] = im; }
            else {
                A72[2 * (j * 6 + i)] = re; A72[2 * (j * 6 + i) + 1] = im;
                A72[2 * (i * 6 + j)] = re; A72[2 * (i * 6 + j) + 1] = im;
            }
        }
}
