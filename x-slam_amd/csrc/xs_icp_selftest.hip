// xs_icp_selftest.hip — self-test of the gate shortcut of the ICP search (re_sqrt_exceeds, xs_icp_search.h): a test hook, no product path.
#include "xs_icp_search.h"
#include "../../include/xslam_amd.h"

using namespace xs;

__global__ void k_icp_gate_check(const float *z2n, int n, float thres, int or_equal, unsigned *counts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const cfloat z(z2n[2 * i], z2n[2 * i + 1]);
    const bool fast = re_sqrt_exceeds(z, thres, or_equal != 0);
    const float r = sqrt(z).re;
    const bool full = or_equal ? r >= thres : r > thres;
    if (fast != full) atomicAdd(&counts[0], 1u);
    const float lo2 = fmaxf(z.re, 0.0f), hi2 = fabsf(z.re) + fabsf(z.im), t2 = thres * thres;
    if (!(hi2 * (1.0f + 1e-5f) < t2) && !(lo2 > t2 * (1.0f + 1e-5f))) atomicAdd(&counts[1], 1u);
}
/* Gate shortcut of the ICP search (re_sqrt_exceeds) against the full complex square root on n complex values (device, re / im
 * interleaved): counts_dev[0] = values on which the two disagree (must be 0), counts_dev[1] = values the shortcut could not
 * settle from its bounds.  counts_dev: two zeroed 32-bit words of device memory.  Test hook; no synchronisation. */
extern "C" int xs_icp_gate_selftest(const float *z2n_dev, int n, float thres, int or_equal, unsigned *counts_dev, void *stream) {
    if (!z2n_dev || !counts_dev || n < 0) return xs_set_error(hipErrorInvalidValue, "xs_icp_gate_selftest: bad argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_icp_gate_check, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, z2n_dev, n, thres, or_equal, counts_dev);
    XS_CHECK(hipGetLastError());
    return 0;
}
