// xs_icp_search.h — the correspondence search of the ICP reduction (ICP.cu:196-244, search_newton): a pixel of the current frame is moved
// by the pose, projected into the model maps, and kept if its match passes the distance and the angle gate.  One search, four forms,
// because the instances of k_icp (xs_icp.hip) have their loads in flight at different times:
//   search               the four-wave instance (lanes stride over the tiles): loads the six current-frame values, then search_loaded
//   search_loaded        the search proper on values already in registers
//   search_vertex_loaded the one-tile-per-wave instances (8/1, 8/2, 8/3): the vertex was requested before the pose was known
//   search_issue/_finish the balanced instances (8/2/BAL, 16/2/BAL): two tiles in lock step, requests of both before either's answers
// All four give the same outcome for every pixel; the gates they end in are stated once (search_gates).  The six-value model gather is NOT:
// see the note at search_loaded.
#pragma once
#include "xs_icp_args.h"

namespace {
// ICP.cu:196-244
// the six current-frame values of a pixel: they depend on nothing but the pixel, so the one-tile-per-wave instance requests them
// before it even has its pose (a posted launch spends ~3 us waiting for it)
__device__ __forceinline__ void load_vertex(const IcpArgs &a, int x, int y, cfloat3 &vcurr) {
    if (a.vreal) {   // wave-uniform
        vcurr.x = cfloat(row_ptr(a.vreal, a.rstep, y)[x], 0.0f);
        vcurr.y = cfloat(row_ptr(a.vreal, a.rstep, y + a.rows)[x], 0.0f);
        vcurr.z = cfloat(row_ptr(a.vreal, a.rstep, y + 2 * a.rows)[x], 0.0f);
        return;
    }
    vcurr.x = row_ptr(a.vmap_curr, a.mstep, y)[x];
    vcurr.y = row_ptr(a.vmap_curr, a.mstep, y + a.rows)[x];
    vcurr.z = row_ptr(a.vmap_curr, a.mstep, y + 2 * a.rows)[x];
}
__device__ __forceinline__ void load_normal(const IcpArgs &a, int x, int y, cfloat3 &ncurr) {
    // all three are requested before the sentinel is looked at (the y / z planes of an invalid pixel are allocated, merely
    // unused): one memory round trip instead of two
    if (a.nreal) {
        ncurr.x = cfloat(row_ptr(a.nreal, a.rstep, y)[x], 0.0f);
        ncurr.y = cfloat(row_ptr(a.nreal, a.rstep, y + a.rows)[x], 0.0f);
        ncurr.z = cfloat(row_ptr(a.nreal, a.rstep, y + 2 * a.rows)[x], 0.0f);
        return;
    }
    ncurr.x = row_ptr(a.nmap_curr, a.mstep, y)[x];
    ncurr.y = row_ptr(a.nmap_curr, a.mstep, y + a.rows)[x];
    ncurr.z = row_ptr(a.nmap_curr, a.mstep, y + 2 * a.rows)[x];
}
__device__ __forceinline__ void load_current(const IcpArgs &a, int x, int y, cfloat3 &ncurr, cfloat3 &vcurr) {
    load_normal(a, x, y, ncurr);
    load_vertex(a, x, y, vcurr);
}
// The two gates of ICP.cu:232-241 compare the REAL part of a complex square root with a threshold and use nothing else of
// it.  For z = a + ib, Re sqrt z = sqrt((|z| + a) / 2) lies in [sqrt(max(a, 0)), sqrt(|a| + |b|)], and the float sequence
// the reference runs (hypot, sqrt, atan2, cos, one product — or the short form of xs_complex.h) lands within a few ulp of it:
// with a margin three hundred times that (1e-5 relative on the squares) the comparison is settled from a and b alone unless
// the value sits on the threshold, and only then does the lane run the square root itself (~330 instructions when the
// argument is outside the short form's cone, which is where matched pixels live: |d| of a millimetre, sine ~ 0).  The same
// booleans as the full evaluation for every input (xs_icp_gate_selftest sweeps the neighbourhood of the threshold).
__device__ __forceinline__ bool re_sqrt_exceeds(cfloat z, float thres, bool or_equal) {
    const float lo2 = fmaxf(z.re, 0.0f), hi2 = fabsf(z.re) + fabsf(z.im), t2 = thres * thres;
    constexpr float M = 1e-5f;
    if (thres > 0x1p-60f && thres < 0x1p60f) {   // NaN operands fail both tests and take the full path
        if (hi2 * (1.0f + M) < t2) return false;
        if (lo2 > t2 * (1.0f + M)) return true;
    }
    const float r = sqrt(z).re;
    return or_equal ? r >= thres : r > thres;
}
// the distance gate, the angle gate and the result (ICP.cu:232-244): the end of every form of the search
__device__ __forceinline__ bool search_gates(const IcpArgs &a, const MatS33 &Rcurr, const cfloat3 &ncurr, const cfloat3 &vcurr_g, const cfloat3 &nprev_g,
                                             const cfloat3 &vprev_g, cfloat3 &n, cfloat3 &d, cfloat3 &s) {
    if (re_sqrt_exceeds(squarednorm(vprev_g - vcurr_g), a.distThres, false)) return false;   // norm(...).re > distThres
    const cfloat3 ncurr_g = Rcurr * ncurr;
    if (re_sqrt_exceeds(squarednorm(cross(ncurr_g, nprev_g)), a.angleThres, true)) return false;   // norm(...).re >= angleThres
    n = nprev_g; d = vprev_g; s = vcurr_g;
    return true;
}
// (The six model-map loads stand in each of the three forms below.  As one function with two cfloat3& out-parameters they changed the text
// of the twelve non-balanced instances of k_icp, 85 to 1 175 lines each — the balanced ones stayed identical; values that leave a function
// through references or a returned struct moved the register allocation wherever else it was tried too: profiles/icp_split_kernels.txt.)
__device__ __forceinline__ bool search_loaded(const IcpArgs &a, const MatS33 &Rcurr, const cfloat3 &tcurr, const cfloat3 &ncurr, const cfloat3 &vcurr,
                                              cfloat3 &n, cfloat3 &d, cfloat3 &s) {
    if (isnan(ncurr.x.re)) return false;
    const cfloat3 vcurr_g = Rcurr * vcurr + tcurr;
    const cfloat3 vcp = a.Rprev_inv * (vcurr_g - a.tprev);
    const float cpx = vcp.x.re, cpy = vcp.y.re, cpz = vcp.z.re;
    const int ux = __float2int_rn(cpx * a.intr.fx / cpz + a.intr.cx);
    const int uy = __float2int_rn(cpy * a.intr.fy / cpz + a.intr.cy);
    if (ux < 0 || uy < 0 || ux >= a.cols || uy >= a.rows || cpz < 0) return false;
    cfloat3 nprev_g, vprev_g;  // likewise: the six model-map values of the matched pixel together
    nprev_g.x = row_ptr(a.nmap_g_prev, a.mstep, uy)[ux];
    nprev_g.y = row_ptr(a.nmap_g_prev, a.mstep, uy + a.rows)[ux];
    nprev_g.z = row_ptr(a.nmap_g_prev, a.mstep, uy + 2 * a.rows)[ux];
    vprev_g.x = row_ptr(a.vmap_g_prev, a.mstep, uy)[ux];
    vprev_g.y = row_ptr(a.vmap_g_prev, a.mstep, uy + a.rows)[ux];
    vprev_g.z = row_ptr(a.vmap_g_prev, a.mstep, uy + 2 * a.rows)[ux];
    if (isnan(nprev_g.x.re)) return false;
    return search_gates(a, Rcurr, ncurr, vcurr_g, nprev_g, vprev_g, n, d, s);
}
// The same search for a wave that already holds its pixel's vertex (requested before the pose was known): the three normal
// values are requested here, and their sentinel is looked at only after the model-map gather — they are not needed before,
// and asking for them up front with the vertices doubled the burst of requests (14.7 MB at level 0) that the workgroups'
// mailbox polls then queued behind.  Same outcome for every pixel: the gate only moves past statements without side effects
// (a NaN vertex converts to pixel (0, 0), which is in range).
__device__ __forceinline__ bool search_vertex_loaded(const IcpArgs &a, const MatS33 &Rcurr, const cfloat3 &tcurr, int x, int y, const cfloat3 &vcurr,
                                                     cfloat3 &n, cfloat3 &d, cfloat3 &s) {
    cfloat3 ncurr;
    load_normal(a, x, y, ncurr);
    const cfloat3 vcurr_g = Rcurr * vcurr + tcurr;
    const cfloat3 vcp = a.Rprev_inv * (vcurr_g - a.tprev);
    const float cpx = vcp.x.re, cpy = vcp.y.re, cpz = vcp.z.re;
    // (an invalid pixel's vertex is NaN and its normal's sentinel has not been looked at yet: the conversion of a NaN is
    // kept out of the picture — such a pixel reads model pixel (0, 0) and is rejected below)
    const float fu = cpx * a.intr.fx / cpz + a.intr.cx, fv = cpy * a.intr.fy / cpz + a.intr.cy;
    const int ux = fu == fu ? __float2int_rn(fu) : 0;
    const int uy = fv == fv ? __float2int_rn(fv) : 0;
    if (ux < 0 || uy < 0 || ux >= a.cols || uy >= a.rows || cpz < 0) return false;
    cfloat3 nprev_g, vprev_g;
    nprev_g.x = row_ptr(a.nmap_g_prev, a.mstep, uy)[ux];
    nprev_g.y = row_ptr(a.nmap_g_prev, a.mstep, uy + a.rows)[ux];
    nprev_g.z = row_ptr(a.nmap_g_prev, a.mstep, uy + 2 * a.rows)[ux];
    vprev_g.x = row_ptr(a.vmap_g_prev, a.mstep, uy)[ux];
    vprev_g.y = row_ptr(a.vmap_g_prev, a.mstep, uy + a.rows)[ux];
    vprev_g.z = row_ptr(a.vmap_g_prev, a.mstep, uy + 2 * a.rows)[ux];
    if (isnan(ncurr.x.re)) return false;      // ICP.cu:202-204
    if (isnan(nprev_g.x.re)) return false;
    return search_gates(a, Rcurr, ncurr, vcurr_g, nprev_g, vprev_g, n, d, s);
}
// search_vertex_loaded in two stages, for a wave that works through two tiles (the balanced level-0 instance): stage 1 asks for the
// pixel's normal, projects it and asks for the six model-map values — of pixel (0, 0) where the projection leaves the image: resident,
// never used — without a branch, so that the requests of the second tile go out before the first tile's answers are looked at (two tiles
// one after the other were two dependent chains of memory round trips: the pixel phase of those waves took 6.2 us against 4.4); stage 2
// applies the rejection tests in the order of ICP.cu:202-241.  Same outcome for every pixel as search_vertex_loaded.
struct SearchStage { cfloat3 ncurr, vcurr_g, nprev_g, vprev_g; bool inb; };
__device__ __forceinline__ void search_issue(const IcpArgs &a, const MatS33 &Rcurr, const cfloat3 &tcurr, int x, int y, const cfloat3 &vcurr, SearchStage &st) {
    load_normal(a, x, y, st.ncurr);
    st.vcurr_g = Rcurr * vcurr + tcurr;
    const cfloat3 vcp = a.Rprev_inv * (st.vcurr_g - a.tprev);
    const float cpx = vcp.x.re, cpy = vcp.y.re, cpz = vcp.z.re;
    const float fu = cpx * a.intr.fx / cpz + a.intr.cx, fv = cpy * a.intr.fy / cpz + a.intr.cy;
    int ux = fu == fu ? __float2int_rn(fu) : 0;
    int uy = fv == fv ? __float2int_rn(fv) : 0;
    st.inb = !(ux < 0 || uy < 0 || ux >= a.cols || uy >= a.rows || cpz < 0);
    ux = st.inb ? ux : 0; uy = st.inb ? uy : 0;
    st.nprev_g.x = row_ptr(a.nmap_g_prev, a.mstep, uy)[ux];
    st.nprev_g.y = row_ptr(a.nmap_g_prev, a.mstep, uy + a.rows)[ux];
    st.nprev_g.z = row_ptr(a.nmap_g_prev, a.mstep, uy + 2 * a.rows)[ux];
    st.vprev_g.x = row_ptr(a.vmap_g_prev, a.mstep, uy)[ux];
    st.vprev_g.y = row_ptr(a.vmap_g_prev, a.mstep, uy + a.rows)[ux];
    st.vprev_g.z = row_ptr(a.vmap_g_prev, a.mstep, uy + 2 * a.rows)[ux];
}
__device__ __forceinline__ bool search_finish(const IcpArgs &a, const MatS33 &Rcurr, const SearchStage &st, cfloat3 &n, cfloat3 &d, cfloat3 &s) {
    if (!st.inb) return false;
    if (isnan(st.ncurr.x.re)) return false;      // ICP.cu:202-204
    if (isnan(st.nprev_g.x.re)) return false;
    return search_gates(a, Rcurr, st.ncurr, st.vcurr_g, st.nprev_g, st.vprev_g, n, d, s);
}
__device__ __forceinline__ bool search(const IcpArgs &a, const MatS33 &Rcurr, const cfloat3 &tcurr, int x, int y, cfloat3 &n, cfloat3 &d,
                                       cfloat3 &s) {
    cfloat3 ncurr, vcurr;
    load_current(a, x, y, ncurr, vcurr);
    return search_loaded(a, Rcurr, tcurr, ncurr, vcurr, n, d, s);
}
// the row of a matched pixel, whose 27 products k_icp adds up
__device__ __forceinline__ void fill_row(cfloat (&r)[7], const cfloat3 &n, const cfloat3 &d, const cfloat3 &s) {
    const cfloat3 cr = cross(s, n);  // ICP.cu:257-259
    r[0] = cr.x; r[1] = cr.y; r[2] = cr.z;
    r[3] = n.x; r[4] = n.y; r[5] = n.z;
    r[6] = dot(n, d - s);
}
}  // namespace
