// xs_gn_band.h — what the dense residual kernels of xs_residual.hip and the band index of xs_band.hip share: the kernel arguments, the
// record fold (registers -> wave -> LDS -> one record per workgroup -> the last workgroup adds the records in index order), the walk that
// deals the band voxels (gt != 0, |gt| <= 0.95) of a slab out to the lanes, the six-pose CSFD residual of the Gauss-Newton pass, the
// dual-complex squared residual of the Hessian kernels and the real-valued one of the loss kernels.
// Included by exactly those two files, by xs_align.hip for the record fold and the wave's float tree alone, and by xs_register.hip for the
// record fold alone.
#pragma once
#include <type_traits>
#include "xs_device.h"
#include "xs_env.h"

using namespace xs;
// The record hand-offs of block_fold_and_finish_of (relaxed agent-scope stores + s_waitcnt vmcnt(0) + a relaxed ticket, no release fence) are
// correct because gfx942 / gfx950 implement an agent-scope atomic store as a write-through (sc1) store that is acknowledged from memory; that is
// outside the HIP / LLVM memory model, so a file that includes this refuses to build for anything else rather than publish stale records there.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx942__) && !defined(__gfx950__)
#error "write-through record publish: gfx942 / gfx950 only (use a release fence + acq_rel ticket on other targets)"
#endif

struct HessArgs {
    const float *depth; size_t dstep; int drows, dcols;
    int X, Y, Z, z0, z1, zchunk;
    float voxel_size, tranc_dist, tranc_dist_inv;
    Intr intr;
    const float *gt;      // dense, unpitched: index z*Y*X + y*X + x, storage starts at z0
    double *partials;     // [blocks][8]
    unsigned *ticket;
    double *out;          // hessian: {loss, grad, hessian, count}; loss: {loss, count}
    float *real_out, *grad_out, *hess_out; int *count_out;  // optional per-voxel volumes (same indexing as gt)
    int tiles_x, tiles_y, tiles_z;  // (64 x 4 x zchunk) tiles — (256 x 4 x zchunk) when wide; workgroups stride over them
    double *publish; unsigned long long publish_seq;   // optional, host-coherent pinned memory: the last workgroup stores the sums there + the word [32] = seq
    const unsigned *mailbox; unsigned mailbox_seq;     // k_tsdf_gauss_newton<true>: the six poses arrive through a mailbox (xs_gn_post_poses)
    int il;               // wide == 2: consecutive planes a workgroup takes together before its neighbours' (1, 2, 4, 8)
    int wide;             // a lane scans four x-neighbours with 16-byte loads (X % 4 == 0 and gt 16-byte aligned): for_band_voxels_wide; 2: planes interleaved
};
struct HessPoseD { MatD33 R; dcfloat3 t; };
struct HessPoseF { float R[9]; float t[3]; };

// all 64 lanes, all of them active: v[l] + v[l ^ 1], then ^ 2, 4, 8 (DPP within a row of 16), 16, 32 — a pairwise tree, the same bits in every lane
// (float addition commutes)
__device__ __forceinline__ float wave_tree_sum_f32(float v) {
    auto dpp = [](float x, auto ctrl) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, 0xf, 0xf, false)); };
    v += dpp(v, std::integral_constant<int, 0xb1>());    // quad_perm [1, 0, 3, 2]
    v += dpp(v, std::integral_constant<int, 0x4e>());    // quad_perm [2, 3, 0, 1]
    v += dpp(v, std::integral_constant<int, 0x141>());   // row_half_mirror: quad q with quad q ^ 1 (a quad's lanes are equal by now)
    v += dpp(v, std::integral_constant<int, 0x140>());   // row_mirror: the row's halves
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// The arrival ticket: bits 0 .. 15 count the workgroups that arrived (at most XS_TSDF_REDUCE_MAX_BLOCKS = 4096 per launch), bits 16 .. 31 those of
// them that LEFT without summing (k_tsdf_gauss_newton<true>: told to, or their poses never came).  Every workgroup of a launch arrives exactly once,
// whatever it did, so the last one always exists: it puts the ticket back to zero and publishes — the sums, or, if any workgroup left (some may
// have seen their poses just before the deadline and others not), the sequence word with bit 63 set and no sums.
enum { XS_TSDF_REDUCE_MAX_BLOCKS_C = 4096 };   // workgroups per launch (they stride over the tiles); records of up to 32 doubles
enum : unsigned { TICKET_ARRIVED = 1u, TICKET_LEFT = 0x10000u, TICKET_COUNT_MASK = 0xffffu };
// (block_fold_and_finish_of: the same for a workgroup that is record `bid` of `nblocks` on its ticket — the band replay keeps one ticket per
// frame, and the records of a frame then add up exactly as those of the dense launch do)
template <int NV>
__device__ __forceinline__ void block_fold_and_finish_of(double (&v)[NV], double *partials, unsigned *ticket, double *out, double *publish,
                                                         unsigned long long publish_seq, bool left, unsigned nblocks, unsigned bid) {
    constexpr int STRIDE = NV <= 8 ? 8 : 32;  // doubles per workgroup record
    __shared__ double sm[4][NV];
    __shared__ unsigned s_last;
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    if (!left) {   // (workgroup-uniform)
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const double s = wave_sum_f64(v[k]);
            if (lane == 0) sm[wave][k] = s;
        }
        __syncthreads();
        if (tid < NV) {
            const double s = ((sm[0][tid] + sm[1][tid]) + sm[2][tid]) + sm[3][tid];
            __hip_atomic_store(&partials[(size_t)bid * STRIDE + tid], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // The record went out with agent-scope write-through stores from lanes of wave 0 (NV <= 64): once they are acknowledged the
    // record is in memory, and the same wave's first lane takes the ticket — no release fence, whose write-back of the whole
    // L2 per workgroup is what used to cap the grid at 1024 workgroups (xs_icp.hip has the measurements)
    static_assert(NV <= 64, "the record is stored by one wave");
    static_assert(XS_TSDF_REDUCE_MAX_BLOCKS_C <= (int)TICKET_COUNT_MASK, "the ticket counts arrivals in sixteen bits");
    if (wave == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) {
        const unsigned tk = __hip_atomic_fetch_add(ticket, left ? TICKET_ARRIVED + TICKET_LEFT : TICKET_ARRIVED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (tk & TICKET_COUNT_MASK) != nblocks - 1 ? 0u : ((tk >> 16) != 0 || left ? 2u : 1u);   // 2: the last one of a launch some workgroup left
        if (s_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (s_last == 2u) {
        if (tid == 0) {
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (publish) __hip_atomic_store(reinterpret_cast<unsigned long long *>(publish) + 32, publish_seq | (1ull << 63), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    if (s_last) {
        // After the acquire + barrier plain loads see every record.  All 256 threads take part: thread (g, c)
        // adds column c of records g, g + G, g + 2G, ... in that order with 16 loads in flight, and the G row
        // groups are then added in group order — fixed association, deterministic.  (One wave reading the
        // records one dependent load at a time took longer than the rest of the kernel.)
        constexpr int G = 256 / STRIDE;
        __shared__ double s_red[G][STRIDE];
        const int c = tid % STRIDE, g = tid / STRIDE;
        const double *p = partials + c;
        double s = 0.0;
        unsigned b = g;
        for (; b + G * 15 < nblocks; b += G * 16) {
            double v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = p[(size_t)(b + G * k) * STRIDE];
#pragma unroll
            for (int k = 0; k < 16; ++k) s += v[k];
        }
        for (; b < nblocks; b += G) s += p[(size_t)b * STRIDE];
        s_red[g][c] = s;
        __syncthreads();
        if (tid < NV) {
            double t = s_red[0][tid];
#pragma unroll
            for (int gg = 1; gg < G; ++gg) t += s_red[gg][tid];
            out[tid] = t;
            // the host's copy: system-scope stores into pinned memory by lanes of wave 0 (NV <= 64), then — once they are acknowledged — the
            // sequence word by its first lane: a host that sees the word sees the sums (the protocol of the ICP records: publish_host_record of xs_icp.hip, xs_icp_sum_records of xs_icp_host.hip)
            if (publish) __hip_atomic_store(&publish[tid], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        // the ticket goes back to zero for the next launch on this workspace (xs_tsdf_reduce_workspace_init zeroes it once): no fill per launch
        if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (publish && wave == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            if (tid == 0) __hip_atomic_store(reinterpret_cast<unsigned long long *>(publish) + 32, publish_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

template <int NV>
__device__ __forceinline__ void block_fold_and_finish(double (&v)[NV], double *partials, unsigned *ticket, double *out, double *publish = nullptr,
                                                      unsigned long long publish_seq = 0, bool left = false) {
    block_fold_and_finish_of(v, partials, ticket, out, publish, publish_seq, left, gridDim.x * gridDim.y * gridDim.z,
                             blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z));
}

// The dense ground-truth read is the kernels' only N^3 traffic, and a plain z loop keeps one 4-byte load
// per lane in flight (measured: 0.85 TB/s for the Hessian kernel at 512^3).  Here a lane requests thirty-two
// planes of its column at once and keeps a bit per plane whose voxel is in the band (gt != 0, |gt| <= 0.95).
// The band is a sheet: where it lies across the columns every lane holds a handful of band voxels, but where it
// runs ALONG them (a wall parallel to the z axis) six lanes of a wave hold thirty-two each and the other
// fifty-eight none — a wave that let every lane work through its own voxels ran the dual-complex body at a tenth
// of its lanes (the relocalisation pass of a box room at 1024^3: 4.7 ms against 1.4 ms for a wall across z).  So
// the voxels are dealt out again: plane by plane, the lanes that hold a band voxel append its coordinates to a
// per-wave queue in LDS (one ballot + one prefix count per plane), and whenever sixty-four are waiting every lane
// takes one — full lanes whatever the sheet's orientation; the queue runs on across chunks and tiles and is
// drained once at the end.  The order in which a lane's double sums meet their terms differs from the reference's
// thrust::reduce (unspecified there) by association only.
// (Scanning the slab as one flat array — contiguous 8 KB per wave — streamed only 6 % faster; four columns per
// lane with 16-byte loads no faster either.)
struct BandQueue {
    enum { CAP = 128 };                 // entries per wave: at most 63 left over + 64 appended
    unsigned long long (*q)[CAP];       // [wave][CAP] in LDS: x | y << 21 | z << 42
    unsigned head, tail;
};
template <class F>
__device__ __forceinline__ void band_queue_take(const HessArgs &a, BandQueue &Q, int wave, int lane, unsigned count, F &&body) {
    // lanes 0 .. count - 1 take the entries head .. head + count - 1 (the appends are this wave's own: LDS operations of
    // a wave complete in order, and the compiler may not move memory accesses across the asm)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if ((unsigned)lane < count) {
        const unsigned long long e = Q.q[wave][(Q.head + lane) % BandQueue::CAP];
        const int x = (int)(e & 0x1fffff), y = (int)((e >> 21) & 0x1fffff), z = (int)(e >> 42);
        const size_t index = ((size_t)(z - a.z0) * a.Y + y) * a.X + x;
        body(x, y, z, index, a.gt[index]);   // (re-read: a cache hit, instead of thirty-two live registers)
    }
    Q.head += count;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads are done before a later append may reuse the slots
}
// the queue's side of the scan: the lanes whose voxel (bit b of their mask) is in the band append it; sixty-four waiting are dealt out
template <class F, class XYZ>
__device__ __forceinline__ void band_queue_append(const HessArgs &a, BandQueue &Q, int wave, int lane, bool mine, XYZ &&xyz, F &&body) {
    const unsigned long long who = __ballot(mine);
    if (!who) return;
    if (mine) {
        const unsigned pos = Q.tail + __popcll(who & ((1ull << lane) - 1ull));
        Q.q[wave][pos % BandQueue::CAP] = xyz();
    }
    Q.tail += (unsigned)__popcll(who);
    if (Q.tail - Q.head >= 64u) band_queue_take(a, Q, wave, lane, 64u, body);
}
// The ground truth is read ONCE per launch and is larger than the 256 MiB Infinity Cache (512 MiB at 512^3, 4 GiB at 1024^3): the scan's
// loads are NONTEMPORAL (round 6, profiles/r06_hess_scan.txt).  With the default policy every line read is allocated in the cache, and
// allocating evicts — what the predecessor left dirty first: the same scan streamed 3.0-3.8 TB/s behind a kernel that had written 1 GiB and
// 4.1-5.9 TB/s back to back, against 5.9-6.4 TB/s either way without allocation.
typedef float xs_f4 __attribute__((ext_vector_type(4)));
template <class F>
__device__ __forceinline__ void for_band_voxels(const HessArgs &a, BandQueue &Q, int wave, int lane, int x, int y, bool in_volume, int zb, int ze,
                                                F &&body) {
    constexpr int ZB = 32;
    const size_t plane = (size_t)a.Y * a.X;
    const size_t first = in_volume ? (size_t)(zb - a.z0) * plane + (size_t)y * a.X + x : 0;
    for (int zc = zb; zc < ze; zc += ZB) {
        const float *col = a.gt + first + (size_t)(zc - zb) * plane;
        unsigned mask = 0;
        if (in_volume) {
#pragma unroll
            for (int j = 0; j < ZB; ++j) {
                const float g = (zc + j < ze) ? col[(size_t)j * plane] : 0.f;   // (the fallback for rows that are no multiple of 16 bytes: as round 5 measured it)
                if (!(g == 0 || fabsf(g) > 0.95)) mask |= 1u << j;
            }
        }
        if (!__ballot(mask != 0)) continue;                       // free space: the usual case
        for (int j = 0; j < ZB; ++j)
            band_queue_append(a, Q, wave, lane, (mask >> j) & 1u,
                              [&] { return (unsigned long long)x | ((unsigned long long)y << 21) | ((unsigned long long)(zc + j) << 42); }, body);
    }
}
// Round 6: sixteen bytes per lane.  A lane takes FOUR x-neighbours (x0 .. x0 + 3: a wave reads 1 KiB of a row per instruction, a
// workgroup four rows) and requests eight planes at once — the same 32 registers and 32 mask bits as the column form, bit 4 j + k =
// voxel (x0 + k, y, zc + j), dealt out through the same queue.  Scan alone (a map with one wall, nothing but the read, the band test and
// the ballots; profiles/tools/scan_probe.hip on one MI355X): 4.4-4.6 TB/s for the column form at 512^3 (5.1-5.2 at 1024^3), 5.9 (5.4-5.9)
// for this shape, 6.2-6.3 (6.4) for this shape with nontemporal loads; a flat sweep of the array, which knows no coordinates: 6.5 (6.7).
template <class F>
__device__ __forceinline__ void for_band_voxels_wide(const HessArgs &a, BandQueue &Q, int wave, int lane, int x0, int y, bool in_volume, int zfirst, int zstep, int zend,
                                                     F &&body) {
    // this tile's planes: zfirst, zfirst + zstep, ... below a.z1 — INTERLEAVED with the other workgroups that share its columns.  A band is
    // a sheet a few planes thick: cut into runs of consecutive planes, a wall across z would put all of its voxels into the one run that
    // holds it (1 workgroup in 16 at 512^3 did the whole dual-complex evaluation: 0.145 ms against 0.117); plane by plane it goes to seven.
    constexpr int ZB = 8;
    const size_t plane = (size_t)a.Y * a.X;
    const int il = a.il;                                       // consecutive planes taken together (1, 2, 4 or 8); zstep counts such groups
    auto zof = [&](int zc, int j) { return zc + (j % il) + (j / il) * il * zstep; };
    const float *col = a.gt + (in_volume ? (size_t)(zfirst - a.z0) * plane + (size_t)y * a.X + x0 : 0);
    for (int zc = zfirst; zc < zend; zc += ZB * zstep, col += (size_t)ZB * zstep * plane) {
        unsigned mask = 0;
        if (in_volume) {
            xs_f4 v[ZB];
#pragma unroll
            for (int j = 0; j < ZB; ++j)
                v[j] = (zof(zc, j) < zend) ? __builtin_nontemporal_load(reinterpret_cast<const xs_f4 *>(col + (size_t)(zof(zc, j) - zc) * plane)) : xs_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < ZB; ++j) {
                if (!(v[j].x == 0 || fabsf(v[j].x) > 0.95)) mask |= 1u << (4 * j);
                if (!(v[j].y == 0 || fabsf(v[j].y) > 0.95)) mask |= 2u << (4 * j);
                if (!(v[j].z == 0 || fabsf(v[j].z) > 0.95)) mask |= 4u << (4 * j);
                if (!(v[j].w == 0 || fabsf(v[j].w) > 0.95)) mask |= 8u << (4 * j);
            }
        }
        if (!__ballot(mask != 0)) continue;                       // free space: the usual case
        for (int b = 0; b < 32; ++b)
            band_queue_append(a, Q, wave, lane, (mask >> b) & 1u,
                              [&] { return (unsigned long long)(x0 + (b & 3)) | ((unsigned long long)y << 21) | ((unsigned long long)zof(zc, b >> 2) << 42); }, body);
    }
}
// the tile walk the three kernels share: a bounded number of workgroups (each pays a ticket when it retires) stride over the
// (64 x 4 x zchunk) tiles — (256 x 4 x zchunk) in the wide form — one column (four) per lane, one row of columns per wave
template <class F>
__device__ __forceinline__ void walk_band(const HessArgs &a, F &&body) {
    __shared__ unsigned long long s_queue[4][BandQueue::CAP];
    BandQueue Q{s_queue, 0u, 0u};
    const int lane = threadIdx.x, wave = threadIdx.y;            // blockDim = (64, 4)
    const int ntiles = a.tiles_x * a.tiles_y * a.tiles_z;
    const bool skew = a.wide == 2 && (gridDim.x % (unsigned)a.tiles_z) == 0;   // (else consecutive rounds already land in different z groups)
    for (int tile = blockIdx.x, round = 0; tile < ntiles; tile += gridDim.x, ++round) {
        if (a.wide == 2) {   // z group fastest: tile = column * G + g, planes a.z0 + (g + k G) il + (0 .. il - 1)
            const int G = a.tiles_z, column = tile / G, g = (tile % G + (skew ? round : 0)) % G;
            const int x0 = 4 * (int)threadIdx.x + (column % a.tiles_x) * 256, y = threadIdx.y + (column / a.tiles_x) * 4;
            for_band_voxels_wide(a, Q, wave, lane, x0, y, x0 < a.X && y < a.Y, a.z0 + g * a.il, G, a.z1, body);
            continue;
        }
        const int y = threadIdx.y + ((tile / a.tiles_x) % a.tiles_y) * 4;
        const int zb = a.z0 + (tile / (a.tiles_x * a.tiles_y)) * a.zchunk, ze = min(zb + a.zchunk, a.z1);
        if (a.wide) {
            const int x0 = 4 * (int)threadIdx.x + (tile % a.tiles_x) * 256;
            for_band_voxels_wide(a, Q, wave, lane, x0, y, x0 < a.X && y < a.Y, zb, 1, ze, body);
        } else {
            const int x = threadIdx.x + (tile % a.tiles_x) * 64;
            for_band_voxels(a, Q, wave, lane, x, y, x < a.X && y < a.Y, zb, ze, body);
        }
    }
    band_queue_take(a, Q, wave, lane, Q.tail - Q.head, body);   // what is left: fewer than sixty-four
}

// ---- the six-pose residual of the Gauss-Newton terms (k_tsdf_gauss_newton; described there) ----
struct GnPoses { MatS33 R[6]; cfloat3 t[6]; };
__device__ __forceinline__ bool tsdf_error_c(const HessArgs &a, const MatS33 &R, const cfloat3 &t, float vgx, float vgy, float vgz, float gt,
                                             cfloat &error) {
    cfloat3 v_g; v_g.x = cfloat(vgx); v_g.y = cfloat(vgy); v_g.z = cfloat(vgz);
    cfloat3 v_c;
    v_c.x = dot(R.data[0], v_g) + t.x;
    v_c.y = dot(R.data[1], v_g) + t.y;
    v_c.z = dot(R.data[2], v_g) + t.z;
    const cfloat inv_z = cfloat(1.0f) / v_c.z;
    if (inv_z.re < 0) return false;
    const cfloat image_x = v_c.x * inv_z * a.intr.fx + a.intr.cx;
    const cfloat image_y = v_c.y * inv_z * a.intr.fy + a.intr.cy;
    const int coo_x = __float2int_rd(image_x.re - 0.5f), coo_y = __float2int_rd(image_y.re - 0.5f);
    if (!(coo_x > 1 && coo_y > 1 && coo_x < a.dcols - 1 && coo_y < a.drows - 1)) return false;
    const int near_x = __float2int_rn(image_x.re), near_y = __float2int_rn(image_y.re);
    cfloat Dp(row_ptr(a.depth, a.dstep, near_y)[near_x]);
    const float d00 = row_ptr(a.depth, a.dstep, coo_y)[coo_x], d10 = row_ptr(a.depth, a.dstep, coo_y)[coo_x + 1];
    const float d01 = row_ptr(a.depth, a.dstep, coo_y + 1)[coo_x], d11 = row_ptr(a.depth, a.dstep, coo_y + 1)[coo_x + 1];
    if (d00 != 0.0f && d01 != 0.0f && d10 != 0.0f && d11 != 0.0f) {
        const cfloat one(1.0f);
        const cfloat fa = image_x - cfloat(float(coo_x) + 0.5f);
        const cfloat fb = image_y - cfloat(float(coo_y) + 0.5f);
        Dp = d00 * (one - fa) * (one - fb) + d10 * fa * (one - fb) + d01 * (one - fa) * fb + d11 * fa * fb;
    }
    if (Dp.re > 5 || Dp.re < 0.2) return false;
    const cfloat xl = (image_x - a.intr.cx) / a.intr.fx;
    const cfloat yl = (image_y - a.intr.cy) / a.intr.fy;
    const cfloat3 v_c_1 = mk3(Dp * xl, Dp * yl, Dp);
    const cfloat distance = norm(v_c_1) - norm(v_c);
    const cfloat gt_distance = cfloat(gt) * a.tranc_dist;
    error = (distance - gt_distance) * a.tranc_dist_inv;
    return !(fabsf(error.re) > 1);
}

// One band voxel's contribution to the 29 sums of the six seeded poses (k_tsdf_gauss_newton, k_band_gauss_newton): a voxel counts only if
// every seeded evaluation keeps it (they share their real parts).  The order of the additions is part of the band replay's bit-identity.
__device__ __forceinline__ void gn_terms_add(const HessArgs &a, const GnPoses &P, int xq, int yq, int z, float gt, double (&acc)[29]) {
    const float vgx = (float(xq) + 0.5f) * a.voxel_size, vgy = (float(yq) + 0.5f) * a.voxel_size, vgz = (float(z) + 0.5f) * a.voxel_size;
    cfloat e[6];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        ok = ok && tsdf_error_c(a, P.R[k], P.t[k], vgx, vgy, vgz, gt, e[k]);
        // one evaluation at a time: left to itself the scheduler interleaves all six (256 registers, one wave per SIMD)
        asm volatile("" : "+v"(e[k].re), "+v"(e[k].im) :: "memory");
    }
    if (!ok) return;
    const double r = (double)e[0].re;
    int s = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int k = j; k < 6; ++k) acc[s++] += (double)e[j].im * (double)e[k].im;
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[21 + k] += (double)e[k].im * r;
    acc[27] += r * r;
    acc[28] += 1.0;
}

// ---- the dual-complex squared residual of the Hessian kernels (k_tsdf_hessian, k_band_pose_hessian) ----
// One band voxel's loss = error^2 at the dual-complex pose P: value() the squared residual, grad() its derivative along the eps1 seed times h,
// hessian() the mixed second derivative times h^2.  False where a gate of ComputeLocalTsdfHessianKernel (TsdfFusion.cu:204-283) drops the voxel;
// the gates read real parts only.
__device__ __forceinline__ bool tsdf_loss_d(const HessArgs &a, const HessPoseD &P, int xq, int yq, int z, float gt, dcfloat &loss) {
    const dcfloat gt_tsdf(gt);
    const dcfloat vgx((float(xq) + 0.5f) * a.voxel_size);
    const dcfloat vgy((float(yq) + 0.5f) * a.voxel_size);
    const dcfloat vgz((float(z) + 0.5f) * a.voxel_size);
    dcfloat3 v_g; v_g.x = vgx; v_g.y = vgy; v_g.z = vgz;
    dcfloat3 v_c;
    v_c.x = dot(P.R.data[0], v_g) + P.t.x;
    v_c.y = dot(P.R.data[1], v_g) + P.t.y;
    v_c.z = dot(P.R.data[2], v_g) + P.t.z;
    const dcfloat inv_z = dcfloat(1.0f) / v_c.z;
    if (inv_z.value() < 0) return false;
    const dcfloat image_x = v_c.x * inv_z * a.intr.fx + a.intr.cx;
    const dcfloat image_y = v_c.y * inv_z * a.intr.fy + a.intr.cy;
    const int coo_x = __float2int_rd(image_x.value() - 0.5f), coo_y = __float2int_rd(image_y.value() - 0.5f);
    if (!(coo_x > 1 && coo_y > 1 && coo_x < a.dcols - 1 && coo_y < a.drows - 1)) return false;
    const int near_x = __float2int_rn(image_x.value()), near_y = __float2int_rn(image_y.value());
    dcfloat Dp(row_ptr(a.depth, a.dstep, near_y)[near_x]);
    const dcfloat d00(row_ptr(a.depth, a.dstep, coo_y)[coo_x]), d10(row_ptr(a.depth, a.dstep, coo_y)[coo_x + 1]);
    const dcfloat d01(row_ptr(a.depth, a.dstep, coo_y + 1)[coo_x]), d11(row_ptr(a.depth, a.dstep, coo_y + 1)[coo_x + 1]);
    if (d00.value() != 0.0f && d01.value() != 0.0f && d10.value() != 0.0f && d11.value() != 0.0f) {  // :248-251, threshold unused
        const dcfloat one(1.0f);
        const dcfloat fa = image_x - dcfloat(float(coo_x) + 0.5f);
        const dcfloat fb = image_y - dcfloat(float(coo_y) + 0.5f);
        Dp = d00 * (one - fa) * (one - fb) + d10 * fa * (one - fb) + d01 * (one - fa) * fb + d11 * fa * fb;
    }
    if (Dp.value() > 5 || Dp.value() < 0.2) return false;
    const dcfloat xl = (image_x - a.intr.cx) / a.intr.fx;
    const dcfloat yl = (image_y - a.intr.cy) / a.intr.fy;
    dcfloat3 v_c_1; v_c_1.x = Dp * xl; v_c_1.y = Dp * yl; v_c_1.z = Dp;
    const dcfloat distance = norm(v_c_1) - norm(v_c);
    const dcfloat gt_distance = gt_tsdf * a.tranc_dist;
    const dcfloat error = (distance - gt_distance) * a.tranc_dist_inv;
    if (fabsf(error.value()) > 1) return false;
    loss = error * error;
    return true;
}

// ---- the real-valued squared residual of the loss kernels (k_tsdf_loss, k_band_score_poses) ----
// One band voxel's loss = error^2 at the real pose P, the float twin of tsdf_loss_d: projection, the inv_z < 0 gate, the image gate, nearest
// and bilinear depth, the 0.2 - 5 m gate and the |error| > 1 gate of ComputeLocalTsdfLossKernel (TsdfFusion.cu:335-410).  False where a gate
// drops the voxel.  Both kernels take a voxel's float and its keep / drop decision from here, so their counts are equal and their sums add the
// same terms.
__device__ __forceinline__ bool tsdf_loss_f(const HessArgs &a, const HessPoseF &P, int xq, int yq, int z, float gt, float &loss) {
    const float vgx = (float(xq) + 0.5f) * a.voxel_size, vgy = (float(yq) + 0.5f) * a.voxel_size, vgz = (float(z) + 0.5f) * a.voxel_size;
    const float vcx = (P.R[0] * vgx + P.R[1] * vgy + P.R[2] * vgz) + P.t[0];
    const float vcy = (P.R[3] * vgx + P.R[4] * vgy + P.R[5] * vgz) + P.t[1];
    const float vcz = (P.R[6] * vgx + P.R[7] * vgy + P.R[8] * vgz) + P.t[2];
    const float inv_z = 1.0f / vcz;
    if (inv_z < 0) return false;
    const float image_x = vcx * inv_z * a.intr.fx + a.intr.cx;
    const float image_y = vcy * inv_z * a.intr.fy + a.intr.cy;
    const int coo_x = __float2int_rd(image_x - 0.5f), coo_y = __float2int_rd(image_y - 0.5f);
    if (!(coo_x > 1 && coo_y > 1 && coo_x < a.dcols - 1 && coo_y < a.drows - 1)) return false;
    const int near_x = __float2int_rn(image_x), near_y = __float2int_rn(image_y);
    float Dp = row_ptr(a.depth, a.dstep, near_y)[near_x];
    const float d00 = row_ptr(a.depth, a.dstep, coo_y)[coo_x], d10 = row_ptr(a.depth, a.dstep, coo_y)[coo_x + 1];
    const float d01 = row_ptr(a.depth, a.dstep, coo_y + 1)[coo_x], d11 = row_ptr(a.depth, a.dstep, coo_y + 1)[coo_x + 1];
    if (d00 != 0.0f && d01 != 0.0f && d10 != 0.0f && d11 != 0.0f) {
        const float one = 1.0f;
        const float fa = image_x - (float(coo_x) + 0.5f), fb = image_y - (float(coo_y) + 0.5f);
        Dp = d00 * (one - fa) * (one - fb) + d10 * fa * (one - fb) + d01 * (one - fa) * fb + d11 * fa * fb;
    }
    if (Dp > 5 || Dp < 0.2) return false;
    const float xl = (image_x - a.intr.cx) / a.intr.fx, yl = (image_y - a.intr.cy) / a.intr.fy;
    const float v1x = Dp * xl, v1y = Dp * yl, v1z = Dp;
    const float distance = sqrtf(v1x * v1x + v1y * v1y + v1z * v1z) - sqrtf(vcx * vcx + vcy * vcy + vcz * vcz);
    const float gt_distance = gt * a.tranc_dist;
    const float error = (distance - gt_distance) * a.tranc_dist_inv;
    if (fabsf(error) > 1) return false;
    loss = error * error;
    return true;
}

// host: the walk's tiling and grid for the slab [z0, z1) of gt (xs_residual.hip; heavy_body: the interleaved form of the six-pose and Hessian kernels)
int hess_tiling(HessArgs &a, const int *res, const float *gt, int z0, int z1, dim3 &grid, bool heavy_body);
