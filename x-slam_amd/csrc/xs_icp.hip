// xs_icp.hip — ICP point-to-plane normal equations for gfx950.  Replaces
// XKinectFusion/src/ICP.cu:166-281 (Combined: search_newton + operator()), :5-118 (LDS tree
// reductions), :120-164 (TranformReduction second kernel) and :365-429 (estimateCombined).
//
// Reference shape: one pixel per thread, 27 complex products each pushed through an LDS tree
// (27 x 2 barriers + 8 steps), 518 KB of per-block partials, and a second 27-block launch to
// add them up; the tree's tail relies on 32-wide warp-synchronous execution (ICP.cu:40-65).
// Here: one 64-pixel tile per wave, eight waves per workgroup (every level of a 640 x 480 frame; larger images fall back to four
// waves striding over the tiles with the sums in registers).  The 27 complex products of a pixel (complex float, ICP.cu:273) go
// to an LDS tile as floats and are added there in double — lanes in a fixed interleaved order, then the waves in order — as the
// reference accumulates in double (ICP.cu:274); the workgroup writes one 448-byte record with write-through stores and takes a
// ticket; the last workgroup to arrive adds the records in a fixed order, so the result is deterministic and there is no
// second launch.  The 55 sums go to device memory, or straight into host-coherent pinned memory with a completion word behind them
// (done_flag), or — the orchestrator's form since round 6 — as 55 stores of {launch number, sum} that need no word behind them
// (XS_ICP_PUBLISH_PAIRS).  How each phase was measured: profiles/tools/trace_icp.sh, profiles/r02_icp_phases.txt.
//
// This file: the two kernels, k_icp as a sequence of phases, and everything that launches them.  Beside it: xs_icp_args.h (what a launch
// receives), xs_icp_search.h (the correspondence search and the row of a match), xs_icp_fold.h (the additions that are functions),
// xs_icp_launch.h (the instances, what an entry point asks for, its validation into kernel arguments),
// xs_icp_host.hip (the host halves of the publish protocols, estimateCombined), xs_icp_selftest.hip (the gate self-test).
#include "xs_device.h"
#include "xs_mailbox.h"
#include "xs_icp_args.h"
#include "xs_icp_search.h"
#include "xs_icp_fold.h"
#include "xs_icp_launch.h"
#include "../../include/xslam_amd.h"

// The record hand-offs below (relaxed agent-scope stores + s_waitcnt vmcnt(0) + a relaxed ticket, no release fence) are correct because
// gfx942 / gfx950 implement an agent-scope atomic store as a write-through (sc1) store that is acknowledged from memory; that is
// outside the HIP / LLVM memory model, so the file refuses to build for anything else rather than publish stale records there.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx942__) && !defined(__gfx950__)
#error "write-through record publish: gfx942 / gfx950 only (use a release fence + acq_rel ticket on other targets)"
#endif

// Phase stamps of every workgroup (experiment build -DXS_ICP_TRACE, profiles/tools/trace_icp.sh): 100 MHz wall clock at entry, pose ready,
// pixels done, fold done, record stored, released, ticket back, (last workgroup:) acquired, gathered, result out.
#ifdef XS_ICP_TRACE
__device__ unsigned long long g_icp_trace[768 * 16];
#define XS_STAMP(i) do { if (threadIdx.x == 0) { g_icp_trace[blockIdx.x * 16 + (i)] = wall_clock64(); \
    if ((i) == 0) g_icp_trace[blockIdx.x * 16 + 10] = ((unsigned long long)__builtin_amdgcn_s_getreg(0xF814) << 32) | __builtin_amdgcn_s_getreg(0xF804); } } while (0)
extern "C" int xs_debug_icp_trace(unsigned long long *out_host) {
    return (int)hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_icp_trace), sizeof(g_icp_trace));
}
#else
#define XS_STAMP(i) do { } while (0)
#endif

// ---- the phases of k_icp that publish -----------------------------------------------------------------------------------------------
// host-visible completion word: push everything out, then publish the sequence number
__device__ __forceinline__ void publish_done(const IcpArgs &a) {
    // (a system-scope release store is the write-back of what precedes it + the store; a __threadfence_system() in front of it
    // wrote back a second time and invalidated for nothing)
    __hip_atomic_store(a.done_flag, a.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// the give-up of a posted launch whose pose never came: the launch's number with kIcpTimeoutBit, in a word the host watches
__device__ __forceinline__ void store_gave_up(unsigned long long *word, unsigned long long seq) {
    __hip_atomic_store(word, seq | kIcpTimeoutBit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// Host fold: the record goes straight to host-coherent pinned memory (28 16-byte stores of wave 0), then — once
// those stores are acknowledged and released at system scope — its last word receives the launch's sequence
// number, and the workgroup is done: no ticket, no write-back of this XCD's L2 for another workgroup to read,
// no last workgroup gathering 512 records from memory.  The host spins on the sequence words and adds the
// records in index order (xs_icp_sum_records): the same deterministic association for every launch.
template <int SLOTS>
__device__ __forceinline__ void publish_host_record(const IcpArgs &a, const double (*smem)[NP]) {
    if (threadIdx.x < 64) {
        if (threadIdx.x < NP / 2) {
            const int k0 = 2 * threadIdx.x, k1 = k0 + 1;
            d2 v = wave_order_sum2<SLOTS>(smem, k0);
            if (k1 > NS) v.y = 0.0;   // (the pad column of smem is never written)
            if (k1 <= NS) reinterpret_cast<d2 *>(a.host_records)[(size_t)blockIdx.x * (NP / 2) + threadIdx.x] = v;
            else a.host_records[(size_t)blockIdx.x * NP + k0] = v.x;      // the count; the pad word is the sequence slot
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0)
            __hip_atomic_store(reinterpret_cast<unsigned long long *>(a.host_records) + (size_t)blockIdx.x * NP + (NP - 1), a.record_seq,
                               __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// publish: the storing wave waits until its write-through stores are acknowledged, then its first lane takes a ticket
// (same wave, program order: no barrier in between); the atomic is performed at agent scope after the records are in memory.
// s_last: whether this workgroup is the last to arrive; the caller follows with a workgroup barrier.
__device__ __forceinline__ void take_ticket(const IcpArgs &a, unsigned &s_last) {
    if (threadIdx.x < 64) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        XS_STAMP(4);
    }
    if (threadIdx.x == 0) {
        XS_STAMP(5);
        const unsigned tk = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (tk == gridDim.x - 1) ? 1u : 0u;
        XS_STAMP(6);
        if (s_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            // the ticket re-arms itself: the next launch on this stream starts from zero
            __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // holds the barrier until the invalidate has completed
            XS_STAMP(7);
        }
    }
}
// the last workgroup's output: sums 2 q and 2 q + 1 of thread q < 28, plain or as pairs
__device__ __forceinline__ void store_sums(const IcpArgs &a, d2 t) {
    if (a.pairs) {
        // Every sum leaves as ONE 16-byte store {sequence number, sum}: a store of one lane cannot be seen in halves, so the host
        // needs no word that is ordered behind the others — and the kernel no wait for its stores' acknowledgement, barrier and
        // release store between the sums and that word (profiles/r06_ab_icp_publish_pairs.txt).
        typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
        ull2 *pairs = reinterpret_cast<ull2 *>(a.out);
        __builtin_nontemporal_store(ull2{a.done_seq, (unsigned long long)__double_as_longlong(t.x)}, pairs + 2 * threadIdx.x);
        if (2 * threadIdx.x + 1 < NS + 1)
            __builtin_nontemporal_store(ull2{a.done_seq, (unsigned long long)__double_as_longlong(t.y)}, pairs + 2 * threadIdx.x + 1);
    } else {
        a.out[2 * threadIdx.x] = t.x;
        if (2 * threadIdx.x + 1 < NS + 1) a.out[2 * threadIdx.x + 1] = t.y;
    }
}

#ifdef XS_ICP_WAVES_PER_EU   // experiment switch (profiles/tools/ab_icp_occupancy.sh): force the occupancy of the reduction kernel
#define XS_ICP_OCC __attribute__((amdgpu_waves_per_eu(XS_ICP_WAVES_PER_EU, XS_ICP_WAVES_PER_EU)))
#else
#define XS_ICP_OCC
#endif
// WAVES = 4: lanes stride over the tiles and carry the 27 complex sums in registers (54 doubles, 190 VGPRs: two waves per SIMD) —
// any image size.  WAVES = 8: one tile per wave, chosen whenever all tiles can be resident at once (a 640 x 480 level 0 has
// 4 800): nothing is carried from tile to tile, so the products go straight from the row to the LDS fold as floats and the kernel
// needs 80-104 registers.  PASSES: the LDS tile holds all 55 values of the eight waves at once (123 KB: one workgroup per CU —
// launches of up to 256 workgroups: levels 1 and 2), 28 in two passes (64 KB, two per CU at four waves per SIMD, up to 512) or 19
// in three (45 KB, three per CU at six waves per SIMD, 80 VGPRs: up to 768 — level 0's 600).
// BAL (round 3; PASSES = 2): a launch whose tiles outnumber the resident waves by up to a quarter — level 0 of a 640 x 480 frame: 4 800 tiles
// for 4 096 — deals them out evenly instead of launching a third workgroup on some CUs: workgroup b takes ntiles / grid tiles, the first
// ntiles % grid one more, and its first WAVES / 4 waves work through a second tile (in lock step: search_issue / search_finish).  With 600
// one-tile-per-wave workgroups 88 of the 256 CUs held three of them (24 tiles on the busiest against 18.75 on average) and the launch lasted
// as long as those.  WAVES = 8: 512 workgroups (two per CU) of nine or ten tiles — 22.3 -> 20.4 us per launch inside the loop; WAVES = 16
// (the default): 256 workgroups (one per CU, 158 KB of LDS) of 18 or 19 — half the records for the last workgroup to add and half the
// tickets: 18.9 us (profiles/r03_ab_icp_balanced_fps.txt).  The partition is a function of the launch geometry alone, so the sums keep one
// fixed association (slot order = tile order inside a workgroup).
// The body is a sequence of phases, each under its heading.  A phase is a function of its own only where that left the text of all 18
// instances as it was (publish_host_record, take_ticket, sum_row_groups, store_sums, store_gave_up, fill_row, search_gates); the others were
// tried as __forceinline__ functions too and moved the register allocation of whole instances — which phase, in which forms, how many
// lines: profiles/icp_split_kernels.txt — so they stand here, in the one body whose schedule and registers were measured.
template <int POSE_SRC, int WAVES, int PASSES, bool BAL = false>
__global__ void __launch_bounds__(64 * WAVES)
    __attribute__((amdgpu_waves_per_eu(WAVES == 4 || PASSES == 1 ? 2 : (PASSES == 2 ? 4 : 6), WAVES == 4 || PASSES == 1 ? 2 : (PASSES == 2 ? 4 : 6))))
    k_icp(const IcpArgs a) {
    static_assert(!BAL || ((WAVES == 8 || WAVES == 16) && PASSES == 2), "the balanced instances are the eight- and sixteen-wave, two-pass ones");
    constexpr int EXTRA = BAL ? WAVES / 4 : 0;   // waves that work through a second tile
    constexpr int SLOTS = WAVES + EXTRA;         // tiles a workgroup can take
    XS_STAMP(0);
#ifndef XS_ICP_NO_PRIO
    // an ICP launch is a chain of dependent steps on few waves; the announced next frame's bilateral filter (HintNextFrame) shares its
    // SIMDs with them and is throughput work: these waves go first at the issue arbiter
    __builtin_amdgcn_s_setprio(3);
#endif
    // ---- phase: tile assignment and vertex prefetch ----
    // one tile per wave: the tile's current-frame vertices are on their way before the pose is (a pixel outside the image reads
    // pixel (0, y0): resident, never used)
    cfloat3 pre_v, pre_v2;
    bool pre_ok = false, pre_ok2 = false;
    int pre_x = 0, pre_y = a.y0, pre_x2 = 0, pre_y2 = a.y0;
    if constexpr (WAVES >= 8) {
        const int tiles_x0 = (a.cols + 63) / 64;
        const int nt0 = tiles_x0 * (a.y1 - a.y0);
        int t0 = blockIdx.x * WAVES + (threadIdx.x >> 6), t1 = nt0;
        if constexpr (BAL) {
            const int base = nt0 / (int)gridDim.x, rem = nt0 % (int)gridDim.x;
            const int start = (int)blockIdx.x * base + min((int)blockIdx.x, rem), cnt = base + ((int)blockIdx.x < rem ? 1 : 0);
            const int w = threadIdx.x >> 6;
            t0 = w < cnt ? start + w : nt0;
            t1 = WAVES + w < cnt ? start + WAVES + w : nt0;
        }
        const int y = a.y0 + t0 / tiles_x0, x = (t0 % tiles_x0) * 64 + (threadIdx.x & 63);
        pre_ok = t0 < nt0 && x < a.cols;
        if (pre_ok) { pre_x = x; pre_y = y; }
#ifndef XS_ICP_NO_PREFETCH
        load_vertex(a, pre_x, pre_y, pre_v);
#endif
        if constexpr (BAL) {
            if (threadIdx.x < 64 * EXTRA) {   // the first waves: a second tile
                const int y2 = a.y0 + t1 / tiles_x0, x2 = (t1 % tiles_x0) * 64 + (threadIdx.x & 63);
                pre_ok2 = t1 < nt0 && x2 < a.cols;
                if (pre_ok2) { pre_x2 = x2; pre_y2 = y2; }
                load_vertex(a, pre_x2, pre_y2, pre_v2);
            }
        }
    }
    // ---- phase: the pose, per POSE_SRC ----
    // (the decode of the 24 floats stands twice here and once in k_icp_solve: one decode_pose(word functor) changed 12 to 3 510 lines of the
    // twelve instances that decode, and 34 of k_icp_solve)
    MatS33 Rcurr = a.Rcurr;
    cfloat3 tcurr = a.tcurr;
    // (readfirstlane: the 24 floats are wave-uniform and belong in scalar registers, like the kernel
    // arguments they replace)
    auto uni = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    if (POSE_SRC == POSE_DEVICE) {
        // the pose left by the previous launch on this stream; a failed solve ends the loop
        if (a.pose->status != 0) {
            if (blockIdx.x == 0 && threadIdx.x == 0 && a.done_flag) publish_done(a);
            return;
        }
        const float *pr = a.pose->R, *pt = a.pose->t;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            Rcurr.data[r].x = cfloat(uni(pr[6 * r + 0]), uni(pr[6 * r + 1]));
            Rcurr.data[r].y = cfloat(uni(pr[6 * r + 2]), uni(pr[6 * r + 3]));
            Rcurr.data[r].z = cfloat(uni(pr[6 * r + 4]), uni(pr[6 * r + 5]));
        }
        tcurr.x = cfloat(uni(pt[0]), uni(pt[1])); tcurr.y = cfloat(uni(pt[2]), uni(pt[3])); tcurr.z = cfloat(uni(pt[4]), uni(pt[5]));
    }
    if (POSE_SRC == POSE_POSTED) {
        // Pose mailbox (xs_icp_post_pose writes it; xs_icp_mailbox_alloc puts it in
        // device memory the CPU reaches through the large BAR, so polling stays off the PCIe link — 512
        // workgroups polling pinned host memory cost 50 us per iteration): four 32-byte sectors, each starting
        // with the sequence number, carrying cmd (0 = run, 1 = abandon the launch) and the 18 floats of Rcurr followed by the 6 of
        // tcurr — layout and reasons in xs_mailbox.h.  The load that finds the launch's number in all four sectors holds the payload.
        // One wave per workgroup polls the mailbox (system-scope loads: never cached) until
        // both lines carry this launch's sequence number, then hands the 32 words to the others through
        // LDS.  Bounded: after MAILBOX_MAX_POLLS the launch gives up and says so in the completion word.
        __shared__ unsigned s_mail[MAILBOX_WORDS];
        if (threadIdx.x < 64) mailbox_wait(a.mailbox, a.mailbox_seq, s_mail, (int)threadIdx.x);   // (xs_mailbox.h)
        __syncthreads();
        const unsigned cmd = s_mail[1];
        if (cmd != 0) {
            // the give-up, in whichever words the host watches.  (The three conditions stay as they are: folded into one
            // `cmd == 2 && threadIdx.x == 0` around three tests they changed 354 to 962 lines of the six posted instances.)
            if (cmd == 2 && threadIdx.x == 0 && a.done_flag) store_gave_up(a.done_flag, a.done_seq);
            if (cmd == 2 && threadIdx.x == 0 && a.pairs)   // (the first pair's sequence word carries the give-up)
                store_gave_up(reinterpret_cast<unsigned long long *>(a.out), a.done_seq);
            if (cmd == 2 && threadIdx.x == 0 && a.host_records)   // host fold: the give-up shows in the record's sequence word
                store_gave_up(reinterpret_cast<unsigned long long *>(a.host_records) + (size_t)blockIdx.x * NP + (NP - 1), a.record_seq);
            return;
        }
        auto word = [&](int i) { return uni(__uint_as_float(s_mail[mailbox_word_of(i)])); };
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            Rcurr.data[r].x = cfloat(word(6 * r + 0), word(6 * r + 1));
            Rcurr.data[r].y = cfloat(word(6 * r + 2), word(6 * r + 3));
            Rcurr.data[r].z = cfloat(word(6 * r + 4), word(6 * r + 5));
        }
        tcurr.x = cfloat(word(18), word(19)); tcurr.y = cfloat(word(20), word(21)); tcurr.z = cfloat(word(22), word(23));
    }
    XS_STAMP(1);
    // 64 consecutive columns per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tiles_x = (a.cols + 63) / 64;
    const int ntiles = tiles_x * (a.y1 - a.y0);
    __shared__ __attribute__((aligned(16))) double smem[SLOTS][NP];   // (wave_order_sum2 reads it in 16-byte pairs)
    // one LDS buffer for the fold's tile and, afterwards, the last workgroup's row-group sums
    constexpr int PV = (NS + 1 + PASSES - 1) / PASSES;   // eight-wave instance: 55, 28 or 19 values per pass
    constexpr int RS = 68;                               // ... in rows 68 floats apart
    constexpr int TILE_BYTES = WAVES == 4 ? 4 * 28 * 65 * 8 : SLOTS * PV * RS * 4;
    __shared__ __attribute__((aligned(16))) unsigned char lds_tile[TILE_BYTES];
    if constexpr (WAVES == 4) {
    // ---- phase: pixels, four waves striding over the tiles ----
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    double cnt = 0.0;
    // workgroups stride over (row, column-tile) pairs
    for (int t = blockIdx.x * 4 + wave; t < ntiles; t += gridDim.x * 4) {
        const int y = a.y0 + t / tiles_x;
        const int x = (t % tiles_x) * 64 + lane;
        if (x >= a.cols) continue;
        cfloat3 n, d, s;
        if (!search(a, Rcurr, tcurr, x, y, n, d, s)) continue;
        cfloat row[7];
        const cfloat3 cr = cross(s, n);  // ICP.cu:257-259 (fill_row here changed 296 lines of k_icp<POSE_ARGS, 4, 2>)
        row[0] = cr.x; row[1] = cr.y; row[2] = cr.z;
        row[3] = n.x; row[4] = n.y; row[5] = n.z;
        row[6] = dot(n, d - s);
        int shift = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 7; ++j) {
                const cfloat p = row[i] * row[j];
                acc[2 * shift] += (double)p.re;
                acc[2 * shift + 1] += (double)p.im;
                ++shift;
            }
        cnt += 1.0;
    }
    // ---- phase: fold to smem, four-wave register form ----
    // Fold the 256 lanes of the workgroup: every lane parks its 55 values (54 sums + count) in an
    // LDS tile [wave][value][lane] (rows padded to 65 doubles: conflict-free both ways), then four
    // threads per value each add one wave's 64 entries in lane order and the four results are
    // added in wave order — fixed association, no cross-lane shuffles (55 dependent 6-step
    // ds_bpermute chains cost ~20 us here).  Two passes of 28 values keep the tile at 58 KB.
    double (*tile)[28][65] = reinterpret_cast<double (*)[28][65]>(lds_tile);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (half) __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 28; ++kk) {
            const int k = half * 28 + kk;
            if (k < NS) tile[wave][kk][lane] = acc[k];
            else if (k == NS) tile[wave][kk][lane] = cnt;
        }
        __syncthreads();
        const int kk = threadIdx.x >> 2, q = threadIdx.x & 3;
        if (kk < 28 && half * 28 + kk <= NS) {
            double sacc = 0.0;
#pragma unroll 8
            for (int i = 0; i < 64; ++i) sacc += tile[q][kk][i];
            smem[q][half * 28 + kk] = sacc;
        }
    }
    } else {
    // ---- phase: pixels, one tile per wave, or two tiles in lock step ----
    // one tile per wave: the row's 27 complex products (complex<f32>, ICP.cu:273) go to the LDS tile as they are formed —
    // floats, one row per (wave, value), in one, two or three passes — and are added in double, lane order then wave order, as above
    cfloat row[7];
    float one = 0.0f;
    cfloat row2[BAL ? 7 : 1];
    float one2 = 0.0f;
    if constexpr (BAL) {
        // both tiles of waves 0 and 1 in lock step (search_issue / search_finish, xs_icp_search.h); the other waves' single tile the same way
        SearchStage sa, sb;
        search_issue(a, Rcurr, tcurr, pre_x, pre_y, pre_v, sa);
        const bool two = wave < EXTRA;   // (wave-uniform)
        if (two) search_issue(a, Rcurr, tcurr, pre_x2, pre_y2, pre_v2, sb);
        cfloat3 n, d, s;
#pragma unroll
        for (int i = 0; i < 7; ++i) { row[i] = cfloat(0.0f, 0.0f); row2[i] = cfloat(0.0f, 0.0f); }   // ICP.cu:262: a rejected pixel contributes zeros
        if (pre_ok && search_finish(a, Rcurr, sa, n, d, s)) { fill_row(row, n, d, s); one = 1.0f; }
        if (two && pre_ok2 && search_finish(a, Rcurr, sb, n, d, s)) { fill_row(row2, n, d, s); one2 = 1.0f; }   // a workgroup with nine tiles leaves wave 1's second slot all zeros
    } else {
        bool ok = false;
        cfloat3 n, d, s;
#ifdef XS_ICP_NO_PREFETCH
        load_vertex(a, pre_x, pre_y, pre_v);
#endif
        if (pre_ok) ok = search_vertex_loaded(a, Rcurr, tcurr, pre_x, pre_y, pre_v, n, d, s);
        if (ok) {
            fill_row(row, n, d, s);
            one = 1.0f;
        } else {
#pragma unroll
            for (int i = 0; i < 7; ++i) row[i] = cfloat(0.0f, 0.0f);   // ICP.cu:262: a rejected pixel contributes zeros
        }
    }
    XS_STAMP(2);
    // ---- phase: fold to smem, tile form ----
    // Rows of 64 floats, one per (wave, value), 68 floats apart: 16-byte aligned with an odd number of 16-byte chunks between
    // rows, so the wave's row-wise stores and the adders' 128-bit loads (eight consecutive lanes = eight consecutive rows, or
    // four rows x two halves) are both free of bank conflicts.  A row is added by two lanes, 32 entries each, when the
    // workgroup has the threads for it (two or three passes), by one otherwise.
    constexpr int SPLIT = 16 * PV <= 512 ? 2 : 1;   // (the balanced instance's 280 rows: a few lanes take a second one)
    float *tile = reinterpret_cast<float *>(lds_tile);
#pragma unroll
    for (int pass = 0; pass < PASSES; ++pass) {
        if (pass) __syncthreads();
        int shift = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 7; ++j) {
                const int kre = 2 * shift, kim = 2 * shift + 1;
                if (kre / PV == pass || kim / PV == pass) {
                    const cfloat p = row[i] * row[j];
                    if (kre / PV == pass) tile[(wave * PV + kre % PV) * RS + lane] = p.re;
                    if (kim / PV == pass) tile[(wave * PV + kim % PV) * RS + lane] = p.im;
                    if constexpr (BAL) {
                        if (wave < EXTRA) {
                            const cfloat p2 = row2[i] * row2[j];
                            if (kre / PV == pass) tile[((WAVES + wave) * PV + kre % PV) * RS + lane] = p2.re;
                            if (kim / PV == pass) tile[((WAVES + wave) * PV + kim % PV) * RS + lane] = p2.im;
                        }
                    }
                }
                ++shift;
            }
        if (pass == NS / PV) {
            tile[(wave * PV + NS % PV) * RS + lane] = one;
            if constexpr (BAL) { if (wave < EXTRA) tile[((WAVES + wave) * PV + NS % PV) * RS + lane] = one2; }
        }
        XS_STAMP(11 + 2 * (pass & 1));   // (trace build: this wave's products of the pass are on their way to LDS)
        __syncthreads();
        const int h = threadIdx.x % SPLIT;
#pragma unroll
        for (int r = threadIdx.x / SPLIT; r < SLOTS * PV; r += (64 * WAVES) / SPLIT) {
            // four interleaved partial sums (entries i, i + 4, ... each) per lane; with two lanes per row the halves are added
            // partial by partial, then ((s0 + s1) + (s2 + s3)): the same fixed association every launch.  The second lane
            // walks its eight chunks starting from the fifth, which keeps the pair on different banks.
            // (the float4 -> four doubles loop stands three times: as one function it changed 18 to 107 lines of the fifteen tile instances)
            const float4 *p = reinterpret_cast<const float4 *>(tile + r * RS);
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            if constexpr (SPLIT == 1) {
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const float4 f = p[c];
                    s0 += (double)f.x; s1 += (double)f.y; s2 += (double)f.z; s3 += (double)f.w;
                }
            } else {
                const float4 *pa = p + 12 * h, *pb = p + 4 + 4 * h;   // lane 0: chunks 0-3 then 4-7; lane 1: 12-15 then 8-11
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float4 f = pa[c];
                    s0 += (double)f.x; s1 += (double)f.y; s2 += (double)f.z; s3 += (double)f.w;
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float4 f = pb[c];
                    s0 += (double)f.x; s1 += (double)f.y; s2 += (double)f.z; s3 += (double)f.w;
                }
                s0 += pair_swap(s0); s1 += pair_swap(s1); s2 += pair_swap(s2); s3 += pair_swap(s3);
            }
            const int w = r / PV, v = r % PV;
            if (h == 0 && pass * PV + v <= NS) smem[w][pass * PV + v] = (s0 + s1) + (s2 + s3);
        }
        XS_STAMP(12 + 2 * (pass & 1));   // (trace build: this wave's rows of the pass are added)
    }
    }
    __syncthreads();
    XS_STAMP(3);
    // ---- phase: publish the record — to the host, or write-through plus ticket ----
    if (a.host_records) {
        publish_host_record<SLOTS>(a, smem);
        return;
    }
    if (threadIdx.x < NP / 2) {
        // The record: 28 lanes of wave 0 store two doubles each (the pad entry is written as zero) with agent-scope
        // write-through stores — they go through this XCD's L2 to memory on their own, so nothing is left for a write-back of
        // the whole L2 (what an agent-scope release fence does here: 0.6 us when one workgroup does it, up to 3 us when
        // six hundred do).  (Stands here: as a function beside publish_host_record, take_ticket and sum_row_groups — any three of
        // the four hold, all four changed 2 lines of the three k_icp<., 8, 1> instances.)
        const int k0 = 2 * threadIdx.x, k1 = k0 + 1;
        double *rec = a.partials + (size_t)blockIdx.x * NP;
        const d2 v = wave_order_sum2<SLOTS>(smem, k0);
        __hip_atomic_store(rec + k0, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(rec + k1, k1 <= NS ? v.y : 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (the pad column of smem is never written)
    }
    __shared__ unsigned s_last;
    take_ticket(a, s_last);
    __syncthreads();
    if (s_last) {
        // ---- phase: the last workgroup's gather and output ----
        // after the acquire (this CU's L1 invalidated) + barrier, plain loads see every record.  The records
        // come from memory (other XCDs wrote them), so the sum is latency-bound: a record is 28 16-byte
        // chunks; thread (g, q) adds chunk q of records g, g+9, g+18, ... in that order with 32 loads in
        // flight, and the row groups are then added in group order — a fixed association, so
        // deterministic — leaving two or three memory round trips where a plain loop had sixteen.  (Level 0's 600 records
        // are 269 KB through one CU's 64 B / clk: ~1.8 us of the 3.4 us this takes is that, whatever the depth.)
        // (eight waves: twice the threads, so eighteen row groups with sixteen loads each in flight — the same bytes in
        // flight per workgroup at half the registers per lane, which is what lets this instance run at four waves per SIMD)
        constexpr int G = WAVES == 16 ? 36 : (WAVES == 8 ? 18 : 9), DEPTH = WAVES == 16 ? 8 : (WAVES == 8 ? 16 : 32);
        static_assert(TILE_BYTES >= G * 28 * 16, "row-group sums live in the fold's tile");
        d2 (*s_red)[28] = reinterpret_cast<d2 (*)[28]>(lds_tile);   // every wave is past the fold (barriers above)
        const int q = threadIdx.x % 28, g = threadIdx.x / 28;
        if (g < G) {
            const d2 *p = reinterpret_cast<const d2 *>(a.partials) + q;
            d2 acc2 = {0.0, 0.0};
            unsigned b = g;
            const unsigned nb = gridDim.x;
            for (; b + G * (DEPTH - 1) < nb; b += G * DEPTH) {
                d2 v[DEPTH];
#pragma unroll
                for (int k = 0; k < DEPTH; ++k) v[k] = p[(size_t)(b + G * k) * (NP / 2)];
#pragma unroll
                for (int k = 0; k < DEPTH; ++k) { acc2.x += v[k].x; acc2.y += v[k].y; }
            }
            {   // the tail, still issued together
                d2 v[DEPTH];
#pragma unroll
                for (int k = 0; k < DEPTH; ++k) {
                    const unsigned bb = b + G * k;
                    v[k] = bb < nb ? p[(size_t)bb * (NP / 2)] : d2{0.0, 0.0};
                }
#pragma unroll
                for (int k = 0; k < DEPTH; ++k)
                    if (b + G * k < nb) { acc2.x += v[k].x; acc2.y += v[k].y; }
            }
            s_red[g][q] = acc2;
        }
        __syncthreads();
        XS_STAMP(8);
        if (threadIdx.x < 28) sum_row_groups<G>(s_red, [&](d2 t) { store_sums(a, t); });
        if (a.done_flag) {
            // out (and the flag) may live in host-coherent pinned memory: push the sums out, then
            // publish the sequence number the host is spinning on — no copy, no stream sync
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (threadIdx.x == 0) publish_done(a);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        XS_STAMP(9);
    }
}

// ---- pose update on the device (xs_icp_iterate) ---------------------------------------------
// KinectFusionReconstruction.cpp:203-224 as a one-workgroup kernel behind the reduction: wave 1 takes
// the determinant gate while wave 0 factors and solves (one matrix row per lane); three lanes then
// evaluate the three angles' sin / cos side by side and form one row each of Rinc, Rinc*tcurr + tinc
// and Rinc*Rcurr.  It lives in its own kernel because the double-precision solve wants ~100 registers
// of its own: inside k_icp it cost the pixel loop its second wave per SIMD.
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, 1))) k_icp_solve(const IcpSolveArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (!a.load_pose && a.pose->status != 0) {  // the loop ended at an earlier iteration
        if (threadIdx.x == 0 && a.done_flag) {
            __threadfence_system();
            __hip_atomic_store(a.done_flag, a.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    __shared__ double s_sums[NP];
    __shared__ double s_det;
    __shared__ cfloat s_res[6], s_sn[3], s_cs[3];
    if (threadIdx.x < NS + 1) {
        const double v = a.sums[threadIdx.x];
        s_sums[threadIdx.x] = v;
        if (a.sums_host) a.sums_host[threadIdx.x] = v;
    }
    __syncthreads();
    if (wave == 1) {
        const double det = icp_solve::real_determinant6_wave(s_sums, lane);
        if (lane == 0) s_det = det;
    } else {
        const cdouble sol = icp_solve::llt_solve6_wave(s_sums, lane);
        if (lane < 6) s_res[lane] = cfloat((float)sol.re, (float)sol.im);
        // (same wave: the three angles are in LDS once its writes have landed)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (lane < 3) icp_solve::csincos(s_res[lane], s_sn[lane], s_cs[lane]);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int i = threadIdx.x;
        MatS33 Rcurr = a.Rcurr;
        cfloat3 tcurr = a.tcurr;
        int iters = 1;
        if (!a.load_pose) {
            const cfloat *pr = reinterpret_cast<const cfloat *>(a.pose->R), *pt = reinterpret_cast<const cfloat *>(a.pose->t);
#pragma unroll
            for (int r = 0; r < 3; ++r) { Rcurr.data[r].x = pr[3 * r]; Rcurr.data[r].y = pr[3 * r + 1]; Rcurr.data[r].z = pr[3 * r + 2]; }
            tcurr.x = pt[0]; tcurr.y = pt[1]; tcurr.z = pt[2];
            iters = a.pose->iters + 1;
        }
        const double det = s_det;
        const int status = (det != det) ? 2 : (fabs(det) < 1e-15 ? 1 : 0);
        icp_solve::Row3 Rn;
        cfloat tn;
        if (status == 0) icp_solve::compose_pose_rows(i, s_res, s_sn, s_cs, Rcurr, tcurr, Rn, tn);
        else {  // the pose stays where it was
            const cfloat3 r = i == 0 ? Rcurr.data[0] : (i == 1 ? Rcurr.data[1] : Rcurr.data[2]);
            Rn.v[0] = r.x; Rn.v[1] = r.y; Rn.v[2] = r.z;
            tn = i == 0 ? tcurr.x : (i == 1 ? tcurr.y : tcurr.z);
        }
        // every lane has read the old pose by now (same wave, program order), so it can be overwritten
        __builtin_amdgcn_wave_barrier();
        IcpPoseState *dst[2] = {a.pose, a.pose_host};
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            IcpPoseState *ps = dst[d];
            if (!ps) continue;
#pragma unroll
            for (int j = 0; j < 3; ++j) { ps->R[6 * i + 2 * j] = Rn.v[j].re; ps->R[6 * i + 2 * j + 1] = Rn.v[j].im; }
            ps->t[2 * i] = tn.re; ps->t[2 * i + 1] = tn.im;
            if (i == 0) { ps->status = status; ps->iters = iters; ps->det = det; }
        }
    }
    if (a.done_flag) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence_system();
            __hip_atomic_store(a.done_flag, a.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ---- launching (xs_icp_launch.h: the instances, the request, its validation) ----
template <int POSE_SRC>
static void icp_dispatch(const IcpGrid &g, hipStream_t st, const IcpArgs &a) {
    switch (g.instance) {
    case IcpInstance::W8_BAL: hipLaunchKernelGGL((k_icp<POSE_SRC, 8, 2, true>), dim3(g.blocks), dim3(512), 0, st, a); break;
    case IcpInstance::W16_BAL: hipLaunchKernelGGL((k_icp<POSE_SRC, 16, 2, true>), dim3(g.blocks), dim3(1024), 0, st, a); break;
    case IcpInstance::W8_P1: hipLaunchKernelGGL((k_icp<POSE_SRC, 8, 1>), dim3(g.blocks), dim3(512), 0, st, a); break;
    case IcpInstance::W8_P2: hipLaunchKernelGGL((k_icp<POSE_SRC, 8, 2>), dim3(g.blocks), dim3(512), 0, st, a); break;
    case IcpInstance::W8_P3: hipLaunchKernelGGL((k_icp<POSE_SRC, 8, 3>), dim3(g.blocks), dim3(512), 0, st, a); break;
    case IcpInstance::W4_P2: hipLaunchKernelGGL((k_icp<POSE_SRC, 4, 2>), dim3(g.blocks), dim3(256), 0, st, a); break;
    }
}

// Enqueue a plan: the reduction and, for xs_icp_iterate, the one-workgroup solve behind it.  No synchronisation.
static int icp_enqueue(const IcpPlan &p, hipStream_t st) {
    if (p.pose_src == POSE_DEVICE) icp_dispatch<POSE_DEVICE>(p.grid, st, p.a);
    else if (p.pose_src == POSE_POSTED) icp_dispatch<POSE_POSTED>(p.grid, st, p.a);
    else icp_dispatch<POSE_ARGS>(p.grid, st, p.a);
    if (p.solve) hipLaunchKernelGGL(k_icp_solve, dim3(1), dim3(128), 0, st, p.sa);
    XS_CHECK(hipGetLastError());
    return 0;
}
// what every launching entry point ends in
static int icp_launch(const IcpLaunch &l) {
    IcpPlan p;
    if (const int rc = icp_plan(l, p)) return rc;
    return icp_enqueue(p, (hipStream_t)l.stream);
}

// ---- C ABI: the entry points that launch ----------------------------------------------------------------------------------------------
extern "C" size_t xs_icp_workspace_bytes(void) { return (size_t)XS_ICP_MAX_BLOCKS * NP * sizeof(double) + 256; }
/* zero the arrival ticket once after allocating the workspace (launches re-arm it themselves) */
extern "C" int xs_icp_workspace_init(void *workspace, void *stream) {
    if (!workspace) return xs_set_error(hipErrorInvalidValue, "xs_icp_workspace_init: null pointer");
    XS_CHECK(hipMemsetAsync(workspace, 0, 256, (hipStream_t)stream));
    return 0;
}

/* estimateCombined(const MatS33& Rcurr, const devComplex3& tcurr, const MapArr& vmap_curr,
 *     const MapArr& nmap_curr, const MatS33& Rprev_inv, const devComplex3& tprev, const Intr&,
 *     const MapArr& vmap_g_prev, const MapArr& nmap_g_prev, float distThres, float angleThres,
 *     DeviceArray2D<devComplexICP>& gbuf, DeviceArray<devComplexICP>& mbuf,
 *     hostComplexICP* A, hostComplexICP* b)                 ICP.h:24-31, ICP.cu:365-429
 * Device half: enqueue the reduction; sums_dev receives 55 doubles = the 27 complex<double>
 * sums in the reference's mbuf order (ICP.cu:266-280) followed by the inlier count.
 * workspace: xs_icp_workspace_bytes() bytes of device memory (replaces gbuf).  [y0, y1): pixel
 * rows covered (0, rows for one GPU).  done_flag (optional, with sums_dev in host-coherent pinned
 * memory): after the sums are written the kernel stores done_seq there with system-scope release,
 * so a host thread can spin on it instead of copying and synchronising.  No synchronisation. */
extern "C" int xs_icp_accumulate(const float *Rcurr18, const float *tcurr6, const float *vmap_curr, const float *nmap_curr,
                                 const float *Rprev_inv18, const float *tprev6, const float *intr4, const float *vmap_g_prev,
                                 const float *nmap_g_prev, size_t map_step, int rows, int cols, float distThres, float angleThres,
                                 int y0, int y1, void *workspace, double *sums_dev, unsigned long long *done_flag,
                                 unsigned long long done_seq, void *stream) {
    if (!Rcurr18 || !tcurr6) return xs_set_error(hipErrorInvalidValue, "xs_icp_accumulate: null pointer");
    IcpLaunch l;
    l.who = "xs_icp_accumulate: null pointer";
    l.Rcurr18 = Rcurr18; l.tcurr6 = tcurr6;
    l.vmap_curr = vmap_curr; l.nmap_curr = nmap_curr; l.Rprev_inv18 = Rprev_inv18; l.tprev6 = tprev6; l.intr4 = intr4;
    l.vmap_g_prev = vmap_g_prev; l.nmap_g_prev = nmap_g_prev; l.map_step = map_step; l.rows = rows; l.cols = cols; l.distThres = distThres; l.angleThres = angleThres;
    l.y0 = y0; l.y1 = y1; l.workspace = workspace; l.sums_dev = sums_dev; l.done_flag = done_flag; l.done_seq = done_seq; l.stream = stream;
    return icp_launch(l);
}

/* xs_icp_accumulate with the current-frame maps' real parts given as float planes too (xs_create_vnmaps_real: 3 x rows rows of
 * cols floats, pitch real_step bytes): the kernel reads those instead of vmap_curr / nmap_curr — whose imaginary parts must be
 * zeros, as they are for maps made from a real depth image — and forms (value, 0).  Same sums (an imaginary part that was -0 in the
 * complex map is +0 here).  vmap_curr / nmap_curr may be NULL when the planes are given. */
extern "C" int xs_icp_accumulate_real(const float *Rcurr18, const float *tcurr6, const float *vmap_curr, const float *nmap_curr,
                                      const float *vmap_curr_real, const float *nmap_curr_real, size_t real_step, const float *Rprev_inv18,
                                      const float *tprev6, const float *intr4, const float *vmap_g_prev, const float *nmap_g_prev, size_t map_step,
                                      int rows, int cols, float distThres, float angleThres, int y0, int y1, void *workspace, double *sums_dev,
                                      unsigned long long *done_flag, unsigned long long done_seq, void *stream) {
    if (!Rcurr18 || !tcurr6) return xs_set_error(hipErrorInvalidValue, "xs_icp_accumulate_real: null pointer");
    IcpLaunch l;
    l.who = "xs_icp_accumulate_real: null pointer";
    l.Rcurr18 = Rcurr18; l.tcurr6 = tcurr6;
    l.vmap_curr = vmap_curr; l.nmap_curr = nmap_curr; l.Rprev_inv18 = Rprev_inv18; l.tprev6 = tprev6; l.intr4 = intr4;
    l.vmap_g_prev = vmap_g_prev; l.nmap_g_prev = nmap_g_prev; l.map_step = map_step; l.rows = rows; l.cols = cols; l.distThres = distThres; l.angleThres = angleThres;
    if (const int rc = icp_real_planes(l, vmap_curr_real, nmap_curr_real, real_step, "xs_icp_accumulate_real: real planes")) return rc;
    l.y0 = y0; l.y1 = y1; l.workspace = workspace; l.sums_dev = sums_dev; l.done_flag = done_flag; l.done_seq = done_seq; l.stream = stream;
    return icp_launch(l);
}

/* estimateCombined with the pose posted after the launch.  The launch is enqueued while the previous
 * iteration is still running; its workgroups become resident, poll `mailbox` (xs_icp_mailbox_bytes()
 * bytes of host-coherent pinned memory, zero before first use) and start on the pixels as soon as
 * xs_icp_post_pose has written Rcurr / tcurr with sequence number mailbox_seq — what is left of an
 * iteration's turnaround is the host's solve and one PCIe read instead of a kernel launch.
 * xs_icp_post_pose(..., cmd = 1) makes the launch return without touching anything (the host left
 * the loop: singular system).  A launch whose pose never arrives gives up after about a second and
 * stores done_seq | 1<<63 to done_flag; re-initialise the workspace (xs_icp_workspace_init) after that.
 * Everything else as xs_icp_accumulate. */
extern "C" int xs_icp_accumulate_posted(const void *mailbox, unsigned mailbox_seq, const float *vmap_curr, const float *nmap_curr,
                                        const float *Rprev_inv18, const float *tprev6, const float *intr4, const float *vmap_g_prev,
                                        const float *nmap_g_prev, size_t map_step, int rows, int cols, float distThres, float angleThres,
                                        int y0, int y1, void *workspace, double *sums_dev, unsigned long long *done_flag,
                                        unsigned long long done_seq, void *stream) {
    if (!mailbox) return xs_set_error(hipErrorInvalidValue, "xs_icp_accumulate_posted: null pointer");
    IcpLaunch l;
    l.who = "xs_icp_accumulate_posted: null pointer";
    l.mailbox = mailbox; l.mailbox_seq = mailbox_seq;
    l.vmap_curr = vmap_curr; l.nmap_curr = nmap_curr; l.Rprev_inv18 = Rprev_inv18; l.tprev6 = tprev6; l.intr4 = intr4;
    l.vmap_g_prev = vmap_g_prev; l.nmap_g_prev = nmap_g_prev; l.map_step = map_step; l.rows = rows; l.cols = cols; l.distThres = distThres; l.angleThres = angleThres;
    l.y0 = y0; l.y1 = y1; l.workspace = workspace; l.sums_dev = sums_dev; l.done_flag = done_flag; l.done_seq = done_seq; l.stream = stream;
    return icp_launch(l);
}
/* xs_icp_accumulate_posted with the real planes of xs_icp_accumulate_real */
extern "C" int xs_icp_accumulate_posted_real(const void *mailbox, unsigned mailbox_seq, const float *vmap_curr, const float *nmap_curr,
                                             const float *vmap_curr_real, const float *nmap_curr_real, size_t real_step, const float *Rprev_inv18,
                                             const float *tprev6, const float *intr4, const float *vmap_g_prev, const float *nmap_g_prev,
                                             size_t map_step, int rows, int cols, float distThres, float angleThres, int y0, int y1, void *workspace,
                                             double *sums_dev, unsigned long long *done_flag, unsigned long long done_seq, void *stream) {
    if (!mailbox) return xs_set_error(hipErrorInvalidValue, "xs_icp_accumulate_posted_real: null pointer");
    IcpLaunch l;
    l.who = "xs_icp_accumulate_posted_real: null pointer";
    l.mailbox = mailbox; l.mailbox_seq = mailbox_seq;
    l.vmap_curr = vmap_curr; l.nmap_curr = nmap_curr; l.Rprev_inv18 = Rprev_inv18; l.tprev6 = tprev6; l.intr4 = intr4;
    l.vmap_g_prev = vmap_g_prev; l.nmap_g_prev = nmap_g_prev; l.map_step = map_step; l.rows = rows; l.cols = cols; l.distThres = distThres; l.angleThres = angleThres;
    if (const int rc = icp_real_planes(l, vmap_curr_real, nmap_curr_real, real_step, "xs_icp_accumulate_posted_real: real planes")) return rc;
    l.y0 = y0; l.y1 = y1; l.workspace = workspace; l.sums_dev = sums_dev; l.done_flag = done_flag; l.done_seq = done_seq; l.stream = stream;
    return icp_launch(l);
}

/* estimateCombined with the final addition on the host.  Same kernel and the same per-workgroup records as xs_icp_accumulate, but
 * every workgroup stores its record (56 doubles: 54 sums, inlier count, sequence word) straight into `records_host` — host-coherent
 * pinned memory of xs_icp_records_bytes() bytes — and leaves; the sequence word is written last (system-scope release).  Nothing is
 * gathered on the device: the launch has no ticket, no second pass over the records and no completion word.  The host adds the records
 * with xs_icp_sum_records, which waits for each record's sequence word in index order.  Pose: Rcurr18 / tcurr6, or both NULL with a
 * mailbox (as xs_icp_accumulate_posted).  seq: non-zero, different from the previous launch's on the same buffer. */
extern "C" size_t xs_icp_records_bytes(void) { return (size_t)XS_ICP_MAX_BLOCKS * NP * sizeof(double); }
extern "C" int xs_icp_records_count(int cols, int y0, int y1) { return icp_blocks(cols, y0, y1).blocks; }
extern "C" int xs_icp_accumulate_records(const float *Rcurr18, const float *tcurr6, const void *mailbox, unsigned mailbox_seq, const float *vmap_curr,
                                         const float *nmap_curr, const float *Rprev_inv18, const float *tprev6, const float *intr4,
                                         const float *vmap_g_prev, const float *nmap_g_prev, size_t map_step, int rows, int cols, float distThres,
                                         float angleThres, int y0, int y1, double *records_host, unsigned long long seq, void *stream) {
    if (!records_host || seq == 0 || (seq >> 63)) return xs_set_error(hipErrorInvalidValue, "xs_icp_accumulate_records: bad records / seq");
    if ((Rcurr18 == nullptr) != (tcurr6 == nullptr) || (!Rcurr18 && !mailbox))
        return xs_set_error(hipErrorInvalidValue, "xs_icp_accumulate_records: give a pose or a mailbox");
    IcpLaunch l;
    l.who = "xs_icp_accumulate_records: null pointer";
    l.Rcurr18 = Rcurr18; l.tcurr6 = tcurr6;
    if (!Rcurr18) { l.mailbox = mailbox; l.mailbox_seq = mailbox_seq; }
    l.vmap_curr = vmap_curr; l.nmap_curr = nmap_curr; l.Rprev_inv18 = Rprev_inv18; l.tprev6 = tprev6; l.intr4 = intr4;
    l.vmap_g_prev = vmap_g_prev; l.nmap_g_prev = nmap_g_prev; l.map_step = map_step; l.rows = rows; l.cols = cols; l.distThres = distThres; l.angleThres = angleThres;
    l.y0 = y0; l.y1 = y1; l.host_records = records_host; l.record_seq = seq; l.stream = stream;
    return icp_launch(l);
}

/* One whole ICP iteration on the device: estimateCombined (ICP.cu:365-429) followed by the pose
 * update the reference's host performs before the next launch (KinectFusionReconstruction.cpp:203-224:
 * determinant gate, complex<double> LLT solve, cast to complex<float>, AngleAxis Z*Y*X, Rcurr / tcurr
 * composition).  pose_state: xs_icp_pose_state_bytes() bytes of device memory holding
 * {float R[18]; float t[6]; int status; int iters; double det; double pad[2]} (128 bytes); when Rcurr18 / tcurr6 are
 * given the launch starts from them (first iteration of a frame) and otherwise from the state the
 * previous launch on the stream left.  status: 0 ok, 1 |det| < 1e-15, 2 NaN; once non-zero the
 * following launches return at once (the reference leaves PoseEstimate there).  sums_dev: device
 * memory, as in xs_icp_accumulate; sums_host / pose_state_host (optional, host-coherent pinned
 * memory) receive a copy of the 55 sums and of the state after every solve, then done_seq is
 * published to done_flag (optional).  Two launches (reduction, one-workgroup solve); no synchronisation. */
extern "C" size_t xs_icp_pose_state_bytes(void) { return sizeof(IcpPoseState); }
extern "C" int xs_icp_iterate(const float *Rcurr18, const float *tcurr6, const float *vmap_curr, const float *nmap_curr,
                              const float *Rprev_inv18, const float *tprev6, const float *intr4, const float *vmap_g_prev,
                              const float *nmap_g_prev, size_t map_step, int rows, int cols, float distThres, float angleThres,
                              void *workspace, double *sums_dev, double *sums_host, void *pose_state, void *pose_state_host,
                              unsigned long long *done_flag, unsigned long long done_seq, void *stream) {
    if (!pose_state || ((Rcurr18 == nullptr) != (tcurr6 == nullptr))) return xs_set_error(hipErrorInvalidValue, "xs_icp_iterate: null pointer");
    IcpLaunch l;
    l.who = "xs_icp_iterate: null pointer";
    l.Rcurr18 = Rcurr18; l.tcurr6 = tcurr6;
    l.pose = (IcpPoseState *)pose_state; l.pose_host = (IcpPoseState *)pose_state_host; l.sums_host = sums_host;
    l.vmap_curr = vmap_curr; l.nmap_curr = nmap_curr; l.Rprev_inv18 = Rprev_inv18; l.tprev6 = tprev6; l.intr4 = intr4;
    l.vmap_g_prev = vmap_g_prev; l.nmap_g_prev = nmap_g_prev; l.map_step = map_step; l.rows = rows; l.cols = cols; l.distThres = distThres; l.angleThres = angleThres;
    l.y0 = 0; l.y1 = rows; l.workspace = workspace; l.sums_dev = sums_dev; l.done_flag = done_flag; l.done_seq = done_seq; l.stream = stream;
    return icp_launch(l);
}
