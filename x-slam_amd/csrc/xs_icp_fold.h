// xs_icp_fold.h — the pieces of the ICP reduction's additions (k_icp, xs_icp.hip) that are functions of their own: the lane-pair swap, the
// 16-byte pair of doubles, the sum of a workgroup's tile slots in wave order, and the last workgroup's batched sum of its row groups.  Each
// keeps one fixed association.  The workgroup fold (both forms) and the gather of the records stand in k_icp's body: as functions they
// changed the kernels' text (profiles/icp_split_kernels.txt).
#pragma once
#include "xs_icp_args.h"

// the value held by the neighbouring lane (lane ^ 1): two quad-permute moves, no LDS
__device__ __forceinline__ double pair_swap(double v) {
    const unsigned long long u = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_mov_dpp((int)(unsigned)u, 0xB1, 0xF, 0xF, true);          // quad_perm [1, 0, 3, 2]
    const int hi = __builtin_amdgcn_mov_dpp((int)(unsigned)(u >> 32), 0xB1, 0xF, 0xF, true);
    return __longlong_as_double(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// two neighbouring doubles moved as one 16-byte value (a record chunk, a pair of sums)
struct alignas(16) d2 { double x, y; };

// The per-wave partial sums of a workgroup, added in wave order — values k0 (even) and k0 + 1 together: one 16-byte LDS read per slot
// fetches both, the reads go out ten slots at a time before anything is added, and the two chains advance side by side.  (One value
// at a time this was two ladders of read -> wait -> add, 2 x 19 dependent steps on the sixteen-wave instance, with two or three reads
// in flight.)  The register tie after each batch keeps the next batch's reads behind it and both chains in step — without it the compiler
// sinks the y chain into the caller's guarded store and reads that half again, value by value; it never sits between the reads of a batch.
// smem rows are 448 bytes apart and 16-byte aligned.
template <int SLOTS>
__device__ __forceinline__ d2 wave_order_sum2(const double (*smem)[NP], int k0) {
    constexpr int BATCH = 10;
    const d2 *p = reinterpret_cast<const d2 *>(&smem[0][k0]);
    d2 t = {0.0, 0.0};
#pragma unroll
    for (int w0 = 0; w0 < SLOTS; w0 += BATCH) {
        d2 v[BATCH];
#pragma unroll
        for (int k = 0; k < BATCH; ++k)
            if (w0 + k < SLOTS) v[k] = p[(w0 + k) * (NP / 2)];
#pragma unroll
        for (int k = 0; k < BATCH; ++k)
            if (w0 + k < SLOTS) {
                if (w0 + k == 0) t = v[k];
                else { t.x += v[k].x; t.y += v[k].y; }
            }
        asm volatile("" : "+v"(t.x), "+v"(t.y));
    }
    return t;
}

// The last workgroup's G row-group sums of chunk threadIdx.x (one of the first 28 threads), added in group order and handed to `sink`.
// (A sink, not a return value: returning the pair, or writing it through a reference, changed 8 to 42 lines of every instance.)
template <int G, class Sink>
__device__ __forceinline__ void sum_row_groups(const d2 (*s_red)[28], Sink sink) {
    d2 t = s_red[0][threadIdx.x];
#ifdef XS_ICP_TAIL_BASELINE
#pragma unroll
    for (int gg = 1; gg < G; ++gg) { t.x += s_red[gg][threadIdx.x].x; t.y += s_red[gg][threadIdx.x].y; }
#else
    // The group sums are read nine at a time — all reads of a batch go out before its first addition — and added in group
    // order, both chains side by side.  Both chains are tied to registers after every batch: left alone the compiler sinks
    // the y chain into the guarded store below, keeps all G y values live across the x chain — 36 x 4 registers at sixteen
    // waves — and spills them: five dependent scratch reloads, 2-3.5 us at the very end of every level-0 launch
    // (profiles/r03_icp_phases.txt).  The tie used to follow every addition, and no LDS read moved across it: 35 round trips
    // of read -> wait -> add where four batches do (profiles/icp_tail_chain.txt).
    constexpr int BATCH = 9;
#pragma unroll
    for (int g0 = 1; g0 < G; g0 += BATCH) {
        d2 v[BATCH];
#pragma unroll
        for (int k = 0; k < BATCH; ++k)
            if (g0 + k < G) v[k] = s_red[g0 + k][threadIdx.x];
#pragma unroll
        for (int k = 0; k < BATCH; ++k)
            if (g0 + k < G) { t.x += v[k].x; t.y += v[k].y; }
        asm volatile("" : "+v"(t.x), "+v"(t.y));
    }
#endif
    sink(t);   // (store_sums, xs_icp.hip: the guarded store)
}
