// xs_score_fold.h — how a scoring launch over tiles of 64 hypotheses ends, stated once for k_align_score (xs_align.hip: map-to-map transforms over
// a band index) and k_register_score (xs_register.hip: transforms of a point cloud, section 4.32).  Both kernels run a
// grid of (nblocks, tiles) workgroups of four waves; lane l of every wave holds, for hypothesis 64 tile + l, a double sum and an unsigned count
// over the chunks that wave met.  From there: the four waves in wave order, one record of 64 doubles + 64 counts per workgroup, an arrival
// ticket per tile, and the tile's last workgroup adds the records in index order and writes {sum, count} per hypothesis.  Every step's order is a
// function of nblocks alone.
#pragma once
#include "xs_device.h"

namespace xs {

enum { SCORE_TILE = 64, SCORE_MAX_BLOCKS = 1024, SCORE_RECORD_BYTES = SCORE_TILE * (sizeof(double) + sizeof(unsigned)) };

// acc, cnt: this lane's sum and count for hypothesis p0 + lane of tile blockIdx.y (np of the tile's 64 exist: the other lanes hold zeros).
// records: [tiles][nblocks]{64 doubles, 64 unsigned}; tickets: [tiles], zero between launches; out: [hypotheses][2].  Called by every thread of
// the workgroup (it holds barriers).
__device__ __forceinline__ void score_tile_fold_and_finish(double acc, unsigned cnt, char *records, unsigned *tickets, double *out, int p0, int np) {
    __shared__ double s_sum[4][SCORE_TILE];
    __shared__ unsigned s_cnt[4][SCORE_TILE];
    __shared__ unsigned s_last;
    const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(threadIdx.y), tid = wave * 64 + lane;
    const unsigned nblocks = gridDim.x, bid = blockIdx.x, tile = blockIdx.y;
    // the four waves in wave order, then one record per workgroup: hypothesis lane's sum and count, stored by the lanes of wave 0
    s_sum[wave][lane] = acc;
    s_cnt[wave][lane] = cnt;
    __syncthreads();
    char *tile_records = records + (size_t)tile * nblocks * SCORE_RECORD_BYTES;
    if (tid < SCORE_TILE) {
        const double s = ((s_sum[0][tid] + s_sum[1][tid]) + s_sum[2][tid]) + s_sum[3][tid];
        const unsigned n = ((s_cnt[0][tid] + s_cnt[1][tid]) + s_cnt[2][tid]) + s_cnt[3][tid];
        char *rec = tile_records + (size_t)bid * SCORE_RECORD_BYTES;
        __hip_atomic_store(reinterpret_cast<double *>(rec) + tid, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(reinterpret_cast<unsigned *>(rec + SCORE_TILE * sizeof(double)) + tid, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // the hand-off of block_fold_and_finish_of (xs_gn_band.h): write-through record stores by wave 0, acknowledged, then its first lane's ticket
    if (wave == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) {
        const unsigned tk = __hip_atomic_fetch_add(tickets + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = tk == nblocks - 1 ? 1u : 0u;
        if (s_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (!s_last) return;
    // the tile's last workgroup: thread (q, l) adds hypothesis l's records q, q + 4, ... in that order, eight loads in flight; the four row
    // groups are then added in group order
    {
        const int l = tid % SCORE_TILE, q = tid / SCORE_TILE;
        double s = 0.0;
        unsigned long long n = 0;
        auto rsum = [&](unsigned b) { return reinterpret_cast<const double *>(tile_records + (size_t)b * SCORE_RECORD_BYTES)[l]; };
        auto rcnt = [&](unsigned b) { return reinterpret_cast<const unsigned *>(tile_records + (size_t)b * SCORE_RECORD_BYTES + SCORE_TILE * sizeof(double))[l]; };
        unsigned b = q;
        for (; b + 4 * 7 < nblocks; b += 4 * 8) {
            double v[8]; unsigned m[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { v[k] = rsum(b + 4 * k); m[k] = rcnt(b + 4 * k); }
#pragma unroll
            for (int k = 0; k < 8; ++k) { s += v[k]; n += m[k]; }
        }
        for (; b < nblocks; b += 4) { s += rsum(b); n += rcnt(b); }
        __shared__ unsigned long long s_n[4][SCORE_TILE];
        s_sum[q][l] = s;   // (wave 0 read its workgroup's own sums before the ticket's barrier)
        s_n[q][l] = n;
        __syncthreads();
        if (tid < np) {
            out[2 * (size_t)(p0 + tid)] = ((s_sum[0][tid] + s_sum[1][tid]) + s_sum[2][tid]) + s_sum[3][tid];
            out[2 * (size_t)(p0 + tid) + 1] = (double)(((s_n[0][tid] + s_n[1][tid]) + s_n[2][tid]) + s_n[3][tid]);
        }
        // the ticket goes back to zero for the next launch on this workspace (xs_tsdf_reduce_workspace_init zeroes it once)
        if (tid == 0) __hip_atomic_store(tickets + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace xs
