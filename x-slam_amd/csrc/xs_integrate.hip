// xs_integrate.hip — TSDF volume kernels for gfx950: initialise, per-voxel complex integrate.
// Replaces XKinectFusion/src/TsdfFusion.cu:4-43 (initVolume), :85-201 (tsdfFusionKernal /
// integrateTsdfVolume).  Its parts: xs_integrate_voxel.h (the per-voxel contract), xs_integrate_stream.h
// (the streamed columns), xs_integrate_boxes.h and xs_integrate_classify.hip (what a brick is before
// a voxel is touched), xs_integrate_args.h (the host's argument builder); depth scaling is
// xs_scale_depth.hip, signed re-integration xs_reintegrate.hip.
//
// Volume layout (TsdfVolume.cpp:17-20): value f32, weight i32, grad f32, each a pitched 2-D
// array with rows = Y*Z and cols = X; voxel (x,y,z) at row (y + z*Y), column x.  A z-slab
// [z0, z1) owned by one GPU is the row range [z0*Y, z1*Y); the pointers passed here are the
// base of the slab's own storage and z runs over global indices.
//
// Integrate design (CDNA4).  A wave is 64 consecutive x of one (y, z-chunk): every load and
// store of value/weight/grad is a 256 B coalesced row segment.  A thread walks z.  The part
// of Rv2c*v_g that does not depend on z is formed once per thread in the reference's own
// operation order (x term + y term), so each z step adds one product and the translation —
// the same additions the reference performs, hence the same bits.  A voxel whose projection
// falls outside the image by more than one pixel is rejected on the un-divided coordinates
// (u*fx vs c*(bound)), before the two IEEE divides; anything within a pixel of the border
// takes the exact path.  Only voxels that pass the reference's predicate touch memory.
#include <hip/hip_ext.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include "xs_device.h"
#include "xs_env.h"
#include "xs_integrate_voxel.h"
#include "xs_integrate_boxes.h"
#include "xs_integrate_stream.h"
#include "xs_integrate_args.h"
#include "../../include/xslam_amd.h"

using namespace xs;

// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_init_volume(float *value, int *weight, float *grad, size_t step, int X, long long rows) {
    // one thread per 4 consecutive x of one row; rows = Y * (z1 - z0)
    int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    long long row = blockIdx.y;
    for (; row < rows; row += gridDim.y) {
        if (x4 + 3 < X && (step % 16) == 0) {
            float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(row_ptr(value, step, 0) + (size_t)row * (step / 4) + x4) = z4;
            *reinterpret_cast<int4 *>(row_ptr(weight, step, 0) + (size_t)row * (step / 4) + x4) = make_int4(0, 0, 0, 0);
            *reinterpret_cast<float4 *>(row_ptr(grad, step, 0) + (size_t)row * (step / 4) + x4) = z4;
        } else {
            for (int x = x4; x < X && x < x4 + 4; ++x) {
                ((float *)((char *)value + (size_t)row * step))[x] = 0.f;
                ((int *)((char *)weight + (size_t)row * step))[x] = 0;
                ((float *)((char *)grad + (size_t)row * step))[x] = 0.f;
            }
        }
    }
}

extern "C" int xs_init_volume(float *value, int *weight, float *grad, size_t step_bytes, const int *res, int z0, int z1, void *stream) {
    if (!value || !weight || !grad || !res || z1 < z0) return xs_set_error(hipErrorInvalidValue, "xs_init_volume: bad argument");
    long long rows = (long long)res[1] * (z1 - z0);
    if (rows == 0 || res[0] == 0) return 0;
    dim3 block(64, 1);
    dim3 grid(div_up(div_up(res[0], 4), 64), (unsigned)(rows < 65535 ? rows : 65535));
    hipLaunchKernelGGL(k_init_volume, grid, block, 0, (hipStream_t)stream, value, weight, grad, step_bytes, res[0], rows);
    XS_CHECK(hipGetLastError());
    return 0;
}

// One atomic per workgroup (a same-address atomic costs ~12 ns on this chip: one per wave of a
// few thousand bricks would serialise into tens of microseconds), spread over `nslots` words.
__device__ __forceinline__ void block_count_add(unsigned n_upd, unsigned long long *slots, unsigned nslots) {
    __shared__ unsigned s_cnt[4];
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    const unsigned s = wave_sum_u32(n_upd);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const unsigned t = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        const unsigned b = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        if (t) atomicAdd(slots + (b % nslots), (unsigned long long)t);
    }
}
// The brick kernel's update counts: one word per workgroup (COUNT_ROOM_WORDS of them, behind the workspace's 256-byte header), each added to
// by the one workgroup that owns it.  Round 5: they were 16 words in ONE cache line of the header, and atomics to a line are served one at a
// time whatever the word (~8 ns each): a launch whose 2 200 workgroups with work each add once could not end before ~3 + 2 200 x 0.008 =
// 21 us, whatever else was done to it (bricks in two entries, a smaller grid: no change until the counts moved;
// profiles/r05_ab_count_room.txt) — and at 1024^3 8 192 workgroups x 8 ns = 65 us of an 80 us launch.
__device__ __forceinline__ void room_count_add(unsigned n_upd, unsigned *room) {
    __shared__ unsigned s_cnt[4];
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    const unsigned s = wave_sum_u32(n_upd);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const unsigned t = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        if (t) atomicAdd(room + (blockIdx.x % COUNT_ROOM_WORDS), t);   // (an atomic: a grid may be larger than the room)
    }
}
enum { FOLD_COUNT_BLOCK = 1024 };
__global__ void __launch_bounds__(FOLD_COUNT_BLOCK) k_fold_count(unsigned *room, unsigned long long *updated) {
    // device-scope exchanges (which also leave the words zero for the next launch): the words were written by atomics from every XCD,
    // and a plain load here can be served from this XCD's L2 copy of a line an earlier fold pulled in — observed as lost counts when the
    // counts shared a line with the brick count that every workgroup reads
    // (all of a thread's exchanges go out before the first result is used: one round trip, where a loop that adds as it goes takes eight)
    unsigned v[COUNT_ROOM_WORDS / FOLD_COUNT_BLOCK];
#pragma unroll
    for (int k = 0; k < COUNT_ROOM_WORDS / FOLD_COUNT_BLOCK; ++k) v[k] = atomicExch(room + threadIdx.x + k * FOLD_COUNT_BLOCK, 0u);
    unsigned long long t = 0;
#pragma unroll
    for (int k = 0; k < COUNT_ROOM_WORDS / FOLD_COUNT_BLOCK; ++k) t += v[k];
    __shared__ unsigned long long s_v[FOLD_COUNT_BLOCK / 64];
    t = wave_sum_u64(t);
    if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (int k = 0; k < FOLD_COUNT_BLOCK / 64; ++k) all += s_v[k];
        if (all) atomicAdd(updated, all);
    }
}

// ---- path 1: column walk (no workspace): thread (x, y) walks its clipped z interval ---------
template <bool BILINEAR, bool SIGN = false>
__global__ void __launch_bounds__(256) k_integrate(const IntegrateArgs a) {
    const int x = threadIdx.x + blockIdx.x * 64;
    const int y = threadIdx.y + blockIdx.y * 4;
    unsigned n_upd = 0;
    if (x < a.X && y < a.Y) {
        int zb = a.z0 + blockIdx.z * a.zchunk;
        int ze = min(zb + a.zchunk, a.z1);
        clip_column(a.cp, far_limit(a), x, y, zb, ze);
        if (zb < ze) n_upd = integrate_span<BILINEAR, false, SIGN>(a, PoseRT{a.R, a.t}, x, y, zb, ze);
    }
    if (a.updated) block_count_add(n_upd, a.updated, 1);
}

// ---- path 2: resident workgroups stride over the brick list that xs_integrate_classify.hip left in the workspace -------------------------
#ifndef XS_INTEGRATE_WAVES
// Workgroups per CU = waves per SIMD the brick kernel is compiled for.  8 (64 VGPRs, 78 SGPRs) was round 3's choice: with the free-space
// path and the class look-up next to the walk the instance the pipeline runs then spills 36-48 bytes per lane, and a spill is not free
// even when it is rare: every wave's scratch lines are written back to HBM (2-3 KB per wave, ~15 MB per S1 launch: the traffic counters,
// profiles/r04_integrate_pmc.json).  At 6 (80 VGPRs, 106 SGPRs) far fewer scalars live in VGPR lanes and, when this was
// measured, no instance had scratch: the S1 kernel inside the pipeline 33 -> 28 us, S2 unchanged (profiles/r04_ab_integrate_waves.txt).
// Today's build: three of the four instances have none, k_integrate_bricks<true, true> (bilinear depth + sign map) has a private segment of
// 12 bytes per lane (profiles/integrate_split_kernels.txt lists every kernel's figures); recorded, not yet looked into.
#define XS_INTEGRATE_WAVES 6
#endif
template <bool BILINEAR, bool SIGN = false>
__global__ void __launch_bounds__(256, XS_INTEGRATE_WAVES) k_integrate_bricks(const IntegrateArgs a) {
    PoseRT ps{a.R, a.t};
#if defined(XS_EXPERIMENTS) && defined(XS_WG_TIMES)   // measurement only: every workgroup's begin / end on the 100 MHz wall clock, 512 KiB into the tile room of the workspace
    const unsigned long long probe_t0 = wall_clock64();
#endif
    const unsigned nwalk = a.brick_count[a.pair_word], count = nwalk + a.brick_count[a.pair_word + 1];   // (xs_integrate_boxes.h, "the list and its order")
    unsigned n_upd = 0;
    const float far = far_limit(a);
    // The column clip's 20 plane scalars are used once per brick, outside the voxel loop.  Held in scalar registers for the
    // whole kernel they push the voxel loop's own operands out (99 spilled scalars, ~30 v_readlane per voxel to fetch them
    // back — VALU slots, and this kernel is bound by VALU issue: 101 M wave instructions per S2 launch): they live in LDS.
    __shared__ ClipPlanes s_cp;
    float cp_word = 0.f;
    if (threadIdx.y == 0 && threadIdx.x < (int)(sizeof(ClipPlanes) / 4)) cp_word = reinterpret_cast<const float *>(&a.cp)[threadIdx.x];
    // (A bit-reversed entry order for launches with fewer bricks than workgroups — so that list neighbours, the bricks of one surface, land
    // on different CUs — measured 29 -> 42 us on S1: the dispatcher deals consecutive workgroups round the CUs, so the eight workgroups of
    // a CU already take entries 256 apart; profiles/r04_integrate_wg_times.txt.)
    const unsigned first = blockIdx.x, stride = gridDim.x;
    // A list without classes (k_classify_bricks alone) is in plane order (z slowest).  Where the camera looks up the z axis the bricks of
    // the surfaces — the walked, expensive ones — come last, and a launch ends with a tail of them, bound by instruction issue, after the
    // free-space bricks have streamed: taken from its far end the list starts with them and the streaming fills in around (KF_FAR_FIRST,
    // set by the launcher from the pose; never for a list that is ordered by class).
    const bool far_first = (a.kflags & KF_FAR_FIRST) != 0;
    auto entry = [&](unsigned e) { return list_at(far_first ? count - 1u - e : e, nwalk, a.list_cap); };
    // the first entry and its class are requested together, in front of the barrier
    int b_next = 0, cls_next = BOX_MIXED;
    if (first < count) {
        b_next = a.brick_list[entry(first)];
        if (a.box_class) cls_next = (int)a.box_class[entry(first) * BOXES_PER_BRICK + threadIdx.y];
    }
    if (threadIdx.y == 0 && threadIdx.x < (int)(sizeof(ClipPlanes) / 4)) reinterpret_cast<float *>(&s_cp)[threadIdx.x] = cp_word;
    __syncthreads();
    for (unsigned e = first; e < count; e += stride) {
        // (the list was written by the classification kernel, so the compiler reads it with a vector load — back to a scalar,
        // or every address derived from it would be a 64-bit vector quantity)
        if (e != first) {
            b_next = a.brick_list[entry(e)];
            if (a.box_class) cls_next = (int)a.box_class[entry(e) * BOXES_PER_BRICK + threadIdx.y];
        }
        const int b = __builtin_amdgcn_readfirstlane(b_next);
        const int cls_now = cls_next;
        const int bx = b & 1023, by = (b >> 10) & 1023, bz = b >> 20;
        const int t256 = (int)(threadIdx.y * 64 + threadIdx.x);
        const int lx = t256 % BRICK_X, ly = t256 / BRICK_X;
        const int x = bx * BRICK_X + lx, y = by * BRICK_Y + ly;
        int walk_lo = a.z0, walk_hi = a.z1;   // the planes this wave walks voxel by voxel (all of the brick's unless the box's word says otherwise)
        {
            if (a.box_class) {   // what k_classify_boxes found for this wave's part of the brick: free planes at one end, empty ones at the other
                const unsigned word = (unsigned)__builtin_amdgcn_readfirstlane(cls_now);
                const int zb0 = a.z0 + bz * a.brick_z, ze0 = min(zb0 + a.brick_z, a.z1);
                const int nf = (int)(word & 0xffu), ne = (int)((word >> 8) & 0xffu);
                const bool falls = ((word >> 16) & 1u) != 0u;
                const int f0 = falls ? ze0 - nf : zb0, f1 = falls ? ze0 : zb0 + nf;       // free planes [f0, f1)
                walk_lo = falls ? zb0 + ne : zb0 + nf; walk_hi = falls ? ze0 - nf : ze0 - ne;
                if (nf > 0 && !(word & BOX_NO_STREAM_BIT) && x < a.X && y < a.Y) {
                    const size_t ubase = ((size_t)(f0 - a.z0) * a.Y + (size_t)by * BRICK_Y) * a.vstep + (size_t)bx * BRICK_X * 4;
                    char *fv = reinterpret_cast<char *>(a.value) + ubase, *fw = reinterpret_cast<char *>(a.weight) + ubase, *fg = reinterpret_cast<char *>(a.grad) + ubase;
                    const unsigned foff = (unsigned)ly * (unsigned)a.vstep + (unsigned)lx * 4u, fplane = (unsigned)a.Y * (unsigned)a.vstep;
                    if (word & BOX_SPECKLE_BIT) n_upd += integrate_valid_column(a, ps, (word & BOX_EDGE_BIT) != 0u, fv, fw, fg, foff, fplane, x, y, f0, f1);   // (a box that sees an invalid pixel)
                    else if (word & BOX_EDGE_BIT) n_upd += integrate_edge_column(a, ps, fv, fw, fg, foff, fplane, x, y, f0, f1);   // (a box on the frustum's side)
                    else n_upd += integrate_free_column(a, fv, fw, fg, foff, fplane, f0, f1);
                }
                if (walk_lo >= walk_hi) continue;
            }
        }
        if (x < a.X && y < a.Y) {
            const int zb0 = a.z0 + bz * a.brick_z;
            int zb = zb0, ze = min(zb + a.brick_z, a.z1);
            clip_column(s_cp, far, x, y, zb, ze);
            zb = max(zb, walk_lo); ze = min(ze, walk_hi);
            if (zb < ze) {
                const size_t ubase = ((size_t)(zb0 - a.z0) * a.Y + (size_t)by * BRICK_Y) * a.vstep + (size_t)bx * BRICK_X * 4;
                n_upd += integrate_span<BILINEAR, true, SIGN>(a, ps, x, y, zb, ze, ubase, zb0, (unsigned)ly * (unsigned)a.vstep + (unsigned)lx * 4u);
            }
        }
    }
#if defined(XS_EXPERIMENTS) && defined(XS_WG_TIMES)
    if (a.box_class && threadIdx.x == 0) {
        unsigned *rec = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(a.box_class) + a.probe_offset) + 4u * (blockIdx.x * 4 + threadIdx.y);
        rec[0] = (unsigned)probe_t0; rec[1] = (unsigned)wall_clock64(); rec[2] = blockIdx.x < count ? (unsigned)a.box_class[entry(blockIdx.x) * BOXES_PER_BRICK + threadIdx.y] : 99u; rec[3] = (n_upd & 0xffu) | ((__builtin_amdgcn_s_getreg(0xF814) & 0xfu) << 8) | (__builtin_amdgcn_s_getreg(0xF804) << 16);   // + XCC_ID, HW_ID (wave, SIMD, pipe, CU, SH, SE)
    }
#endif
    if (a.updated) room_count_add(n_upd, a.count_room);
}

/* the fold of the update counts' room into updated_dev, for a caller that passes XS_INTEGRATE_NO_FOLD (xs_integrate_workspace_clear,
 * xs_integrate_classify.hip, is the other of the two launches such a caller takes off its critical path) */
extern "C" int xs_integrate_fold_counts(void *workspace, unsigned long long *updated_dev, void *stream) {
    if (!workspace || !updated_dev) return xs_set_error(hipErrorInvalidValue, "xs_integrate_fold_counts: null pointer");
    hipLaunchKernelGGL(k_fold_count, dim3(1), dim3(FOLD_COUNT_BLOCK), 0, (hipStream_t)stream, reinterpret_cast<unsigned *>((char *)workspace + WS_HEADER_BYTES), updated_dev);
    XS_CHECK(hipGetLastError());
    return 0;
}
// camera depth grows with z: the far bricks end the list, and the list is taken from that end (KF_FAR_FIRST)
static bool far_end_first(const IntegrateArgs &a) {
    static const char *env_order = exp_env_str("XS_INTEGRATE_ORDER");   // A/B aid: "near" / "far" force the list direction
    return env_order ? !strcmp(env_order, "far") : a.R.data[2].z.re > 0.0f;
}
extern "C" int xs_integrate_scaled(const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4, int max_weight,
                                   const int *res, float voxel_size, const float *Rv2c18, const float *tv2c6, float tranc_dist,
                                   float *value, int *weight, float *grad, size_t vol_step, float threshold, int z0, int z1,
                                   unsigned long long *updated_dev, const float *depth_max_dev, void *workspace, void *stream) {
    return xs_integrate_scaled_ex(depth_scaled, scaled_step, rows, cols, intr4, max_weight, res, voxel_size, Rv2c18, tv2c6, tranc_dist, value, weight,
                                  grad, vol_step, threshold, z0, z1, updated_dev, depth_max_dev, workspace, 0u, stream);
}
extern "C" int xs_integrate_scaled_ex(const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4, int max_weight,
                                      const int *res, float voxel_size, const float *Rv2c18, const float *tv2c6, float tranc_dist,
                                      float *value, int *weight, float *grad, size_t vol_step, float threshold, int z0, int z1,
                                      unsigned long long *updated_dev, const float *depth_max_dev, void *workspace, unsigned flags, void *stream) {
    xs_integrate_opts o = {};   // the plain entry point: flags alone
    o.struct_bytes = sizeof(o); o.flags = flags;
    return xs_integrate_scaled_ex2(depth_scaled, scaled_step, rows, cols, intr4, max_weight, res, voxel_size, Rv2c18, tv2c6, tranc_dist, value, weight, grad,
                                   vol_step, threshold, z0, z1, updated_dev, depth_max_dev, workspace, &o, stream);
}
extern "C" int xs_integrate_scaled_ex2(const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4, int max_weight,
                                       const int *res, float voxel_size, const float *Rv2c18, const float *tv2c6, float tranc_dist,
                                       float *value, int *weight, float *grad, size_t vol_step, float threshold, int z0, int z1,
                                       unsigned long long *updated_dev, const float *depth_max_dev, void *workspace, const xs_integrate_opts *opts,
                                       void *stream) {
    if (!opts || opts->struct_bytes != sizeof(xs_integrate_opts)) return xs_set_error(hipErrorInvalidValue, "xs_integrate_scaled_ex2: opts->struct_bytes is not sizeof(xs_integrate_opts)");
    const unsigned flags = opts->flags;
    // (bit 16 asked for the posted launch of ABI 2, which took its pose from a mailbox: refused, or an old caller would integrate with the
    // list pose it passes as arguments)
    if (flags & 16u) return xs_set_error(hipErrorInvalidValue, "xs_integrate_scaled_ex: flag bit 16 (the posted launch, removed in ABI 3) is not supported");
    const hipEvent_t ev0 = (hipEvent_t)opts->start_event, ev1 = (hipEvent_t)opts->stop_event;
    const DepthTile *depth_tiles = static_cast<const DepthTile *>(opts->depth_tiles);
    if (!depth_scaled || !intr4 || !res || !Rv2c18 || !tv2c6 || !value || !weight || !grad)
        return xs_set_error(hipErrorInvalidValue, "xs_integrate_scaled: null pointer");
    if ((flags & (XS_INTEGRATE_HEADER_IS_CLEAR | XS_INTEGRATE_NO_FOLD | XS_INTEGRATE_LIST_IS_READY)) && !workspace)
        return xs_set_error(hipErrorInvalidValue, "xs_integrate_scaled_ex: the flags concern the workspace path");
    if (z0 < 0 || z1 > res[2] || z1 < z0 || (vol_step % 4) != 0 || vol_step < (size_t)res[0] * 4)
        return xs_set_error(hipErrorInvalidValue, "xs_integrate_scaled: bad slab or pitch");
    hipStream_t st = (hipStream_t)stream;
    if (z1 == z0 || res[0] == 0 || res[1] == 0) {   // nothing to launch: the caller's timing / completion events are recorded all the same
        if (ev0) XS_CHECK(hipEventRecord(ev0, st));
        if (ev1) XS_CHECK(hipEventRecord(ev1, st));
        return 0;
    }
    IntegrateArgs a;
    integrate_args(a, rows, cols, intr4, res, voxel_size, Rv2c18, tv2c6, tranc_dist, z0, z1, depth_max_dev);
    a.depth = depth_scaled; a.dstep = scaled_step;
    a.value = value; a.weight = weight; a.grad = grad; a.vstep = vol_step;
    a.max_weight = max_weight; a.threshold = threshold; a.updated = updated_dev;
    static const bool env_always = exp_env_set("XS_INTEGRATE_ALWAYS_STORE");   // measurement aid, as the flag
    if (env_always || (flags & XS_INTEGRATE_ALWAYS_STORE)) a.kflags |= KF_ALWAYS_STORE;
    if (flags & XS_INTEGRATE_COUNT_CLASSES) a.kflags |= KF_COUNT_CLASSES;
    if (far_end_first(a)) a.kflags |= KF_FAR_FIRST;
    a.signmap = static_cast<unsigned char *>(opts->signmap);   // (a slab launch marks the bricks of its own planes: the map is indexed by whole-volume coordinates)
    const int nz = z1 - z0;
    a.zchunk = nz;
    dim3 block(64, 4);
    // The brick kernel addresses a brick's voxels as a wave-uniform base (the brick's first voxel) + one 32-bit byte offset per lane: a brick
    // must span less than 4 GiB of an array — always, short of absurd pitches (rows of more than 128 K floats at Y = 1024); such a volume takes
    // the column walk below.  (Round 6: the brick kernel's 64-bit-pointer instances, which no test could reach, are gone.)
    const bool off32 = ((size_t)a.brick_z * a.Y + BRICK_Y) * a.vstep < (1ull << 32);
    if (workspace && off32 && a.bricks_x <= 1024 && a.bricks_y <= 1024 && a.bricks_z <= 2047) {  // packed brick ids: 10 + 10 + 11 bits
        bind_workspace(a, res, nz, workspace);
        const int nb = a.bricks_x * a.bricks_y * a.bricks_z;
        const bool sign = a.signmap != nullptr;
        // the boxes' classes (free space / nothing to write / exact walk) and the list's order: those xs_integrate_classify left for this
        // list, or decided here with the launch's own pose — from the caller's tile table (opts->depth_tiles) or one built here,
        // in the workspace
        static const bool env_no_tiles = exp_env_set("XS_INTEGRATE_NO_TILES");   // A/B aid, as the flag
        // the classes xs_integrate_classify* left hold for this launch only if its pose lies within the slack they were padded for: checked here
        ClassesAhead ca;
        bool classes_ahead = (flags & XS_INTEGRATE_LIST_IS_READY) && classes_ahead_take(workspace, ca) && !(flags & XS_INTEGRATE_RECLASSIFY_BOXES);
        if (classes_ahead)   // ... for this slab of this volume, this camera and band, this frame's tile table?
            classes_ahead = ca.z0 == z0 && ca.z1 == z1 && !memcmp(ca.res, res, sizeof(ca.res)) && ca.rows == rows && ca.cols == cols && !memcmp(ca.intr, intr4, sizeof(ca.intr)) &&
                            ca.voxel_size == voxel_size && ca.tranc_dist == tranc_dist && ca.tiles == depth_tiles;
        if (classes_ahead) {
            IntegrateArgs l = a;
            load_mat(ca.R18, l.R); load_vec(ca.t6, l.t);
            // (classes decided for a pose whose imaginary parts passed stream_margins do not hold for one whose do not)
            classes_ahead = box_slack_covers(l, a, res, ca.slack_scale) && !(a.kflags & KF_NO_TESTED_STREAM);
        }
        const bool use_tiles = !env_no_tiles && !(flags & XS_INTEGRATE_NO_TILES);
        auto tile_table = [&]() -> const DepthTile * {   // the caller's, or one built in the workspace's tile room
            if (depth_tiles || xs_depth_tiles_bytes(rows, cols) > TILE_ROOM_BYTES) return depth_tiles;
            DepthTile *own = reinterpret_cast<DepthTile *>((char *)workspace + workspace_list_bytes(res, nz) + workspace_class_bytes(res, nz));
            launch_depth_tiles(depth_scaled, scaled_step, rows, cols, own, st);
            return own;
        };
        if (!(flags & XS_INTEGRATE_LIST_IS_READY)) {   // (else: xs_integrate_classify has run on this stream for a covering pose)
            if (!(flags & XS_INTEGRATE_HEADER_IS_CLEAR))
                XS_CHECK(hipMemsetAsync(a.brick_count, 0, WS_LIST_OFFSET, st));  // list pairs + the update counts' room: one fill
            launch_classification(a, res, nz, workspace, use_tiles ? tile_table() : nullptr, st);
        } else if (use_tiles) {
            if (classes_ahead) bind_ordered_list(a, res, nz, workspace);
            else launch_box_classes(a, res, nz, workspace, tile_table(), st);
        }
        if (a.box_class) a.kflags &= ~(unsigned)KF_FAR_FIRST;   // the list is ordered by class
        // resident workgroups stride over the list: 256 CUs x 8
        static const int env_g = exp_env_int("XS_BRICK_GRID", 0);
        const int gmax = env_g > 0 ? env_g : 8192;
        const int g = nb < gmax ? nb : gmax;
        // profiling: the event pair rides on the dispatch packet itself (hipExtLaunchKernelGGL: start / stop are
        // the kernel's own begin / end timestamps), so it adds no marker packets to the stream and times what
        // rocprofv3 times
        // (either event may be null: a completion event alone lets another stream wait for this kernel without a marker packet)
        void (*kern)(const IntegrateArgs) = sign ? (threshold > 0.0f ? k_integrate_bricks<true, true> : k_integrate_bricks<false, true>)
                                                 : (threshold > 0.0f ? k_integrate_bricks<true> : k_integrate_bricks<false>);
        static const int env_lds = exp_env_int("XS_INTEGRATE_DYN_LDS", 0);   // experiment: dynamic LDS bytes per workgroup = a cap on the workgroups resident per CU
        if (ev0 || ev1) hipExtLaunchKernelGGL(kern, dim3(g), block, env_lds, st, ev0, ev1, 0, a);
        else hipLaunchKernelGGL(kern, dim3(g), block, env_lds, st, a);
        if (updated_dev && !(flags & XS_INTEGRATE_NO_FOLD))
            hipLaunchKernelGGL(k_fold_count, dim3(1), dim3(FOLD_COUNT_BLOCK), 0, st, a.count_room, updated_dev);
    } else {
        int gx = div_up(a.X, 64), gy = div_up(a.Y, 4), zsplit = 1;
        while ((long long)gx * gy * zsplit < 4096 && zsplit < nz && nz / (zsplit * 2) >= 16) zsplit *= 2;
        a.zchunk = div_up(nz, zsplit);
        dim3 grid(gx, gy, div_up(nz, a.zchunk));
        // (the events opts->start_event / stop_event name ride on this dispatch too: a caller that waits on the stop event — the
        // orchestrator's auxiliary stream does — must find it recorded whichever kernel ran)
        void (*kern)(const IntegrateArgs) = a.signmap ? (threshold > 0.0f ? k_integrate<true, true> : k_integrate<false, true>)
                                                      : (threshold > 0.0f ? k_integrate<true> : k_integrate<false>);
        if (ev0 || ev1) hipExtLaunchKernelGGL(kern, grid, block, 0, st, ev0, ev1, 0, a);
        else hipLaunchKernelGGL(kern, grid, block, 0, st, a);
    }
    XS_CHECK(hipGetLastError());
    return 0;
}

// The reference's launcher (TsdfFusion.cu:173-201): u16 millimetres in, scale then integrate.
// depth_scaled is caller-owned workspace (rows x cols floats) — the reference allocates and
// frees it on every call (:180,:198); here it is resident.
extern "C" int xs_integrate_tsdf_volume(const uint16_t *depth, size_t depth_step, int rows, int cols, const float *intr4, int max_weight,
                                        const int *res, float voxel_size, const float *Rv2c18, const float *tv2c6, float tranc_dist,
                                        float *value, int *weight, float *grad, size_t vol_step, float *depth_scaled,
                                        size_t scaled_step, float threshold, int z0, int z1, unsigned long long *updated_dev,
                                        void *stream) {
    int rc = xs_scale_depth(depth, depth_step, rows, cols, depth_scaled, scaled_step, stream);
    if (rc) return rc;
    return xs_integrate_scaled(depth_scaled, scaled_step, rows, cols, intr4, max_weight, res, voxel_size, Rv2c18, tv2c6, tranc_dist, value,
                               weight, grad, vol_step, threshold, z0, z1, updated_dev, nullptr, nullptr, stream);
}
