// xs_integrate_classify.hip — what an integrate launch knows before it touches a voxel, for gfx950: the bricks the view frustum can see
// (k_classify_bricks), their wave-sized boxes' classes and the list in the order the integrate kernel takes it (k_classify_boxes), the
// workspace these live in, and the classification as a call of its own for a pose that is only nearly the final one (xs_integrate_classify*,
// the "classes ahead" table, xs_integrate_list_covers).  No reference counterpart.  xs_integrate_boxes.h has the formats.
#include <hip/hip_ext.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <mutex>
#include "xs_device.h"
#include "xs_env.h"
#include "xs_integrate_boxes.h"
#include "xs_integrate_args.h"
#include "../../include/xslam_amd.h"

using namespace xs;

// ---- one box ---------------------------------------------------------------------------------------------------------------------------
namespace {
__device__ __forceinline__ float dpp_xor1(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true)); }    // quad_perm [1, 0, 3, 2]
__device__ __forceinline__ float dpp_xor2(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true)); }    // quad_perm [2, 3, 0, 1]
__device__ __forceinline__ float dpp_half_mirror(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true)); }   // lane i <- 7 - i of its 8
__device__ __forceinline__ float dpp_row_mirror(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, true)); }    // lane i <- 15 - i of its 16
template <bool MAX> __device__ __forceinline__ float pick(float a, float b) { return MAX ? fmaxf(a, b) : fminf(a, b); }
template <bool MAX> __device__ __forceinline__ float fold8(float v) {   // over each group of eight lanes, result in all of them
    v = pick<MAX>(v, dpp_xor1(v)); v = pick<MAX>(v, dpp_xor2(v)); return pick<MAX>(v, dpp_half_mirror(v));
}
template <bool MAX> __device__ __forceinline__ float fold64(float v) {  // over the wave, result wave-uniform
    v = fold8<MAX>(v); v = pick<MAX>(v, dpp_row_mirror(v));
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return pick<MAX>(pick<MAX>(r0, r1), pick<MAX>(r2, r3));
}
__device__ __forceinline__ float dpp_fold4min(float v) { v = fminf(v, dpp_xor1(v)); return fminf(v, dpp_xor2(v)); }
__device__ __forceinline__ float dpp_fold4max(float v) { v = fmaxf(v, dpp_xor1(v)); return fmaxf(v, dpp_xor2(v)); }
// box = voxel indices [x0, x1) x [y0, y1) x [z0, z1), not empty.  Eight lanes per box (a wave classifies eight boxes at once): lane
// c of the group evaluates corner c, cross-lane steps fold the group, the group's lanes share the tile reads and then take a plane
// each; every lane of a group returns the group's word.
__device__ __forceinline__ unsigned classify_box(const IntegrateArgs &a, const BoxSlack &sl, int x0, int x1, int y0, int y1, int z0, int z1, int corner) {
    const int nz = z1 - z0;
    const unsigned all_walk = box_word(0, 0, 0), all_empty = box_word(0, nz, 0);
    // voxel centres, in the exact path's own units: (index + 0.5) * voxel_size
    const float vx = (((corner & 1) ? x1 - 1 : x0) + 0.5f) * a.voxel_size;
    const float vy = (((corner & 2) ? y1 - 1 : y0) + 0.5f) * a.voxel_size;
    const float vz = (((corner & 4) ? z1 - 1 : z0) + 0.5f) * a.voxel_size;
    const float X = ((a.R.data[0].x.re * vx + a.R.data[0].y.re * vy) + a.R.data[0].z.re * vz) + a.t.x.re;
    const float Y = ((a.R.data[1].x.re * vx + a.R.data[1].y.re * vy) + a.R.data[1].z.re * vz) + a.t.y.re;
    const float c = ((a.R.data[2].x.re * vx + a.R.data[2].y.re * vy) + a.R.data[2].z.re * vz) + a.t.z.re;
    const float cmin = fold8<false>(c) - sl.dC, cmax = fold8<true>(c) + sl.dC;
    if (!(cmin > 1e-3f)) return all_walk;            // the camera plane cuts the box (or nearly): no hull argument
    const float rc = __builtin_amdgcn_rcpf(c);
    const float un = X * rc, vn = Y * rc;            // normalised image coordinates of the corner
    const float u = a.intr.fx * un + a.intr.cx, v = a.intr.fy * vn + a.intr.cy;
    // what a pose within the slack can move a projection by: |d(X/c)| <= (dX + |X/c| dC) / (c - dC)
    const float rcm = __builtin_amdgcn_rcpf(cmin);
    const float pad_u = 1.5f + fabsf(a.intr.fx) * (sl.dX + fold8<true>(fabsf(un)) * sl.dC) * rcm * 1.01f;
    const float pad_v = 1.5f + fabsf(a.intr.fy) * (sl.dY + fold8<true>(fabsf(vn)) * sl.dC) * rcm * 1.01f;
    const float ulo = fold8<false>(u) - pad_u, uhi = fold8<true>(u) + pad_u, vlo = fold8<false>(v) - pad_v, vhi = fold8<true>(v) + pad_v;
    if (!(ulo > -1e6f && uhi < 1e6f && vlo > -1e6f && vhi < 1e6f)) return all_walk;   // (NaN / overflow: take the exact walk)
    const int px0 = __float2int_rd(ulo), px1 = __float2int_ru(uhi), py0 = __float2int_rd(vlo), py1 = __float2int_ru(vhi);
    const bool inside = px0 >= 2 && py0 >= 2 && px1 <= a.dcols - 2 && py1 <= a.drows - 2;
    // the part of the pixel range that lies in the image (what is outside is never written)
    const int qx0 = max(px0, 0), qx1 = min(px1, a.dcols - 1), qy0 = max(py0, 0), qy1 = min(py1, a.drows - 1);
    if (qx0 > qx1 || qy0 > qy1) return all_empty;
    // the depth range over the pixel range: from the tiles, or — a box near the camera covers hundreds of them — from the super tiles
    int tx0 = qx0 / DEPTH_TILE, tx1 = qx1 / DEPTH_TILE, ty0 = qy0 / DEPTH_TILE, ty1 = qy1 / DEPTH_TILE, pitch = a.dt.tiles_x;
    const DepthTile *table = a.dt.tiles;
    if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > BOX_MAX_TILES) {
        tx0 = qx0 / SUPER_W; tx1 = qx1 / SUPER_W; ty0 = qy0 / SUPER_H; ty1 = qy1 / SUPER_H; pitch = a.dt.supers_x; table = a.dt.supers;
        if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > 4 * BOX_MAX_TILES) return all_walk;
    }
    // (four rows of the range per trip, requested together — a row index past the range repeats its last row, which changes neither bound:
    // a box of the benchmark scene sees 3 x 7 tiles with the slack's pads, i.e. one trip of one round of loads where row by row took three)
    float lo = __builtin_inff(), hi = 0.f, neg = 0.f;   // lo: over the valid pixels; neg < 0: a tile of the range holds an invalid one
    for (int ty = ty0; ty <= ty1; ty += 4) {
        const int r0 = ty * pitch, r1 = min(ty + 1, ty1) * pitch, r2 = min(ty + 2, ty1) * pitch, r3 = min(ty + 3, ty1) * pitch;
        for (int tx = tx0 + corner; tx <= tx1; tx += 8) {
            const DepthTile t0 = table[r0 + tx], t1 = table[r1 + tx], t2 = table[r2 + tx], t3 = table[r3 + tx];
            lo = fminf(lo, fminf(fminf(fabsf(t0.lo), fabsf(t1.lo)), fminf(fabsf(t2.lo), fabsf(t3.lo))));
            neg = fminf(neg, fminf(fminf(t0.lo, t1.lo), fminf(t2.lo, t3.lo)));
            hi = fmaxf(hi, fmaxf(fmaxf(t0.hi, t1.hi), fmaxf(t2.hi, t3.hi)));
        }
    }
    lo = fold8<false>(lo); hi = fold8<true>(hi);
    const bool speckle = fold8<false>(neg) < 0.f;             // the box can see an invalid pixel
    const float band = (a.tranc_dist * 1.001f + 1e-5f) + 2e-4f;   // the walk's own band (update_voxel) + margin
    if (cmin - hi > band) return all_empty;                 // behind everything the box can see (hi = 0: nothing valid there)
    // plain free space needs the whole range in the image and valid; else the free planes are streamed with the tests that are left
    // (BOX_EDGE_BIT / BOX_SPECKLE_BIT), which are derived for voxels that are not at the camera
    const bool tested = !inside || speckle;
    const bool may_stream = !tested || (cmin >= XS_EDGE_CMIN && !(a.kflags & KF_NO_TESTED_STREAM));   // (cmin carries the pose slack: it bounds every covered pose's c)
    if (may_stream && lo - cmax > band) return box_word(nz, 0, 0, !inside, speckle);   // in front of everything valid it can see
    if (nz > 8) return all_walk;                            // (more planes per brick than lanes per box: a tuning configuration)
    // Plane by plane.  The four corners of the box's first plane are lanes 0 - 3 (corner bit 2 clear), of its last plane lanes 4 - 7; c moves
    // by dzc per plane at every (x, y).  Lane j takes plane j with the c range of the first plane's corners shifted j planes along.
    const float q_lo = dpp_fold4min(c), q_hi = dpp_fold4max(c);                 // per quad: this plane's corners
    const float o_lo = dpp_half_mirror(q_lo), o_hi = dpp_half_mirror(q_hi);     // the other quad's
    const float c0_lo = (corner & 4) ? o_lo : q_lo, c0_hi = (corner & 4) ? o_hi : q_hi;   // first plane
    const float dzc = a.R.data[2].z.re * a.voxel_size;
    const float pl_lo = (c0_lo + (float)corner * dzc) - sl.dC - 1e-5f, pl_hi = (c0_hi + (float)corner * dzc) + sl.dC + 1e-5f;   // plane `corner`'s c range
    const bool p_ok = corner < nz;
    const bool p_free = p_ok && may_stream && lo - pl_hi > band, p_empty = p_ok && pl_lo - hi > band;
    const int shift = (int)(threadIdx.x & 63u) & ~7;          // the group's first lane in the wave
    const unsigned fm = (unsigned)(__builtin_amdgcn_ballot_w64(p_free) >> shift) & 0xffu, em = (unsigned)(__builtin_amdgcn_ballot_w64(p_empty) >> shift) & 0xffu;
    const int falls = dzc < 0.f ? 1 : 0;
    int n_free, n_empty;
    if (!falls) {   // c grows with z: free planes from the first plane on, empty ones from the last plane back
        n_free = __builtin_ctz(~fm | 0x100u);
        n_empty = __builtin_clz((~em & ((1u << nz) - 1u)) << (32 - nz) | (1u << (31 - nz)));
    } else {
        n_free = __builtin_clz((~fm & ((1u << nz) - 1u)) << (32 - nz) | (1u << (31 - nz)));
        n_empty = __builtin_ctz(~em | 0x100u);
    }
    n_free = min(n_free, nz); n_empty = min(n_empty, nz - n_free);
    return box_word(n_free, n_empty, falls, !inside && n_free > 0, speckle && n_free > 0);
}
}  // namespace

// ---- path 2: brick work list ------------------------------------------------------------------
// Phase A (here): one thread per brick tests it against the padded frustum (and the far limit) and
// appends survivors to a list — a wave ballots, one atomic per wave.  Phase B (k_integrate_bricks, xs_integrate.hip): resident
// workgroups stride over the list; each handles one 32x8x8 brick (a wave: 32 columns x 2 rows — 128-byte row segments;
// 64x4 bricks list 15 % more of them on the benchmark scene, 2 224 against 1 892, i.e. more than the 2 048 resident workgroups,
// and 16x16 ones stream a quarter slower: profiles/tools/ab_brick_shape.sh).  The voxels that can be
// written (a few % of an ICL-like volume) are thereby spread over every CU instead of being
// concentrated in the few columns that cross the frustum.
// (round 5: one reservation per WORKGROUP of 1 024 threads instead of one per wave — same-address atomics are served one at a time, ~12 ns
// each, and the listed bricks of a 1024^3 frustum sit in ~600 waves: 7 of the kernel's 8.9 us; entries stay in thread order, i.e. plane order)
enum { CLASSIFY_BRICKS_BLOCK = 1024 };
__global__ void __launch_bounds__(CLASSIFY_BRICKS_BLOCK) k_classify_bricks(const IntegrateArgs a) {
    const int nb = a.bricks_x * a.bricks_y * a.bricks_z;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    bool active = false;
    if (b < nb) {
        const int bx = b % a.bricks_x, by = (b / a.bricks_x) % a.bricks_y, bz = b / (a.bricks_x * a.bricks_y);
        const int x0 = bx * BRICK_X, y0 = by * BRICK_Y, z0 = a.z0 + bz * a.brick_z;
        const Frustum f = device_frustum(a);
        active = box_may_pass(f, x0, min(x0 + BRICK_X, a.X), y0, min(y0 + BRICK_Y, a.Y), z0, min(z0 + a.brick_z, a.z1));
    }
    const unsigned long long m = __ballot(active);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ unsigned s_n[CLASSIFY_BRICKS_BLOCK / 64], s_base;
    if (lane == 0) s_n[wave] = (unsigned)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { const unsigned n = s_n[w]; s_n[w] = total; total += n; }   // exclusive prefix: each wave's place
        s_base = total ? atomicAdd(a.brick_count, total) : 0u;
    }
    __syncthreads();
    if (active) {  // packed (bx, by, bz), 10 bits each: the consumer decodes with shifts
        const int bx = b % a.bricks_x, by = (b / a.bricks_x) % a.bricks_y, bz = b / (a.bricks_x * a.bricks_y);
        a.brick_list[s_base + s_n[wave] + __popcll(m & ((1ull << lane) - 1ull))] = bx | (by << 10) | (bz << 20);
    }
}

// One brick's four boxes by the 32 lanes of a half-wave (8 lanes per box, see classify_box); the box's word in all of its eight lanes, bit
// 31 set when the box has planes to walk.  KF_COUNT_CLASSES: counted in the header.
__device__ __forceinline__ unsigned classify_brick_boxes(const IntegrateArgs &a, const BoxSlack &sl, int b, int box, int corner) {
    const int bx = b & 1023, by = (b >> 10) & 1023, bz = b >> 20;
    const int wx0 = bx * BRICK_X + (box * 64) % BRICK_X, wy0 = by * BRICK_Y + (box * 64) / BRICK_X;
    const int zb0 = a.z0 + bz * a.brick_z, ze0 = min(zb0 + a.brick_z, a.z1);
    const int nz = ze0 - zb0;
    unsigned word = box_word(0, nz, 0);   // a wave without a column of the brick in the volume: nothing to write
    if (wx0 < a.X && wy0 < a.Y) word = classify_box(a, sl, wx0, min(wx0 + BOX_WX, a.X), wy0, min(wy0 + BOX_WY, a.Y), zb0, ze0, corner);
    const int nf = (int)(word & 0xff), ne = (int)((word >> 8) & 0xff);
    if (corner == 0 && (a.kflags & KF_COUNT_CLASSES)) {   // boxes wholly free / wholly empty / with planes to walk; + the planes walked
        atomicAdd(a.brick_count + CLASS_COUNT_WORD + (nf == nz ? 0 : ne == nz ? 1 : 2), 1u);
        atomicAdd(a.brick_count + CLASS_COUNT_WORD + 3, (unsigned)(nz - nf - ne));
        if (word & BOX_SPECKLE_BIT) atomicAdd(a.brick_count + CLASS_COUNT_WORD + 7, (unsigned)nf);   // planes streamed with the validity test (with or without the in-image test)
        else if (word & BOX_EDGE_BIT) atomicAdd(a.brick_count + CLASS_COUNT_WORD + 6, (unsigned)nf);   // planes streamed with the in-image test alone (words + 4, + 5: the second ListPair)
    }
    return word | (nf + ne < nz ? 1u << 31 : 0u);
}
// What a workgroup does with the n bricks it holds in LDS (s_brick; their boxes' words in s_word, bit 31 = planes to walk): the first
// wave ranks them inside the two runs, reserves room for both with one atomic, and all threads write the entries and the classes.
// Call from every thread; s_pos: n words; s_base: 2 words.
//
// A brick in TWO entries (split, small launches only): a wave that walks a whole box inside a surface's band is one chain of ~8 x 1 500
// instructions, and a wave alone on its SIMD issues at half the SIMD's rate (profiles/r05_valu_issue_calibration.txt: 2.3 ns per instruction
// against 1.2 with two waves) — a launch whose bricks are all resident at once lasts as long as that chain (17-19 us of scene S1's 21) while
// most SIMDs hold one such wave or none.  A brick with a box that walks >= SPLIT_MIN_PLANES planes therefore takes two neighbouring entries
// of the front run: the first streams the boxes' free planes and walks the half of each box's walked planes next to them, the second walks
// the half next to the empty planes and does not stream (BOX_NO_STREAM_BIT).  The halves are expressed in the class words themselves: the first entry counts the second's planes as empty,
// the second counts the first's as free-and-not-to-be-streamed; every voxel is still visited once.
#ifndef XS_SPLIT_MIN_PLANES
#define XS_SPLIT_MIN_PLANES 6
#endif
enum { SPLIT_MIN_PLANES = XS_SPLIT_MIN_PLANES, POS_OTHER_BIT = 1u << 31, POS_SPLIT_BIT = 1u << 30 };
__device__ __forceinline__ void list_append(const IntegrateArgs &a, unsigned *pair, int *region, unsigned n, const int *s_brick, const unsigned *s_word,
                                            unsigned *s_pos, unsigned *s_base, bool split) {
    const unsigned tid = threadIdx.x;
    if (tid < 64u) {
        unsigned nw = 0, no = 0;
        const unsigned long long below = (1ull << tid) - 1ull;
        for (unsigned c = 0; c < n; c += 64u) {
            const unsigned k = c + tid;
            const bool live = k < n;
            const bool walk = live && ((s_word[k * 4] | s_word[k * 4 + 1] | s_word[k * 4 + 2] | s_word[k * 4 + 3]) >> 31) != 0u;
            bool heavy = false;
            if (split && walk) {
                const int nz = min(a.brick_z, a.z1 - (a.z0 + (s_brick[k] >> 20) * a.brick_z));
                const int most = max(max(box_walked_planes(s_word[k * 4], nz), box_walked_planes(s_word[k * 4 + 1], nz)),
                                     max(box_walked_planes(s_word[k * 4 + 2], nz), box_walked_planes(s_word[k * 4 + 3], nz)));
                heavy = most >= SPLIT_MIN_PLANES;
            }
            const unsigned long long m1 = __ballot(walk), m2 = __ballot(live && !walk), mh = __ballot(heavy);
            if (live) s_pos[k] = walk ? (nw + (unsigned)__popcll(m1 & below) + (unsigned)__popcll(mh & below)) | (heavy ? (unsigned)POS_SPLIT_BIT : 0u)
                                      : (unsigned)POS_OTHER_BIT | (no + (unsigned)__popcll(m2 & below));
            nw += (unsigned)__popcll(m1) + (unsigned)__popcll(mh); no += (unsigned)__popcll(m2);
        }
        if (tid == 0 && n) {
            const unsigned long long was = list_reserve(pair, nw, no);
            s_base[0] = (unsigned)was; s_base[1] = (unsigned)(was >> 32);
        }
    }
    __syncthreads();
    for (unsigned i = tid; i < n * BOXES_PER_BRICK; i += blockDim.x) {
        const unsigned k = i / BOXES_PER_BRICK, r = s_pos[k];
        const unsigned pos = (r >> 31) ? a.list_cap - 1u - (s_base[1] + (r & 0x7fffffffu)) : s_base[0] + (r & ~(unsigned)POS_SPLIT_BIT);
        const unsigned word = s_word[i] & 0x7fffffffu;
        if ((r >> 31) == 0u && (r & POS_SPLIT_BIT)) {
            const int nz = min(a.brick_z, a.z1 - (a.z0 + (s_brick[k] >> 20) * a.brick_z));
            const int wk = box_walked_planes(word, nz), h = wk >> 1;
            a.box_class[(size_t)pos * BOXES_PER_BRICK + i % BOXES_PER_BRICK] = word + ((unsigned)h << 8);             // the second entry's planes: not this one's
            a.box_class[(size_t)(pos + 1u) * BOXES_PER_BRICK + i % BOXES_PER_BRICK] =
                ((word & ~(0xffu | BOX_EDGE_BIT | BOX_SPECKLE_BIT)) | ((word & 0xffu) + (unsigned)(wk - h))) | BOX_NO_STREAM_BIT;
            if (i % BOXES_PER_BRICK == 0) { region[pos] = s_brick[k]; region[pos + 1u] = s_brick[k]; }
            continue;
        }
        a.box_class[(size_t)pos * BOXES_PER_BRICK + i % BOXES_PER_BRICK] = word;
        if (i % BOXES_PER_BRICK == 0) region[pos] = s_brick[k];
    }
}

// The boxes' classes for the list k_classify_bricks left (the primary pair and region), and the list again in the order
// k_integrate_bricks takes it (the second pair and region: ord).  Eight lanes per box, 8 bricks per workgroup and trip; a reservation
// per 8 bricks while the launch is small, per ORDER_BATCH = 32 beyond (S2's 23 000 bricks then take 720 atomics instead of 2 900; ~12 ns each on one
// address).  Batches are runs of list neighbours and arrive roughly in list order, so each run of the ordered list keeps the plane order
// of the first — which matters: the same bricks dealt round the workgroups of a fused kernel (frustum test + classes in one launch, no
// faster: 12.5 us against 3.8 + 8.4) came out in an order that made the S2 launch 9 % slower (profiles/r04_ab_classify_fused.txt).
// The second pair is zero when the kernel starts (the launcher clears it).
struct BoxOrder { int *list; };
#ifndef XS_SPLIT_HEAVY
#define XS_SPLIT_HEAVY 1
#endif
#ifndef XS_ORDER_BATCH
#define XS_ORDER_BATCH 32   // bricks per reservation beyond 4 096 listed ones.  A workgroup takes its batch in rounds of 8 bricks (8 lanes per box, 4 boxes): 64
                            // was eight dependent rounds (18 us at 1024^3's 12.5 K bricks), 32 is four — 1024^3 tracking +0.5-1 %, scene S2's whole call
                            // 0.173 -> 0.169 ms; 16 doubles the same-address atomics again and loses (profiles/r05_ab_order_batch.txt)
#endif
enum { ORDER_BATCH = XS_ORDER_BATCH };
// (1 024-thread workgroups — a batch of 32 in ONE round — measured 14.5 us against 15.1 at 1024^3: the rounds are not what the kernel waits for.)
__global__ void __launch_bounds__(256) k_classify_boxes(const IntegrateArgs a, const BoxSlack sl, const BoxOrder ord) {
    const unsigned nwalk = a.brick_count[PAIR_PRIMARY], count = nwalk + a.brick_count[PAIR_PRIMARY + 1];
    const int tid = (int)threadIdx.x, corner = tid & 7, box = (tid >> 3) & (BOXES_PER_BRICK - 1), slot = tid >> 5;
    __shared__ unsigned s_word[ORDER_BATCH * BOXES_PER_BRICK], s_pos[ORDER_BATCH], s_base[2];
    __shared__ int s_brick[ORDER_BATCH];
    const unsigned batch = count <= 4096u ? 8u : (unsigned)ORDER_BATCH;
    // (a launch that small has every brick resident at once and lasts as long as its longest wave: list_append, "a brick in TWO entries";
    // a brick with >= SPLIT_MIN_PLANES >= 6 planes leaves room for both entries in a region laid out for 2-plane bricks)
    const bool split = XS_SPLIT_HEAVY != 0 && count <= 4096u && a.brick_z >= SPLIT_MIN_PLANES && SPLIT_MIN_PLANES >= 4;
    for (unsigned e0 = blockIdx.x * batch; e0 < count; e0 += gridDim.x * batch) {
        const unsigned n = min(batch, count - e0);
        for (unsigned r = 0; r < n; r += 8u) {
            const unsigned k = r + slot;
            if (k >= n) continue;    // (whole groups of 32 lanes)
            const int b = a.brick_list[list_at(e0 + k, nwalk, a.list_cap)];
            const unsigned word = classify_brick_boxes(a, sl, b, box, corner);
            if (corner == 0) {
                s_word[k * BOXES_PER_BRICK + box] = word;
                if (box == 0) s_brick[k] = b;
            }
        }
        __syncthreads();
        list_append(a, a.brick_count + PAIR_SECOND, ord.list, n, s_brick, s_word, s_pos, s_base, split);
        __syncthreads();
    }
}

extern "C" size_t xs_integrate_workspace_bytes(const int *res, int nz) {
    if (!res || nz <= 0) return 0;
    return workspace_order_offset(res, nz) + ((workspace_bricks(res, nz) * sizeof(int) + 255) & ~(size_t)255);
}

// ---- classes ahead: the records of struct ClassesAhead (xs_integrate_boxes.h), process-wide ---------------------------------------------
namespace {
std::mutex g_ca_mu;
ClassesAhead g_ca_tab[16];
int g_ca_n = 0, g_ca_next = 0;
void classes_ahead_forget(const void *workspace) {
    std::lock_guard<std::mutex> lk(g_ca_mu);
    for (int i = 0; i < g_ca_n; ++i) if (g_ca_tab[i].workspace == workspace) g_ca_tab[i].workspace = nullptr;
}
void classes_ahead_put(const ClassesAhead &r) {
    std::lock_guard<std::mutex> lk(g_ca_mu);
    for (int i = 0; i < g_ca_n; ++i) if (g_ca_tab[i].workspace == r.workspace || g_ca_tab[i].workspace == nullptr) { g_ca_tab[i] = r; return; }
    if (g_ca_n < 16) { g_ca_tab[g_ca_n++] = r; return; }
    g_ca_tab[g_ca_next] = r; g_ca_next = (g_ca_next + 1) % 16;   // (more than 16 workspaces with classes pending: the oldest record goes — its call classifies again)
}
}  // namespace
bool xs::classes_ahead_take(const void *workspace, ClassesAhead &out) {   // the record is consumed
    std::lock_guard<std::mutex> lk(g_ca_mu);
    for (int i = 0; i < g_ca_n; ++i)
        if (g_ca_tab[i].workspace == workspace) { out = g_ca_tab[i]; g_ca_tab[i].workspace = nullptr; return true; }
    return false;
}

/* The two tiny launches xs_integrate_scaled wraps around its kernels, for a caller that takes them off its critical path
 * (xs_integrate_scaled_ex with XS_INTEGRATE_HEADER_IS_CLEAR | XS_INTEGRATE_NO_FOLD): the clear of the workspace's 256-byte
 * header (brick count + update-count slots) before the classification, and the fold of the update-count slots into
 * updated_dev after the integrate kernel. */
extern "C" int xs_integrate_workspace_clear(void *workspace, void *stream) {
    if (!workspace) return xs_set_error(hipErrorInvalidValue, "xs_integrate_workspace_clear: null pointer");
    XS_CHECK(hipMemsetAsync(workspace, 0, WS_LIST_OFFSET, (hipStream_t)stream));
    return 0;
}
// What a pose whose box classes a list classified with slack_scale still holds for may differ by from the list's pose, in camera-frame
// metres anywhere in the volume.  Sideways (X, Y) as much as the frustum planes' extra slack lets a pose move (2e-3 of the coordinate
// magnitudes per unit of slack_scale, doubled: 4.4 cm for the benchmark volume at slack 2 — the last ICP update of a scene that slides,
// like S1 along its wall, is centimetres): that only widens a box's pixel range (~8 px at 2.5 m).  Along the viewing axis (C) a third of
// it (6.6 mm): that one thickens the band round every surface in which boxes take the per-voxel walk.  xs_integrate_list_covers
// checks a pose against exactly these (bit 1 of its result).
static BoxSlack box_slack(const IntegrateArgs &a, float slack_scale) {
    const float vs = a.voxel_size, ext = (float)std::max(a.X, std::max(a.Y, a.Z));
    auto mag = [&](const cfloat3 &row, float t) { return fabsf(t) + (fabsf(row.x.re) + fabsf(row.y.re) + fabsf(row.z.re)) * vs * ext; };
    const float k = 2e-3f * (slack_scale - 1.0f);
    static const float lateral = exp_env_float("XS_BOX_SLACK_LATERAL", 2.0f);   // (tuning aids of an XS_EXPERIMENTS build: xs_env.h)
    static const float axial = exp_env_float("XS_BOX_SLACK_AXIAL", 0.3f);
    BoxSlack sl;
    sl.dX = lateral * k * mag(a.R.data[0], a.t.x.re); sl.dY = lateral * k * mag(a.R.data[1], a.t.y.re); sl.dC = axial * k * mag(a.R.data[2], a.t.z.re);
    return sl;
}
// largest camera-frame coordinate difference between two poses over the volume's voxels, per axis
static void pose_delta(const IntegrateArgs &l, const IntegrateArgs &f, const int *res, double d[3]) {
    const cfloat3 *lr = l.R.data, *fr = f.R.data;
    const float lt[3] = {l.t.x.re, l.t.y.re, l.t.z.re}, ft[3] = {f.t.x.re, f.t.y.re, f.t.z.re};
    for (int r = 0; r < 3; ++r)
        d[r] = fabs((double)lt[r] - ft[r]) + (fabs((double)lr[r].x.re - fr[r].x.re) * res[0] + fabs((double)lr[r].y.re - fr[r].y.re) * res[1] +
                                               fabs((double)lr[r].z.re - fr[r].z.re) * res[2]) * (double)l.voxel_size;
}
bool xs::box_slack_covers(const IntegrateArgs &l, const IntegrateArgs &f, const int *res, float slack_scale) {
    const BoxSlack sl = box_slack(l, slack_scale);
    double d[3];
    pose_delta(l, f, res, d);
    return d[0] <= 0.9 * sl.dX && d[1] <= 0.9 * sl.dY && d[2] <= 0.9 * sl.dC;   // (a tenth left for the float evaluation on the device)
}
// k_classify_boxes for the list that is there (the primary one): classes and order go to the second pair and region, which a then names.
// done: completion event to ride on the dispatch, or null.
static bool box_classes_for(IntegrateArgs &a, const int *res, int nz, void *workspace, const DepthTile *tiles, const BoxSlack &sl, hipStream_t st,
                            bool second_pair_is_clear, hipEvent_t done) {
    if (!tiles) return false;
    a.dt = depth_tiles_view(tiles, a.drows, a.dcols);
    bind_classes(a, res, nz, workspace);
    // (a list classed a second time — XS_INTEGRATE_RECLASSIFY_BOXES — finds the first classification's counts there; behind a header clear the pair is zero)
    // (... and its class counters: words CLASS_COUNT_WORD .. + 6 hold the counters, the second pair between them — one fill)
    if (!second_pair_is_clear && hipMemsetAsync(a.brick_count + CLASS_COUNT_WORD, 0, 8 * sizeof(unsigned), st) != hipSuccess) return false;
    const int nb = a.bricks_x * a.bricks_y * a.bricks_z;
    BoxOrder ord;
    ord.list = reinterpret_cast<int *>((char *)workspace + workspace_order_offset(res, nz));
    const dim3 grid(div_up(nb, 8) < 2048 ? div_up(nb, 8) : 2048);
    if (done) hipExtLaunchKernelGGL(k_classify_boxes, grid, dim3(256), 0, st, nullptr, done, 0, a, sl, ord);
    else hipLaunchKernelGGL(k_classify_boxes, grid, dim3(256), 0, st, a, sl, ord);
    a.brick_list = ord.list; a.pair_word = PAIR_SECOND;
    return true;
}
// The classification of a launch (header clear): the bricks against the frustum, then — with a tile table — their boxes' classes and the
// list in order; true = a.box_class is being written.  done: completion event to ride on the last dispatch, or null.
static bool classification_for(IntegrateArgs &a, const int *res, int nz, void *workspace, const DepthTile *tiles, const BoxSlack &sl, hipStream_t st,
                               hipEvent_t done) {
    const int nb = a.bricks_x * a.bricks_y * a.bricks_z;
    if (done && !tiles) hipExtLaunchKernelGGL(k_classify_bricks, dim3(div_up(nb, CLASSIFY_BRICKS_BLOCK)), dim3(CLASSIFY_BRICKS_BLOCK), 0, st, nullptr, done, 0, a);
    else hipLaunchKernelGGL(k_classify_bricks, dim3(div_up(nb, CLASSIFY_BRICKS_BLOCK)), dim3(CLASSIFY_BRICKS_BLOCK), 0, st, a);
    return box_classes_for(a, res, nz, workspace, tiles, sl, st, true, done);
}
// ... and the two as the integrate call launches them: with its own pose — no slack — and no event
bool xs::launch_box_classes(IntegrateArgs &a, const int *res, int nz, void *workspace, const DepthTile *tiles, hipStream_t st) {
    return box_classes_for(a, res, nz, workspace, tiles, BoxSlack{0.f, 0.f, 0.f}, st, false, nullptr);
}
bool xs::launch_classification(IntegrateArgs &a, const int *res, int nz, void *workspace, const DepthTile *tiles, hipStream_t st) {
    return classification_for(a, res, nz, workspace, tiles, BoxSlack{0.f, 0.f, 0.f}, st, nullptr);
}
/* The brick classification of an integrate call on its own, for a pose that is only NEARLY the one the call will be made with — the
 * orchestrator enqueues it behind the last ICP launch, with the pose that launch started from, so that the list is there when the
 * final pose is: the launch latency of the classification (and half of the integrate kernel's) leaves the frame's critical path.
 * The frustum's slack is multiplied by slack_scale (> 1): the list then holds every brick any pose covered by
 * xs_integrate_list_covers(..., this pose, slack_scale, that pose) would list.  Clears the workspace header first unless flags has
 * XS_INTEGRATE_HEADER_IS_CLEAR.  Follow with xs_integrate_scaled_ex(..., XS_INTEGRATE_LIST_IS_READY | XS_INTEGRATE_HEADER_IS_CLEAR, ...)
 * on the same stream, workspace, volume slab and image size.  No synchronisation. */
extern "C" int xs_integrate_classify(int rows, int cols, const float *intr4, const int *res, float voxel_size, const float *Rv2c18, const float *tv2c6,
                                     float tranc_dist, int z0, int z1, const float *depth_max_dev, void *workspace, float slack_scale, unsigned flags,
                                     void *stream) {
    xs_integrate_opts o = {};   // the plain entry point: the list alone (no tile table: the integrate call decides the boxes itself)
    o.struct_bytes = sizeof(o); o.flags = flags;
    return xs_integrate_classify_ex(rows, cols, intr4, res, voxel_size, Rv2c18, tv2c6, tranc_dist, z0, z1, depth_max_dev, workspace, slack_scale, &o, stream);
}
extern "C" int xs_integrate_classify_ex(int rows, int cols, const float *intr4, const int *res, float voxel_size, const float *Rv2c18, const float *tv2c6,
                                        float tranc_dist, int z0, int z1, const float *depth_max_dev, void *workspace, float slack_scale,
                                        const xs_integrate_opts *opts, void *stream) {
    if (!opts || opts->struct_bytes != sizeof(xs_integrate_opts)) return xs_set_error(hipErrorInvalidValue, "xs_integrate_classify_ex: opts->struct_bytes is not sizeof(xs_integrate_opts)");
    const unsigned flags = opts->flags;
    const DepthTile *depth_tiles = static_cast<const DepthTile *>(opts->depth_tiles);
    if (!intr4 || !res || !Rv2c18 || !tv2c6 || !workspace || !(slack_scale >= 1.0f))
        return xs_set_error(hipErrorInvalidValue, "xs_integrate_classify: bad argument");
    if (z0 < 0 || z1 > res[2] || z1 <= z0 || res[0] <= 0 || res[1] <= 0) return xs_set_error(hipErrorInvalidValue, "xs_integrate_classify: bad slab");
    IntegrateArgs a;
    integrate_args(a, rows, cols, intr4, res, voxel_size, Rv2c18, tv2c6, tranc_dist, z0, z1, depth_max_dev);
    if (!(a.bricks_x <= 1024 && a.bricks_y <= 1024 && a.bricks_z <= 2047)) return xs_set_error(hipErrorInvalidValue, "xs_integrate_classify: volume too large for the brick list");
    for (int p = 0; p < 6; ++p) a.fr.slack[p] *= slack_scale;
    bind_workspace(a, res, z1 - z0, workspace);
    hipStream_t st = (hipStream_t)stream;
    if (!(flags & XS_INTEGRATE_HEADER_IS_CLEAR)) XS_CHECK(hipMemsetAsync(a.brick_count, 0, WS_LIST_OFFSET, st));
    // the boxes' classes, valid for every pose xs_integrate_list_covers accepts for this list (needs the frame's tile table:
    // opts->depth_tiles; without it the integrate call classifies with its own pose)
    static const bool env_no_tiles = exp_env_set("XS_INTEGRATE_NO_TILES");
    classes_ahead_forget(workspace);
    // (the 32-bit-offset condition on the tightest pitch: the integrate call tests the real one and decides the boxes itself when it disagrees)
    const bool off32 = ((size_t)a.brick_z * a.Y + BRICK_Y) * ((size_t)res[0] * 4) < (1ull << 32);
    const bool boxes = !env_no_tiles && !(flags & XS_INTEGRATE_NO_TILES) && off32 && depth_tiles;
    if (flags & XS_INTEGRATE_COUNT_CLASSES) a.kflags |= KF_COUNT_CLASSES;
    // (the caller's completion event — opts->stop_event — rides on the dispatch)
    if (classification_for(a, res, z1 - z0, workspace, boxes ? depth_tiles : nullptr, box_slack(a, slack_scale), st, (hipEvent_t)opts->stop_event)) {
        ClassesAhead r;
        r.workspace = workspace; r.tiles = depth_tiles; r.slack_scale = slack_scale; r.voxel_size = voxel_size; r.tranc_dist = tranc_dist;
        memcpy(r.R18, Rv2c18, sizeof(r.R18)); memcpy(r.t6, tv2c6, sizeof(r.t6)); memcpy(r.intr, intr4, sizeof(r.intr)); memcpy(r.res, res, sizeof(r.res));
        r.z0 = z0; r.z1 = z1; r.rows = rows; r.cols = cols;
        classes_ahead_put(r);
    }
    XS_CHECK(hipGetLastError());
    return 0;
}
/* Host only: 1 if a list classified with (Rv2c18_list, tv2c6_list, slack_scale) holds every brick the classification of
 * (Rv2c18, tv2c6) with the standard slack would — each half-space of the second pose, anywhere in the volume, lies inside the
 * first one's widened half-space — else 0 (then classify again: xs_integrate_scaled_ex without XS_INTEGRATE_LIST_IS_READY). */
extern "C" int xs_integrate_list_covers(int rows, int cols, const float *intr4, const int *res, float voxel_size, const float *Rv2c18_list,
                                        const float *tv2c6_list, float slack_scale, const float *Rv2c18, const float *tv2c6) {
    if (!intr4 || !res || !Rv2c18_list || !tv2c6_list || !Rv2c18 || !tv2c6) return 0;
    IntegrateArgs l, f;
    integrate_args(l, rows, cols, intr4, res, voxel_size, Rv2c18_list, tv2c6_list, 1.0f, 0, res[2], nullptr);
    integrate_args(f, rows, cols, intr4, res, voxel_size, Rv2c18, tv2c6, 1.0f, 0, res[2], nullptr);
    for (int p = 0; p < 6; ++p) {
        // a brick passes plane p when max over the brick of (alpha + b . index) >= -1.5 slack (box_may_pass); the two maxima differ
        // by at most the largest pointwise difference of the two affine forms over the volume
        const double d = fabs((double)l.fr.alpha[p] - f.fr.alpha[p]) + fabs((double)l.fr.bx[p] - f.fr.bx[p]) * res[0] +
                         fabs((double)l.fr.by[p] - f.fr.by[p]) * res[1] + fabs((double)l.fr.bz[p] - f.fr.bz[p]) * res[2];
        const double room = 1.5 * ((double)slack_scale * l.fr.slack[p] - f.fr.slack[p]);
        if (!(d <= 0.9 * room)) return 0;   // (a tenth of the room left for the kernel's float evaluation of the forms)
    }
    const bool tested_ok = !(f.kflags & KF_NO_TESTED_STREAM) || (l.kflags & KF_NO_TESTED_STREAM);   // (stream_margins: EDGE / SPECKLE classes need the final pose to allow them)
    return box_slack_covers(l, f, res, slack_scale) && tested_ok ? 3 : 1;   // bit 1: the boxes' classes hold for the pose too
}
