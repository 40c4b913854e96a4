// xs_raycast.hip — volume raycast for gfx950.  Replaces XKinectFusion/src/RayCaster.cu:26-141
// (RayCaster fields, get_ray_next, checkInds, readTsdf, getVoxel, interpolateTrilineary),
// :197-310 (operator()), :324 (rayCastKernel), :327-368 (raycast launcher).
//
// One ray per lane; a wave covers an 8x8 pixel tile and a workgroup a 16x16 tile, so the
// voxels a wave touches while marching stay within a few cache lines of each other (the march
// is a chain of dependent gathers: L2/latency-bound, not HBM-bound).  Only the real part of
// the position feeds the fixed-step march (RayCaster.cu:236-247), so the march reads the
// value volume alone and in real arithmetic — the same float operations the reference's
// real(ray_start + ray_dir * t) performs; the gradient volume is read only at the crossing,
// where the 2 + 6 trilinear samples run in complex arithmetic.
//
// In file order: Vol (the volume, its trilinear samples); the pieces of k_raycast as a ray meets them — wave_tile, signmap_iterations
// (the wave's iteration mask), ray_setup, crossing; the march: march_gather and march_events, one eight-step batch for the plain and the
// slab kind alike, plain_batch / slab_batch on top of them, signmap_march (the one loop that jumps over what the sign map clears),
// plain_march / slab_march; tile_pyramid and count_hits; k_raycast itself, a dispatcher over RayMode; the launchers with what they
// share (raycast_common_args, raycast_bind_signmap, raycast_instance); the composite kernels.
#include <hip/hip_ext.h>
#include "xs_device.h"
#include "xs_env.h"
#include "xs_signmap.h"
#include "xs_pyramid.h"
#include <type_traits>
#include "../../include/xslam_amd.h"

using namespace xs;
xs::ConstDiv xs_const_div_get(float c);   // xs_constdiv.hip

struct RaycastArgs {
    MatS33 Rc2v; cfloat3 tc2v; MatS33 Rv2w; cfloat3 tv2w;
    int X, Y, Z;
    float voxel_size, time_step;
    float inv_vs_lo, inv_vs_hi;  // 1/voxel_size nudged 4 ulp down / up (march index shortcut when the constant is not prepared)
    ConstDiv dv;                 // division by voxel_size (xs_const_div_prepare)
    int cols, rows;
    const float *value; const float *grad; size_t vstep;
    Intr intr;
    cfloat *vmap; cfloat *nmap; size_t mstep;
    int zs0, zs1;  // z planes resident behind value/grad: storage starts at plane zs0 (whole volume: 0, Z)
    int z0, z1;    // z planes this launch owns (slab mode): only steps whose sample lands here are evaluated
    int wshift;    // log2 of the wave's pixel-tile width (tile = 2^wshift x 64/2^wshift pixels)
    float *cross_t; // two-kernel path: per pixel, the march time of the step before the crossing (or < 0)
    int *keys;     // slab mode: per pixel, (step << 1 | no_hit) of the first event among owned steps, INT_MAX if none
    unsigned long long *hits;
    int *steps;    // optional (measurement): per pixel, the march iterations the reference's loop (RayCaster.cu:222-247) runs for this ray
    SignMap sm;    // sm.dil != null (the march kernels): evaluate only the iterations the sign map leaves (xs_signmap.h)
    float sm_dt; int sm_rounds;   // sign map: spacing of the per-wave samples along the tile's centre ray; 64 * sm_rounds of them
    PyramidArgs pyr;              // pyr.mid[0] != null (the fused one-launch form): every workgroup also builds levels 1 and 2 of both maps under its own tile
};

namespace {
__device__ __forceinline__ int sgn(float v) { return (0.0f < v) - (v < 0.0f); }

// floor(fl(p / vs)) — getVoxel, RayCaster.cu:80-86 — without the IEEE divide: the two products bracket
// fl(p / vs) (the reciprocals are 4 ulp either side of 1/vs), so when their floors agree that is the
// answer; otherwise (the quotient lies within ~8 ulp of an integer, ~1e-4 of the samples) the
// divide is done.
template <bool SHORT>
__device__ __forceinline__ int voxel_index(float p, float vs, float r_lo, float r_hi, const ConstDiv &dv) {
    // SHORT (the march kernels, when xs_const_div_prepare has checked voxel_size over all 2^32 operands): the exact short division,
    // six branch-free instructions; else two reciprocal products that bracket the quotient, with the divide where they disagree.
    // (Measured, round 3: march 48-51 us against 52-53; the crossing kernel and the integrate band keep their IEEE divides — the
    // compiler hoists the divisor's half of that sequence (v_rcp, v_div_scale, refinement) out of the loop as the divisor is a launch
    // constant, so a divide costs ~6 instructions there, and the short form made the crossing 8-18 % SLOWER: profiles/r03_ab_const_div.txt)
    if (SHORT) return floor_div_by<true>(p, dv);
    const int f_lo = cvt_floor(p * r_lo), f_hi = cvt_floor(p * r_hi);
    if (__builtin_expect(f_lo == f_hi, 1)) return f_lo;
    return __float2int_rd(p / vs);
}

// OFF32: the resident planes of one array span at most 4 GiB, so a voxel's byte offset fits 32 bits
// (two 24-bit multiply-adds and a shift instead of 64-bit multiplies; the load takes a scalar base +
// 32-bit lane offset).  The kernels are VALU-bound: the march spends a fifth of its instructions on
// addresses otherwise.
template <bool OFF32>
struct Vol {
    const float *value; const float *grad; size_t vstep; int X, Y, Z; float vs; int zs0, zs1;
    __device__ __forceinline__ unsigned offset32(int x, int y, int z) const {
        const unsigned row = __umul24((unsigned)(z - zs0), (unsigned)Y) + (unsigned)y;  // < 2^24 for every supported volume
        return (__umul24(row, (unsigned)(vstep >> 2)) + (unsigned)x) << 2;
    }
    __device__ __forceinline__ float value_at(unsigned off) const { return *reinterpret_cast<const float *>(reinterpret_cast<const char *>(value) + off); }
    __device__ __forceinline__ float load_value(int x, int y, int z) const {
        if (OFF32) return *reinterpret_cast<const float *>(reinterpret_cast<const char *>(value) + offset32(x, y, z));
        return row_ptr(value, vstep, Y * (z - zs0) + y)[x];
    }
    __device__ __forceinline__ float read_value(int x, int y, int z) const { return load_value(x, y, z) + 1e-5f; }  // RayCaster.cu:76
    __device__ __forceinline__ cfloat read(int x, int y, int z) const {  // readTsdf, :69-78
        // readTsdf wraps its indices with % resolution; every caller here passes 0 <= index < resolution
        // (interp() rejects cells outside [1, N-2] before touching the +1 neighbours), where the wrap is
        // the identity — and an integer modulo by a run-time value costs ~35 VALU ops, 192 of them per hit
        z = min(max(z, zs0), zs1 - 1);  // stay inside the resident planes (a no-op unless a slab's halo were too thin)
        cfloat r;
        if (OFF32) {
            const unsigned off = offset32(x, y, z);
            r = unpack_tsdf(*reinterpret_cast<const float *>(reinterpret_cast<const char *>(value) + off),
                            *reinterpret_cast<const float *>(reinterpret_cast<const char *>(grad) + off));
        } else
            r = unpack_tsdf(row_ptr(value, vstep, Y * (z - zs0) + y)[x], row_ptr(grad, vstep, Y * (z - zs0) + y)[x]);
        r += 1e-5f;
        return r;
    }
    // interpolateTrilineary, :99-141, in two halves: the cell a sample falls into with its three weights, and the blend of the
    // cell's eight corners.  A sample outside [1, N-2] is NaN; its cell is a resident one instead, for callers that load first
    // and look at `ok` afterwards (interp2).
    struct Cell { int gx, gy, gz; bool ok; cfloat a0, b0, c0; };
    __device__ __forceinline__ Cell locate(const cfloat3 &p) const {
        Cell c;
        int gx = __float2int_rd(p.x.re / vs), gy = __float2int_rd(p.y.re / vs), gz = __float2int_rd(p.z.re / vs);
        c.ok = !(gx <= 0 || gx >= X - 1) && !(gy <= 0 || gy >= Y - 1) && !(gz <= 0 || gz >= Z - 1);
        const float vx = (gx + 0.5f) * vs, vy = (gy + 0.5f) * vs, vz = (gz + 0.5f) * vs;
        gx += -(sgn(vx - p.x.re) + 1) >> 1;
        gy += -(sgn(vy - p.y.re) + 1) >> 1;
        gz += -(sgn(vz - p.z.re) + 1) >> 1;
        c.a0 = (p.x - (gx + 0.5f) * vs) / vs;
        c.b0 = (p.y - (gy + 0.5f) * vs) / vs;
        c.c0 = (p.z - (gz + 0.5f) * vs) / vs;
        c.gx = c.ok ? gx : 0; c.gy = c.ok ? gy : 0; c.gz = c.ok ? gz : zs0;
        return c;
    }
    __device__ __forceinline__ cfloat blend(const Cell &c, const cfloat (&lo)[4], const cfloat (&hi)[4]) const {
        const cfloat one(1.0f, 0.0f);
        const cfloat a1 = one - c.a0, b1 = one - c.b0, c1 = one - c.c0;
        const cfloat r = lo[0] * a1 * b1 * c1 + lo[1] * a1 * b1 * c.c0 + lo[2] * a1 * c.b0 * c1 + lo[3] * a1 * c.b0 * c.c0 +
                         hi[0] * c.a0 * b1 * c1 + hi[1] * c.a0 * b1 * c.c0 + hi[2] * c.a0 * c.b0 * c1 + hi[3] * c.a0 * c.b0 * c.c0;
        return c.ok ? r : cfloat(qnan_f(), 0.f);
    }
    __device__ __forceinline__ cfloat interp(const cfloat3 &p) const {
        const Cell c = locate(p);
        if (!c.ok) return cfloat(qnan_f(), 0.f);
        cfloat lo[4], hi[4];
        read2(c.gx, c.gy + 0, c.gz + 0, lo[0], hi[0]); read2(c.gx, c.gy + 0, c.gz + 1, lo[1], hi[1]);
        read2(c.gx, c.gy + 1, c.gz + 0, lo[2], hi[2]); read2(c.gx, c.gy + 1, c.gz + 1, lo[3], hi[3]);
        return blend(c, lo, hi);
    }
    // Two samples at once: both cells are located first, then the sixteen 8-byte loads of the two go out together and the
    // two blends follow — one memory round trip where two calls of interp() make two (the crossing kernel is a chain of
    // eight dependent samples per pixel: Ft / Ftdt, then the three central differences of the normal).  Same values as
    // interp(p), interp(q): the loads of a sample outside go to a resident cell and are not used.
    __device__ __forceinline__ void interp2(const cfloat3 &p, const cfloat3 &q, cfloat &Fp, cfloat &Fq) const {
        const Cell cp = locate(p), cq = locate(q);
        cfloat lp[4], hp[4], lq[4], hq[4];
        read2(cp.gx, cp.gy + 0, cp.gz + 0, lp[0], hp[0]); read2(cp.gx, cp.gy + 0, cp.gz + 1, lp[1], hp[1]);
        read2(cp.gx, cp.gy + 1, cp.gz + 0, lp[2], hp[2]); read2(cp.gx, cp.gy + 1, cp.gz + 1, lp[3], hp[3]);
        read2(cq.gx, cq.gy + 0, cq.gz + 0, lq[0], hq[0]); read2(cq.gx, cq.gy + 0, cq.gz + 1, lq[1], hq[1]);
        read2(cq.gx, cq.gy + 1, cq.gz + 0, lq[2], hq[2]); read2(cq.gx, cq.gy + 1, cq.gz + 1, lq[3], hq[3]);
        Fp = blend(cp, lp, hp);
        Fq = blend(cq, lq, hq);
    }
    // read(x, y, z) and read(x + 1, y, z): the corners (gx, ·, ·) and (gx + 1, ·, ·) are neighbours in memory, one 8-byte load per array
    // fetches both (a global load needs 4-byte alignment only) — 8 address-unit trips per sample instead of 16
    __device__ __forceinline__ void read2(int x, int y, int z, cfloat &lo, cfloat &hi) const {
        struct __attribute__((packed, aligned(4))) pair { float a, b; };
        z = min(max(z, zs0), zs1 - 1);
        const pair *pv, *pg;
        if (OFF32) {
            const unsigned off = offset32(x, y, z);
            pv = reinterpret_cast<const pair *>(reinterpret_cast<const char *>(value) + off);
            pg = reinterpret_cast<const pair *>(reinterpret_cast<const char *>(grad) + off);
        } else {
            pv = reinterpret_cast<const pair *>(row_ptr(value, vstep, Y * (z - zs0) + y) + x);
            pg = reinterpret_cast<const pair *>(row_ptr(grad, vstep, Y * (z - zs0) + y) + x);
        }
        const pair v = *pv, g = *pg;
        lo = unpack_tsdf(v.a, g.a); lo += 1e-5f;
        hi = unpack_tsdf(v.b, g.b); hi += 1e-5f;
    }
};
}  // namespace

// What one launch of k_raycast does with its rays.  The values are the template arguments that traces and profiles/ show
// (k_raycast<0, true, true, true>), which is why MODE stays an int in the kernel's parameter list.  (1, a slab's whole ray in one
// kernel, is gone: nothing launched it.)
enum RayMode : int {
    RAY_WHOLE = 0,       // whole ray in one kernel: the march, then the crossing
    RAY_MARCH = 2,       // march only: records the march time of the step before the crossing
    RAY_CROSS = 3,       // crossing only (trilinear samples, vertex, normal) for the pixels RAY_MARCH marked
    RAY_SLAB_MARCH = 4,  // one rank's slab, march only (what xs_raycast_slab launches: eight waves per SIMD with eight gathers in flight, like RAY_MARCH)
    RAY_SLAB_CROSS = 5,  // one rank's slab, the crossing for the pixels RAY_SLAB_MARCH marked
};
// (crossing kernels: five waves per SIMD — a 640 x 480 frame is 4 800 waves on 1 024 SIMDs, all resident at once; the
// two-samples-per-round-trip form would otherwise take 104 registers, i.e. four)
#ifndef XS_RAYCAST_CROSS_WAVES
#define XS_RAYCAST_CROSS_WAVES 5
#endif
constexpr int raycast_min_waves(int mode, bool map) { return mode == RAY_CROSS || mode == RAY_SLAB_CROSS || (mode == RAY_WHOLE && map) ? XS_RAYCAST_CROSS_WAVES : 1; }
constexpr float MAX_TIME = 5.0f;   // the march runs while time_curr < MAX_TIME (RayCaster.cu:222)
constexpr int NS = 8;              // march steps per batch

namespace {
// lane -> pixel inside an 8x8 tile; 4 waves -> 16x16 tile per workgroup.  Workgroups are dealt
// round-robin over the 8 XCDs (each with its own 4 MB L2): the linear id is remapped so that
// XCD k marches one contiguous band of image tiles — an eighth of the frustum, which fits its
// L2 — instead of every XCD pulling every line.  Placement only affects speed.
struct Tile {
    int lane, wave, wx, wy;   // wave tile: wx x wy pixels; the workgroup covers 2 x 2 of them
    int tiles_x, tile;
    bool ok;                  // the workgroup has a tile at all (the grid is rounded up to the XCDs)
    int x0, y0, x, y;         // the wave tile's first pixel; this lane's
};
__device__ __forceinline__ Tile wave_tile(const RaycastArgs &a) {
    Tile t;
    t.lane = threadIdx.x & 63; t.wave = threadIdx.x >> 6;
    t.wx = 1 << a.wshift; t.wy = 64 >> a.wshift;
    t.tiles_x = (a.cols + 2 * t.wx - 1) / (2 * t.wx);
    const int tiles_y = (a.rows + 2 * t.wy - 1) / (2 * t.wy), ntiles = t.tiles_x * tiles_y;
    const int per_xcd = (ntiles + 7) / 8;
    t.tile = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    t.ok = t.tile < ntiles;
    t.x0 = (t.tile % t.tiles_x) * 2 * t.wx + (t.wave & 1) * t.wx;
    t.y0 = (t.tile / t.tiles_x) * 2 * t.wy + (t.wave >> 1) * t.wy;
    t.x = t.x0 + (t.lane & (t.wx - 1));
    t.y = t.y0 + (t.lane >> a.wshift);
    return t;
}

// MAP: which iterations of the reference's loop this wave's rays have to evaluate, as a wave-uniform bit mask (bit k = iteration k)
constexpr int UW = SIGNMAP_MAX_STEPS / 64;
struct Unsafe {
    unsigned long long w[UW];
    // first iteration >= k that has to be evaluated, or -1 (wave-uniform)
    __device__ __forceinline__ int next(int k) const {
        int r = -1;
#pragma unroll
        for (int i = UW - 1; i >= 0; --i) {
            const unsigned long long m = (k >> 6) < i ? w[i] : ((k >> 6) == i ? w[i] & (~0ull << (k & 63)) : 0ull);
            r = m ? 64 * i + (int)__builtin_ctzll(m) : r;
        }
        return r;
    }
};
__device__ __forceinline__ void signmap_iterations(const RaycastArgs &a, const Tile &tl, Unsafe &unsafe) {
    // Sign map, one pass per WAVE.  The 64 lanes sample the ray through the centre of the wave's pixel tile at t_i = 0.2 + i * dt — every
    // sample of the ray in one or two byte gathers from a table the L2 holds.  Every ray of the tile stays within t * delta of the
    // centre ray (delta: the tile's half diagonal in normalised image coordinates — normalising vectors of length >= 1 does not
    // stretch their difference), and the host chose dt with dt + (5.2 + dt) * delta <= 0.9 brick edges: every point any of the tile's
    // rays reaches at a parameter in [t_i, t_i + dt] lies in sample i's brick or one of its 26 neighbours, so a clear byte (xs_signmap.h)
    // says that no iteration whose sample falls into that stretch can see an event, on any of these rays.
    cfloat3 rc;
    rc.x = cfloat(((float)tl.x0 + 0.5f * (float)(tl.wx - 1) - a.intr.cx) / a.intr.fx);
    rc.y = cfloat(((float)tl.y0 + 0.5f * (float)(tl.wy - 1) - a.intr.cy) / a.intr.fy);
    rc.z = cfloat(1.f);
    const cfloat3 dc = normalized((a.Rc2v * rc + a.tc2v) - a.tc2v);
    const float inv_edge = 1.0f / (a.voxel_size * (float)(1 << a.sm.shift));
    unsigned long long flagged[2] = {~0ull, ~0ull};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h < a.sm_rounds) {
            const float tt = 0.2f + a.sm_dt * (float)(tl.lane + 64 * h);
            const int qx = cvt_floor((a.tc2v.x.re + dc.x.re * tt) * inv_edge), qy = cvt_floor((a.tc2v.y.re + dc.y.re * tt) * inv_edge),
                      qz = cvt_floor((a.tc2v.z.re + dc.z.re * tt) * inv_edge);
            const bool in = (unsigned)qx < (unsigned)a.sm.nx && (unsigned)qy < (unsigned)a.sm.ny && (unsigned)qz < (unsigned)a.sm.nz;
            const unsigned char f = a.sm.dil[in ? (qz * a.sm.ny + qy) * a.sm.nx + qx : 0];
            flagged[h] = __builtin_amdgcn_ballot_w64(!in || f);
        }
    }
    // Iteration k (lane k % 64 of word k / 64) samples the volume at parameter t[k + 1] and holds that sample against the one at t[k]
    // (the clamped start voxel for k = 0) — the table holds the reference's running float sum t[0] = 0.2, t[j + 1] = t[j] + time_step.
    // It is marked for evaluation when t[k + 1] lies in the stretch of a flagged sample (within 2 % of a stretch's end, of the
    // neighbouring one as well: the float error of the position is ~1e-6 of it) — and iteration 0 also when the start, t[0], does.
    // That alone would miss one event: the '- to +' that ends a march (RayCaster.cu:243) is decided by the PREVIOUS sample, and a ray
    // that leaves a negative region has t[k] flagged and t[k + 1] clear.  But then iteration k - 1 was evaluated and its sample — this
    // iteration's previous one — is in hand: the march does not jump while any of the wave's unfinished rays carries a negative value
    // out of a batch (signmap_march).  Every iteration that is jumped over therefore has a positive previous sample, which is what
    // the jump assumes.  (Marking every iteration whose t[k] OR t[k + 1] is flagged, the simpler static rule, costs one more
    // iteration behind every flagged run a ray leaves: raycast alone 42.2 us against 41.4, profiles/r04_ab_signmap_rule.txt.)
    const float inv_dt = 1.0f / a.sm_dt;
    auto is_set = [&](int i) -> bool {   // sample i flagged (or none such: beyond the samples taken)
        return (unsigned)i >= (unsigned)(64 * a.sm_rounds) || (((i < 64 ? flagged[0] : flagged[1]) >> (i & 63)) & 1ull) != 0ull;
    };
#pragma unroll
    for (int w = 0; w < UW; ++w) {
        const int k = 64 * w + tl.lane;
        if (64 * w <= a.sm.nt - 2) {   // (wave-uniform)
            const bool runs = k <= a.sm.nt - 2;   // iteration k runs while t[k] < max_time, i.e. k <= nt - 2
            auto flagged_at = [&](float tau) -> bool {
                const float xq = (tau - 0.2f) * inv_dt;
                const int i = cvt_floor(xq);
                const float fr = xq - (float)i;
                return is_set(i) || (fr < 0.02f && is_set(i - 1)) || (fr > 0.98f && is_set(i + 1));
            };
#if defined(XS_EXPERIMENTS) && defined(XS_SIGNMAP_BOTH)   // measurement only: the simpler static rule (see above)
            const bool uns = flagged_at(a.sm.t[runs ? k + 1 : 0]) || (k == 0 ? is_set(0) : flagged_at(a.sm.t[runs ? k : 0]));
#else
            const bool uns = flagged_at(a.sm.t[runs ? k + 1 : 0]) || (k == 0 && is_set(0));   // (t[0] = 0.2 is sample 0's own position)
#endif
            unsafe.w[w] = __builtin_amdgcn_ballot_w64(runs && uns);
        }
    }
}

// One pixel's ray in volume coordinates (get_ray_next, RayCaster.cu:44-52, and :206-220), and the clamped voxel of its start
struct Ray { int x, y; cfloat3 start, dir; int gx, gy, gz; };
__device__ __forceinline__ Ray ray_setup(const RaycastArgs &a, int x, int y) {
    Ray r;
    r.x = x; r.y = y;
    r.start = a.tc2v;
    cfloat3 rn;
    rn.x = cfloat((x - a.intr.cx) / a.intr.fx);
    rn.y = cfloat((y - a.intr.cy) / a.intr.fy);
    rn.z = cfloat(1.f);
    const cfloat3 ray_next = a.Rc2v * rn + a.tc2v;
    r.dir = normalized(ray_next - r.start);
    r.dir.x = (r.dir.x == 0.f) ? cfloat(1e-15f) : r.dir.x;
    r.dir.y = (r.dir.y == 0.f) ? cfloat(1e-15f) : r.dir.y;
    r.dir.z = (r.dir.z == 0.f) ? cfloat(1e-15f) : r.dir.z;
    const float vs = a.voxel_size, time_curr = 0.2f;
    r.gx = __float2int_rd((r.start.x.re + r.dir.x.re * time_curr) / vs);
    r.gy = __float2int_rd((r.start.y.re + r.dir.y.re * time_curr) / vs);
    r.gz = __float2int_rd((r.start.z.re + r.dir.z.re * time_curr) / vs);
    r.gx = max(0, min(r.gx, a.X - 1)); r.gy = max(0, min(r.gy, a.Y - 1)); r.gz = max(0, min(r.gz, a.Z - 1));
    return r;
}

// zero crossing between tc and tc + time_step (RayCaster.cu:247-306): returns 1 if a vertex was written.  PAIRS: the eight samples
// two at a time (interp2)
template <bool SLAB, bool PAIRS, bool OFF32>
__device__ __forceinline__ int crossing(const RaycastArgs &a, const Vol<OFF32> &vol, const Ray &r, float tc) {
    const int x = r.x, y = r.y;
    const float vs = a.voxel_size, tn = tc + a.time_step;
    cfloat Ftdt, Ft;
    if (PAIRS) {   // the crossing kernels: both samples in one round trip
        vol.interp2(r.start + r.dir * tn, r.start + r.dir * tc, Ftdt, Ft);
        if (isnan(Ftdt.re) || isnan(Ft.re)) return 0;
    } else {
        Ftdt = vol.interp(r.start + r.dir * tn);
        if (isnan(Ftdt.re)) return 0;
        Ft = vol.interp(r.start + r.dir * tc);
        if (isnan(Ft.re)) return 0;
    }
    const cfloat coef = Ft / (Ftdt - Ft);
    if (Ft.re < 0.0f || Ftdt.re > 0.0f) return 0;
    const cfloat Ts = tc - a.time_step * coef;
    const cfloat3 vertex_found = r.start + r.dir * Ts;
    const cfloat3 vw = a.Rv2w * vertex_found + a.tv2w;
    row_ptr(a.vmap, a.mstep, y)[x] = vw.x;
    row_ptr(a.vmap, a.mstep, y + a.rows)[x] = vw.y;
    row_ptr(a.vmap, a.mstep, y + 2 * a.rows)[x] = vw.z;
    const int vx = __float2int_rd(vertex_found.x.re / vs);
    const int vy = __float2int_rd(vertex_found.y.re / vs);
    const int vz = __float2int_rd(vertex_found.z.re / vs);
    if (SLAB) row_ptr(a.nmap, a.mstep, y)[x] = cfloat(qnan_f(), 0.f);  // until a normal is written
    if (vx > 1 && vy > 1 && vz > 1 && vx < a.X - 2 && vy < a.Y - 2 && vz < a.Z - 2) {
        cfloat3 t, n;
        const float half = vs * 0.5f;
        if (PAIRS) {
            cfloat3 u;
            cfloat F1, F2;
            // (one pair at a time: left to itself the scheduler issues all 48 loads of the six samples at once and
            // keeps their 96 values and 36 weights live — 284 registers, one wave per SIMD)
            t = vertex_found; t.x += half; u = vertex_found; u.x -= half; vol.interp2(t, u, F1, F2); n.x = F1 - F2;
            asm volatile("" : "+v"(n.x.re), "+v"(n.x.im) :: "memory");
            t = vertex_found; t.y += half; u = vertex_found; u.y -= half; vol.interp2(t, u, F1, F2); n.y = F1 - F2;
            asm volatile("" : "+v"(n.y.re), "+v"(n.y.im) :: "memory");
            t = vertex_found; t.z += half; u = vertex_found; u.z -= half; vol.interp2(t, u, F1, F2); n.z = F1 - F2;
        } else {
            t = vertex_found; t.x += half; const cfloat Fx1 = vol.interp(t);
            t = vertex_found; t.x -= half; const cfloat Fx2 = vol.interp(t);
            n.x = Fx1 - Fx2;
            t = vertex_found; t.y += half; const cfloat Fy1 = vol.interp(t);
            t = vertex_found; t.y -= half; const cfloat Fy2 = vol.interp(t);
            n.y = Fy1 - Fy2;
            t = vertex_found; t.z += half; const cfloat Fz1 = vol.interp(t);
            t = vertex_found; t.z -= half; const cfloat Fz2 = vol.interp(t);
            n.z = Fz1 - Fz2;
        }
        if (squarednorm(n).re == 0) return 1;
        const cfloat3 n_g = a.Rv2w * normalized(n);
        row_ptr(a.nmap, a.mstep, y)[x] = n_g.x;
        row_ptr(a.nmap, a.mstep, y + a.rows)[x] = n_g.y;
        row_ptr(a.nmap, a.mstep, y + 2 * a.rows)[x] = n_g.z;
    }
    return 1;
}

// ---- the march: eight steps at a time -------------------------------------------------------------------------------------------
// The sample positions do not depend on the loaded values, so a batch issues its eight steps together, straight-line (eight gathers in
// flight per lane instead of one dependent chain): positions, clamped (always valid) gathers, then event masks that are tested in
// order — the lowest set bit is the first event along the ray, whatever lies behind it is discarded; one branch per eight steps.  The
// times are the same float running sum the reference's one-step loop forms.
//
// Plain: a step out of range or past the end, - to + (no vertex), + to - (crossing).
// Slab: every rank walks the same steps and looks only at those whose sample voxel it owns; the sample before (at most 3 planes away)
// is in the halo it also stores.  Per step, in order: a sample outside the volume ends the march without an event; an owned step whose
// previous sample is not stored ends it with (step << 1 | 1) (never expected: halo too thin); - to + ends it with (step << 1 | 1);
// + to - ends it with a crossing for RAY_SLAB_CROSS to evaluate; any other owned step leaves "no event".
struct Gathered { float val[NS]; unsigned end, own, stored; };   // bit j: step j ends the march (outside, or past MAX_TIME); slab: its voxel is owned / stored by this rank
struct Events { unsigned thin, up, down; };                      // bit j: (slab) previous sample not stored; - to +; + to -
template <bool SLAB> struct Carry { float val; };                // the previous sample, as one batch hands it to the next
template <> struct Carry<true> { float val; bool stored; };      // slab: and whether this rank stores it
template <bool SLAB> __device__ __forceinline__ Carry<SLAB> carry_of(float val, bool stored) {
    Carry<SLAB> c;
    c.val = val;
    if constexpr (SLAB) c.stored = stored;
    return c;
}

// the eight samples behind time t (advanced past them: the running sum)
template <bool SLAB, bool OFF32, bool SHORT>
__device__ __forceinline__ Gathered march_gather(const RaycastArgs &a, const Vol<OFF32> &vol, const Ray &r, float &t) {
    Gathered g;
    g.end = g.own = g.stored = 0;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const float tn = t + a.time_step;
        const int jx = voxel_index<SHORT>(r.start.x.re + r.dir.x.re * tn, a.voxel_size, a.inv_vs_lo, a.inv_vs_hi, a.dv);
        const int jy = voxel_index<SHORT>(r.start.y.re + r.dir.y.re * tn, a.voxel_size, a.inv_vs_lo, a.inv_vs_hi, a.dv);
        const int jz = voxel_index<SHORT>(r.start.z.re + r.dir.z.re * tn, a.voxel_size, a.inv_vs_lo, a.inv_vs_hi, a.dv);
        // (one unsigned compare per axis; a step whose voxel is not read reads voxel (0, 0, first plane), always resident,
        // and its value is never looked at)
        const bool inb = (unsigned)jx < (unsigned)a.X && (unsigned)jy < (unsigned)a.Y && (unsigned)jz < (unsigned)a.Z;
        const bool runs = (t < MAX_TIME) && inb;
        const bool rd = SLAB ? inb && jz >= a.zs0 && jz < a.zs1 : runs;
        g.end |= (runs ? 0u : 1u) << j;
        if (SLAB) {
            g.own |= ((inb && jz >= a.z0 && jz < a.z1) ? 1u : 0u) << j;
            g.stored |= (rd ? 1u : 0u) << j;
        }
        if (OFF32) g.val[j] = vol.value_at(rd ? vol.offset32(jx, jy, jz) : 0u) + 1e-5f;
        else g.val[j] = vol.read_value(rd ? jx : 0, rd ? jy : 0, rd ? jz : a.zs0);
        t += a.time_step;
    }
    // (the own mask as one VGPR: when the compiler sees through it, the bits of own and stored stay sixteen lane masks in SGPR pairs
    // until the events are formed, and the slab marches go from 76-90 SGPRs to 102-106, one wave per SIMD less)
    if (SLAB) asm("" : "+v"(g.own));
    return g;
}
// the batch's events from the sample carried in; leaves the batch's last sample in c
template <bool SLAB>
__device__ __forceinline__ Events march_events(Carry<SLAB> &c, const Gathered &g) {
    Events m = {0u, 0u, 0u};
    float prev = c.val;
    bool prev_st = true;
    if constexpr (SLAB) prev_st = c.stored;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const bool o = SLAB ? (g.own >> j) & 1u : true;
        if (SLAB) m.thin |= ((o && !prev_st) ? 1u : 0u) << j;
        m.up |= ((o && prev_st && prev < 0.f && g.val[j] > 0.f) ? 1u : 0u) << j;
        m.down |= ((o && prev_st && prev > 0.f && g.val[j] < 0.f) ? 1u : 0u) << j;
        prev = g.val[j];
        if (SLAB) prev_st = (g.stored >> j) & 1u;
    }
    c = carry_of<SLAB>(prev, prev_st);
    return m;
}
// time_curr of step e of the batch that began at tb: the same e additions once more (once per ray — the batch does not keep its
// eight times in registers for this)
__device__ __forceinline__ float event_time(float tb, int e, float time_step) {
    float tce = tb;
    for (int j = 0; j < e; ++j) tce += time_step;
    return tce;
}

// One batch of the plain march from time t (advanced).  True when the march ends in it: `cross` is then time_curr of the first event's
// step if that is a crossing, and `ran` the number of the batch's iterations the reference's loop (RayCaster.cu:222-247) runs.
template <bool OFF32, bool SHORT>
__device__ __forceinline__ bool plain_batch(const RaycastArgs &a, const Vol<OFF32> &vol, const Ray &r, float &t, Carry<false> &c, float &cross, int &ran) {
    const float tb = t;
    const Gathered g = march_gather<false, OFF32, SHORT>(a, vol, r, t);
    const Events m = march_events<false>(c, g);
    const unsigned ev = g.end | m.down | m.up;
    ran = NS;
    if (!ev) return false;
    const int e = __ffs(ev) - 1;
    const float tce = event_time(tb, e, a.time_step);
    if (!((g.end >> e) & 1u) && ((m.down >> e) & 1u)) cross = tce;
    ran = e + (tce < MAX_TIME ? 1 : 0);   // the reference's loop runs iteration e of this batch unless its own condition (time_curr < max_time) ends it first
    return true;
}
// One batch of the slab march from time t (advanced), step0 the index of its first step.  True when the march ends in it: `key` is then
// (step << 1 | 1) of the event, and a crossing leaves (time of the step before it, marker 1) in the vertex map's x plane for RAY_SLAB_CROSS.
template <bool OFF32, bool SHORT>
__device__ __forceinline__ bool slab_batch(const RaycastArgs &a, const Vol<OFF32> &vol, const Ray &r, float &t, int step0, Carry<true> &c, int &key) {
    const float tb = t;
    const Gathered g = march_gather<true, OFF32, SHORT>(a, vol, r, t);
    const Events m = march_events<true>(c, g);
    const unsigned ev = g.end | m.thin | m.up | m.down;
    if (!ev) return false;
    const int e = __ffs(ev) - 1;
    if (!((g.end >> e) & 1u)) {
        key = ((step0 + e) << 1) | 1;
        if ((m.down >> e) & 1u) row_ptr(a.vmap, a.mstep, r.y)[r.x] = cfloat(event_time(tb, e, a.time_step), 1.0f);
    }
    return true;
}

// The march over the iterations the wave has to evaluate (signmap_iterations), eight at a time; stretches in between are jumped over.
// batch(k, c) evaluates iterations k .. k + 7 from the carried sample c — the times are the reference's own running sum from t[k] — and
// says whether the ray's march ended.  An iteration that is left out has its sample in a brick without negative voxels, so the value the
// reference carries out of it is positive: the first iteration behind a jump starts from "positive" (its magnitude never matters),
// iteration 0 from start(), the clamped start voxel as in the reference.  The '- to +' event is decided by the previous sample, so there
// is no jump while an unfinished ray of the wave carries a negative value out of a batch (its next iteration may be that exit).
// Slab: the map knows the negative voxels of the planes this rank stores — owned slab + halo, marked by its own integrate calls — and an
// iteration whose sample lies elsewhere is not this rank's to evaluate anyway.  Behind a jump the previous sample is taken as stored
// as well: it lies in a brick without negative voxels, within one step of an owned sample, i.e. inside the halo.
template <bool SLAB, class Start, class Batch>
__device__ __forceinline__ void signmap_march(const RaycastArgs &a, const Unsafe &unsafe, Start &&start, Batch &&batch) {
    int k = unsafe.next(0);
    Carry<SLAB> c = carry_of<SLAB>(1.0f, true);
    if (k == 0) c = start();
    bool done = false;
    while (k >= 0) {
        if (!done) done = batch(k, c);
        if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
        const bool inside = __builtin_amdgcn_ballot_w64(!done && c.val < 0.f) != 0ull;
        const int kn = inside ? (k + NS <= a.sm.nt - 2 ? k + NS : -1) : unsafe.next(k + NS);
        if (kn != k + NS) c = carry_of<SLAB>(1.0f, true);
        k = kn;
    }
}

// RAY_WHOLE / RAY_MARCH: the march, the crossing time for RAY_CROSS, or the crossing itself; returns 1 if a vertex was written
template <int MODE, bool OFF32, bool SHORT, bool MAP>
__device__ __forceinline__ unsigned plain_march(const RaycastArgs &a, const Vol<OFF32> &vol, const Ray &r, const Unsafe &unsafe) {
    float cross = -1.f;
    int nsteps = 0;   // iterations of the reference's loop (only stored when a.steps is given)
    auto start = [&]() { return carry_of<false>(vol.read_value(r.gx, r.gy, r.gz), true); };
    if (MAP) {
        nsteps = a.sm.nt - 1;   // (no event: the loop runs until its own condition ends it)
        signmap_march<false>(a, unsafe, start, [&](int k, Carry<false> &c) {
            float t = a.sm.t[k];
            int ran;
            const bool ended = plain_batch<OFF32, SHORT>(a, vol, r, t, c, cross, ran);
            if (ended) nsteps = k + ran;
            return ended;
        });
    } else {
        Carry<false> c = start();
        float t = 0.2f;
        bool done = false;
        while (!done && t < MAX_TIME) {
            int ran;
            done = plain_batch<OFF32, SHORT>(a, vol, r, t, c, cross, ran);
            nsteps += ran;
        }
    }
    unsigned hit = 0;
    if (MODE == RAY_WHOLE && cross >= 0.f) hit = crossing<false, MAP>(a, vol, r, cross);   // (behind the loop: the wave's hit lanes together)
    if (MODE == RAY_MARCH || (MAP && a.cross_t)) a.cross_t[r.y * a.cols + r.x] = cross;   // (the fused launch fills the workspace too: same contract)
    if (a.steps) a.steps[r.y * a.cols + r.x] = nsteps;
    return hit;
}
// RAY_SLAB_MARCH: returns the pixel's key, (step << 1 | 1) of the first event among this rank's steps or INT_MAX
template <bool OFF32, bool SHORT, bool MAP>
__device__ __forceinline__ int slab_march(const RaycastArgs &a, const Vol<OFF32> &vol, const Ray &r, const Unsafe &unsafe) {
    int key = 0x7fffffff;
    auto start = [&]() {
        const bool stored = r.gz >= a.zs0 && r.gz < a.zs1;
        return carry_of<true>(stored ? vol.read_value(r.gx, r.gy, r.gz) : 0.f, stored);
    };
    if (MAP) {
        signmap_march<true>(a, unsafe, start, [&](int k, Carry<true> &c) {
            float t = a.sm.t[k];
            return slab_batch<OFF32, SHORT>(a, vol, r, t, k, c, key);
        });
    } else {
        Carry<true> c = start();
        float t = 0.2f;
        bool done = false;
        for (int step = 0; !done && t < MAX_TIME; step += NS) done = slab_batch<OFF32, SHORT>(a, vol, r, t, step, c, key);
    }
    return key;
}

// what a pixel holds before its ray is cast
template <int MODE>
__device__ __forceinline__ void init_pixel(const RaycastArgs &a, int x, int y) {
    if (MODE == RAY_SLAB_MARCH) {
        // contributions of the ranks are added (as int32 bit patterns) after the first event
        // along each ray has been agreed on: start from all-zero entries
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            row_ptr(a.vmap, a.mstep, y + p * a.rows)[x] = cfloat(0.f, 0.f);
            row_ptr(a.nmap, a.mstep, y + p * a.rows)[x] = cfloat(0.f, 0.f);
        }
    } else if (MODE != RAY_CROSS && MODE != RAY_SLAB_CROSS) {
        row_ptr(a.vmap, a.mstep, y)[x] = cfloat(qnan_f(), 0.f);
        row_ptr(a.nmap, a.mstep, y)[x] = cfloat(qnan_f(), 0.f);
    }
}

// The model-map pyramid (resizeVMap / resizeNMap twice, KinectFusionReconstruction.cpp:272-277) of this workgroup's own tile: a
// level-2 pixel needs the 4 x 4 level-0 pixels under it, and the tile's origin and size are multiples of four — so the two
// halvings need nothing another workgroup writes, and the frame's tail loses a launch (~16 us: dispatch + a kernel that reads the
// maps back from memory).  The tile's vertices / normals went out with plain stores: once they have completed (release at
// workgroup scope + barrier) the lanes of wave 0 read them back through this CU's L1 / L2.  One lane per level-2 pixel and map,
// through the pyramid kernel's own function: the same values.
__device__ __forceinline__ void tile_pyramid(const RaycastArgs &a, const Tile &tl) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // level 1: the tile's 64 pixels of each map, one per lane of waves 0 and 1 (wave 0: vertices, wave 1: normals); their values
    // pass to level 2 through LDS: the 16 pixels of each map, one per lane of the first half of wave 0
    __shared__ cfloat3 s_l1[2][64];
    __shared__ unsigned char s_ok1[2][64];
    const int rows1 = a.pyr.rows0 / 2, cols1 = a.pyr.cols0 / 2;
    const int n1x = tl.wx;                                     // level-1 pixels per tile: (2 wx / 2) x (2 wy / 2) = wx x wy = 64
    const int x1o = (tl.tile % tl.tiles_x) * tl.wx, y1o = (tl.tile / tl.tiles_x) * tl.wy;   // the tile's first level-1 pixel
    if (tl.ok && threadIdx.x < 128) {
        const int m = (int)threadIdx.x >> 6, q = (int)threadIdx.x & 63;
        const int x1 = x1o + q % n1x, y1 = y1o + q / n1x;
        cfloat3 n;
        bool ok = false;
        if (x1 < cols1 && y1 < rows1) ok = m == 0 ? pyramid_level1_pixel<false>(a.pyr, 0, x1, y1, n) : pyramid_level1_pixel<true>(a.pyr, 1, x1, y1, n);
        if (ok) s_l1[m][q] = n;
        s_ok1[m][q] = ok ? 1 : 0;
    }
    __syncthreads();
    if (tl.ok && threadIdx.x < 32) {
        const int m = (int)threadIdx.x >> 4, r = (int)threadIdx.x & 15;
        const int n2x = n1x >> 1;
        const int lx = r % n2x, ly = r / n2x;                  // level-2 pixel inside the tile
        const int x2 = (x1o >> 1) + lx, y2 = (y1o >> 1) + ly;
        if (x2 < cols1 / 2 && y2 < rows1 / 2) {
            cfloat3 l1[4];
            bool ok[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int q = (2 * ly + (c >> 1)) * n1x + 2 * lx + (c & 1);
                ok[c] = s_ok1[m][q] != 0;
                if (ok[c]) l1[c] = s_l1[m][q];
            }
            if (m == 0) pyramid_level2_pixel<false>(a.pyr, 0, x2, y2, l1, ok);
            else pyramid_level2_pixel<true>(a.pyr, 1, x2, y2, l1, ok);
        }
    }
}
// one atomic per workgroup: same-address atomics cost ~12 ns each at the memory side, and one
// per wave (4800 of them) would by itself take longer than the kernel
__device__ __forceinline__ void count_hits(const RaycastArgs &a, const Tile &tl, unsigned hit) {
    __shared__ unsigned s_hits[4];
    const unsigned s = wave_sum_u32(hit);
    if (tl.lane == 0) s_hits[tl.wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = (s_hits[0] + s_hits[1]) + (s_hits[2] + s_hits[3]);
        if (t) atomicAdd(a.hits, (unsigned long long)t);
    }
}
}  // namespace

template <int MODE, bool OFF32, bool SHORT, bool MAP = false>   // MAP (RAY_WHOLE, RAY_MARCH, RAY_SLAB_MARCH): the march evaluates only the iterations the sign map (a.sm) leaves
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(raycast_min_waves(MODE, MAP)))) k_raycast(const RaycastArgs a) {
    constexpr bool SLAB = MODE == RAY_SLAB_MARCH || MODE == RAY_SLAB_CROSS;
    const Tile tl = wave_tile(a);
    unsigned hit = 0;
    // (the grid is rounded up to the XCDs: a workgroup may have no tile.  ONE test around the sign-map pass and the pixel's work: the
    // pass then dominates ray_setup, which reuses its products with Rc2v — tested separately, the fused kernel loads its arguments as
    // 16-dword tuples, spills 56 SGPRs instead of 15 and takes 44 us instead of 41: profiles/raycast_refactor_resources.txt)
    if (tl.ok) {
        Unsafe unsafe = {};
        if (MAP) signmap_iterations(a, tl, unsafe);
        if (tl.x < a.cols && tl.y < a.rows) {
            const int x = tl.x, y = tl.y;
            init_pixel<MODE>(a, x, y);
            const Vol<OFF32> vol{a.value, a.grad, a.vstep, a.X, a.Y, a.Z, a.voxel_size, a.zs0, a.zs1};
            const Ray r = ray_setup(a, x, y);
            if (MODE == RAY_CROSS) {
                const float tc = a.cross_t[y * a.cols + x];
                if (tc >= 0.f) hit = crossing<SLAB, true>(a, vol, r, tc);
            } else if (MODE == RAY_SLAB_CROSS) {
                // the slab march left (time of the step before the crossing, marker 1) in the vertex map's x plane where
                // this rank's first event is a + to - crossing, and the provisional key (step << 1 | 1)
                int key = a.keys[y * a.cols + x];
                const cfloat mark = row_ptr(a.vmap, a.mstep, y)[x];
                if (mark.im == 1.0f) {
                    row_ptr(a.vmap, a.mstep, y)[x] = cfloat(0.f, 0.f);
                    if (crossing<SLAB, true>(a, vol, r, mark.re)) { key = key & ~1; hit = 1; }
                }
                a.keys[y * a.cols + x] = key;   // (rewrites the key it read: even where the crossing gave a vertex)
            } else if (MODE == RAY_SLAB_MARCH)
                a.keys[y * a.cols + x] = slab_march<OFF32, SHORT, MAP>(a, vol, r, unsafe);
            else
                hit = plain_march<MODE, OFF32, SHORT, MAP>(a, vol, r, unsafe);
        }
    }
    if (MODE == RAY_WHOLE && a.pyr.mid[0]) tile_pyramid(a, tl);   // (the fused one-launch form)
    if (a.hits) count_hits(a, tl, hit);
}

static int ray_wshift() {
    static const int env_ws = exp_env_int("XS_RAY_WSHIFT", 3);
    return (env_ws >= 0 && env_ws <= 6) ? env_ws : 3;
}
// spacing of the per-wave sign-map samples (k_raycast, MAP): dt + (5.2 + dt) * delta <= 0.9 brick edges, delta = the pixel tile's half
// diagonal in normalised image coordinates (+ 1 %); at most two samples per lane must reach from t = 0.2 past max_time = 5
static bool sign_map_spacing(float fx, float fy, int wshift, float voxel_size, int shift, float &dt_out, int &rounds_out) {
    const float hx = 0.5f * (float)((1 << wshift) - 1) / fabsf(fx), hy = 0.5f * (float)((64 >> wshift) - 1) / fabsf(fy);
    const float delta = 1.01f * sqrtf(hx * hx + hy * hy) + 1e-6f, edge = voxel_size * (float)(1 << shift);
    const float dt = (0.9f * edge - 5.2f * delta) / (1.0f + delta);
    const int need = dt > 0.0f ? (int)ceilf(4.9f / dt) + 1 : 1 << 30;
    if (!(need <= 128)) return false;
    dt_out = dt; rounds_out = need <= 64 ? 1 : 2;
    return true;
}
extern "C" int xs_raycast_signmap_shift(const float *intr4, float voxel_size, float tranc_dist) {
    if (!intr4 || !(voxel_size > 0.0f) || signmap_steps(tranc_dist * 0.8f) == 0) return 0;
    float dt; int rounds;
    for (int shift = 2; shift <= 6; ++shift)
        if (sign_map_spacing(intr4[0], intr4[1], ray_wshift(), voxel_size, shift, dt, rounds)) return shift;
    return 0;
}


// do the resident planes of one volume array span at most 4 GiB (and the 24-bit products hold)?
static bool fits32(const RaycastArgs &a) {
    const unsigned long long rows = (unsigned long long)(a.zs1 - a.zs0) * (unsigned long long)a.Y;
    return (a.vstep % 4) == 0 && rows < (1ull << 24) && (a.vstep >> 2) < (1ull << 24) && rows * a.vstep <= (1ull << 32);
}
static void set_inv_vs(RaycastArgs &a) {
    float lo = 1.0f / a.voxel_size, hi = lo;
    for (int i = 0; i < 4; ++i) { lo = nextafterf(lo, 0.f); hi = nextafterf(hi, INFINITY); }
    a.inv_vs_lo = lo; a.inv_vs_hi = hi;
    a.dv = xs_const_div_get(a.voxel_size);
}
// What both launchers pass alike: poses, volume, maps, intrinsics, the march constants, the tile shape; no sign map, no pyramid, no
// optional outputs.  The planes resident behind value / grad, the owned ones and the keys are the caller's to set.  Returns the grid.
static dim3 raycast_common_args(RaycastArgs &a, const float *intr4, const float *Rc2v18, const float *tc2v6, const float *Rv2w18, const float *tv2w6,
                                float tranc_dist, const int *res, float voxel_size, const float *value, const float *grad, size_t vol_step, float *vmap,
                                float *nmap, size_t map_step, int rows, int cols) {
    load_mat(Rc2v18, a.Rc2v); load_vec(tc2v6, a.tc2v); load_mat(Rv2w18, a.Rv2w); load_vec(tv2w6, a.tv2w);
    a.X = res[0]; a.Y = res[1]; a.Z = res[2];
    a.voxel_size = voxel_size;
    a.time_step = tranc_dist * 0.8f;  // RayCaster.cu:350
    set_inv_vs(a);
    a.cols = cols; a.rows = rows;
    a.value = value; a.grad = grad; a.vstep = vol_step;
    a.intr = Intr{intr4[0], intr4[1], intr4[2], intr4[3]};
    a.vmap = (cfloat *)vmap; a.nmap = (cfloat *)nmap; a.mstep = map_step;
    a.hits = nullptr; a.cross_t = nullptr; a.steps = nullptr; a.keys = nullptr;
    a.sm = SignMap{};
    a.sm_dt = 0.0f; a.sm_rounds = 0;
    a.pyr = PyramidArgs{};
    a.wshift = ray_wshift();
    return dim3(div_up(div_up(cols, 2 << a.wshift) * div_up(rows, 128 >> a.wshift), 8) * 8);
}
// Binds the caller's sign map (o.signmap != null) to the march: a.sm, and the spacing of the wave's samples.  `who` names the entry point
// in the error messages.
static int raycast_bind_signmap(RaycastArgs &a, const xs_raycast_opts &o, const int *res, const char *who) {
    char msg[192];
    // the map's time table was written for one truncation distance (xs_signmap_reset): any other would resume at wrong times
    if (o.signmap_tranc_dist * 0.8f != a.time_step || o.signmap_shift < 2 || o.signmap_shift > 6) {
        snprintf(msg, sizeof(msg), "%s: the sign map was prepared for another truncation distance", who);
        return xs_set_error(hipErrorInvalidValue, msg);
    }
    static thread_local float nt_for = 0.0f;
    static thread_local int nt = 0;
    if (nt_for != a.time_step) { nt = signmap_steps(a.time_step); nt_for = a.time_step; }
    if (nt == 0) {
        snprintf(msg, sizeof(msg), "%s: the march has more steps than the sign map's time table holds", who);
        return xs_set_error(hipErrorInvalidValue, msg);
    }
    a.sm = signmap_view(const_cast<void *>(o.signmap), res, o.signmap_shift, nt);
    if (!sign_map_spacing(a.intr.fx, a.intr.fy, a.wshift, a.voxel_size, a.sm.shift, a.sm_dt, a.sm_rounds)) {
        snprintf(msg, sizeof(msg), "%s: the sign map's bricks are too small for a wave's pixel tile (xs_raycast_signmap_shift gives a usable shift)", who);
        return xs_set_error(hipErrorInvalidValue, msg);
    }
    return 0;
}
// The instance for (MODE, MAP): 32-bit voxel offsets where the resident planes allow them, and in the marches that have it the short
// division where voxel_size has been prepared for the floor (dv.ok bit 1)
typedef void (*RaycastKernel)(const RaycastArgs);
template <int MODE, bool MAP>
static RaycastKernel raycast_instance(bool off32, const ConstDiv &dv) {
    constexpr bool HAS_SHORT = MODE == RAY_MARCH || MODE == RAY_SLAB_MARCH || (MODE == RAY_WHOLE && MAP);
    if (!off32) return k_raycast<MODE, false, false, MAP>;
    if constexpr (HAS_SHORT)
        if (dv.ok & 2u) return k_raycast<MODE, true, true, MAP>;
    return k_raycast<MODE, true, false, MAP>;
}

/* raycast(const Intr&, const MatS33& Rc2v, const devComplex3& tc2v, const MatS33& Rv2w,
 *         const devComplex3& tv2w, float tranc_dist, const int3& res, float voxel_size,
 *         const PtrStep<float>& value, const PtrStep<float>& grad, MapArr& vmap, MapArr& nmap)
 *                                                   RayCaster.h:21-25, RayCaster.cu:327-368
 * rows/cols: size of one map plane.  hits_dev: optional device counter of pixels that got a
 * vertex.  workspace: optional rows*cols floats; with it the ray is split into a march kernel
 * and a crossing kernel (same arithmetic, higher occupancy).  No synchronisation (neither does
 * the reference, :367). */
// the reference's launcher proper: no sign map, no pyramid, no event (xs_raycast_ex takes those as an options struct)
extern "C" int xs_raycast(const float *intr4, const float *Rc2v18, const float *tc2v6, const float *Rv2w18, const float *tv2w6,
                          float tranc_dist, const int *res, float voxel_size, const float *value, const float *grad, size_t vol_step,
                          float *vmap, float *nmap, size_t map_step, int rows, int cols, unsigned long long *hits_dev, float *workspace,
                          void *stream) {
    xs_raycast_opts o = {};
    o.struct_bytes = sizeof(o);
    return xs_raycast_ex(intr4, Rc2v18, tc2v6, Rv2w18, tv2w6, tranc_dist, res, voxel_size, value, grad, vol_step, vmap, nmap, map_step, rows, cols, hits_dev,
                         workspace, &o, stream);
}
extern "C" int xs_raycast_ex(const float *intr4, const float *Rc2v18, const float *tc2v6, const float *Rv2w18, const float *tv2w6,
                             float tranc_dist, const int *res, float voxel_size, const float *value, const float *grad, size_t vol_step,
                             float *vmap, float *nmap, size_t map_step, int rows, int cols, unsigned long long *hits_dev, float *workspace,
                             xs_raycast_opts *opts, void *stream) {
    xs_raycast_opts none = {};
    none.struct_bytes = sizeof(none);
    xs_raycast_opts &o = opts ? *opts : none;
    if (o.struct_bytes != sizeof(xs_raycast_opts)) return xs_set_error(hipErrorInvalidValue, "xs_raycast_ex: opts->struct_bytes is not sizeof(xs_raycast_opts)");
    o.pyramid_built = 0;
    if (!intr4 || !Rc2v18 || !tc2v6 || !Rv2w18 || !tv2w6 || !res || !value || !grad || !vmap || !nmap)
        return xs_set_error(hipErrorInvalidValue, "xs_raycast: null pointer");
    if (rows <= 0 || cols <= 0) return 0;
    RaycastArgs a;
    const dim3 block(256), grid = raycast_common_args(a, intr4, Rc2v18, tc2v6, Rv2w18, tv2w6, tranc_dist, res, voxel_size, value, grad, vol_step, vmap, nmap, map_step, rows, cols);
    a.zs0 = 0; a.zs1 = res[2]; a.z0 = 0; a.z1 = res[2];
    a.hits = hits_dev; a.cross_t = workspace; a.steps = o.steps_dev;
    if (o.signmap && workspace)
        if (const int err = raycast_bind_signmap(a, o, res, "xs_raycast")) return err;
    const bool off32 = fits32(a);
    const hipStream_t s = (hipStream_t)stream;
    bool fused = a.sm.dil != nullptr;
#ifdef XS_EXPERIMENTS
    static const bool env_pair = exp_env_set("XS_RAY_MAP_TWO_KERNELS");   // measurement: the mapped march and the crossing as two launches
    if (env_pair) fused = false;
#endif
    if (!workspace)
        hipLaunchKernelGGL((raycast_instance<RAY_WHOLE, false>(off32, a.dv)), grid, block, 0, s, a);
    else if (fused) {
        // with the sign map the march is a few batches long: it and the crossing are one launch (five waves per SIMD hold the
        // frame's 4 800 waves either way) — no second dispatch, no crossing-time plane written and read back
        static const bool env_no_pyr = exp_env_set("XS_RAY_NO_PYRAMID");   // A/B aid: the pyramid stays a launch of its own
        if (o.pyr_vmap1 && o.pyr_nmap1 && o.pyr_vmap2 && o.pyr_nmap2 && !env_no_pyr) {
            a.pyr.mid[0] = (cfloat *)o.pyr_vmap1; a.pyr.mid[1] = (cfloat *)o.pyr_nmap1; a.pyr.out[0] = (cfloat *)o.pyr_vmap2; a.pyr.out[1] = (cfloat *)o.pyr_nmap2;
            a.pyr.mstep = o.pyr_step1; a.pyr.ostep = o.pyr_step2;
            a.pyr.in[0] = a.vmap; a.pyr.in[1] = a.nmap; a.pyr.istep = map_step; a.pyr.rows0 = rows; a.pyr.cols0 = cols;
            o.pyramid_built = 1;
        }
        const RaycastKernel kern = raycast_instance<RAY_WHOLE, true>(off32, a.dv);
        if (o.completion_event) hipExtLaunchKernelGGL(kern, grid, block, 0, s, nullptr, (hipEvent_t)o.completion_event, 0, a);
        else hipLaunchKernelGGL(kern, grid, block, 0, s, a);
    } else {
        // march (few registers, many waves, eight gathers in flight per lane) then the crossings
        RaycastKernel march = raycast_instance<RAY_MARCH, false>(off32, a.dv);
#ifdef XS_EXPERIMENTS
        if (a.sm.dil) march = raycast_instance<RAY_MARCH, true>(off32, a.dv);
#endif
        a.hits = nullptr;
        hipLaunchKernelGGL(march, grid, block, 0, s, a);
        a.hits = hits_dev;
        hipLaunchKernelGGL((raycast_instance<RAY_CROSS, false>(off32, a.dv)), grid, block, 0, s, a);
    }
    XS_CHECK(hipGetLastError());
    return 0;
}

/* Slab form of raycast for a z-sharded volume (no reference counterpart: the reference is
 * single-GPU; semantics are those of RayCaster.cu:197-310 restricted to one rank's steps).
 * value / grad hold planes [zs0, zs1) (owned slab + halo); only march steps whose sample voxel
 * lies in the owned planes [z0, z1) are evaluated.  keys_dev[rows*cols] receives, per pixel,
 * (step << 1 | no_vertex) of the first event among those steps or INT_MAX; vmap / nmap receive
 * this rank's vertex / normal for its own event and zeros elsewhere.  The caller takes the
 * minimum of the keys over ranks, calls xs_raycast_compose_mask, adds the maps over ranks as
 * int32, then xs_raycast_compose_finish.  Halo needed: 6 planes. */
extern "C" int xs_raycast_slab(const float *intr4, const float *Rc2v18, const float *tc2v6, const float *Rv2w18, const float *tv2w6,
                               float tranc_dist, const int *res, float voxel_size, const float *value, const float *grad, size_t vol_step,
                               int zs0, int zs1, int z0, int z1, float *vmap, float *nmap, size_t map_step, int rows, int cols,
                               int *keys_dev, void *stream) {
    xs_raycast_opts o = {};
    o.struct_bytes = sizeof(o);
    return xs_raycast_slab_ex(intr4, Rc2v18, tc2v6, Rv2w18, tv2w6, tranc_dist, res, voxel_size, value, grad, vol_step, zs0, zs1, z0, z1, vmap, nmap, map_step, rows,
                              cols, keys_dev, &o, stream);
}
extern "C" int xs_raycast_slab_ex(const float *intr4, const float *Rc2v18, const float *tc2v6, const float *Rv2w18, const float *tv2w6,
                                  float tranc_dist, const int *res, float voxel_size, const float *value, const float *grad, size_t vol_step,
                                  int zs0, int zs1, int z0, int z1, float *vmap, float *nmap, size_t map_step, int rows, int cols,
                                  int *keys_dev, const xs_raycast_opts *opts, void *stream) {
    xs_raycast_opts none = {};
    none.struct_bytes = sizeof(none);
    const xs_raycast_opts &o = opts ? *opts : none;
    if (o.struct_bytes != sizeof(xs_raycast_opts)) return xs_set_error(hipErrorInvalidValue, "xs_raycast_slab_ex: opts->struct_bytes is not sizeof(xs_raycast_opts)");
    if (!intr4 || !Rc2v18 || !tc2v6 || !Rv2w18 || !tv2w6 || !res || !value || !grad || !vmap || !nmap || !keys_dev)
        return xs_set_error(hipErrorInvalidValue, "xs_raycast_slab: null pointer");
    if (zs0 < 0 || zs1 > res[2] || z0 < zs0 || z1 > zs1 || z1 < z0) return xs_set_error(hipErrorInvalidValue, "xs_raycast_slab: bad slab");
    if (rows <= 0 || cols <= 0) return 0;
    RaycastArgs a;
    const dim3 block(256), grid = raycast_common_args(a, intr4, Rc2v18, tc2v6, Rv2w18, tv2w6, tranc_dist, res, voxel_size, value, grad, vol_step, vmap, nmap, map_step, rows, cols);
    a.zs0 = zs0; a.zs1 = zs1; a.z0 = z0; a.z1 = z1; a.keys = keys_dev;
    // this rank's sign map (marked by its own integrate calls: owned slab + halo): the march evaluates the iterations it leaves
    if (o.signmap)
        if (const int err = raycast_bind_signmap(a, o, res, "xs_raycast_slab")) return err;
    const bool off32 = fits32(a);
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((a.sm.dil ? raycast_instance<RAY_SLAB_MARCH, true>(off32, a.dv) : raycast_instance<RAY_SLAB_MARCH, false>(off32, a.dv)), grid, block, 0, s, a);
    hipLaunchKernelGGL((raycast_instance<RAY_SLAB_CROSS, false>(off32, a.dv)), grid, block, 0, s, a);
    XS_CHECK(hipGetLastError());
    return 0;
}

__global__ void __launch_bounds__(256) k_compose_mask(const int *own_keys, const int *min_keys, cfloat *vmap, cfloat *nmap, size_t mstep, int rows, int cols) {
    const int x = threadIdx.x + blockIdx.x * 64, y = threadIdx.y + blockIdx.y * 4;
    if (x >= cols || y >= rows) return;
    const int k = own_keys[y * cols + x], m = min_keys[y * cols + x];
    if (k == m && !(k & 1) && k != 0x7fffffff) return;  // this rank holds the ray's first event and it has a vertex
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        row_ptr(vmap, mstep, y + p * rows)[x] = cfloat(0.f, 0.f);
        row_ptr(nmap, mstep, y + p * rows)[x] = cfloat(0.f, 0.f);
    }
}
__global__ void __launch_bounds__(256) k_compose_finish(const int *min_keys, cfloat *vmap, cfloat *nmap, size_t mstep, int rows, int cols,
                                                        unsigned long long *hits) {
    // a few hundred workgroups stride over the 64x4 pixel tiles and add their hit count with ONE atomic each
    // (one per wave to the same word — 4800 of them at ~12 ns — made this the second longest kernel of the frame)
    const int tiles_x = (cols + 63) / 64, tiles_y = (rows + 3) / 4;
    unsigned hit = 0;
    for (int tile = blockIdx.x; tile < tiles_x * tiles_y; tile += gridDim.x) {
        const int x = threadIdx.x + (tile % tiles_x) * 64, y = threadIdx.y + (tile / tiles_x) * 4;
        if (x < cols && y < rows) {
            const int m = min_keys[y * cols + x];
            if ((m & 1) || m == 0x7fffffff) {  // no vertex on this ray: the NaN sentinel of RayCaster.cu:204-205
                row_ptr(vmap, mstep, y)[x] = cfloat(qnan_f(), 0.f);
                row_ptr(nmap, mstep, y)[x] = cfloat(qnan_f(), 0.f);
            } else
                ++hit;
        }
    }
    if (hits) {
        __shared__ unsigned s_hits[4];
        const int tid = threadIdx.y * 64 + threadIdx.x;
        const unsigned s = wave_sum_u32(hit);
        if ((tid & 63) == 0) s_hits[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) {
            const unsigned t = (s_hits[0] + s_hits[1]) + (s_hits[2] + s_hits[3]);
            if (t) atomicAdd(hits, (unsigned long long)t);
        }
    }
}
// ---- owner-compacted exchange of the composite (round 4) ---------------------------------------------------------------------------
// Adding the ranks' maps moves every pixel's 48 bytes through a ring all-reduce although one rank at most has anything but zeros there:
// 2 (N - 1) / N x 14.7 MB per rank and frame.  Instead every rank packs the pixels it owns — {pixel index, vertex (3 complex), normal
// (3 complex)}: 13 words — the ranks' packs are gathered (variable sizes: the counts travel first, as an int32 sum with one non-zero
// entry per rank) and a scatter writes them into the maps: (N - 1) / N x 52 bytes x hits received per rank, about half.
enum { COMPOSE_ENTRY_WORDS = 13 };
__global__ void __launch_bounds__(256) k_compose_pack(const int *own_keys, const int *min_keys, const cfloat *vmap, const cfloat *nmap, size_t mstep, int rows,
                                                      int cols, unsigned *entries, int *count) {
    // one workgroup-wide slot reservation per 256 pixels: a ballot per wave, one LDS exchange, one atomic
    __shared__ unsigned s_base[5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int p0 = blockIdx.x * 256; p0 < rows * cols; p0 += gridDim.x * 256) {
        const int p = p0 + tid;
        bool mine = false;
        int x = 0, y = 0;
        if (p < rows * cols) {
            const int k = own_keys[p], m = min_keys[p];
            mine = k == m && !(k & 1) && k != 0x7fffffff;
            y = p / cols; x = p - y * cols;
        }
        const unsigned long long b = __builtin_amdgcn_ballot_w64(mine);
        if (lane == 0) s_base[wave] = (unsigned)__popcll(b);
        __syncthreads();
        if (tid == 0) {
            const unsigned n0 = s_base[0], n1 = s_base[1], n2 = s_base[2], n3 = s_base[3];
            const unsigned tot = n0 + n1 + n2 + n3;
            const unsigned base = tot ? (unsigned)atomicAdd(count, (int)tot) : 0u;
            s_base[0] = base; s_base[1] = base + n0; s_base[2] = base + n0 + n1; s_base[3] = base + n0 + n1 + n2;
        }
        __syncthreads();
        if (mine) {
            unsigned *e = entries + (size_t)(s_base[wave] + (unsigned)__popcll(b & ((1ull << lane) - 1ull))) * COMPOSE_ENTRY_WORDS;
            e[0] = (unsigned)p;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const cfloat v = row_ptr(vmap, mstep, y + q * rows)[x], n = row_ptr(nmap, mstep, y + q * rows)[x];
                e[1 + 2 * q] = __float_as_uint(v.re); e[2 + 2 * q] = __float_as_uint(v.im);
                e[7 + 2 * q] = __float_as_uint(n.re); e[8 + 2 * q] = __float_as_uint(n.im);
            }
        }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256) k_compose_scatter(const unsigned *entries, long n, cfloat *vmap, cfloat *nmap, size_t mstep, int rows, int cols) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        const unsigned *e = entries + i * COMPOSE_ENTRY_WORDS;
        const unsigned p = e[0];
        if (p >= (unsigned)(rows * cols)) continue;   // (never: the packs hold pixel indices)
        const int y = (int)(p / (unsigned)cols), x = (int)(p - (unsigned)y * (unsigned)cols);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            row_ptr(vmap, mstep, y + q * rows)[x] = cfloat(__uint_as_float(e[1 + 2 * q]), __uint_as_float(e[2 + 2 * q]));
            row_ptr(nmap, mstep, y + q * rows)[x] = cfloat(__uint_as_float(e[7 + 2 * q]), __uint_as_float(e[8 + 2 * q]));
        }
    }
}
/* The pixels this rank owns with a vertex (own key == min key, event with a vertex), packed: entries_dev receives 13 32-bit words per
 * pixel {pixel index y * cols + x, vertex x / y / z (re, im), normal x / y / z (re, im)} in no particular order, *count_dev is advanced
 * by their number (the caller zeroes it; room for rows * cols entries). */
extern "C" int xs_raycast_compose_pack(const int *own_keys_dev, const int *min_keys_dev, const float *vmap, const float *nmap, size_t map_step, int rows,
                                       int cols, void *entries_dev, int *count_dev, void *stream) {
    if (!own_keys_dev || !min_keys_dev || !vmap || !nmap || !entries_dev || !count_dev) return xs_set_error(hipErrorInvalidValue, "xs_raycast_compose_pack: null pointer");
    if (rows <= 0 || cols <= 0) return 0;
    const int blocks = div_up(rows * cols, 256);
    hipLaunchKernelGGL(k_compose_pack, dim3(blocks < 1024 ? blocks : 1024), dim3(256), 0, (hipStream_t)stream, own_keys_dev, min_keys_dev, (const cfloat *)vmap,
                       (const cfloat *)nmap, map_step, rows, cols, (unsigned *)entries_dev, count_dev);
    XS_CHECK(hipGetLastError());
    return 0;
}
/* n packed entries (any ranks') written into the maps */
extern "C" int xs_raycast_compose_scatter(const void *entries_dev, long n, float *vmap, float *nmap, size_t map_step, int rows, int cols, void *stream) {
    if (!entries_dev || !vmap || !nmap) return xs_set_error(hipErrorInvalidValue, "xs_raycast_compose_scatter: null pointer");
    if (n <= 0 || rows <= 0 || cols <= 0) return 0;
    const long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_compose_scatter, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)stream, (const unsigned *)entries_dev, n, (cfloat *)vmap,
                       (cfloat *)nmap, map_step, rows, cols);
    XS_CHECK(hipGetLastError());
    return 0;
}
extern "C" size_t xs_raycast_compose_entry_bytes(void) { return COMPOSE_ENTRY_WORDS * sizeof(unsigned); }
/* keep this rank's vertex / normal only where it owns the ray's first event (own key == min key) */
extern "C" int xs_raycast_compose_mask(const int *own_keys_dev, const int *min_keys_dev, float *vmap, float *nmap, size_t map_step, int rows,
                                       int cols, void *stream) {
    if (!own_keys_dev || !min_keys_dev || !vmap || !nmap) return xs_set_error(hipErrorInvalidValue, "xs_raycast_compose_mask: null pointer");
    dim3 block(64, 4), grid(div_up(cols, 64), div_up(rows, 4));
    hipLaunchKernelGGL(k_compose_mask, grid, block, 0, (hipStream_t)stream, own_keys_dev, min_keys_dev, (cfloat *)vmap, (cfloat *)nmap, map_step, rows, cols);
    XS_CHECK(hipGetLastError());
    return 0;
}
/* after the maps were added over ranks: write the NaN sentinel where the first event has no vertex */
extern "C" int xs_raycast_compose_finish(const int *min_keys_dev, float *vmap, float *nmap, size_t map_step, int rows, int cols,
                                         unsigned long long *hits_dev, void *stream) {
    if (!min_keys_dev || !vmap || !nmap) return xs_set_error(hipErrorInvalidValue, "xs_raycast_compose_finish: null pointer");
    const int ntiles = div_up(cols, 64) * div_up(rows, 4);
    dim3 block(64, 4), grid(ntiles < 256 ? ntiles : 256);
    hipLaunchKernelGGL(k_compose_finish, grid, block, 0, (hipStream_t)stream, min_keys_dev, (cfloat *)vmap, (cfloat *)nmap, map_step, rows, cols, hits_dev);
    XS_CHECK(hipGetLastError());
    return 0;
}
