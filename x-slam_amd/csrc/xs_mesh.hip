// xs_mesh.hip — marching-cubes triangle mesh of the TSDF for gfx950, with the complex-step derivative of every vertex.  No working
// counterpart in the reference: its extractMesh (ExtractPointCloud.cu:364-715) is never called and cannot run as written.
//
// Cube (x, y, z) spans voxels x..x+1, y..y+1, z..z+1.  It is live when its 8 corners all have weight >= min_weight and value < 0.99 and
// its case (bit c = corner c negative, value < 0) is neither 0 nor 255.  One vertex per sign-changing edge of a live cube, keyed
// ((z * Y + y) * X + x) * 3 + axis by its lower endpoint; triangles from xs_mesh_table.h (gen_mesh_table.py: crack-free by construction).
//
// Shape: a segment is one row (z, y) of keys, and one wave owns a segment: lane = x, 64 consecutive voxels per step, so every row read
// is one coalesced segment.  Pass 1 counts each segment's vertices and triangles, a three-kernel scan turns the counts into 64-bit
// offsets, pass 2 writes the vertices in key order (lane order, then axis, inside a step) and pass 3 the triangles in cube order.  Pass 3
// finds a corner's vertex by binary search over the keys pass 2 wrote, inside the range of the segment that holds the edge's lower
// endpoint (a handful of entries).  The output order is fixed by the keys alone: no atomics.
#include "xs_device.h"
#include "xs_env.h"
#include "xs_mesh_table.h"
#include "xs_signmap.h"
#include "../../include/xslam_amd.h"

using namespace xs;

namespace {
struct MeshArgs {
    const float *value; const int *weight; const float *grad; size_t vstep;
    int X, Y, Z, zs0, zs1, z0, z1, min_weight;
    float voxel_size;
    const unsigned char *dil; int shift, bnx, bny;   // sign map (dil == nullptr: none)
    unsigned nseg;                                    // rows (z, y) for z in [z0, z1]
    unsigned *vcnt, *tcnt;                            // [nseg] pass 1 out
    unsigned long long *voff, *toff;                  // [nseg + 1] exclusive offsets
    float *verts, *vim, *normals; unsigned long long *keys; int *tris;
    int global_search;                                // A/B (XS_EXPERIMENTS): search all keys instead of the segment's
};

__device__ __forceinline__ size_t at(const MeshArgs &a, int x, int y, int z) {   // element offset of voxel (x, y, z) in a pitched array
    return (size_t)(a.Y * (z - a.zs0) + y) * (a.vstep / 4) + x;
}
// ok / neg bits of the corners (x + dx, y + dy, z + dz), d in [LO, 1]; bit (dz + 1) * 9 + (dy + 1) * 3 + dx + 1.  A corner outside the
// volume or outside planes [z0, z1] is not ok, so no cube it belongs to is live.
template <int LO>
__device__ __forceinline__ void load_corners(const MeshArgs &a, int x, int y, int z, unsigned &ok, unsigned &neg) {
    ok = 0; neg = 0;
#pragma unroll
    for (int dz = LO; dz <= 1; ++dz)
#pragma unroll
        for (int dy = LO; dy <= 1; ++dy)
#pragma unroll
            for (int dx = LO; dx <= 1; ++dx) {
                const int xx = x + dx, yy = y + dy, zz = z + dz;
                if (xx < 0 || xx >= a.X || yy < 0 || yy >= a.Y || zz < a.z0 || zz > a.z1) continue;
                const size_t i = at(a, xx, yy, zz);
                const float v = a.value[i];
                const int w = a.weight[i];
                const unsigned bit = 1u << ((dz + 1) * 9 + (dy + 1) * 3 + dx + 1);
                if (w >= a.min_weight && v < 0.99f) ok |= bit;
                if (v < 0.0f) neg |= bit;
            }
}
__device__ __forceinline__ unsigned cbit(int dx, int dy, int dz) { return 1u << ((dz + 1) * 9 + (dy + 1) * 3 + dx + 1); }
// case of the cube whose corner 0 is at offset (ox, oy, oz) from the lane's voxel, or -1 if it is not live
__device__ __forceinline__ int live_case(unsigned ok, unsigned neg, int ox, int oy, int oz) {
    int c = 0;
    bool all = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned b = cbit(ox + (k & 1), oy + ((k >> 1) & 1), oz + (k >> 2));
        all = all && (ok & b);
        if (neg & b) c |= 1 << k;
    }
    return (all && c != 0 && c != 255) ? c : -1;
}
// bit a: the edge from the lane's voxel along axis a is a vertex (sign change, and one of the four cubes around it is live)
__device__ __forceinline__ unsigned vertex_axes(unsigned ok, unsigned neg) {
    unsigned m = 0;
    const bool n0 = neg & cbit(0, 0, 0);
    if (n0 != (bool)(neg & cbit(1, 0, 0)) &&
        (live_case(ok, neg, 0, 0, 0) >= 0 || live_case(ok, neg, 0, -1, 0) >= 0 || live_case(ok, neg, 0, 0, -1) >= 0 || live_case(ok, neg, 0, -1, -1) >= 0))
        m |= 1;
    if (n0 != (bool)(neg & cbit(0, 1, 0)) &&
        (live_case(ok, neg, 0, 0, 0) >= 0 || live_case(ok, neg, -1, 0, 0) >= 0 || live_case(ok, neg, 0, 0, -1) >= 0 || live_case(ok, neg, -1, 0, -1) >= 0))
        m |= 2;
    if (n0 != (bool)(neg & cbit(0, 0, 1)) &&
        (live_case(ok, neg, 0, 0, 0) >= 0 || live_case(ok, neg, -1, 0, 0) >= 0 || live_case(ok, neg, 0, -1, 0) >= 0 || live_case(ok, neg, -1, -1, 0) >= 0))
        m |= 4;
    return m;
}
__device__ __forceinline__ int tri_count(int c) {
    int n = 0;
    while (n < 5 && MESH_TRIS[c][3 * n] >= 0) ++n;
    return n;
}
// a sign map brick whose dil byte is clear has no negative voxel within one brick: none of the 7 cubes a voxel of it touches is live
__device__ __forceinline__ bool may_be_live(const MeshArgs &a, int x, int y, int z) {
    if (!a.dil) return true;
    return a.dil[((size_t)(z >> a.shift) * a.bny + (y >> a.shift)) * a.bnx + (x >> a.shift)] != 0;
}
// exclusive prefix of a small per-lane count over the wave, and the wave total
__device__ __forceinline__ unsigned wave_excl(unsigned v, unsigned &total) {
    const int lane = threadIdx.x & 63;
    unsigned s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(s, off, 64);
        if (lane >= off) s += t;
    }
    total = __shfl(s, 63, 64);
    return s - v;
}

// trilinear TSDF and normal at a point: the sampling of k_extract_normals (xs_extract.hip), normalised by the length
__device__ __forceinline__ float read_tsdf(const MeshArgs &a, int x, int y, int z) {
    z = min(max(z, a.zs0), a.zs1 - 1);
    return a.value[at(a, x, y, z)];
}
__device__ __forceinline__ float interp(const MeshArgs &a, float px, float py, float pz) {
    const float vs = a.voxel_size;
    int gx = __float2int_rd(px / vs), gy = __float2int_rd(py / vs), gz = __float2int_rd(pz / vs);
    const float vx = (gx + 0.5f) * vs, vy = (gy + 0.5f) * vs, vz = (gz + 0.5f) * vs;
    gx = (px < vx) ? (gx - 1) : gx;
    gy = (py < vy) ? (gy - 1) : gy;
    gz = (pz < vz) ? (gz - 1) : gz;
    const float fa = (px - (gx + 0.5f) * vs) / vs, fb = (py - (gy + 0.5f) * vs) / vs, fc = (pz - (gz + 0.5f) * vs) / vs;
    return read_tsdf(a, gx + 0, gy + 0, gz + 0) * (1 - fa) * (1 - fb) * (1 - fc) + read_tsdf(a, gx + 0, gy + 0, gz + 1) * (1 - fa) * (1 - fb) * fc +
           read_tsdf(a, gx + 0, gy + 1, gz + 0) * (1 - fa) * fb * (1 - fc) + read_tsdf(a, gx + 0, gy + 1, gz + 1) * (1 - fa) * fb * fc +
           read_tsdf(a, gx + 1, gy + 0, gz + 0) * fa * (1 - fb) * (1 - fc) + read_tsdf(a, gx + 1, gy + 0, gz + 1) * fa * (1 - fb) * fc +
           read_tsdf(a, gx + 1, gy + 1, gz + 0) * fa * fb * (1 - fc) + read_tsdf(a, gx + 1, gy + 1, gz + 1) * fa * fb * fc;
}
__device__ __forceinline__ void normal_at(const MeshArgs &a, float px, float py, float pz, float *out) {
    const float vs = a.voxel_size;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    const int gx = __float2int_rd(px / vs), gy = __float2int_rd(py / vs), gz = __float2int_rd(pz / vs);
    if (gx > 1 && gy > 1 && gz > 1 && gx < a.X - 2 && gy < a.Y - 2 && gz < a.Z - 2) {
        nx = interp(a, px + vs, py, pz) - interp(a, px - vs, py, pz);
        ny = interp(a, px, py + vs, pz) - interp(a, px, py - vs, pz);
        nz = interp(a, px, py, pz + vs) - interp(a, px, py, pz - vs);
        const float len = sqrtf(nx * nx + ny * ny + nz * nz);
        if (len > 0.f) { nx = nx / len; ny = ny / len; nz = nz / len; }
    }
    out[0] = nx; out[1] = ny; out[2] = nz;
}
}  // namespace

// PASS 1 counts, PASS 2 writes the vertices, PASS 3 the triangles.  Four waves per workgroup, one segment (row) per wave.
template <int PASS>
__global__ void __launch_bounds__(256) k_mesh(const MeshArgs a) {
    const int lane = threadIdx.x & 63;
    const unsigned seg = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= a.nseg) return;   // (wave-uniform; the kernel has no barrier)
    const int z = a.z0 + (int)(seg / (unsigned)a.Y), y = (int)(seg % (unsigned)a.Y);
    unsigned long long running = PASS == 2 ? a.voff[seg] : PASS == 3 ? a.toff[seg] : 0ull;
    unsigned vtotal = 0, ttotal = 0;
    for (int x0 = 0; x0 < a.X; x0 += 64) {
        const int x = x0 + lane;
        unsigned ok = 0, neg = 0;
        const bool maybe = x < a.X && may_be_live(a, x, y, z);
        if (PASS == 3) {
            if (maybe && z < a.z1) load_corners<0>(a, x, y, z, ok, neg);
            const int c = live_case(ok, neg, 0, 0, 0);
            const unsigned n = c >= 0 ? tri_count(c) : 0u;
            unsigned wt;
            const unsigned long long base = running + wave_excl(n, wt);
            for (unsigned t = 0; t < n; ++t)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const signed char *e = MESH_EDGE[MESH_TRIS[c][3 * t + k]];
                    const int ex = x + e[1], ey = y + e[2], ez = z + e[3];
                    const unsigned long long key = (((unsigned long long)ez * a.Y + ey) * a.X + ex) * 3ull + e[0];
                    const unsigned s = (unsigned)(ez - a.z0) * (unsigned)a.Y + (unsigned)ey;
                    unsigned long long lo = a.global_search ? 0ull : a.voff[s], hi = a.global_search ? a.voff[a.nseg] : a.voff[s + 1];
                    while (lo < hi) {   // first key >= the edge's (it is there: pass 2 wrote every vertex of a live cube)
                        const unsigned long long mid = (lo + hi) >> 1;
                        if (a.keys[mid] < key) lo = mid + 1; else hi = mid;
                    }
                    a.tris[3 * (base + t) + k] = (int)lo;
                }
            running += wt;
            continue;
        }
        if (maybe) load_corners<-1>(a, x, y, z, ok, neg);
        const unsigned m = vertex_axes(ok, neg);
        const unsigned nv = __popc(m);
        if (PASS == 1) {
            const int c = live_case(ok, neg, 0, 0, 0);
            vtotal += nv;
            ttotal += c >= 0 ? tri_count(c) : 0u;
            continue;
        }
        unsigned wv;
        unsigned long long slot = running + wave_excl(nv, wv);
        if (m) {
            const size_t i0 = at(a, x, y, z);
            const float F = a.value[i0];
            const float vs = a.voxel_size;
            const float V[3] = {(x + 0.5f) * vs, (y + 0.5f) * vs, (z + 0.5f) * vs};
            const unsigned long long key0 = (((unsigned long long)z * a.Y + y) * a.X + x) * 3ull;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                if (!(m >> ax & 1)) continue;
                const size_t i1 = at(a, x + (ax == 0), y + (ax == 1), z + (ax == 2));
                const float Fn = a.value[i1];
                float p[3] = {V[0], V[1], V[2]};
                p[ax] = V[ax] - (F / (Fn - F)) * vs;   // xs_extract.hip, crossings(): the point export's expression
                a.verts[3 * slot] = p[0]; a.verts[3 * slot + 1] = p[1]; a.verts[3 * slot + 2] = p[2];
                a.keys[slot] = key0 + ax;
                if (a.vim) {   // the same expression on (value, grad) pairs: Im of the vertex, in units of the seed step
                    const cfloat Fc(F, a.grad[i0]), Fnc(Fn, a.grad[i1]);
                    const cfloat q = V[ax] - (Fc / (Fnc - Fc)) * vs;
                    a.vim[3 * slot] = ax == 0 ? q.im : 0.f; a.vim[3 * slot + 1] = ax == 1 ? q.im : 0.f; a.vim[3 * slot + 2] = ax == 2 ? q.im : 0.f;
                }
                if (a.normals) normal_at(a, p[0], p[1], p[2], a.normals + 3 * slot);
                ++slot;
            }
        }
        running += wv;
    }
    if (PASS == 1) {
        vtotal = wave_sum_u32(vtotal);
        ttotal = wave_sum_u32(ttotal);
        if (lane == 0) { a.vcnt[seg] = vtotal; a.tcnt[seg] = ttotal; }
    }
}

// exclusive scan of the two count arrays (blockIdx.y selects one) into 64-bit offsets: 1024 entries per workgroup ...
__global__ void __launch_bounds__(256) k_mesh_scan_blocks(const unsigned *c0, const unsigned *c1, unsigned long long *o0, unsigned long long *o1,
                                                          unsigned long long *b0, unsigned long long *b1, unsigned n) {
    const unsigned *cnt = blockIdx.y ? c1 : c0;
    unsigned long long *off = blockIdx.y ? o1 : o0, *bsum = blockIdx.y ? b1 : b0;
    __shared__ unsigned long long s_part[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned i0 = blockIdx.x * 1024u + 4u * tid;
    unsigned long long v[4], t = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = i0 + k < n ? cnt[i0 + k] : 0u; t += v[k]; }
    unsigned long long s = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(s, o, 64);
        if (lane >= o) s += u;
    }
    if (lane == 63) s_part[wave] = s;
    __syncthreads();
    unsigned long long base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { if (w < wave) base += s_part[w]; total += s_part[w]; }
    unsigned long long e = base + s - t;
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (i0 + k < n) off[i0 + k] = e; e += v[k]; }
    if (tid == 0) bsum[blockIdx.x] = total;
}
// ... the workgroup sums in one workgroup (exclusive, in place; the grand total into off[n]) ...
__global__ void __launch_bounds__(256) k_mesh_scan_top(unsigned long long *b0, unsigned long long *b1, unsigned nb, unsigned long long *o0,
                                                       unsigned long long *o1, unsigned n) {
    unsigned long long *bsum = blockIdx.x ? b1 : b0, *off = blockIdx.x ? o1 : o0;
    __shared__ unsigned long long s_part[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long carry = 0;
    for (unsigned base = 0; base < nb; base += 256) {
        const unsigned i = base + tid;
        const unsigned long long v = i < nb ? bsum[i] : 0ull;
        unsigned long long s = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long u = __shfl_up(s, o, 64);
            if (lane >= o) s += u;
        }
        if (lane == 63) s_part[wave] = s;
        __syncthreads();
        unsigned long long wb = 0, chunk = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { if (w < wave) wb += s_part[w]; chunk += s_part[w]; }
        if (i < nb) bsum[i] = carry + wb + s - v;
        carry += chunk;
        __syncthreads();
    }
    if (tid == 0) off[n] = carry;
}
// ... and the workgroup offsets added back
__global__ void __launch_bounds__(256) k_mesh_scan_add(unsigned long long *o0, unsigned long long *o1, const unsigned long long *b0,
                                                       const unsigned long long *b1, unsigned n) {
    unsigned long long *off = blockIdx.y ? o1 : o0;
    const unsigned long long add = (blockIdx.y ? b1 : b0)[blockIdx.x];
    const unsigned i0 = blockIdx.x * 1024u + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i0 + 256u * k < n) off[i0 + 256u * k] += add;
}

namespace {
struct WsLayout { size_t vcnt, tcnt, voff, toff, b0, b1, total; unsigned nseg, nblk; };
WsLayout ws_layout(const int *res, int z0, int z1) {
    WsLayout l;
    l.nseg = (unsigned)res[1] * (unsigned)(z1 - z0 + 1);
    l.nblk = (l.nseg + 1023u) / 1024u;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    l.vcnt = 0;
    l.tcnt = l.vcnt + up((size_t)l.nseg * 4);
    l.voff = l.tcnt + up((size_t)l.nseg * 4);
    l.toff = l.voff + up(((size_t)l.nseg + 1) * 8);
    l.b0 = l.toff + up(((size_t)l.nseg + 1) * 8);
    l.b1 = l.b0 + up((size_t)l.nblk * 8);
    l.total = l.b1 + up((size_t)l.nblk * 8);
    return l;
}
bool mesh_opts_ok(const int *res, const xs_mesh_opts *o) {
    return res && o && o->struct_bytes >= sizeof(xs_mesh_opts) && res[0] >= 2 && res[1] >= 2 && res[2] >= 2 && o->z0 >= o->zs0 &&
           o->z1 >= o->z0 && o->z1 <= res[2] - 1 && (o->zs1 == 0 || o->zs1 > o->z1) && (size_t)res[1] * (size_t)(o->z1 - o->z0 + 1) < (1ull << 31);
}
}  // namespace

extern "C" size_t xs_mesh_workspace_bytes(const int *res, const xs_mesh_opts *opts) {
    if (!res || res[0] < 2 || res[1] < 2 || res[2] < 2) return 0;
    if (opts && !mesh_opts_ok(res, opts)) return 0;
    return ws_layout(res, opts ? opts->z0 : 0, opts ? opts->z1 : res[2] - 1).total;
}

extern "C" int xs_mesh_case_table(int cube_case, signed char out16[16]) {
    if (cube_case < 0 || cube_case > 255 || !out16) return xs_set_error(hipErrorInvalidValue, "xs_mesh_case_table: bad argument");
    for (int i = 0; i < 16; ++i) out16[i] = MESH_TRIS[cube_case][i];
    return 0;
}

extern "C" int xs_extract_mesh(const float *value, const int *weight, const float *grad, size_t vol_step, const int *res, float voxel_size,
                               const xs_mesh_opts *opts, float *vertices_dev, float *vertex_im_dev, float *normals_dev,
                               unsigned long long *keys_dev, size_t vertex_capacity, int *triangles_dev, size_t triangle_capacity, void *workspace,
                               size_t *vertex_count_host, size_t *triangle_count_host, void *stream) {
    if (!value || !weight || !workspace || !vertex_count_host || !triangle_count_host)
        return xs_set_error(hipErrorInvalidValue, "xs_extract_mesh: null pointer");
    if (!mesh_opts_ok(res, opts) || (vol_step % 4) != 0) return xs_set_error(hipErrorInvalidValue, "xs_extract_mesh: bad options or plane range");
    if (opts->signmap && (opts->signmap_shift < 2 || opts->signmap_shift > 6))
        return xs_set_error(hipErrorInvalidValue, "xs_extract_mesh: bad sign map shift");
    *vertex_count_host = 0; *triangle_count_host = 0;
    if (opts->z1 == opts->z0) return 0;
    const WsLayout l = ws_layout(res, opts->z0, opts->z1);
    char *ws = static_cast<char *>(workspace);
    MeshArgs a{};
    a.value = value; a.weight = weight; a.vstep = vol_step;
    a.X = res[0]; a.Y = res[1]; a.Z = res[2]; a.zs0 = opts->zs0; a.zs1 = opts->zs1 ? opts->zs1 : res[2];
    a.z0 = opts->z0; a.z1 = opts->z1; a.min_weight = opts->min_weight > 1 ? opts->min_weight : 1;
    a.voxel_size = voxel_size;
    if (opts->signmap) {
        const SignMap m = signmap_view(const_cast<void *>(opts->signmap), res, opts->signmap_shift, 0);
        a.dil = m.dil; a.shift = m.shift; a.bnx = m.nx; a.bny = m.ny;
    }
    a.nseg = l.nseg;
    a.vcnt = (unsigned *)(ws + l.vcnt); a.tcnt = (unsigned *)(ws + l.tcnt);
    a.voff = (unsigned long long *)(ws + l.voff); a.toff = (unsigned long long *)(ws + l.toff);
    a.global_search = exp_env_int("XS_MESH_GLOBAL_SEARCH", 0);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((l.nseg + 3) / 4), block(256);
    hipLaunchKernelGGL(k_mesh<1>, grid, block, 0, st, a);
    unsigned long long *b0 = (unsigned long long *)(ws + l.b0), *b1 = (unsigned long long *)(ws + l.b1);
    hipLaunchKernelGGL(k_mesh_scan_blocks, dim3(l.nblk, 2), dim3(256), 0, st, a.vcnt, a.tcnt, a.voff, a.toff, b0, b1, l.nseg);
    hipLaunchKernelGGL(k_mesh_scan_top, dim3(2), dim3(256), 0, st, b0, b1, l.nblk, a.voff, a.toff, l.nseg);
    hipLaunchKernelGGL(k_mesh_scan_add, dim3(l.nblk, 2), dim3(256), 0, st, a.voff, a.toff, b0, b1, l.nseg);
    XS_CHECK(hipGetLastError());
    unsigned long long tot[2] = {0, 0};
    XS_CHECK(hipMemcpyAsync(&tot[0], a.voff + l.nseg, 8, hipMemcpyDeviceToHost, st));
    XS_CHECK(hipMemcpyAsync(&tot[1], a.toff + l.nseg, 8, hipMemcpyDeviceToHost, st));
    XS_CHECK(hipStreamSynchronize(st));
    *vertex_count_host = (size_t)tot[0]; *triangle_count_host = (size_t)tot[1];
    if (tot[0] > vertex_capacity || tot[1] > triangle_capacity) return XS_MESH_OVER_CAPACITY;
    if (tot[0] > 0x7fffffffull) return xs_set_error(hipErrorInvalidValue, "xs_extract_mesh: more than 2^31 - 1 vertices (int32 indices)");
    if (tot[0] == 0) return 0;
    if (!vertices_dev || !keys_dev || !triangles_dev || (opts->want_normals && !normals_dev))
        return xs_set_error(hipErrorInvalidValue, "xs_extract_mesh: null output array");
    a.verts = vertices_dev; a.keys = keys_dev; a.tris = triangles_dev;
    a.normals = opts->want_normals ? normals_dev : nullptr;
    a.grad = grad; a.vim = grad ? vertex_im_dev : nullptr;
    hipLaunchKernelGGL(k_mesh<2>, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_mesh<3>, grid, block, 0, st, a);
    XS_CHECK(hipGetLastError());
    XS_CHECK(hipStreamSynchronize(st));
    return 0;
}
