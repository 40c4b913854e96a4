// xs_pack.hip — the volume as bricks of 8 x 8 x 8 voxels, each of its three arrays either one word or 512, for gfx950: the
// kernels behind the brick-sparse checkpoint XSTSDF3.  No counterpart in the reference, whose checkpoint is a dense dump.
//
// Classify, gather and unpack share one shape.  A workgroup of four waves takes a RUN of eight bricks adjacent in x: lane = x within the run, so a
// wave's access to a volume row is 64 consecutive words, 256 contiguous bytes, and the lane's brick is lane >> 3.  A brick has 64 rows (8 y by 8 z);
// wave w takes the 16 rows of local planes 2 w and 2 w + 1.  Classify: each lane ORs (word XOR its brick's first-voxel word) over its rows, one
// ballot per wave and array gives eight 8-lane slices, the four waves meet in 96 bytes of LDS and lanes 0 .. 7 of wave 0 write the eight class
// bytes: no atomics, each byte written once.  Rows and columns past the volume's high edge are clamped into the brick: they compare in-volume words
// a second time, which changes nothing, and no load leaves the volume.  Gather and unpack move the dense arrays between volume rows (256-byte
// accesses) and the payload (32-byte pieces of a brick's 512 words); an array that is uniform in every brick of the run costs the wave one test.
//
// The offsets are an exclusive sum of small integers: per 4096 bricks a sum, one workgroup that scans those sums, and a pass that adds the three
// levels up.  Integer sums: the result does not depend on the order.
#include "xs_device.h"
#include "../host/pack_host.hpp"
#include "../../include/xslam_amd.h"

using namespace xs;
using xs_host::pack_class_words;

namespace {
enum { PACK_HEADER_BYTES = 256, SCAN_ITEMS = 16, SCAN_CHUNK = 256 * SCAN_ITEMS };

struct PackArgs {
    const unsigned *arr[3];          // value, weight, grad at the first stored plane, read as words
    size_t step;
    int X, Y, planes;
    int nbx, nby, runs_x;
    const unsigned char *cls;
    const unsigned long long *offsets;
    unsigned long long brick0, brick1, run0;
    unsigned *payload;
};
struct UnpackArgs {
    unsigned *arr[3];
    size_t step;
    int X, Y, planes;
    int nbx, nby, runs_x;
    const unsigned char *cls;
    const unsigned long long *offsets;
    unsigned long long brick0, brick1, run0;
    const unsigned *payload;
};

__device__ __forceinline__ const unsigned *crow(const unsigned *base, size_t step, int Y, int y, int z) {
    return (const unsigned *)((const char *)base + ((size_t)Y * (size_t)z + (size_t)y) * step);
}
__device__ __forceinline__ unsigned *wrow(unsigned *base, size_t step, int Y, int y, int z) {
    return (unsigned *)((char *)base + ((size_t)Y * (size_t)z + (size_t)y) * step);
}

// exclusive sum over the 256 threads of a workgroup (four waves); *total: the sum of all.  s4: four words of LDS.  Two barriers.
__device__ __forceinline__ unsigned long long block_scan_excl(unsigned long long v, unsigned long long *s4, unsigned long long *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(s, o, 64);
        if (lane >= o) s += u;
    }
    __syncthreads();   // (s4 may still be read from the previous round)
    if (lane == 63) s4[wave] = s;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += s4[w];
        all += s4[w];
    }
    *total = all;
    return before + s - v;
}
}  // namespace

// ---- classify ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pack_classify(const unsigned *value, const unsigned *weight, const unsigned *grad, size_t step, int X, int Y,
                                                       int planes, int nbx, int nby, unsigned char *cls) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int by = (int)blockIdx.y, bz = (int)blockIdx.z;
    const int bx = (int)blockIdx.x * 8 + (lane >> 3);
    const bool valid = bx < nbx;
    // clamped into the volume: a lane past the high edge reads a word of its own (or, where its brick does not exist, of some) brick again
    const int x = min((int)blockIdx.x * 64 + lane, X - 1), xf = min(8 * bx, X - 1);
    const unsigned *arr[3] = {value, weight, grad};
    __shared__ unsigned long long s_bal[4][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const unsigned first = crow(arr[a], step, Y, 8 * by, 8 * bz)[xf];
        unsigned w[16];   // the sixteen loads in flight together
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int y = min(8 * by + (r & 7), Y - 1), z = min(8 * bz + 2 * wave + (r >> 3), planes - 1);
            w[r] = __builtin_nontemporal_load(crow(arr[a], step, Y, y, z) + x);
        }
        unsigned diff = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) diff |= w[r] ^ first;
        const unsigned long long m = __ballot(valid && diff != 0u);
        if (lane == 0) s_bal[wave][a] = m;
    }
    __syncthreads();
    if (wave == 0 && lane < 8) {
        const int b = (int)blockIdx.x * 8 + lane;
        if (b < nbx) {
            unsigned c = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const unsigned long long m = s_bal[0][a] | s_bal[1][a] | s_bal[2][a] | s_bal[3][a];
                if ((m >> (8 * lane)) & 0xFFull) c |= 1u << a;
            }
            cls[((size_t)bz * (size_t)nby + (size_t)by) * (size_t)nbx + (size_t)b] = (unsigned char)c;
        }
    }
}

// ---- the offsets: sums of 4096 bricks, a scan of those, the offsets themselves -----------------------------------------------------------
__global__ void __launch_bounds__(256) k_pack_chunk_sums(const unsigned char *cls, unsigned long long nbricks, unsigned long long *sums) {
    __shared__ unsigned long long s4[4];
    const unsigned long long base = (unsigned long long)blockIdx.x * SCAN_CHUNK;
    unsigned long long v = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        const unsigned long long b = base + (unsigned long long)i * 256 + threadIdx.x;
        if (b < nbricks) v += pack_class_words(cls[b]);
    }
    unsigned long long total;
    block_scan_excl(v, s4, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one workgroup: sums[0 .. n) becomes its own exclusive sum, *last the total
__global__ void __launch_bounds__(256) k_pack_scan_sums(unsigned long long *sums, unsigned long long n, unsigned long long *last) {
    __shared__ unsigned long long s4[4];
    unsigned long long carry = 0;
    for (unsigned long long i0 = 0; i0 < n; i0 += 256) {
        const unsigned long long i = i0 + threadIdx.x;
        const unsigned long long v = i < n ? sums[i] : 0ull;
        unsigned long long total;
        const unsigned long long e = block_scan_excl(v, s4, &total);
        if (i < n) sums[i] = carry + e;
        carry += total;
    }
    if (threadIdx.x == 0) *last = carry;
}
__global__ void __launch_bounds__(256) k_pack_offsets(const unsigned char *cls, unsigned long long nbricks, const unsigned long long *sums,
                                                      unsigned long long *offsets) {
    __shared__ unsigned long long s4[4];
    const unsigned long long base = (unsigned long long)blockIdx.x * SCAN_CHUNK;
    unsigned long long carry = sums[blockIdx.x];
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        const unsigned long long b = base + (unsigned long long)i * 256 + threadIdx.x;
        const unsigned long long v = b < nbricks ? pack_class_words(cls[b]) : 0u;
        unsigned long long total;
        const unsigned long long e = block_scan_excl(v, s4, &total);
        if (b < nbricks) offsets[b] = carry + e;
        carry += total;
    }
}

// ---- gather and unpack ------------------------------------------------------------------------------------------------------------------
namespace {
// what a lane of a run knows of its brick
struct LaneBrick {
    int x, i, by, bz;
    bool active;                    // the brick exists and lies in [brick0, brick1)
    unsigned c;                     // its class (0 where inactive)
    unsigned long long pos[3];      // where its value, weight and grad words start in the chunk's payload
    int xf;                         // its first voxel's x
};
template <class A> __device__ __forceinline__ LaneBrick lane_brick(const A &a) {
    LaneBrick L;
    const int lane = threadIdx.x & 63;
    const unsigned long long run = a.run0 + blockIdx.x;
    const int rx = (int)(run % (unsigned long long)a.runs_x);
    const unsigned long long rest = run / (unsigned long long)a.runs_x;
    L.by = (int)(rest % (unsigned long long)a.nby);
    L.bz = (int)(rest / (unsigned long long)a.nby);
    const int bx = rx * 8 + (lane >> 3);
    L.i = lane & 7;
    L.x = rx * 64 + lane;
    L.xf = 8 * bx;
    const unsigned long long b = rest * (unsigned long long)a.nbx + (unsigned long long)bx;
    L.active = bx < a.nbx && b >= a.brick0 && b < a.brick1;
    L.c = 0;
    L.pos[0] = L.pos[1] = L.pos[2] = 0;
    if (L.active) {
        L.c = a.cls[b] & 7u;
        L.pos[0] = a.offsets[b] - a.offsets[a.brick0];
        L.pos[1] = L.pos[0] + ((L.c & 1u) ? 512u : 1u);
        L.pos[2] = L.pos[1] + ((L.c & 2u) ? 512u : 1u);
    }
    return L;
}
}  // namespace

__global__ void __launch_bounds__(256) k_pack_gather(const PackArgs a) {
    const int wave = threadIdx.x >> 6;
    const LaneBrick L = lane_brick(a);
#pragma unroll
    for (int arr = 0; arr < 3; ++arr) {
        const bool dense = L.active && ((L.c >> arr) & 1u);
        const bool any_dense = __ballot(dense) != 0ull;                 // (uniform over the wave)
        const bool writes_one = L.active && !dense && wave == 0 && L.i == 0;
        if (!any_dense && __ballot(writes_one) == 0ull) continue;
        unsigned first = 0;
        if (L.active) first = crow(a.arr[arr], a.step, a.Y, 8 * L.by, 8 * L.bz)[L.xf];   // (always in the volume)
        if (writes_one) a.payload[L.pos[arr]] = first;
        if (!any_dense) continue;
        const bool in_x = L.x < a.X;
#pragma unroll 4
        for (int r = 0; r < 16; ++r) {
            const int j = r & 7, k = 2 * wave + (r >> 3);
            const int y = 8 * L.by + j, z = 8 * L.bz + k;
            if (!dense) continue;
            unsigned w = first;   // positions outside the volume hold the first voxel's word
            if (in_x && y < a.Y && z < a.planes) w = crow(a.arr[arr], a.step, a.Y, y, z)[L.x];
            a.payload[L.pos[arr] + (unsigned)(L.i + 8 * j + 64 * k)] = w;
        }
    }
}

__global__ void __launch_bounds__(256) k_pack_unpack(const UnpackArgs a) {
    const int wave = threadIdx.x >> 6;
    const LaneBrick L = lane_brick(a);
    const bool in_x = L.active && L.x < a.X;
    if (__ballot(in_x) == 0ull) return;
#pragma unroll
    for (int arr = 0; arr < 3; ++arr) {
        const bool dense = (L.c >> arr) & 1u;
        unsigned one = 0;
        if (in_x && !dense) one = a.payload[L.pos[arr]];
#pragma unroll 4
        for (int r = 0; r < 16; ++r) {
            const int j = r & 7, k = 2 * wave + (r >> 3);
            const int y = 8 * L.by + j, z = 8 * L.bz + k;
            if (!in_x || y >= a.Y || z >= a.planes) continue;
            const unsigned w = dense ? a.payload[L.pos[arr] + (unsigned)(L.i + 8 * j + 64 * k)] : one;
            wrow(a.arr[arr], a.step, a.Y, y, z)[L.x] = w;
        }
    }
}

// ---- entry points (include/xslam_amd.h) -------------------------------------------------------------------------------------------------
namespace {
// the refusals the calls share; on success nb3 is the brick grid
int pack_check(const char *who, const void *value, const void *weight, const void *grad, size_t step, const int *res, int planes, int *nb3,
               unsigned long long *nbricks) {
    if (!value || !weight || !grad || !res) return xs_set_error(hipErrorInvalidValue, who);
    const unsigned long long n = xs_host::pack_brick_grid(res[0], res[1], planes, nb3);
    if (n == 0 || res[2] < 1 || res[2] > xs_host::PACK_MAX_AXIS) return xs_set_error(hipErrorInvalidValue, who);
    if (step % 4 != 0 || step < (size_t)res[0] * 4) return xs_set_error(hipErrorInvalidValue, who);
    *nbricks = n;
    return 0;
}
unsigned long long scan_chunks(unsigned long long nbricks) { return (nbricks + SCAN_CHUNK - 1) / SCAN_CHUNK; }

int launch_offsets(const unsigned char *cls, unsigned long long nbricks, unsigned long long *offsets, void *workspace, hipStream_t st) {
    unsigned long long *sums = (unsigned long long *)((char *)workspace + PACK_HEADER_BYTES);
    const unsigned long long chunks = scan_chunks(nbricks);
    hipLaunchKernelGGL(k_pack_chunk_sums, dim3((unsigned)chunks), dim3(256), 0, st, cls, nbricks, sums);
    hipLaunchKernelGGL(k_pack_scan_sums, dim3(1), dim3(256), 0, st, sums, chunks, offsets + nbricks);
    hipLaunchKernelGGL(k_pack_offsets, dim3((unsigned)chunks), dim3(256), 0, st, cls, nbricks, (const unsigned long long *)sums, offsets);
    XS_CHECK(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" size_t xs_tsdf_pack_bricks(const int *res, int planes) {
    if (!res || res[2] < 1 || res[2] > xs_host::PACK_MAX_AXIS) return 0;
    return (size_t)xs_host::pack_brick_grid(res[0], res[1], planes, nullptr);
}

extern "C" size_t xs_tsdf_pack_workspace_bytes(const int *res, int planes) {
    const size_t n = xs_tsdf_pack_bricks(res, planes);
    if (n == 0) return 0;
    return PACK_HEADER_BYTES + ((size_t)scan_chunks(n) * sizeof(unsigned long long) + 255) / 256 * 256;
}

extern "C" int xs_tsdf_pack_offsets(const unsigned char *cls_dev, size_t nbricks, unsigned long long *offsets_dev, void *workspace, void *stream) {
    if (!cls_dev || !offsets_dev || !workspace) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_pack_offsets: null pointer");
    if (nbricks < 1 || nbricks >= ((size_t)1 << 31)) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_pack_offsets: brick count outside [1, 2^31)");
    return launch_offsets(cls_dev, nbricks, offsets_dev, workspace, (hipStream_t)stream);
}

extern "C" int xs_tsdf_pack_classify(const float *value, const int *weight, const float *grad, size_t step, const int *res, int planes,
                                     unsigned char *cls_dev, unsigned long long *offsets_dev, void *workspace, void *stream) {
    int nb[3];
    unsigned long long nbricks = 0;
    if (!cls_dev || !offsets_dev || !workspace) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_pack_classify: null pointer");
    if (int rc = pack_check("xs_tsdf_pack_classify: null array, bad resolution or bad pitch", value, weight, grad, step, res, planes, nb, &nbricks)) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_pack_classify, dim3(div_up(nb[0], 8), nb[1], nb[2]), dim3(256), 0, st, (const unsigned *)value, (const unsigned *)weight,
                       (const unsigned *)grad, step, res[0], res[1], planes, nb[0], nb[1], cls_dev);
    return launch_offsets(cls_dev, nbricks, offsets_dev, workspace, st);
}

namespace {
// the run range of bricks [brick0, brick1): false for a range the contract refuses
template <class A> bool fill_range(A &a, const int *res, int planes, const int *nb, unsigned long long nbricks, size_t brick0, size_t brick1, unsigned *runs) {
    if (brick0 >= brick1 || brick1 > nbricks) return false;
    a.X = res[0]; a.Y = res[1]; a.planes = planes;
    a.nbx = nb[0]; a.nby = nb[1]; a.runs_x = div_up(nb[0], 8);
    a.brick0 = brick0; a.brick1 = brick1;
    auto run_of = [&](unsigned long long b) { return (b / (unsigned long long)a.nbx) * (unsigned long long)a.runs_x + (b % (unsigned long long)a.nbx) / 8; };
    a.run0 = run_of(brick0);
    *runs = (unsigned)(run_of(brick1 - 1) - a.run0 + 1);
    return true;
}
}  // namespace

extern "C" int xs_tsdf_pack_gather(const float *value, const int *weight, const float *grad, size_t step, const int *res, int planes,
                                   const unsigned char *cls_dev, const unsigned long long *offsets_dev, size_t brick0, size_t brick1, unsigned *payload_dev,
                                   void *stream) {
    int nb[3];
    unsigned long long nbricks = 0;
    if (!cls_dev || !offsets_dev || !payload_dev) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_pack_gather: null pointer");
    if (int rc = pack_check("xs_tsdf_pack_gather: null array, bad resolution or bad pitch", value, weight, grad, step, res, planes, nb, &nbricks)) return rc;
    PackArgs a;
    unsigned runs = 0;
    if (!fill_range(a, res, planes, nb, nbricks, brick0, brick1, &runs))
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_pack_gather: empty or reversed brick range, or one outside [0, nbricks]");
    a.arr[0] = (const unsigned *)value; a.arr[1] = (const unsigned *)weight; a.arr[2] = (const unsigned *)grad;
    a.step = step; a.cls = cls_dev; a.offsets = offsets_dev; a.payload = payload_dev;
    hipLaunchKernelGGL(k_pack_gather, dim3(runs), dim3(256), 0, (hipStream_t)stream, a);
    XS_CHECK(hipGetLastError());
    return 0;
}

extern "C" int xs_tsdf_unpack(float *value, int *weight, float *grad, size_t step, const int *res, int planes, const unsigned char *cls_dev,
                              const unsigned long long *offsets_dev, size_t brick0, size_t brick1, const unsigned *payload_dev, void *stream) {
    int nb[3];
    unsigned long long nbricks = 0;
    if (!cls_dev || !offsets_dev || !payload_dev) return xs_set_error(hipErrorInvalidValue, "xs_tsdf_unpack: null pointer");
    if (int rc = pack_check("xs_tsdf_unpack: null array, bad resolution or bad pitch", value, weight, grad, step, res, planes, nb, &nbricks)) return rc;
    UnpackArgs a;
    unsigned runs = 0;
    if (!fill_range(a, res, planes, nb, nbricks, brick0, brick1, &runs))
        return xs_set_error(hipErrorInvalidValue, "xs_tsdf_unpack: empty or reversed brick range, or one outside [0, nbricks]");
    a.arr[0] = (unsigned *)value; a.arr[1] = (unsigned *)weight; a.arr[2] = (unsigned *)grad;
    a.step = step; a.cls = cls_dev; a.offsets = offsets_dev; a.payload = payload_dev;
    hipLaunchKernelGGL(k_pack_unpack, dim3(runs), dim3(256), 0, (hipStream_t)stream, a);
    XS_CHECK(hipGetLastError());
    return 0;
}
