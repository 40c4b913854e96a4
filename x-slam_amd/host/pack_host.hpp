// pack_host.hpp — the host's side of the brick-sparse volume checkpoint XSTSDF3 (INTEGRATION.md "Checkpoint formats"):
// the file header, the words a brick of a given class takes in the payload, the validation of a header with its class bytes against the file's
// length, the exclusive sum of the words per brick, the partition of the bricks into chunks that fit a staging buffer, and the file rules of the
// dense XSTSDF2.  No device call and no HIP header: kf_checkpoint.cpp uses it around the kernels of csrc/xs_pack.hip, in its reader and for
// xs_host_checkpoint_info, xs_pack.hip itself for the brick grid, and tests/cxx/pack_selftest.cpp runs all of it under the sanitizers without a GPU.
//
// The file, little endian:  PackHeader (88 bytes) | n_poses x 128 bytes (Matrix4cf, as XSTSDF2) | nbricks class bytes, zero-padded to a multiple of 4 |
// payload_words 32-bit words.  Brick (bx, by, bz) of 8 x 8 x 8 voxels, bz counted from the first stored plane, has index (bz nby + by) nbx + bx.
// Class bit 0 / 1 / 2 set: the brick's value / weight / grad words are stored densely (512 words, local voxel (i, j, k) at i + 8 j + 64 k, positions
// outside the volume holding the first voxel's word); clear: every in-volume word of that array equals the word at the brick's first voxel, and
// that one word is stored.  Within a brick: value, weight, grad.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define XS_PACK_HD __host__ __device__
#else
#define XS_PACK_HD
#endif

namespace xs_host {

enum { PACK_BRICK_EDGE = 8, PACK_BRICK_WORDS = 512, PACK_MAX_BRICK_WORDS = 3 * 512, PACK_POSE_BYTES = 128, PACK_MAX_AXIS = 65535 * 4,
       PACK_MAX_POSES = 1 << 24 };   // (the pose bound of XSTSDF2: a sanity bound, not a format limit)

// the 52 bytes XSTSDF2 and XSTSDF3 share
struct CkptPrefix {
    char magic[8];
    int32_t res[3];
    float voxel_size, tranc_dist;
    int32_t frame_id, n_poses;
    int32_t zs0, zs1;        // planes held in this file
    int32_t shard_rank, shard_count;
};
struct PackHeader {
    CkptPrefix p;
    int32_t brick_edge, nbx, nby, nbz, reserved;
    uint64_t nbricks, payload_words;
};
static_assert(sizeof(CkptPrefix) == 52 && sizeof(PackHeader) == 88, "XSTSDF3 header layout");

inline bool pack_magic_is(const char *magic8, const char *want7) { return std::memcmp(magic8, want7, 7) == 0 && magic8[7] == 0; }

// words of the payload a brick of class c takes: 1 or 512 per array
XS_PACK_HD inline unsigned pack_class_words(unsigned c) {
    return ((c & 1u) ? 512u : 1u) + ((c & 2u) ? 512u : 1u) + ((c & 4u) ? 512u : 1u);
}

// the brick grid of X x Y x planes voxels; 0 (and nb3 untouched) for an axis outside 1 .. 262140, more rows than 2^31 - 1 or 2^31 bricks and more
inline uint64_t pack_brick_grid(int X, int Y, int planes, int *nb3) {
    if (X < 1 || Y < 1 || planes < 1 || X > PACK_MAX_AXIS || Y > PACK_MAX_AXIS || planes > PACK_MAX_AXIS) return 0;
    if ((long long)Y * (long long)planes >= (1ll << 31)) return 0;
    const int nb[3] = {(X + 7) / 8, (Y + 7) / 8, (planes + 7) / 8};
    const uint64_t n = (uint64_t)nb[0] * (uint64_t)nb[1] * (uint64_t)nb[2];
    if (n >= (1ull << 31)) return 0;
    if (nb3) { nb3[0] = nb[0]; nb3[1] = nb[1]; nb3[2] = nb[2]; }
    return n;
}

inline uint64_t pack_class_bytes_padded(uint64_t nbricks) { return (nbricks + 3) / 4 * 4; }

// What pack_validate found; 0 is a valid file.
enum PackError { PACK_OK = 0, PACK_BAD_MAGIC, PACK_BAD_GEOMETRY, PACK_BAD_BRICK_EDGE, PACK_BAD_RESERVED, PACK_BAD_GRID, PACK_BAD_POSES, PACK_BAD_CLASS,
                 PACK_BAD_PAYLOAD_WORDS, PACK_BAD_LENGTH };

// The header alone: magic, geometry, brick grid, pose count.  The length of the file up to the class bytes' end is returned in *head_bytes.
inline PackError pack_validate_header(const PackHeader &h, uint64_t *head_bytes) {
    if (!pack_magic_is(h.p.magic, "XSTSDF3")) return PACK_BAD_MAGIC;
    if (h.brick_edge != PACK_BRICK_EDGE) return PACK_BAD_BRICK_EDGE;
    if (h.reserved != 0) return PACK_BAD_RESERVED;
    if (h.p.res[2] < 1 || h.p.res[2] > PACK_MAX_AXIS || h.p.zs0 < 0 || h.p.zs1 <= h.p.zs0 || h.p.zs1 > h.p.res[2]) return PACK_BAD_GEOMETRY;
    int nb[3];
    const uint64_t n = pack_brick_grid(h.p.res[0], h.p.res[1], h.p.zs1 - h.p.zs0, nb);
    if (n == 0) return PACK_BAD_GEOMETRY;
    if (h.nbx != nb[0] || h.nby != nb[1] || h.nbz != nb[2] || h.nbricks != n) return PACK_BAD_GRID;
    if (h.p.n_poses < 1 || h.p.n_poses > PACK_MAX_POSES) return PACK_BAD_POSES;
    if (head_bytes) *head_bytes = sizeof(PackHeader) + (uint64_t)h.p.n_poses * PACK_POSE_BYTES + pack_class_bytes_padded(n);
    return PACK_OK;
}

// The whole of the format's validation: the header, every class byte (and its zero padding), the sum of the words per class against
// payload_words, and the exact file length.  cls: the pack_class_bytes_padded(nbricks) bytes behind the poses (only read once the header
// holds and file_bytes says they are there: pass what was read, or null when the file ends before them).  hist8 (optional): bricks per class.
inline PackError pack_validate(const PackHeader &h, const unsigned char *cls, uint64_t file_bytes, uint64_t *hist8) {
    uint64_t head = 0;
    if (PackError e = pack_validate_header(h, &head)) return e;
    if (file_bytes < head || !cls) return PACK_BAD_LENGTH;
    uint64_t hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint64_t b = 0; b < h.nbricks; ++b) {
        if (cls[b] > 7) return PACK_BAD_CLASS;
        ++hist[cls[b]];
    }
    for (uint64_t b = h.nbricks; b < pack_class_bytes_padded(h.nbricks); ++b)
        if (cls[b] != 0) return PACK_BAD_CLASS;
    uint64_t words = 0;   // at most 2^31 bricks of 1536 words: no overflow
    for (unsigned c = 0; c < 8; ++c) words += hist[c] * pack_class_words(c);
    if (hist8) for (int c = 0; c < 8; ++c) hist8[c] = hist[c];
    if (words != h.payload_words) return PACK_BAD_PAYLOAD_WORDS;
    if (file_bytes != head + 4 * words) return PACK_BAD_LENGTH;   // truncated or trailing bytes
    return PACK_OK;
}

// The dense XSTSDF2 file (prefix | n_poses x 128 bytes | value, grad, weight of the stored planes as dense rows): the magic, the planes within the
// resolution, a brick grid pack_brick_grid accepts (the bounds both formats share), the pose count and the exact length.  *words (optional): the
// 32-bit words of the three arrays, written once geometry and pose count hold.
inline PackError pack_validate_dense(const CkptPrefix &p, uint64_t file_bytes, uint64_t *words) {
    if (!pack_magic_is(p.magic, "XSTSDF2")) return PACK_BAD_MAGIC;
    if (p.res[2] < 1 || p.zs0 < 0 || p.zs1 <= p.zs0 || p.zs1 > p.res[2] || pack_brick_grid(p.res[0], p.res[1], p.zs1 - p.zs0, nullptr) == 0) return PACK_BAD_GEOMETRY;
    if (p.n_poses < 1 || p.n_poses > PACK_MAX_POSES) return PACK_BAD_POSES;
    const uint64_t w = 3ull * (uint64_t)p.res[0] * (uint64_t)p.res[1] * (uint64_t)(p.zs1 - p.zs0);
    if (words) *words = w;
    if (file_bytes != sizeof(CkptPrefix) + (uint64_t)p.n_poses * PACK_POSE_BYTES + 4 * w) return PACK_BAD_LENGTH;   // truncated or trailing bytes
    return PACK_OK;
}

// offsets[nbricks + 1]: the exclusive sum of the words per brick, the last entry the payload's length (what xs_tsdf_pack_offsets computes on the device)
inline void pack_offsets(const unsigned char *cls, uint64_t nbricks, uint64_t *offsets) {
    uint64_t s = 0;
    for (uint64_t b = 0; b < nbricks; ++b) { offsets[b] = s; s += pack_class_words(cls[b]); }
    offsets[nbricks] = s;
}

// The end of the chunk that starts at brick b0: the largest b1 in (b0, nbricks] with offsets[b1] - offsets[b0] <= staging_words, by bisection over
// the non-decreasing offsets.  staging_words >= PACK_MAX_BRICK_WORDS, so b1 > b0 always; 0 for arguments that break that.
inline uint64_t pack_chunk_end(const uint64_t *offsets, uint64_t nbricks, uint64_t b0, uint64_t staging_words) {
    if (!offsets || b0 >= nbricks || staging_words < PACK_MAX_BRICK_WORDS) return 0;
    const uint64_t limit = offsets[b0] + staging_words;
    uint64_t lo = b0 + 1, hi = nbricks;   // offsets[lo] <= limit holds throughout
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= limit) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace xs_host
