// pack_selftest.cpp — x-slam_amd/host/pack_host.hpp under the host sanitizers, no GPU: the header's layout, the words per class, the brick grid and
// its refusals, the validation of a header with its class bytes rule by rule, the dense format's file rules, the offsets, the partition of the bricks into chunks (no gap, no
// chunk above the staging words, none that one more brick would fit into), and the 64-bit sums at the brick counts of a 1024^3 volume and beyond.
// Built and run by tests/test_pack_cases_cpu.py with -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off.
#include "pack_host.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace xs_host;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next() {   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

static PackHeader header_for(int X, int Y, int Z, int zs0, int zs1, const std::vector<unsigned char> &cls) {
    PackHeader h{};
    std::memcpy(h.p.magic, "XSTSDF3", 8);
    h.p.res[0] = X; h.p.res[1] = Y; h.p.res[2] = Z;
    h.p.voxel_size = 0.01f; h.p.tranc_dist = 0.03f; h.p.frame_id = 3; h.p.n_poses = 2; h.p.zs0 = zs0; h.p.zs1 = zs1; h.p.shard_rank = 0; h.p.shard_count = 1;
    int nb[3] = {0, 0, 0};
    h.nbricks = pack_brick_grid(X, Y, zs1 - zs0, nb);
    h.brick_edge = 8; h.nbx = nb[0]; h.nby = nb[1]; h.nbz = nb[2]; h.reserved = 0;
    uint64_t w = 0;
    for (uint64_t b = 0; b < h.nbricks && b < cls.size(); ++b) w += pack_class_words(cls[b]);
    h.payload_words = w;
    return h;
}
static uint64_t file_bytes_of(const PackHeader &h) {
    return sizeof(PackHeader) + (uint64_t)h.p.n_poses * PACK_POSE_BYTES + pack_class_bytes_padded(h.nbricks) + 4 * h.payload_words;
}

static void test_layout_and_words() {
    CHECK(sizeof(PackHeader) == 88 && offsetof(PackHeader, brick_edge) == 52 && offsetof(PackHeader, nbricks) == 72 && offsetof(PackHeader, payload_words) == 80);
    const unsigned want[8] = {3, 514, 514, 1025, 514, 1025, 1025, 1536};
    for (unsigned c = 0; c < 8; ++c) CHECK(pack_class_words(c) == want[c]);
    CHECK(pack_class_words(7) == PACK_MAX_BRICK_WORDS);
    CHECK(pack_class_bytes_padded(0) == 0 && pack_class_bytes_padded(1) == 4 && pack_class_bytes_padded(4) == 4 && pack_class_bytes_padded(5) == 8);
    CHECK(pack_magic_is("XSTSDF3\0", "XSTSDF3") && !pack_magic_is("XSTSDF3x", "XSTSDF3") && !pack_magic_is("XSTSDF2\0", "XSTSDF3"));
}

static void test_grid() {
    int nb[3];
    CHECK(pack_brick_grid(1, 1, 1, nb) == 1 && nb[0] == 1 && nb[1] == 1 && nb[2] == 1);
    CHECK(pack_brick_grid(72, 16, 8, nb) == 18 && nb[0] == 9 && nb[1] == 2 && nb[2] == 1);
    CHECK(pack_brick_grid(17, 9, 10, nb) == 12 && nb[0] == 3 && nb[1] == 2 && nb[2] == 2);
    CHECK(pack_brick_grid(1024, 1024, 1024, nb) == 2097152ull && nb[0] == 128);
    CHECK(pack_brick_grid(262140, 8, 8, nullptr) == 32768 && pack_brick_grid(262141, 8, 8, nullptr) == 0);
    CHECK(pack_brick_grid(0, 8, 8, nullptr) == 0 && pack_brick_grid(8, -1, 8, nullptr) == 0 && pack_brick_grid(8, 8, 0, nullptr) == 0);
    CHECK(pack_brick_grid(8, 65536, 32768, nullptr) == 0);          // 2^31 rows
    CHECK(pack_brick_grid(8, 65536, 32767, nullptr) == 8192ull * 4096ull);
    CHECK(pack_brick_grid(262140, 46340, 46340, nullptr) == 0);     // 2^31 bricks and more
    nb[0] = nb[1] = nb[2] = -5;
    CHECK(pack_brick_grid(0, 8, 8, nb) == 0 && nb[0] == -5);          // untouched on refusal
}

static void test_validation() {
    std::vector<unsigned char> cls(pack_class_bytes_padded(12), 0);   // 17 x 9 x 10: 12 bricks
    for (int b = 0; b < 12; ++b) cls[(size_t)b] = (unsigned char)(b % 8);
    const PackHeader good = header_for(17, 9, 10, 0, 10, cls);
    uint64_t hist[8];
    CHECK(pack_validate(good, cls.data(), file_bytes_of(good), hist) == PACK_OK);
    CHECK(hist[0] == 2 && hist[3] == 2 && hist[4] == 1 && hist[7] == 1);
    CHECK(pack_validate(good, cls.data(), file_bytes_of(good), nullptr) == PACK_OK);
    CHECK(pack_validate(good, cls.data(), file_bytes_of(good) - 4, nullptr) == PACK_BAD_LENGTH);
    CHECK(pack_validate(good, cls.data(), file_bytes_of(good) + 1, nullptr) == PACK_BAD_LENGTH);
    CHECK(pack_validate(good, nullptr, file_bytes_of(good), nullptr) == PACK_BAD_LENGTH);
    CHECK(pack_validate(good, cls.data(), 88 + 256 + 11, nullptr) == PACK_BAD_LENGTH);   // ends inside the class bytes: they are not read
    PackHeader h = good;
    h.p.magic[6] = '2';
    CHECK(pack_validate(h, cls.data(), file_bytes_of(h), nullptr) == PACK_BAD_MAGIC);
    h = good; h.brick_edge = 4;
    CHECK(pack_validate(h, cls.data(), file_bytes_of(h), nullptr) == PACK_BAD_BRICK_EDGE);
    h = good; h.reserved = 1;
    CHECK(pack_validate(h, cls.data(), file_bytes_of(h), nullptr) == PACK_BAD_RESERVED);
    h = good; h.nbx += 1;
    CHECK(pack_validate(h, cls.data(), file_bytes_of(h), nullptr) == PACK_BAD_GRID);
    h = good; h.nbz = 1;
    CHECK(pack_validate(h, cls.data(), file_bytes_of(h), nullptr) == PACK_BAD_GRID);
    h = good; h.nbricks = 13;
    CHECK(pack_validate(h, cls.data(), file_bytes_of(h), nullptr) == PACK_BAD_GRID);
    h = good; h.p.res[0] = 0;
    CHECK(pack_validate(h, cls.data(), file_bytes_of(h), nullptr) == PACK_BAD_GEOMETRY);
    h = good; h.p.zs1 = 11;   // past res[2]
    CHECK(pack_validate(h, cls.data(), file_bytes_of(h), nullptr) == PACK_BAD_GEOMETRY);
    h = good; h.p.zs0 = 10;   // empty
    CHECK(pack_validate(h, cls.data(), file_bytes_of(h), nullptr) == PACK_BAD_GEOMETRY);
    h = good; h.p.n_poses = 0;
    CHECK(pack_validate(h, cls.data(), file_bytes_of(h), nullptr) == PACK_BAD_POSES);
    h = good; h.p.n_poses = PACK_MAX_POSES + 1;
    CHECK(pack_validate(h, cls.data(), file_bytes_of(h), nullptr) == PACK_BAD_POSES);
    h = good; h.payload_words += 1;
    CHECK(pack_validate(h, cls.data(), file_bytes_of(h), nullptr) == PACK_BAD_PAYLOAD_WORDS);
    std::vector<unsigned char> bad = cls;
    bad[5] = 8;
    CHECK(pack_validate(good, bad.data(), file_bytes_of(good), nullptr) == PACK_BAD_CLASS);
    bad = cls; bad[3] = 255;
    CHECK(pack_validate(good, bad.data(), file_bytes_of(good), nullptr) == PACK_BAD_CLASS);
    // 10 bricks are padded by two bytes, which are zero
    std::vector<unsigned char> ten(pack_class_bytes_padded(10), 0);
    const PackHeader h10 = header_for(80, 8, 8, 0, 8, ten);
    CHECK(h10.nbricks == 10 && ten.size() == 12 && pack_validate(h10, ten.data(), file_bytes_of(h10), nullptr) == PACK_OK);
    ten[11] = 1;
    CHECK(pack_validate(h10, ten.data(), file_bytes_of(h10), nullptr) == PACK_BAD_CLASS);
    // a rank's planes: the grid follows zs1 - zs0
    std::vector<unsigned char> rk(pack_class_bytes_padded(18), 0);
    const PackHeader hr = header_for(17, 9, 64, 24, 41, rk);
    CHECK(hr.nbricks == 18 && hr.nbz == 3 && pack_validate(hr, rk.data(), file_bytes_of(hr), nullptr) == PACK_OK);
}

// pack_validate_dense: the accepted XSTSDF2 file, and one case per PackError it can return
static void test_dense_validation() {
    PackHeader h3 = header_for(17, 9, 64, 24, 41, {});
    CkptPrefix good = h3.p;   // a rank's planes of a 17 x 9 x 64 volume, two poses
    good.magic[6] = '2';
    const uint64_t words = 3ull * 17 * 9 * 17, bytes = 52 + 2 * 128 + 4 * words;
    auto with = [&](void (*change)(CkptPrefix &)) { CkptPrefix p = good; change(p); return p; };
    struct Row { CkptPrefix p; uint64_t file_bytes; PackError want; const char *what; };
    const Row rows[] = {
        {good, bytes, PACK_OK, "the file"},
        {h3.p, bytes, PACK_BAD_MAGIC, "the sparse format's magic"},
        {with([](CkptPrefix &p) { p.magic[7] = 'x'; }), bytes, PACK_BAD_MAGIC, "a magic without its NUL"},
        {with([](CkptPrefix &p) { p.res[2] = 0; }), bytes, PACK_BAD_GEOMETRY, "no planes in the volume"},
        {with([](CkptPrefix &p) { p.zs0 = -1; }), bytes, PACK_BAD_GEOMETRY, "a first plane below 0"},
        {with([](CkptPrefix &p) { p.zs1 = p.zs0; }), bytes, PACK_BAD_GEOMETRY, "no stored plane"},
        {with([](CkptPrefix &p) { p.zs1 = 65; }), bytes, PACK_BAD_GEOMETRY, "planes past the resolution"},
        {with([](CkptPrefix &p) { p.res[0] = 0; }), bytes, PACK_BAD_GEOMETRY, "an axis the brick grid refuses"},
        {with([](CkptPrefix &p) { p.res[1] = PACK_MAX_AXIS + 1; }), bytes, PACK_BAD_GEOMETRY, "an axis above the brick grid's bound"},
        {with([](CkptPrefix &p) { p.n_poses = 0; }), bytes, PACK_BAD_POSES, "no pose"},
        {with([](CkptPrefix &p) { p.n_poses = PACK_MAX_POSES + 1; }), bytes, PACK_BAD_POSES, "more poses than the bound"},
        {good, bytes - 4, PACK_BAD_LENGTH, "a truncated file"},
        {good, bytes + 1, PACK_BAD_LENGTH, "trailing bytes"},
        {with([](CkptPrefix &p) { p.n_poses = 3; }), bytes, PACK_BAD_LENGTH, "a pose the length does not hold"},
    };
    for (const Row &r : rows) {
        uint64_t w = 77;
        const PackError got = pack_validate_dense(r.p, r.file_bytes, &w);
        if (got != r.want) { std::printf("FAILED pack_validate_dense: %s: %d\n", r.what, (int)got); ++failures; }
        // the words are reported once geometry and pose count hold, whatever the length
        CHECK(w == ((got == PACK_OK || got == PACK_BAD_LENGTH) ? words : 77));
        CHECK(pack_validate_dense(r.p, r.file_bytes, nullptr) == got);
    }
    // a whole 1024^3 volume: the length passes 2^33 bytes
    h3 = header_for(1024, 1024, 1024, 0, 1024, {});
    h3.p.magic[6] = '2';
    uint64_t w = 0;
    CHECK(pack_validate_dense(h3.p, 52 + 256 + 12884901888ull, &w) == PACK_OK && w == 3221225472ull);
}

static void check_partition(const std::vector<uint64_t> &offsets, uint64_t staging) {
    const uint64_t n = offsets.size() - 1;
    uint64_t b0 = 0, chunks = 0;
    while (b0 < n) {
        const uint64_t b1 = pack_chunk_end(offsets.data(), n, b0, staging);
        CHECK(b1 > b0 && b1 <= n);
        if (b1 <= b0 || b1 > n) return;
        CHECK(offsets[b1] - offsets[b0] <= staging);
        CHECK(b1 == n || offsets[b1 + 1] - offsets[b0] > staging);
        b0 = b1;
        ++chunks;
    }
    CHECK(b0 == n && chunks >= (offsets[n] + staging - 1) / staging);
}

static void test_offsets_and_partition() {
    for (uint64_t n : {1ull, 2ull, 7ull, 100ull, 4097ull}) {
        std::vector<unsigned char> cls(n);
        for (auto &c : cls) c = (unsigned char)(next() % 8);
        std::vector<uint64_t> off(n + 1);
        pack_offsets(cls.data(), n, off.data());
        uint64_t s = 0;
        for (uint64_t b = 0; b < n; ++b) { CHECK(off[b] == s); s += pack_class_words(cls[b]); }
        CHECK(off[n] == s);
        for (uint64_t staging : {1536ull, 1537ull, 3000ull, 65536ull, 1ull << 40}) check_partition(off, staging);
        CHECK(pack_chunk_end(off.data(), n, 0, 1535) == 0 && pack_chunk_end(off.data(), n, n, 4096) == 0 && pack_chunk_end(nullptr, n, 0, 4096) == 0);
    }
    // every brick dense at the brick count of 1024^3: the sums pass 2^31 and 2^32 words, the chunks of a 64 MiB buffer hold 10 922 bricks each
    const uint64_t n = pack_brick_grid(1024, 1024, 1024, nullptr);
    std::vector<unsigned char> cls(n, 7);
    std::vector<uint64_t> off(n + 1);
    pack_offsets(cls.data(), n, off.data());
    CHECK(off[n] == 3221225472ull && off[n] > (1ull << 31) && off[n / 2 + 1] - off[n / 2] == 1536);
    CHECK(pack_chunk_end(off.data(), n, 0, 16ull << 20) == 10922 && pack_chunk_end(off.data(), n, n - 5, 16ull << 20) == n);
    check_partition(off, 16ull << 20);
    PackHeader h = header_for(1024, 1024, 1024, 0, 1024, cls);
    CHECK(h.payload_words == 3221225472ull && file_bytes_of(h) == 88 + 256 + 2097152ull + 12884901888ull);
    CHECK(pack_validate(h, cls.data(), file_bytes_of(h), nullptr) == PACK_OK);
    // the largest grid the format admits: 2^31 - 2^16 bricks, all dense, would be 3.3e12 words: the histogram's product stays in 64 bits
    CHECK((uint64_t)((1ull << 31) - 1) * PACK_MAX_BRICK_WORDS < (1ull << 63));
}

int main() {
    test_layout_and_words();
    test_grid();
    test_validation();
    test_dense_validation();
    test_offsets_and_partition();
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all checks held\n");
    return 0;
}
