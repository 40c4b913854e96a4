"""The cases that hold the brick-sparse checkpoint (xs_tsdf_pack_classify, xs_tsdf_pack_gather, xs_tsdf_unpack of x-slam_amd/csrc/xs_pack.hip; the
file format XSTSDF3) to a numpy model written from the contract in include/xslam_amd.h and INTEGRATION.md, not from the kernels: everything is
a comparison of 32-bit words, so the model is exact.  Backend-neutral (tests/test_pack_cases_cpu.py runs it without a GPU; tests/test_pack_gpu.py
and tests/test_pack_pipeline_gpu.py hold the kernels and the orchestrator to it).  Test infrastructure.

A volume here is three uint32 arrays [planes, Y, X] (value, weight, grad as words).  Brick (bx, by, bz) of 8 x 8 x 8 voxels has index
(bz nby + by) nbx + bx; class bit a is set iff some in-volume word of array a differs from the word at the brick's first voxel; a uniform array
takes one word of the payload, a dense array 512 (local voxel (i, j, k) at i + 8 j + 64 k, positions outside the volume holding the first voxel's
word); within a brick value, weight, grad."""
import functools
import struct

import numpy as np

HEADER = struct.Struct("<8s3iff2i4i5iQQ")
assert HEADER.size == 88
POSE_BYTES = 128
NAN_A, NAN_B = 0x7FC00000, 0x7FC00001
NEG_ZERO = 0x80000000

# (X, Y, planes): the smallest shapes at which the kernels can go wrong.  A workgroup takes a run of 8 bricks along x.
SHAPES = [(1, 1, 1), (2, 3, 5),
          (8, 8, 8),                          # one exact brick
          (9, 8, 8), (8, 9, 8), (8, 8, 9),    # one ragged axis each
          (17, 9, 10),
          (64, 8, 8),                         # one exact run
          (72, 16, 8)]                        # nine bricks along x: a run and a ragged run
# last rows beyond 2^31 bytes from the array base at a pitch of 4096 bytes: 2.1 GiB per array on the device, 16 640 bricks for the model
BIG = (16, 1024, 513)
BIG_PITCH = 4096


def grid(shape):
    X, Y, P = shape
    return -(-X // 8), -(-Y // 8), -(-P // 8)


def nbricks(shape):
    nb = grid(shape)
    return nb[0] * nb[1] * nb[2]


def class_words(c):
    c = np.asarray(c).astype(np.int64)
    return 3 + 511 * ((c & 1) + (c >> 1 & 1) + (c >> 2 & 1))


def words(a):
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    return a.view(np.uint32)


# ------------------------------------------------------------------------------------------------
# The model
def _blocks(a):
    """a [P, Y, X] uint32 -> (blocks [nbricks, 512] with the first voxel's word outside the volume, first [nbricks], inside [nbricks, 512])."""
    P, Y, X = a.shape
    nbx, nby, nbz = grid((X, Y, P))
    pad = np.zeros((nbz * 8, nby * 8, nbx * 8), np.uint32)
    pad[:P, :Y, :X] = a
    inside = np.zeros(pad.shape, bool)
    inside[:P, :Y, :X] = True

    def bricked(t):
        return t.reshape(nbz, 8, nby, 8, nbx, 8).transpose(0, 2, 4, 1, 3, 5).reshape(nbz * nby * nbx, 512)   # [brick, k j i]

    b, m = bricked(pad), bricked(inside)
    first = b[:, 0].copy()
    return np.where(m, b, first[:, None]), first, m


def classify(v, w, g):
    """(cls [nbricks] uint8, offsets [nbricks + 1] uint64)."""
    cls = np.zeros(nbricks(words(v).shape[::-1]), np.uint8)
    for a, arr in enumerate((v, w, g)):
        b, first, _ = _blocks(words(arr))
        cls |= ((b != first[:, None]).any(axis=1).astype(np.uint8) << a).astype(np.uint8)
    offsets = np.concatenate([[0], np.cumsum(class_words(cls))]).astype(np.uint64)
    return cls, offsets


def gather(v, w, g, cls, offsets, b0=0, b1=None):
    """The payload words of bricks [b0, b1) as uint32, starting at word 0."""
    b1 = len(cls) if b1 is None else b1
    blocks = [_blocks(words(arr)) for arr in (v, w, g)]
    out = np.zeros(int(offsets[b1]) - int(offsets[b0]), np.uint32)
    for b in range(b0, b1):
        pos = int(offsets[b]) - int(offsets[b0])
        for a in range(3):
            if cls[b] >> a & 1:
                out[pos:pos + 512] = blocks[a][0][b]
                pos += 512
            else:
                out[pos] = blocks[a][1][b]
                pos += 1
        assert pos == int(offsets[b + 1]) - int(offsets[b0])
    return out


def unpack(out, cls, offsets, payload, b0=0, b1=None):
    """Writes bricks [b0, b1) from payload (laid out as gather(b0, b1) leaves it) into out = (v, w, g) uint32 [P, Y, X], in place."""
    P, Y, X = out[0].shape
    nbx, nby, nbz = grid((X, Y, P))
    b1 = len(cls) if b1 is None else b1
    for b in range(b0, b1):
        bx, by, bz = b % nbx, b // nbx % nby, b // (nbx * nby)
        pos = int(offsets[b]) - int(offsets[b0])
        sl = (slice(8 * bz, min(8 * bz + 8, P)), slice(8 * by, min(8 * by + 8, Y)), slice(8 * bx, min(8 * bx + 8, X)))
        ext = tuple(s.stop - s.start for s in sl)
        for a in range(3):
            if cls[b] >> a & 1:
                out[a][sl] = payload[pos:pos + 512].reshape(8, 8, 8)[:ext[0], :ext[1], :ext[2]]
                pos += 512
            else:
                out[a][sl] = payload[pos]
                pos += 1


def chunk_ends(offsets, staging_words):
    """The host's partition: from b0 the largest b1 with offsets[b1] - offsets[b0] <= staging_words; [b0, b1) pairs covering every brick."""
    assert staging_words >= 1536
    n, out, b0 = len(offsets) - 1, [], 0
    while b0 < n:
        b1 = b0 + 1
        while b1 < n and int(offsets[b1 + 1]) - int(offsets[b0]) <= staging_words:
            b1 += 1
        out.append((b0, b1))
        b0 = b1
    return out


# ------------------------------------------------------------------------------------------------
# The file
def write_xstsdf3(v, w, g, res=None, voxel_size=0.01, tranc_dist=0.03, frame_id=1, poses=None, zs0=0, shard=(0, 1)):
    """The file's bytes for the volume (v, w, g) [planes, Y, X], the planes being [zs0, zs0 + planes) of a volume of resolution res
    (None: the arrays' own shape)."""
    P, Y, X = words(v).shape
    res = (X, Y, P) if res is None else tuple(res)
    poses = bytes(POSE_BYTES) if poses is None else bytes(poses)
    assert len(poses) % POSE_BYTES == 0 and len(poses) > 0
    cls, offsets = classify(v, w, g)
    nb = grid((X, Y, P))
    head = HEADER.pack(b"XSTSDF3\0", res[0], res[1], res[2], voxel_size, tranc_dist, frame_id, len(poses) // POSE_BYTES, zs0, zs0 + P, shard[0], shard[1],
                       8, nb[0], nb[1], nb[2], 0, len(cls), int(offsets[-1]))
    return head + poses + cls.tobytes() + bytes(-len(cls) % 4) + gather(v, w, g, cls, offsets).tobytes()


def read_xstsdf3(blob):
    """The reader, with the format's whole validation: ValueError naming the first rule broken.  Returns a dict: the header's fields, poses (bytes),
    cls, offsets, and the volume as three uint32 arrays [planes, Y, X]."""
    if len(blob) < HEADER.size:
        raise ValueError("length")
    (magic, X, Y, Z, vs, td, frame_id, n_poses, zs0, zs1, rank, count, edge, nbx, nby, nbz, reserved, nb, payload_words) = HEADER.unpack(blob[:HEADER.size])
    if magic != b"XSTSDF3\0":
        raise ValueError("magic")
    if edge != 8:
        raise ValueError("brick_edge")
    if reserved != 0:
        raise ValueError("reserved")
    if min(X, Y, Z) < 1 or max(X, Y, Z) > 262140 or not 0 <= zs0 < zs1 <= Z:
        raise ValueError("geometry")
    shape = (X, Y, zs1 - zs0)
    if (nbx, nby, nbz) != grid(shape) or nb != nbricks(shape):
        raise ValueError("brick_grid")
    if not 1 <= n_poses <= 1 << 24:
        raise ValueError("poses")
    at = HEADER.size + n_poses * POSE_BYTES
    padded = -(-nb // 4) * 4
    if len(blob) < at + padded:
        raise ValueError("length")
    cls = np.frombuffer(blob, np.uint8, padded, at)
    if (cls > 7).any() or cls[nb:].any():
        raise ValueError("class_byte")
    cls = cls[:nb].copy()
    offsets = np.concatenate([[0], np.cumsum(class_words(cls))]).astype(np.uint64)
    if int(offsets[-1]) != payload_words:
        raise ValueError("payload_words")
    if len(blob) != at + padded + 4 * payload_words:
        raise ValueError("length")
    payload = np.frombuffer(blob, np.uint32, payload_words, at + padded)
    out = tuple(np.zeros(shape[::-1], np.uint32) for _ in range(3))
    unpack(out, cls, offsets, payload)
    return dict(res=(X, Y, Z), voxel_size=vs, tranc_dist=td, frame_id=frame_id, n_poses=n_poses, planes=(zs0, zs1), shard=(rank, count), brick_grid=(nbx, nby, nbz),
                bricks=nb, payload_words=payload_words, poses=blob[HEADER.size:at], cls=cls, offsets=offsets, volume=out)


def bad_files(blob):
    """name -> bytes: each breaks one rule of the validation (blob: a valid file with one pose)."""
    h = list(HEADER.unpack(blob[:HEADER.size]))
    at = HEADER.size + h[7] * POSE_BYTES

    def with_header(**kw):
        f = list(h)
        for k, v in kw.items():
            f[dict(edge=12, nbx=13, nby=14, nbz=15, reserved=16, nbricks=17, payload_words=18)[k]] = v
        return HEADER.pack(*f) + blob[HEADER.size:]

    X, Y, P = h[1], h[2], h[9] - h[8]
    dense = blob[:8].replace(b"3", b"2") + blob[8:52] + blob[HEADER.size:at] + bytes(12 * X * Y * P)      # a valid XSTSDF2 file of the same geometry
    return {"truncated": blob[:-4], "trailing": blob + bytes(4), "class_8": blob[:at] + b"\x08" + blob[at + 1:],
            "payload_words": with_header(payload_words=h[18] + 1), "reserved": with_header(reserved=1), "brick_edge": with_header(edge=4),
            "grid": with_header(nbx=h[13] + 1), "nbricks": with_header(nbricks=h[17] + 1), "v2_body": b"XSTSDF3\0" + dense[8:]}, dense


# ------------------------------------------------------------------------------------------------
# Case data
def _u32(x, dtype):
    return int(np.array([x], dtype).view(np.uint32)[0])


@functools.lru_cache(maxsize=None)
def volume(shape):
    """(v, w, g) uint32 [planes, Y, X], never modified, and the class every brick was built to have.  Brick b aims at class (b + X + Y + planes + 7)
    % 8; each of its dense arrays differs from uniform in one of seven ways, by (3 b + array) % 7: only local voxel (1, 0, 0); only (7, 7, 7);
    only the brick's last in-volume voxel; +0.0 with one -0.0; one NaN payload with one voxel of another; random words; the first voxel alone.
    Where the brick has no such voxel the last in-volume voxel stands in, and a brick of one voxel stays uniform.  Uniform arrays hold 1.0 / a
    weight / 0.0, every third brick a negative weight, every fifth one NaN pattern throughout its value array."""
    X, Y, P = shape
    rng = np.random.default_rng(1000003 * X + 1009 * Y + P)
    nbx, nby, nbz = grid(shape)
    out = [np.zeros((P, Y, X), np.uint32) for _ in range(3)]
    want = np.zeros(nbricks(shape), np.uint8)
    for b in range(nbricks(shape)):
        bx, by, bz = b % nbx, b // nbx % nby, b // (nbx * nby)
        ext = (min(8, X - 8 * bx), min(8, Y - 8 * by), min(8, P - 8 * bz))           # (i, j, k) extents
        target = (b + X + Y + P + 7) % 8
        base = [_u32(1.0, np.float32), _u32(-3 if b % 3 == 0 else 1 + b % 90, np.int32), _u32(0.0, np.float32)]
        if b % 5 == 1:
            base[0] = NAN_A
        for a in range(3):
            blk = np.full((ext[2], ext[1], ext[0]), base[a], np.uint32)               # [k, j, i]
            if target >> a & 1 and ext != (1, 1, 1):
                kind = (3 * b + a) % 7
                last = (ext[2] - 1, ext[1] - 1, ext[0] - 1)
                spot = {0: (0, 0, 1), 1: (7, 7, 7)}.get(kind, last)
                if any(spot[d] >= blk.shape[d] for d in range(3)):
                    spot = last
                if kind == 3:
                    blk[:] = 0
                    blk[spot] = NEG_ZERO
                elif kind == 4:
                    blk[:] = NAN_A
                    blk[spot] = NAN_B
                elif kind == 5:
                    blk[:] = rng.integers(0, 2 ** 32, blk.shape, dtype=np.uint32)
                    blk[last] = blk[0, 0, 0] ^ 1
                elif kind == 6:
                    blk[0, 0, 0] ^= 0x00400000
                else:
                    blk[spot] ^= 1                                                    # one bit of one word
                want[b] |= 1 << a
            out[a][8 * bz:8 * bz + ext[2], 8 * by:8 * by + ext[1], 8 * bx:8 * bx + ext[0]] = blk
    for a in out:
        a.setflags(write=False)
    want.setflags(write=False)
    return tuple(out), want


@functools.lru_cache(maxsize=None)
def expected(shape):
    """(cls, offsets, payload) of volume(shape) by the model, computed once and shared."""
    (v, w, g), _ = volume(shape)
    cls, offsets = classify(v, w, g)
    payload = gather(v, w, g, cls, offsets)
    for a in (cls, offsets, payload):
        a.setflags(write=False)
    return cls, offsets, payload


def typed(vol):
    """(value float32, weight int32, grad float32) views of three uint32 arrays: what merge_cases.DevVolume3 takes; bits unchanged."""
    return vol[0].view(np.float32), vol[1].view(np.int32), vol[2].view(np.float32)


def splits(n):
    """Brick ranges that cover [0, n): the whole; and a partition whose cuts fall inside runs of 8 and on no multiple of 8 where n allows."""
    cuts = sorted({0, n} | {c for c in (1, 3, 5, 11, 13, n - 1) if 0 < c < n})
    return [(0, n)], list(zip(cuts[:-1], cuts[1:]))
