"""The cases that hold map differencing (xs_tsdf_diff, x-slam_amd/csrc/xs_diff.hip) to a model written from the per-voxel
contract in include/xslam_amd.h and not from the kernel: a numpy statement of the contract in float32, operation by operation (the library is
built with -ffp-contract=off, so the sample s is exact, not close, and every comparison of the tests is for equality).  The steps the
contract takes word for word from the merge (the indices, the cells, the case volumes, maps, shapes and pitches) come from
tests/merge_cases.py; here are the gather of the needed corners, the sample on the value array alone, the classification, the packing of
dense booleans into brick words and back, the counts, and the clusters (scipy.ndimage.label per cell, as tests/frontier_cases.py does it
for the frontier, whose functions are used).  Backend-neutral parts first (tests/test_diff_cases_cpu.py), the device helpers after them
(tests/test_diff_gpu.py hands torch in).  Test infrastructure."""
import functools

import numpy as np

import frontier_cases as fc
from merge_cases import MIN_WEIGHTS, SHAPES, DevVolume3, cells, maps, pitch_pairs, pitches, volume, volumes  # noqa: F401  (re-exported for the tests)

LO, HI = np.float32(0.0), np.float32(0.5)          # the upper layers' defaults
NONVACUOUS_MAPS = ("identity", "shift_plus", "shift_minus", "shift_mixed", "far_face", "perm_a", "perm_b")


# ------------------------------------------------------------------------------------------------
# The model
def sample(src_value, src_weight, m12, dshape):
    """Steps 1 to 3 of the contract for every destination voxel: (inside bool [Z, Y, X], ws int64, s float32).  ws and s are meaningful where
    `inside`; s is computed for every inside voxel (the contract defines it for compared ones, a subset)."""
    sv, sw = np.asarray(src_value, np.float32), np.asarray(src_weight)
    SZ, SY, SX = sv.shape
    dims = (SX, SY, SZ)
    inside, b, f, need = cells(m12, dshape, dims)
    ws = np.full(inside.shape, 1 << 40, np.int64)
    corner = []
    for d in range(8):
        used = inside.copy()
        for a in range(3):
            if d >> a & 1:
                used &= need[a]
        # a corner that is not needed is not read: its index is clamped into the source and its value never selected
        ix = [np.where(used, b[a] + (d >> a & 1), np.minimum(b[a], dims[a] - 1)) for a in range(3)]
        assert all(((ix[a] >= 0) & (ix[a] < dims[a])).all() for a in range(3))
        ws = np.where(used, np.minimum(ws, sw[ix[2], ix[1], ix[0]]), ws)
        corner.append(sv[ix[2], ix[1], ix[0]])
    one = np.float32(1)
    for a in range(3):                                # x, then y, then z; an axis with fraction 0 passes its lower operand through
        stride = 1 << a
        for d in range(0, 8, 2 * stride):
            corner[d] = np.where(need[a], corner[d] * (one - f[a]) + corner[d + stride] * f[a], corner[d])
    assert corner[0].dtype == np.float32
    return inside, ws, corner[0]


def diff(this, other, m12, min_weight=1, lo=LO, hi=HI, details=False):
    """The contract on this = (value, weight[, grad]) [Z, Y, X] and other likewise: (only_this bool [Z, Y, X], only_other, counts
    (compared, only_this, only_other)), and with details also dict(compared, v, s)."""
    v, wp = np.asarray(this[0], np.float32), np.asarray(this[1])
    Z, Y, X = v.shape
    lo, hi = np.float32(lo), np.float32(hi)
    inside, ws, s = sample(other[0], other[1], m12, (X, Y, Z))
    compared = inside & (ws >= min_weight) & (wp >= min_weight)
    only_this = compared & (v < lo) & (s >= hi)
    only_other = compared & (s < lo) & (v >= hi)
    counts = (int(compared.sum()), int(only_this.sum()), int(only_other.sum()))
    out = (only_this, only_other, counts)
    return out + (dict(compared=compared, v=v, s=s),) if details else out


# ------------------------------------------------------------------------------------------------
# Brick words: one uint64 per 4 x 4 x 4 brick, bricks in (bz BY + by) BX + bx order, voxel (lx, ly, lz) at bit lx + 4 ly + 16 lz
def brick_dims(shape_zyx):
    Z, Y, X = shape_zyx
    return (Z + 3) // 4, (Y + 3) // 4, (X + 3) // 4


def pack(mask):
    """uint64 [BZ * BY * BX] from bool [Z, Y, X]; the bits of the overhang are clear."""
    mask = np.asarray(mask, bool)
    Z, Y, X = mask.shape
    BZ, BY, BX = brick_dims(mask.shape)
    padded = np.zeros((4 * BZ, 4 * BY, 4 * BX), bool)
    padded[:Z, :Y, :X] = mask
    bricks = padded.reshape(BZ, 4, BY, 4, BX, 4).transpose(0, 2, 4, 1, 3, 5).reshape(BZ * BY * BX, 64)     # [brick, lz, ly, lx] flattened: bit = 16 lz + 4 ly + lx
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (bricks.astype(np.uint64) * weights).sum(axis=1, dtype=np.uint64)


def unpack(words, shape_zyx):
    """(bool [Z, Y, X], were the overhang bits all clear) from uint64 [BZ * BY * BX]."""
    Z, Y, X = shape_zyx
    BZ, BY, BX = brick_dims(shape_zyx)
    words = np.asarray(words, np.uint64).reshape(BZ * BY * BX)
    bits = ((words[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    padded = bits.reshape(BZ, BY, BX, 4, 4, 4).transpose(0, 3, 1, 4, 2, 5).reshape(4 * BZ, 4 * BY, 4 * BX)
    inside = np.zeros(padded.shape, bool)
    inside[:Z, :Y, :X] = True
    return padded[:Z, :Y, :X].copy(), not bool(padded[~inside].any())


# ------------------------------------------------------------------------------------------------
# Clusters: the frontier's model on another mask
def clusters(mask, cell):
    """uint64 [n, 8] in ascending label order: the records {label, count, sum x, sum y, sum z, packed min, packed max, 0} of the 26-connected
    components of the mask inside each cell of `cell` voxels (0: one cell)."""
    return fc.records(fc.labels(mask, cell))


def select(records, min_size):
    return records[records[:, 1] >= np.uint64(min_size)]


@functools.lru_cache(maxsize=None)
def expected(dshape, sshape, name, min_weight):
    """(only_this words, only_other words, counts) of the case table, computed once and shared."""
    this, other = volumes(dshape, sshape)
    a, b, counts = diff(this, other, maps(dshape, sshape)[name], min_weight)
    out = (pack(a), pack(b), counts)
    for x in out[:2]:
        x.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------
# Device helpers (torch is handed in by the GPU tests)
def mask_words(shape_xyz):
    X, Y, Z = shape_xyz
    return ((X + 3) // 4) * ((Y + 3) // 4) * ((Z + 3) // 4)


class DevMasks:
    """The two masks and the three counts on the device: the masks prefilled with 0xFF bytes (an unwritten word, or a set overhang bit, shows)
    between guards of 64 words of another pattern, the counts between guards too."""
    GUARD, FILL, PATTERN = 64, -1, 0x5A5A5A5A5A5A5A5A

    def __init__(self, torch, shape_xyz, counts=(0, 0, 0)):
        self.torch, self.n = torch, mask_words(shape_xyz)
        self.bufs = []
        for _ in range(2):
            t = torch.full((self.n + 2 * self.GUARD,), self.PATTERN, dtype=torch.int64, device="cuda")
            t[self.GUARD:self.GUARD + self.n] = self.FILL
            self.bufs.append(t)
        self.cbuf = torch.full((3 + 2 * self.GUARD,), self.PATTERN, dtype=torch.int64, device="cuda")
        self.cbuf[self.GUARD:self.GUARD + 3] = torch.tensor(list(counts), dtype=torch.int64)
        self.addr = [t.data_ptr() + 8 * self.GUARD for t in self.bufs]
        self.counts_addr = self.cbuf.data_ptr() + 8 * self.GUARD

    def words(self, k):
        return self.bufs[k][self.GUARD:self.GUARD + self.n].cpu().numpy().view(np.uint64)

    def device_words(self, k):
        return self.bufs[k][self.GUARD:self.GUARD + self.n]

    def counts(self):
        return tuple(int(c) for c in self.cbuf[self.GUARD:self.GUARD + 3].cpu().numpy())

    def guards_untouched(self):
        g = self.GUARD
        return all(bool((t[:g] == self.PATTERN).all()) and bool((t[g + (len(t) - 2 * g):] == self.PATTERN).all()) for t in self.bufs + [self.cbuf])

    def unwritten(self):
        """True when no word of either mask has been written (the refusals)."""
        return all(bool((self.device_words(k) == self.FILL).all()) for k in range(2))


def gpu_diff(torch, capi, this, other, res, sres, m12, min_weight, out, lo=LO, hi=HI, flags=0, workspace=True):
    """Runs xs_tsdf_diff on two DevVolume3 into a DevMasks."""
    ws = torch.zeros(capi.tsdf_diff_workspace_bytes(list(res), list(sres)), dtype=torch.uint8, device="cuda") if workspace else None
    capi.tsdf_diff(this.value.addr, this.weight.addr, this.pitch, list(res), other.value.addr, other.weight.addr, other.pitch, list(sres), m12,
                   out.addr[0], out.addr[1], out.counts_addr, min_weight=min_weight, lo=float(lo), hi=float(hi), flags=flags, workspace=ws)
    torch.cuda.synchronize()
