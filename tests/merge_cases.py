"""The cases that hold the volume merge (xs_tsdf_merge, x-slam_amd/csrc/xs_merge.hip) to a model written from the per-voxel contract in
include/xslam_amd.h and not from the kernel: a numpy statement of the contract in float32, operation by operation (the library is built with
-ffp-contract=off and divides with correct rounding, so the model is exact, not close), and a float64 twin that takes the cell indices and
fractions from the float32 model (no discrete decision can differ) and redoes the interpolation and the blend in float64.  Backend-neutral
parts first (tests/test_merge_cases_cpu.py), the device helpers after them (tests/test_merge_gpu.py hands torch in).  Test infrastructure.

Case data: values and grads in [-1, 1] with magnitudes of at least 2^-60 (no product below is denormal: a fraction and its complement are
multiples of 2^-24 at these index ranges, so a product stays above 2^-84), exact zeros and some -0 among them; weights random in [0, 9], about a
quarter of them zero, max_weight 12: every case has skipped voxels, neighbourhoods that are valid in part, and capped sums.

The bound of the float32 model against its twin (u = 2^-24, first order; ALLOW covers the higher orders), M the largest magnitude among the
values that enter:
  One interpolation stage is lo * (1 - f) + hi * f: the complement carries one rounding, each product one more, the sum one: with exact
  operands the stage is off by at most u (3 |lo| (1 - f) + 2 |hi| f) <= 3 u M, and since its weights are non-negative and sum to 1 it passes
  the error of its operands on without growth.  Three stages: s is off by at most 9 u M (an axis with fraction 0 adds nothing).
  The blend (prev * wp + s * ws) / (wp + ws) has integers below 2^24 as float32 (exact), two products, one sum and one quotient: the error
  of s enters with weight ws / (wp + ws) <= 1, the three roundings of each term and of the quotient add 3 u (|prev| wp + |s| ws) / (wp + ws)
  <= 3 u M.  Into an empty voxel the blend is s itself.
  Together: |model32 - model64| <= MODEL_BOUND_U u M with MODEL_BOUND_U = 12."""
import functools
import itertools

import numpy as np

from extract_cases import VOXEL_SIZES, same_bits  # noqa: F401  (same_bits: re-exported for the tests)

U = 2.0 ** -24
ALLOW = 1.01
MODEL_BOUND_U = 12
MAX_WEIGHT = 12
MIN_WEIGHTS = (1, 3)
TINY = np.float32(2.0 ** -60)

# destination <- source, (X, Y, Z) each.  A workgroup covers 64 x 4 x 16 destination voxels; a brick is 4 x 4 x 4 source voxels.
SHAPES = [((2, 2, 2), (2, 2, 2)),
          ((5, 3, 2), (3, 7, 4)),
          ((64, 4, 2), (64, 4, 2)),          # exactly one workgroup
          ((65, 9, 7), (63, 3, 5)),
          ((129, 5, 3), (70, 11, 9)),
          ((3, 70, 4), (65, 9, 7)),
          ((33, 1028, 3), (9, 10, 130))]     # 257 workgroups along y; 33 brick layers along z


def seed_of(dshape, sshape):
    return 100003 * dshape[0] + 1009 * dshape[1] + dshape[2] + 7 * (100003 * sshape[0] + 1009 * sshape[1] + sshape[2])


def voxel_size_of(shape):
    return float(np.float32(VOXEL_SIZES[sum(shape) % 3]))


# ------------------------------------------------------------------------------------------------
# Volumes: (value, weight, grad), each [Z, Y, X]
def volume(rng, shape):
    X, Y, Z = shape

    def values():
        v = rng.uniform(-1.0, 1.0, (Z, Y, X)).astype(np.float32)
        v[np.abs(v) < TINY] = TINY
        pick = rng.random((Z, Y, X))
        v[pick < 0.05] = np.float32(0.0)
        v[(pick >= 0.05) & (pick < 0.09)] = np.float32(-0.0)
        v[(pick >= 0.09) & (pick < 0.11)] = TINY
        v[(pick >= 0.11) & (pick < 0.13)] = -TINY
        v[(pick >= 0.13) & (pick < 0.15)] = np.float32(1.0)
        v[(pick >= 0.15) & (pick < 0.17)] = np.float32(-1.0)
        return v

    w = rng.integers(1, 10, (Z, Y, X)).astype(np.int32)
    w[rng.random((Z, Y, X)) < 0.25] = 0
    return values(), w, values()


def empty_volume(shape):
    X, Y, Z = shape
    return np.zeros((Z, Y, X), np.float32), np.zeros((Z, Y, X), np.int32), np.zeros((Z, Y, X), np.float32)


# ------------------------------------------------------------------------------------------------
# The model
def indices(m12, dshape):
    """g[a] [Z, Y, X] float32: step 1 of the contract."""
    X, Y, Z = dshape
    m = np.asarray(m12, np.float32)
    x = np.arange(X, dtype=np.float32)[None, None, :]
    y = np.arange(Y, dtype=np.float32)[None, :, None]
    z = np.arange(Z, dtype=np.float32)[:, None, None]
    with np.errstate(over="ignore", invalid="ignore"):
        return [((m[3 * a] * x + m[3 * a + 1] * y) + m[3 * a + 2] * z) + m[9 + a] for a in range(3)]


def cells(m12, dshape, sshape):
    """Steps 1 and 2: (inside [Z, Y, X], b [3] int64, f [3] float32, need [3] bool); b, f and need are 0 outside."""
    g = indices(m12, dshape)
    inside = np.ones(g[0].shape, bool)
    for a in range(3):
        inside &= (g[a] >= 0) & (g[a] <= np.float32(sshape[a] - 1))
    b, f, need = [], [], []
    for a in range(3):
        ga = np.where(inside, g[a], np.float32(0))
        ba = np.floor(ga)
        b.append(ba.astype(np.int64))
        f.append((ga - ba).astype(np.float32))
        need.append(f[a] > 0)
    return inside, b, f, need


def merge(dst, src, m12, min_weight=1, max_weight=MAX_WEIGHT, z0=0, z1=None, dtype=np.float32, details=False):
    """The contract on dst = (value, weight, grad) [Z, Y, X] and src likewise: (value, weight, grad, written) with value and grad in dtype
    (float32: the model; float64: the twin, on the float32 model's cells and fractions).  Planes outside [z0, z1) come back as they were."""
    T = dtype
    dv, dw, dg = dst
    sv, sw, sg = src
    Z, Y, X = dv.shape
    SZ, SY, SX = sv.shape
    z1 = Z if z1 is None else z1
    inside, b, f, need = cells(m12, (X, Y, Z), (SX, SY, SZ))
    dims = (SX, SY, SZ)
    used, idx = [], []
    for d in range(8):
        u = inside.copy()
        ix = []
        for a in range(3):
            if d >> a & 1:
                u &= need[a]
            ix.append(b[a] + (d >> a & 1))
        ix = [np.where(u, ix[a], np.minimum(b[a], dims[a] - 1)) for a in range(3)]   # an unneeded corner: clamped, and never selected below
        assert all(((ix[a] >= 0) & (ix[a] < dims[a])).all() for a in range(3))
        used.append(u)
        idx.append(ix)
    ws = np.full(inside.shape, 1 << 30, np.int64)
    for d in range(8):
        ws = np.where(used[d], np.minimum(ws, sw[idx[d][2], idx[d][1], idx[d][0]]), ws)
    ok = inside & (ws >= min_weight)
    ok[:z0] = False
    ok[z1:] = False
    ws = np.minimum(ws, max_weight)
    one = T(1)

    def interpolate(arr):
        c = [arr[idx[d][2], idx[d][1], idx[d][0]].astype(T) for d in range(8)]
        for a in range(3):
            stride = 1 << a
            fa = f[a].astype(T)
            for d in range(0, 8, 2 * stride):
                c[d] = np.where(need[a], c[d] * (one - fa) + c[d + stride] * fa, c[d])
        return c[0]

    wp = dw.astype(np.int64)
    wt = np.where(ok, wp + ws, 1)

    def blend(prev, s):
        with np.errstate(invalid="ignore", divide="ignore"):
            mixed = (prev.astype(T) * wp.astype(T) + s * ws.astype(T)) / wt.astype(T)
        return np.where(ok, np.where(wp == 0, s, mixed), prev.astype(T))

    nv, ng = blend(dv, interpolate(sv)), blend(dg, interpolate(sg))
    nw = np.where(ok, np.minimum(wp + ws, max_weight), wp).astype(np.int32)
    out = (nv, nw, ng, int(ok.sum()))
    return out + (dict(ok=ok, need=need, inside=inside, used=used),) if details else out


def model_bound(dst, src):
    M = max(float(np.abs(a).max()) if a.size else 0.0 for a in (dst[0], dst[2], src[0], src[2]))
    return ALLOW * MODEL_BOUND_U * U * M


# ------------------------------------------------------------------------------------------------
# Maps: xform12 = 3 x 3 row-major, then 3 offsets (destination voxel indices -> continuous source voxel indices)
def xform(matrix=None, offset=(0, 0, 0)):
    m = np.eye(3) if matrix is None else np.asarray(matrix, np.float64)
    return np.concatenate([m.reshape(9), np.asarray(offset, np.float64)]).astype(np.float32)


def affine64(T, vs_dst, vs_src):
    """merge_affine of x-slam_amd/host/merge_host.hpp restated: float64 in its order of operations, one rounding to float32 at the end."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    vd, vs = np.float64(vs_dst), np.float64(vs_src)
    m = np.zeros(12, np.float64)
    half = np.float64(0.5) * vd
    for a in range(3):
        for c in range(3):
            m[3 * a + c] = T[a, c] * vd / vs
        m[9 + a] = (((T[a, 0] * half + T[a, 1] * half) + T[a, 2] * half) + T[a, 3]) / vs - np.float64(0.5)
    return m.astype(np.float32)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def rigid_between(rng, dshape, sshape, vs_dst, vs_src, angle):
    """A rotation by `angle` about a random axis that takes the destination's centre to a point near the source's centre (metres)."""
    R = rotation(rng.normal(size=3), angle)
    cd = 0.5 * np.array(dshape) * vs_dst
    cs = 0.5 * np.array(sshape) * vs_src + rng.uniform(-0.7, 0.7, 3) * vs_src
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, cs - R @ cd
    return T


def signed_permutations():
    """The 24 proper rotations of the cube as 3 x 3 signed permutation matrices."""
    out = []
    for p in itertools.permutations(range(3)):
        for s in itertools.product((1, -1), repeat=3):
            P = np.zeros((3, 3))
            for a in range(3):
                P[a, p[a]] = s[a]
            if round(np.linalg.det(P)) == 1:
                out.append(P)
    return out


def permutation_map(P, sshape):
    """Source index a = +- destination index p(a), a flipped axis counted down from the source's last voxel."""
    off = [(sshape[a] - 1) if P[a].sum() < 0 else 0 for a in range(3)]
    return xform(P, off)


@functools.lru_cache(maxsize=None)
def maps(dshape, sshape):
    """name -> xform12, at least 16 of them so that a test which gives every map another pitch pair covers all 16 pairs."""
    rng = np.random.default_rng(seed_of(dshape, sshape) + 11)
    vd, vs = voxel_size_of(dshape), voxel_size_of(sshape)
    D, S = np.array(dshape), np.array(sshape)
    P = signed_permutations()
    out = {
        "identity": xform(),
        "shift_plus": xform(offset=(1, 1, 1)),
        "shift_minus": xform(offset=(-1, -1, -1)),
        "shift_mixed": xform(offset=(3, -2, 1)),
        "far_face": xform(offset=S - D),                                  # the last destination voxel lands exactly on S - 1
        "perm_a": permutation_map(P[7], sshape),
        "perm_b": permutation_map(P[5], sshape),
        "perm_c": permutation_map(P[18], sshape),
        "half_x": xform(offset=(0.5, 0, 0)),
        "half_y": xform(offset=(0, 0.5, 0)),
        "half_z": xform(offset=(0, 0, 0.5)),
        "half_xy_far": xform(offset=tuple((S - D)[:2] - 0.5) + (0,)),       # four corners, ending half a voxel inside the far faces
        "rotation_10": affine64(rigid_between(rng, dshape, sshape, vd, vd, np.radians(10.0)), vd, vd),
        "rotation_33": affine64(rigid_between(rng, dshape, sshape, vd, vs, np.radians(33.0)), vd, vs),
        "ratio_2": affine64(np.eye(4), 2 * vs, vs),
        "ratio_half": affine64(np.eye(4), 0.5 * vs, vs),
        "miss": xform(offset=S + 5),
    }
    for v in out.values():
        v.setflags(write=False)
    return out


def pitches(X):
    """As extract_cases.pitches: tight; one float more; rounded up to 256 and 64 more; tight with the base 4 bytes past a 16-byte boundary."""
    tight = X * 4
    return [(tight, 0), (tight + 4, 0), (-(-tight // 256) * 256 + 64, 0), (tight, 4)]


def pitch_pairs(dshape, sshape):
    return list(itertools.product(pitches(dshape[0]), pitches(sshape[0])))


def _frozen(t):
    for a in t:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def volumes(dshape, sshape):
    """(populated destination, source), computed once and shared: never modified."""
    rng = np.random.default_rng(seed_of(dshape, sshape))
    return _frozen(volume(rng, dshape)), _frozen(volume(rng, sshape))


@functools.lru_cache(maxsize=None)
def expected(dshape, sshape, name, min_weight, populated):
    dst, src = volumes(dshape, sshape)
    if not populated:
        dst = empty_volume(dshape)
    return _frozen(merge(dst, src, maps(dshape, sshape)[name], min_weight))


# ------------------------------------------------------------------------------------------------
# Device volumes with guards (torch is handed in by the GPU tests)
class DevVolume3:
    """The three arrays of a volume on the device, one pitch and base offset, each an extract_cases.DevVolume: two guard planes before and
    after, guards and padding filled with words that any kernel that read them as a weight or a value would show (a guard word read as
    a weight is 2^29 and more)."""

    def __init__(self, torch, vol, pitch, offset=0):
        from extract_cases import DevVolume
        v, w, g = vol
        self.shape = v.shape
        self.pitch = int(pitch)
        self.value = DevVolume(torch, np.ascontiguousarray(v, np.float32), pitch, offset)
        self.weight = DevVolume(torch, np.ascontiguousarray(w, np.int32).view(np.float32), pitch, offset)
        self.grad = DevVolume(torch, np.ascontiguousarray(g, np.float32), pitch, offset)

    def untouched(self):
        return self.value.untouched() and self.weight.untouched() and self.grad.untouched()

    def equals(self, vol):
        """The buffers hold exactly vol's bits inside and their original words in guards and padding."""
        Z, Y, X = self.shape
        for dev, want in zip((self.value, self.weight, self.grad), vol[:3]):
            host = dev.host.copy()
            w, off, g = dev.pitch // 4, (dev.addr - dev.buf.data_ptr()) // 4 - dev.GUARD * Y * (dev.pitch // 4), dev.GUARD
            want = np.ascontiguousarray(want)
            host[off:off + (Z + 2 * g) * Y * w].reshape(Z + 2 * g, Y, w)[g:-g, :, :X] = want.view(np.float32) if want.dtype != np.float32 else want
            if not np.array_equal(dev.buf.cpu().numpy().view(np.uint32), host.view(np.uint32)):
                return False
        return True


def gpu_merge(torch, capi, dst, src, res, sres, m12, min_weight, flags=0, z0=0, z1=None, max_weight=MAX_WEIGHT, workspace=True):
    """Runs xs_tsdf_merge on two DevVolume3; returns `written`."""
    written = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(capi.tsdf_merge_workspace_bytes(list(res), list(sres)), dtype=torch.uint8, device="cuda") if workspace else None
    capi.tsdf_merge(dst.value.addr, dst.weight.addr, dst.grad.addr, dst.pitch, list(res), src.value.addr, src.weight.addr, src.grad.addr, src.pitch,
                    list(sres), m12, min_weight=min_weight, max_weight=max_weight, flags=flags, z0=z0, z1=z1, written=written, workspace=ws)
    torch.cuda.synchronize()
    return int(written.item())
