"""The cases that hold surface export (xs_extract_points / xs_extract_normals, x-slam_amd/csrc/xs_extract.hip) against a model written
independently of the oracle: a numpy statement of the formulas as xs_extract.hip and include/xslam_amd.h describe them, evaluated in
float32 operation by operation (both builds compile with -ffp-contract=off, so the model is exact, not close) and, as a twin, in
float64 from the same float32 inputs.  Backend-neutral parts first (tests/test_extract_cases_cpu.py runs them on the model and the CPU
oracle), the guarded device buffers after them (tests/test_extract_ragged_gpu.py hands torch in).  Test infrastructure.

Inputs hold neither NaN nor denormals: the fusion kernel writes neither (a TSDF value is a clipped quotient of normal floats).

Bounds of the float32 model against its float64 twin (u = 2^-24, first order; ALLOW covers the higher orders):

  A point's moving coordinate is p = V - (F / (Fn - F)) * vs with V = (k + 0.5) * vs.  k + 0.5 is exact; V carries one rounding
  (u |V|); Fn - F one, the quotient q one more (|q| <= 1 because the signs differ), q * vs a third (3 u vs together); the final
  subtraction u |p| with |p| <= |V| + vs.  Sum: u (2 |V| + 4 vs), stated as POINT_BOUND = u (2 |V| + 5 vs).  The two fixed coordinates
  are V itself: u |V|, inside the same bound.

  A normal is n / |n|^2 with n_i = I(p + vs e_i) - I(p - vs e_i) and I the eight-term trilinear sum.
  - Coordinates: the shifted argument is rounded (u (g + 2) in voxels, g its cell index), the cell centre (g + 0.5) * vs is rounded
    (u (g + 0.5)), the difference and the division by vs add 2 u of a fraction <= 1: a fraction is off by at most (2 G + 5) u with G the
    largest dimension.  I is continuous across cells and changes by at most L (the largest difference of axis neighbours in the
    field) per unit of a fraction: 3 (2 G + 5) L u.
  - The sum: every term is a value times three weights (three roundings of 1 - f, three products: 6 u), the seven additions from left
    to right add at most 7 u; the weights are non-negative and sum to 1: 13 u M with M the largest |value|.
  So I is off by e_I = u (13 M + 3 (2 G + 5) L), a component by d = 2 e_I + u |n_i|.  The squared length s (three squares, two sums:
  3 u) is off by 2 sqrt(3) d |n| + 3 u s, and the quotient n_i / s by d / s + (|n_i| / s) (2 sqrt(3) d / |n| + 4 u)
  <= (1 + 2 sqrt(3)) d / s + 4 u / |n|: NORMAL_BOUND.  The smooth fields keep |n| above GRAD_FLOOR, so the bound stays small."""
import functools

import numpy as np

PATTERN = 0xA5                                # output buffers and their guards before a launch (as tests/map_cases.py): float -2.87e-16
U = 2.0 ** -24
ALLOW = 1.01                                  # the second-order terms of the bounds above
LIMIT = np.float32(0.99)
EDGE_VALUES = {                               # name -> value; the share of voxels each overwrites is EDGE_SHARE
    "one": np.float32(1.0),
    "limit": LIMIT,
    "below_limit": np.nextafter(LIMIT, np.float32(0)),
    "plus_zero": np.float32(0.0),
    "minus_zero": np.float32(-0.0),
    "plus_tiny": np.float32(1e-30),
    "minus_tiny": np.float32(-1e-30),
}
EDGE_SHARE = {"one": 0.08, "limit": 0.05, "below_limit": 0.05, "plus_zero": 0.04, "minus_zero": 0.04, "plus_tiny": 0.04, "minus_tiny": 0.04}

# (X, Y, Z).  A workgroup covers 64 x 4 columns.
SHAPES = [(2, 2, 2),        # one candidate voxel, no interior
          (64, 4, 2),       # exactly one workgroup
          (63, 3, 5), (65, 9, 7), (129, 5, 3), (3, 70, 4), (70, 11, 9),
          (5, 5, 5),        # exactly one interior cell for normals
          (6, 4, 7)]        # no interior in y
# shape -> workgroups: around the scan's chunk of 256; (65, 1030, 3) has gridDim.x = 2 and three chunks
SCAN_SHAPES = {(33, 1020, 3): 255, (33, 1024, 3): 256, (33, 1028, 3): 257, (65, 1030, 3): 516}
SLAB_SHAPE = (70, 9, 11)                      # non-cubic, Z = 11: plane ranges and slabs
VOXEL_SIZES = (0.1, 0.037, 0.0123)            # none a power of two: every product and quotient rounds
GRAD_FLOOR = 0.05                             # the smooth fields' central differences are longer than this


def voxel_size_of(shape):
    return float(np.float32(VOXEL_SIZES[sum(shape) % 3]))


def seed_of(shape):
    return 100003 * shape[0] + 1009 * shape[1] + shape[2]


def blocks_of(shape):
    return -(-shape[0] // 64), -(-shape[1] // 4)


def pitches(X):
    """(pitch in bytes, byte offset of the base from a 256-byte boundary): tight; one float more (not a multiple of 16); rounded up to
    256 and 64 more; tight with the base 4 bytes past a 16-byte boundary."""
    tight = X * 4
    return [(tight, 0), (tight + 4, 0), (-(-tight // 256) * 256 + 64, 0), (tight, 4)]


# ------------------------------------------------------------------------------------------------
# Fields: value[Z, Y, X] float32
def field(rng, X, Y, Z):
    """Uniform in [-1, 1] with EDGE_SHARE of the voxels overwritten by each of EDGE_VALUES.  Where the volume has room, two structures
    that chance would not deliver: a 3-d checkerboard of signs over x in [0, 65) of two rows and two planes (64 consecutive voxels with
    three crossings each: all three ballots full, lane 63 included), and one row alternating in x alone (a full ballot of single
    crossings)."""
    v = rng.uniform(-1.0, 1.0, (Z, Y, X)).astype(np.float32)
    pick = rng.random((Z, Y, X))
    lo = 0.0
    for name, share in EDGE_SHARE.items():
        v[(pick >= lo) & (pick < lo + share)] = EDGE_VALUES[name]
        lo += share
    if X >= 65 and Y >= 3 and Z >= 3:
        z, y = int(rng.integers(0, Z - 2)), int(rng.integers(0, Y - 2))
        zz, yy, xx = np.meshgrid(np.arange(2), np.arange(2), np.arange(65), indexing="ij")
        mag = rng.uniform(0.05, 0.9, (2, 2, 65)).astype(np.float32)
        v[z:z + 2, y:y + 2, :65] = np.where((zz + yy + xx) % 2 == 0, mag, -mag)
    if X >= 65:
        mag = rng.uniform(0.05, 0.9, 65).astype(np.float32)
        v[Z - 2, Y - 2, :65] = np.where(np.arange(65) % 2 == 0, mag, -mag)   # (the last row and plane that report)
    return v


def sparse_scan_field(shape):
    """All 1.0 (nothing to find) except in the columns of workgroups 0, 255, 256, 257, the last and the last but one, which hold the
    random field: a lost or doubled carry moves a known block of points."""
    X, Y, Z = shape
    gx, gy = blocks_of(shape)
    dense = random_case(shape)["value"]
    v = np.ones_like(dense)
    for wg in sorted({0, 255, 256, 257, gx * gy - 2, gx * gy - 1}):
        if 0 <= wg < gx * gy:
            bx, by = wg % gx, wg // gx
            v[:, 4 * by:4 * by + 4, 64 * bx:64 * bx + 64] = dense[:, 4 * by:4 * by + 4, 64 * bx:64 * bx + 64]
    return v


def sphere_field(X, Y, Z):
    """An off-centre sphere, distance over a truncation of 4 voxels, clipped to [-1, 1]."""
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    c = (0.47 * X, 0.55 * Y, 0.42 * Z)
    r = 0.33 * min(X, Y, Z)
    d = np.sqrt((x + 0.5 - c[0]) ** 2 + (y + 0.5 - c[1]) ** 2 + (z + 0.5 - c[2]) ** 2) - r
    return np.clip(d / 4.0, -1, 1).astype(np.float32)


def plane_field(X, Y, Z):
    """A tilted plane through the volume's middle, distance over a truncation of 3 voxels, clipped to [-1, 1]."""
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    n = np.array([0.31, 0.52, 0.8])
    n /= np.linalg.norm(n)
    d = n[0] * (x + 0.5 - 0.5 * X) + n[1] * (y + 0.5 - 0.5 * Y) + n[2] * (z + 0.5 - 0.5 * Z)
    return np.clip(d / 3.0, -1, 1).astype(np.float32)


SMOOTH = {"sphere": (sphere_field, (70, 40, 31)), "plane": (plane_field, (37, 66, 21)), "small_sphere": (sphere_field, (19, 23, 65))}


# ------------------------------------------------------------------------------------------------
# The model
def crossings(value, res, vs, zs0=0, z0=0, z1=None, dtype=np.float32):
    """Every crossing of planes [z0, z1) of value[planes, Y, X] (plane 0 is stored plane zs0), in the documented order: workgroup
    bx + ceil(X / 64) * by, then z, y, x, direction.  A dict of points [n, 3] (dtype), and per point z, y, x, d and wg."""
    X, Y, Z = (int(r) for r in res)
    z1 = Z - 1 if z1 is None else z1
    T = dtype
    v = np.asarray(value, np.float32).reshape(-1, Y, X).astype(T)
    vs, lim = T(np.float32(vs)), T(LIMIT)
    if z1 <= z0 or X < 2 or Y < 2:
        e = np.zeros(0, np.int64)
        return dict(points=np.zeros((0, 3), T), z=e, y=e, x=e, d=e, wg=e)
    a, b = z0 - zs0, z1 - zs0
    F = v[a:b, :Y - 1, :X - 1, None]
    Fn = np.stack([v[a:b, :Y - 1, 1:X], v[a:b, 1:Y, :X - 1], v[a + 1:b + 1, :Y - 1, :X - 1]], -1)
    ok = (F < lim) & (Fn < lim) & (((F > 0) & (Fn < 0)) | ((F < 0) & (Fn > 0)))
    centre = [(np.arange(lo, hi).astype(T) + T(0.5)) * vs for lo, hi in ((0, X - 1), (0, Y - 1), (z0, z1))]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (F / (Fn - F)) * vs
    P = np.empty(ok.shape + (3,), T)
    P[..., 0] = centre[0][None, None, :, None]
    P[..., 1] = centre[1][None, :, None, None]
    P[..., 2] = centre[2][:, None, None, None]
    for d in range(3):
        P[..., d, d] = P[..., d, d] - t[..., d]
    zi, yi, xi, di = np.nonzero(ok)                                      # C order: z, y, x, direction
    wg = xi // 64 + (-(-X // 64)) * (yi // 4)
    order = np.argsort(wg, kind="stable")
    return dict(points=P[zi, yi, xi, di][order], z=zi[order] + z0, y=yi[order], x=xi[order], d=di[order], wg=wg[order])


def points(value, res, vs, zs0=0, z0=0, z1=None, dtype=np.float32):
    """(points [found, 3] in the documented order, found)"""
    p = crossings(value, res, vs, zs0, z0, z1, dtype)["points"]
    return p, len(p)


def normals(value, res, vs, pts, zs0=0, zs1=None, dtype=np.float32, details=False):
    """The normals at pts [n, 3] from value[planes, Y, X] holding stored planes [zs0, zs1): reads clamp z to the stored planes, the
    border rule is on the full resolution.  With details, also (passes the border rule [n], every read inside the volume [n])."""
    X, Y, Z = (int(r) for r in res)
    zs1 = Z if zs1 is None else zs1
    T = dtype
    v = np.asarray(value, np.float32).reshape(-1, Y, X).astype(T)
    assert v.shape[0] == zs1 - zs0
    vs = T(np.float32(vs))
    p = np.asarray(pts, np.float32).reshape(-1, 3).astype(T)
    half, one = T(0.5), T(1)
    cell = lambda q: np.floor(q / vs).astype(np.int64)
    g = cell(p)
    dims = np.array([X, Y, Z])
    inner = ((g > 1) & (g < dims - 2)).all(axis=1)
    inside = np.ones(int(inner.sum()), bool)                              # per point the border rule lets through: no read left the volume

    def interp(q):
        nonlocal inside
        c = cell(q)
        c = np.where(q < (c.astype(T) + half) * vs, c - 1, c)
        f = (q - (c.astype(T) + half) * vs) / vs
        acc = None
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    ix, iy, iz = c[:, 0] + dx, c[:, 1] + dy, c[:, 2] + dz
                    inside &= (ix >= 0) & (ix < X) & (iy >= 0) & (iy < Y) & (iz >= 0) & (iz < Z)
                    iz = np.clip(iz, zs0, zs1 - 1) - zs0
                    val = v[iz, np.clip(iy, 0, Y - 1), np.clip(ix, 0, X - 1)]
                    term = val * (f[:, 0] if dx else one - f[:, 0]) * (f[:, 1] if dy else one - f[:, 1]) * (f[:, 2] if dz else one - f[:, 2])
                    acc = term if acc is None else acc + term
        return acc

    q = p[inner]
    n = np.zeros((len(q), 3), T)
    ok_reads = np.ones(len(p), bool)
    if len(q):
        for i in range(3):
            e = np.zeros(3, T)
            e[i] = vs
            n[:, i] = interp(q + e) - interp(q - e)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]
            n = n / s[:, None]
        ok_reads[inner] = inside
    out = np.zeros((len(p), 3), T)
    out[inner] = n
    return (out, inner, ok_reads) if details else out


def point_bound(shape, vs):
    """POINT_BOUND of the module's docstring for every coordinate of a point in this volume: |V| <= (largest dimension) * vs."""
    return ALLOW * U * (2 * max(shape) + 5) * vs


def normal_bound(value, shape, n64):
    """NORMAL_BOUND of the module's docstring per point, from the float64 twin's normals n64 = n / |n|^2 (so |n| = 1 / |n64|)."""
    v = np.asarray(value, np.float64)
    L = max(np.abs(np.diff(v, axis=a)).max() for a in range(3))
    M = np.abs(v).max()
    e_i = U * (13 * M + 3 * (2 * max(shape) + 5) * L)
    with np.errstate(divide="ignore"):
        length = 1.0 / np.sqrt((n64 ** 2).sum(axis=1))                    # |n|
    d = 2 * e_i + U * length
    return ALLOW * ((1 + 2 * np.sqrt(3.0)) * d / length ** 2 + 4 * U / length)


# ------------------------------------------------------------------------------------------------
# Cases, computed once and shared: never modified
def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def general_points(shape, vs, seed, n=4000, snapped=300):
    """Points inside and up to a voxel and a half outside the volume, half of them over the cells the border rule lets through, plus
    points snapped to cell faces k * vs and to centres (k + 0.5) * vs in one, two or all three coordinates."""
    rng = np.random.default_rng(seed)
    dims = np.array(shape, np.float64)
    a = rng.uniform(-1.5, dims + 1.5, (n // 2, 3))
    lo, hi = np.full(3, 1.5), np.maximum(dims - 1.5, 2.5)
    b = rng.uniform(lo, hi, (n - n // 2, 3))
    p = (np.concatenate([a, b]) * vs).astype(np.float32)
    k = rng.integers(0, np.array(shape) + 1, (snapped, 3))
    half = rng.random((snapped, 3)) < 0.5
    snap = ((k.astype(np.float32) + np.where(half, np.float32(0.5), np.float32(0))) * np.float32(vs)).astype(np.float32)
    free = (rng.uniform(0, dims, (snapped, 3)) * vs).astype(np.float32)
    keep = rng.random((snapped, 3)) < 0.35
    keep[np.arange(snapped), rng.integers(0, 3, snapped)] = False         # at least one coordinate snapped
    return np.concatenate([p, np.where(keep, free, snap)]).astype(np.float32)


def _with_model(shape, value):
    vs = voxel_size_of(shape)
    X, Y, Z = shape
    c = crossings(value, shape, vs)
    nrm = normals(value, shape, vs, c["points"])
    gp = general_points(shape, vs, seed_of(shape) + 1)
    gn, inner, reads = normals(value, shape, vs, gp, details=True)
    use = ~inner | reads                                                  # the kernel guards its reads by the border rule alone
    gp, gn, inner = gp[use], gn[use], inner[use]
    if len(gp) % 256 == 0:
        gp, gn, inner = gp[:-1], gn[:-1], inner[:-1]
    return _frozen(dict(shape=shape, vs=vs, value=value, points=c["points"], found=len(c["points"]), normals=nrm, general=gp,
                        general_normals=gn, general_inner=inner, **{k: c[k] for k in ("z", "y", "x", "d", "wg")}))


@functools.lru_cache(maxsize=None)
def random_case(shape):
    X, Y, Z = shape
    return _with_model(shape, field(np.random.default_rng(seed_of(shape)), X, Y, Z))


@functools.lru_cache(maxsize=None)
def sparse_case(shape):
    return _with_model(shape, sparse_scan_field(shape))


@functools.lru_cache(maxsize=None)
def empty_case(shape):
    X, Y, Z = shape
    return _with_model(shape, np.ones((Z, Y, X), np.float32))


@functools.lru_cache(maxsize=None)
def smooth_case(name):
    make, shape = SMOOTH[name]
    X, Y, Z = shape
    vs = voxel_size_of(shape)
    return _frozen(dict(shape=shape, vs=vs, value=make(X, Y, Z)))


def crossing_counts(case):
    """[Z - 1, Y - 1, X - 1]: the crossings the model reports per voxel."""
    X, Y, Z = case["shape"]
    n = np.zeros((Z - 1, Y - 1, X - 1), np.int64)
    np.add.at(n, (case["z"], case["y"], case["x"]), 1)
    return n


def full_ballots(case):
    """How many (plane, row, 64-column group) triples have all 64 lanes reporting at least one / three crossings."""
    n = crossing_counts(case)
    X = case["shape"][0]
    one = three = 0
    for bx in range((X - 1) // 64):
        seg = n[:, :, 64 * bx:64 * bx + 64]
        one += int((seg > 0).all(axis=2).sum())
        three += int((seg > 2).all(axis=2).sum())
    return one, three


def edge_pairs(case):
    """name -> (pairs with the value that the model accepts, pairs it rejects only because of that value: the partner is below the
    limit and non-zero, and negative where the value itself is at or above the limit)."""
    X, Y, Z = case["shape"]
    v = case["value"]
    F = v[:Z - 1, :Y - 1, :X - 1, None]
    Fn = np.stack([v[:Z - 1, :Y - 1, 1:X], v[:Z - 1, 1:Y, :X - 1], v[1:Z, :Y - 1, :X - 1]], -1)
    F = np.broadcast_to(F, Fn.shape)
    ok = (F < LIMIT) & (Fn < LIMIT) & (((F > 0) & (Fn < 0)) | ((F < 0) & (Fn > 0)))
    out = {}
    for name, e in EDGE_VALUES.items():
        bits = e.view(np.uint32)
        acc = rej = 0
        for mine, other in ((F, Fn), (Fn, F)):
            has = mine.view(np.uint32) == bits
            live = (other < LIMIT) & (other != 0)
            if e >= LIMIT:
                live = live & (other < 0)
            acc += int((has & ok).sum())
            rej += int((has & ~ok & live).sum())
        out[name] = (acc, rej)
    return out


def offsets_of(case):
    """Exclusive offsets of the workgroups: what the scan has to produce."""
    gx, gy = blocks_of(case["shape"])
    return np.concatenate([[0], np.cumsum(np.bincount(case["wg"], minlength=gx * gy))])


def capacities(case):
    """0, 1, a cut inside one voxel's three points, the offset of workgroup 256 (the first of the scan's second chunk; of the last
    workgroup with points where there are fewer), found - 1, found, found + 5."""
    found = case["found"]
    n = crossing_counts(case)
    key = (case["z"] * n.shape[1] + case["y"]) * n.shape[2] + case["x"]
    triple = np.flatnonzero((n[case["z"], case["y"], case["x"]] == 3) & (case["d"] == 0))
    first = int(triple[len(triple) // 2])
    assert key[first] == key[first + 2]
    off = offsets_of(case)
    at = 256 if len(off) > 257 else int(case["wg"][-1])                   # (fewer workgroups: the last that has points)
    return [0, 1, first + 2, int(off[at]), found - 1, found, found + 5]


# ------------------------------------------------------------------------------------------------
# Device buffers with guards (torch is handed in by the GPU tests)
def guard_words(n):
    """Sign-alternating floats of magnitude 0.5: read as a value, any of them makes or moves a crossing."""
    return np.where(np.arange(n) % 2 == 0, np.float32(0.5), np.float32(-0.5)).astype(np.float32)


class DevVolume:
    """value[planes, Y, X] on the device in rows of pitch bytes, GUARD guard planes of Y rows before and after (two: a normal's
    stencil reaches two planes past its point's, so a read that misses the clamp to the stored planes lands in them), the base
    offset bytes past a 256-byte boundary; guards and padding hold guard_words.  addr: row 0 of plane 0 (what a kernel is given)."""
    GUARD = 2

    def __init__(self, torch, value, pitch, offset=0):
        planes, Y, X = value.shape
        assert pitch >= X * 4 and pitch % 4 == 0 and offset % 4 == 0
        self.pitch, w, off, g = int(pitch), pitch // 4, offset // 4, self.GUARD
        host = guard_words(off + (planes + 2 * g) * Y * w + 4)
        host[off:off + (planes + 2 * g) * Y * w].reshape(planes + 2 * g, Y, w)[g:-g, :, :X] = value
        self.host = host
        self.buf = torch.from_numpy(host).cuda()
        assert self.buf.data_ptr() % 256 == 0
        self.addr = self.buf.data_ptr() + offset + g * Y * self.pitch

    def untouched(self):
        return np.array_equal(self.buf.cpu().numpy().view(np.uint32), self.host.view(np.uint32))


class DevOut:
    """n floats with GUARD floats before and after, PATTERN bytes everywhere.  addr: the first of the n."""
    GUARD = 64

    def __init__(self, torch, n):
        self.n = int(n)
        self.buf = torch.full(((self.n + 2 * self.GUARD) * 4,), PATTERN, dtype=torch.uint8, device="cuda")
        self.addr = self.buf.data_ptr() + self.GUARD * 4

    def host(self):
        """(the n floats, are the guards untouched)"""
        a = self.buf.cpu().numpy()
        g = self.GUARD * 4
        return a[g:g + self.n * 4].view(np.float32).copy(), bool((a[:g] == PATTERN).all() and (a[g + self.n * 4:] == PATTERN).all())


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == PATTERN).all())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_normals(a, b):
    """Equal bits, a NaN (0 / 0 where the central differences vanish) wherever the other has one."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint32), b[ok].view(np.uint32))


def gpu_points(torch, capi, vol, res, vs, capacity, zs0=0, z0=0, z1=None):
    """(count, found, the capacity x 3 floats as the kernel left them, output guards untouched)"""
    ws = torch.zeros(capi.extract_workspace_bytes(list(res)), dtype=torch.uint8, device="cuda")
    out = DevOut(torch, capacity * 3)
    cnt, found = capi.extract_points(vol.addr, vol.pitch, list(res), vs, out.addr, capacity, ws, zs0=zs0, z0=z0, z1=z1)
    got, ok = out.host()
    return cnt, found, got.reshape(-1, 3), ok


def gpu_normals(torch, capi, vol, res, vs, pts, zs0=0, zs1=None):
    """(normals [n, 3], output guards untouched, the points unchanged)"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    n = len(pts)
    dp = DevOut(torch, n * 3)
    dp.buf[DevOut.GUARD * 4:(DevOut.GUARD + n * 3) * 4] = torch.from_numpy(pts.view(np.uint8).reshape(-1).copy()).cuda()
    out = DevOut(torch, n * 3)
    capi.extract_normals(vol.addr, vol.pitch, list(res), vs, dp.addr, n, out.addr, zs0=zs0, zs1=zs1)
    torch.cuda.synchronize()
    got, ok = out.host()
    back, pok = dp.host()
    return got.reshape(-1, 3), ok and pok and same_bits(back.reshape(-1, 3), pts)
