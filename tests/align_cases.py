"""The cases that hold the map alignment (xs_tsdf_align_terms, x-slam_amd/csrc/xs_align.hip; align_host.hpp; KinectFusion.align_map) to a model
written from the per-entry contract in include/xslam_amd.h and not from the kernel.  Test infrastructure; backend-neutral parts first
(tests/test_align_cases_cpu.py), the device helpers after them (the GPU tests hand torch in).

THE MODEL is the contract in numpy float32, operation by operation: real parts in merge_cases' order, complex parts by the multiply and add
of csrc/xs_complex.h restated below (cplx * real = (re y, im y); cplx * cplx = (ac - bd, ad + bc); real - cplx = (-re + x, -im); sums and
differences by component).  The library is built with -ffp-contract=off, so a correct kernel produces the model's float32 residuals bit for bit
and differs from the model's 29 sums only by the association of its double additions.

THE TWIN redoes the same operations in float64 on the float32 map entries, corner values and gt, on the model's own cells b and the model's
own keep / drop decisions (no discrete decision can differ).

THE BOUND.  Every quantity is carried as a triple (float32 value, float64 value, e) with |float32 - float64| <= e, through every operation
of the contract (u = 2^-24):
    exact inputs (map entries, voxel indices, corner values, gt)      e = 0
    z = x + y, x - y                                                    e_z = (e_x + e_y) (1 + u) + u |z|
    z = x y                                                             e_z = (|x| e_y + |y| e_x + e_x e_y) (1 + u) + u |z|
    negation                                                            e_z = e_x
(the rounding of the operation itself, u |z| with |z| the twin's magnitude plus the operands' errors, and the operands' errors passed on: the
standard running error analysis, first and second order kept).  Nothing is fitted: the constant "c" of a sum is the count of operations
between the inputs and the term — 6 for an index (three products, three sums), one for the fraction and one for its complement, 3 per real
stage and 7 per complex stage of the interpolation, one for the residual — applied to the magnitudes the operations actually have instead of
one worst-case magnitude, because the residual F - gt cancels and a bound relative to |r| does not exist.  A term of a sum is a product p q
of two residual parts, formed exactly in double: |p32 q32 - p64 q64| <= |p| e_q + |q| e_p + e_p e_q, added over the kept entries; the double
additions of either side add n 2^-52 sum |terms|.  ALLOW covers the twin's own roundings (2^-53 relative per operation).

Case data.  Source volumes: values uniform in [-0.95, 0.95], a tenth each free space (1.0), +0 and -0; weights 1 .. 9 with a quarter of
the volume at weight 0 in blocks of 3^3 voxels (random single zeros would leave one voxel in ten with eight valid corners; blocks leave
about half).  The index of THIS map: fabricated by hand (random voxels of a destination box with random band values) or built by
xs_tsdf_band_build from a dense volume of the same kind.  Condition on every case, checked on the CPU and kept at zero (near_threshold): no
entry's twin |Re r| lies within its own e of max_residual, for any seed; where a seed of the generator produces one, another seed is chosen.
Counts are therefore required equal."""
import functools

import numpy as np

from merge_cases import affine64, pitches, rotation, xform  # noqa: F401  (re-exported for the tests)

U = 2.0 ** -24
ALLOW = 1.01
H = float(np.float32(1e-7))          # the seed step as the kernels and gn_scale_sums hold it
MIN_WEIGHTS = (1, 3)
MAX_RESIDUAL = 1.0
F32 = np.float32

# (X, Y, Z) of the source volumes the kernel test runs; the first two have a single cell or a single row of cells
SOURCE_SHAPES = [(2, 2, 2), (3, 2, 2), (9, 10, 13), (70, 33, 5)]
INDEX_COUNTS = [0, 1, 63, 64, 65, 255, 257]
FULL_CASE_COUNT = 255     # from this many fabricated entries on, a case must drop entries at every gate and keep some (case())
# The largest displacement of a corner of the 64^3 volume between the final T of the float32 model's loop and of the float64 twin's loop on
# tests/test_align_pipeline_gpu.py's scene and start (ten iterations), computed on the CPU from that scene's two volumes: 4.275e-07 m, 5e-6
# voxel edges (the loop is still contracting by a factor of four per iteration when it stops, so the two have not met).  The constant is
# that measurement rounded up; the GPU's loop, whose sums differ from the model's by association only, is allowed four times it (it came
# to 5.9e-15 m when this was written).
PIPELINE_MODEL_TWIN_CORNER_M = 4.5e-7


# ------------------------------------------------------------------------------------------------
# Volumes and indices
def source(rng, shape):
    """(value, weight) [Z, Y, X] of a source volume."""
    X, Y, Z = shape
    v = rng.uniform(-0.95, 0.95, (Z, Y, X)).astype(F32)
    pick = rng.random((Z, Y, X))
    v[pick < 0.1] = F32(1.0)
    v[(pick >= 0.1) & (pick < 0.2)] = F32(0.0)
    v[(pick >= 0.2) & (pick < 0.3)] = F32(-0.0)
    w = rng.integers(1, 10, (Z, Y, X)).astype(np.int32)
    coarse = rng.random((-(-Z // 3), -(-Y // 3), -(-X // 3))) < 0.25
    if min(shape) <= 3:
        coarse[...] = False
        coarse.reshape(-1)[0] = rng.random() < 0.25
    zero = np.repeat(np.repeat(np.repeat(coarse, 3, 0), 3, 1), 3, 2)[:Z, :Y, :X]
    w[zero] = 0
    return v, w


def dense_this(rng, shape):
    """A dense value volume [Z, Y, X] of THIS map for xs_tsdf_band_build: about two thirds of it in the band."""
    v, _ = source(rng, shape)
    return v


def band_of(dense):
    """The band voxels of a dense volume [Z, Y, X] (gt != 0, |gt| <= 0.95), in raster order: (xyz [n, 3] int64, gt [n] float32)."""
    z, y, x = np.nonzero((dense != 0) & (np.abs(dense) <= F32(0.95)))
    return np.stack([x, y, z], axis=1).astype(np.int64), dense[z, y, x].astype(F32)


def fabricated_index(rng, count, dshape):
    """`count` entries made by hand: voxels of the box dshape (repeats allowed), band values."""
    xyz = np.stack([rng.integers(0, dshape[a], count) for a in range(3)], axis=1).astype(np.int64).reshape(count, 3)
    gt = rng.uniform(0.01, 0.95, count).astype(F32) * np.where(rng.random(count) < 0.5, F32(-1), F32(1))
    return xyz, gt.astype(F32)


def keys_of(xyz):
    return (xyz[:, 0].astype(np.uint64) | (xyz[:, 1].astype(np.uint64) << np.uint64(21)) | (xyz[:, 2].astype(np.uint64) << np.uint64(42))).view(np.int64)


def xyz_of(keys):
    k = np.asarray(keys).view(np.uint64)
    return np.stack([k & np.uint64(0x1fffff), (k >> np.uint64(21)) & np.uint64(0x1fffff), k >> np.uint64(42)], axis=1).astype(np.int64)


# ------------------------------------------------------------------------------------------------
# The seeded maps and the step, restated (align_host.hpp)
def seeded_maps(T, vs_this, vs_other):
    """align_seeded_maps restated: float64 in its order of operations, each part rounded once: [6, 12, 2] float32."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    vd, vs = np.float64(vs_this), np.float64(vs_other)
    re = affine64(T, vd, vs)
    h, half = np.float64(H), np.float64(0.5) * vd
    out = np.zeros((6, 12, 2), F32)
    for k in range(6):
        Im = np.zeros((3, 4), np.float64)
        if k < 3:
            Im[k, 3] = h
        else:
            a = k - 3
            b, c = (a + 1) % 3, (a + 2) % 3
            Im[c, :] = h * T[b, :]
            Im[b, :] = -(h * T[c, :])
        im = np.zeros(12, np.float64)
        for a in range(3):
            for b in range(3):
                im[3 * a + b] = Im[a, b] * vd / vs
            im[9 + a] = (((Im[a, 0] * half + Im[a, 1] * half) + Im[a, 2] * half) + Im[a, 3]) / vs
        out[k, :, 0], out[k, :, 1] = re, im.astype(F32)
    return out


def real_maps(m12):
    """Six seeded maps with the real parts m12 and imaginary parts as if T's linear block were m12's own (for maps given as xform12, not as
    T): seed k < 3 puts h into offset k, seed 3 + a rotates rows b, c of the whole map into each other."""
    m = np.asarray(m12, np.float64)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = m[:9].reshape(3, 3), m[9:] + 0.5 - 0.5 * m[:9].reshape(3, 3).sum(axis=1)   # merge_affine inverted at voxel sizes 1
    out = seeded_maps(T, 1.0, 1.0)
    out[:, :, 0] = np.asarray(m12, F32)
    return out


def se3_exp(delta):
    v, w = np.asarray(delta[:3], np.float64), np.asarray(delta[3:], np.float64)
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    if th < 1e-4:
        A, B, C = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        A, B, C = np.sin(th) / th, (1.0 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + A * W + B * (W @ W)
    E[:3, 3] = (np.eye(3) + B * W + C * (W @ W)) @ v
    return E


def scale_sums(raw):
    s = np.array(raw, np.float64)
    s[:21] /= H * H
    s[21:27] /= H
    return s


def step(s29, damping, T):
    """align_step restated: (taken, T).  Cholesky through numpy."""
    s = np.asarray(s29, np.float64)
    if s[28] < 6:
        return False, T
    A = np.zeros((6, 6))
    q = 0
    for j in range(6):
        for k in range(j, 6):
            A[j, k] = A[k, j] = s[q]
            q += 1
    A[np.arange(6), np.arange(6)] *= 1.0 + damping
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return False, T
    x = np.linalg.solve(L.T, np.linalg.solve(L, -s[21:27]))
    if not np.isfinite(x).all():
        return False, T
    out = np.array(T, np.float64).reshape(4, 4).copy()
    out[:3, :] = (se3_exp(x) @ out)[:3, :]
    return True, out


# ------------------------------------------------------------------------------------------------
# The model, its twin and the bound in one pass
class Q:
    """A real quantity per index entry: a (float32 model), d (float64 twin), e (bound on |a - d|)."""
    __slots__ = ("a", "d", "e")

    def __init__(self, a, d=None, e=0.0):
        self.a = a
        self.d = np.asarray(a, np.float64) if d is None else d
        self.e = e

    def __add__(self, o):
        d = self.d + o.d
        return Q(self.a + o.a, d, (self.e + o.e) * (1 + U) + U * np.abs(d))

    def __sub__(self, o):
        d = self.d - o.d
        return Q(self.a - o.a, d, (self.e + o.e) * (1 + U) + U * np.abs(d))

    def __mul__(self, o):
        d = self.d * o.d
        return Q(self.a * o.a, d, (np.abs(self.d) * o.e + np.abs(o.d) * self.e + self.e * o.e) * (1 + U) + U * np.abs(d))

    def __neg__(self):
        return Q(-self.a, -self.d, self.e)


def c_add(x, y):
    return (x[0] + y[0], x[1] + y[1])


def c_mul_real(x, r):          # cplx * T and T * cplx: (re r, im r)
    return (x[0] * r, x[1] * r)


def c_mul(z, w):               # (ac - bd, ad + bc)
    ac, bd, ad, bc = z[0] * w[0], z[1] * w[1], z[0] * w[1], z[1] * w[0]
    return (ac - bd, ad + bc)


def c_sub_real(x, r):          # cplx - T
    return (x[0] - r, x[1])


def c_real_sub(r, y):          # T - cplx: (-re + x, -im)
    return (-y[0] + r, -y[1])


def evaluate(xyz, gt, src, maps, min_weight=1, max_residual=MAX_RESIDUAL):
    """One transform's pass: the contract on index entries (xyz [n, 3], gt [n]) against src = (value, weight) [Z, Y, X] under maps [6, 12, 2].
    Returns a dict: sums32 / sums64 (the 29 raw sums of the model and of the twin), bound (29), terms (29: sum |terms|), kept [n], the
    entries dropped at each gate (outside, weight, residual), near_threshold (entries that violate the condition on the cases), e (the
    residual parts of the kept entries: [6][2] of Q)."""
    sv, sw = src
    SZ, SY, SX = sv.shape
    S = (SX, SY, SZ)
    n = len(gt)
    m = np.asarray(maps, F32).reshape(6, 12, 2)
    c = [xyz[:, a].astype(F32) for a in range(3)]
    with np.errstate(over="ignore", invalid="ignore"):
        g0 = [((m[0, 3 * a, 0] * c[0] + m[0, 3 * a + 1, 0] * c[1]) + m[0, 3 * a + 2, 0] * c[2]) + m[0, 9 + a, 0] for a in range(3)]
    inside = np.ones(n, bool)
    for a in range(3):
        inside &= (g0[a] >= 0) & (g0[a] < F32(S[a] - 1))
    b = [np.floor(np.where(inside, g0[a], F32(0))).astype(np.int64) for a in range(3)]
    idx = [(b[0] + (d & 1), b[1] + (d >> 1 & 1), b[2] + (d >> 2 & 1)) for d in range(8)]
    assert all(((idx[d][a] >= 0) & (idx[d][a] < S[a])).all() for d in range(8) for a in range(3))
    wmin = np.full(n, 1 << 30, np.int64)
    for d in range(8):
        wmin = np.minimum(wmin, sw[idx[d][2], idx[d][1], idx[d][0]])
    heavy = inside & (wmin >= min_weight)
    sel = np.flatnonzero(heavy)
    one = Q(F32(1))
    x, y, z = (Q(c[a][sel]) for a in range(3))
    bq = [Q(b[a][sel].astype(F32)) for a in range(3)]
    v = [Q(sv[idx[d][2][sel], idx[d][1][sel], idx[d][0][sel]].astype(F32)) for d in range(8)]
    gq = Q(np.asarray(gt, F32)[sel])
    e = []
    ok = np.ones(len(sel), bool)
    near = np.zeros(len(sel), bool)
    for k in range(6):
        me = lambda i: (Q(m[k, i, 0]), Q(m[k, i, 1]))
        f, cm = [], []
        for a in range(3):
            ga = c_add(c_add(c_add(c_mul_real(me(3 * a), x), c_mul_real(me(3 * a + 1), y)), c_mul_real(me(3 * a + 2), z)), me(9 + a))
            f.append(c_sub_real(ga, bq[a]))
            cm.append(c_real_sub(one, f[a]))
        stage1 = [c_add(c_mul_real(cm[0], v[d]), c_mul_real(f[0], v[d + 1])) for d in (0, 2, 4, 6)]
        c0 = c_add(c_mul(stage1[0], cm[1]), c_mul(stage1[1], f[1]))
        c1 = c_add(c_mul(stage1[2], cm[1]), c_mul(stage1[3], f[1]))
        F = c_add(c_mul(c0, cm[2]), c_mul(c1, f[2]))
        r = c_sub_real(F, gq)
        e.append(r)
        ok &= ~(np.abs(r[0].a) > F32(max_residual))
        near |= np.abs(np.abs(r[0].d) - max_residual) <= ALLOW * r[0].e
    kept = np.zeros(n, bool)
    kept[sel[ok]] = True
    e = [(Q(r[0].a[ok], r[0].d[ok], r[0].e[ok]), Q(r[1].a[ok], r[1].d[ok], r[1].e[ok])) for r in e]
    cnt = int(ok.sum())
    s32, s64, bound, terms = (np.zeros(29) for _ in range(4))

    def term(q, p, r):
        a, d = p.a.astype(np.float64) * r.a.astype(np.float64), p.d * r.d
        s32[q], s64[q] = a.sum(), d.sum()
        terms[q] = np.abs(d).sum()
        bound[q] = ALLOW * (np.abs(p.d) * r.e + np.abs(r.d) * p.e + p.e * r.e).sum() + cnt * 2.0 ** -52 * terms[q]

    q = 0
    for j in range(6):
        for k in range(j, 6):
            term(q, e[j][1], e[k][1])
            q += 1
    for k in range(6):
        term(21 + k, e[k][1], e[0][0])
    term(27, e[0][0], e[0][0])
    s32[28] = s64[28] = cnt
    return dict(sums32=s32, sums64=s64, bound=bound, terms=terms, kept=kept, outside=int((~inside).sum()), weight=int((inside & ~heavy).sum()),
                residual=int(len(sel) - cnt), near_threshold=int((near).sum()), e=e)


def loop(xyz, gt, src, T0, vs_this, vs_other, iterations, damping=1e-3, min_weight=1, max_residual=MAX_RESIDUAL, twin=False):
    """The whole alignment loop of one start on the CPU, gn_batch_loop's shape: `iterations` steps and a final loss pass.  Returns
    (ok, T, loss history, the last pass's evaluate)."""
    T = np.array(T0, np.float64).reshape(4, 4).copy()
    hist, ev = [], None
    for p in range(iterations + 1):
        ev = evaluate(xyz, gt, src, seeded_maps(T, vs_this, vs_other), min_weight, max_residual)
        s = scale_sums(ev["sums64" if twin else "sums32"])
        hist.append(s[27] / s[28] if s[28] > 0 else 0.0)
        if p == iterations:
            return True, T, np.array(hist), ev
        taken, T = step(s, damping, T)
        if not taken:
            return False, T, np.array(hist), ev
    return True, T, np.array(hist), ev


def corner_displacement(Ta, Tb, res, voxel_size):
    """The largest distance between the images of the volume's eight corners under Ta and Tb (metres)."""
    ext = np.asarray(res, np.float64) * voxel_size
    worst = 0.0
    for cidx in range(8):
        p = np.array([ext[0] * (cidx & 1), ext[1] * (cidx >> 1 & 1), ext[2] * (cidx >> 2 & 1), 1.0])
        worst = max(worst, float(np.linalg.norm((np.asarray(Ta) @ p - np.asarray(Tb) @ p)[:3])))
    return worst


def perturbed(T_true, res, voxel_size, shift_voxels=(0.3, -0.3, 0.26), degrees=0.5, axis=(0.3, 1.0, -0.4)):
    """T_true with half a voxel edge of translation and a rotation by `degrees` about `axis` through the volume's centre in front of it."""
    c = 0.5 * np.asarray(res, np.float64) * voxel_size
    P = np.eye(4)
    P[:3, :3] = rotation(axis, np.radians(degrees))
    P[:3, 3] = c - P[:3, :3] @ c + np.asarray(shift_voxels, np.float64) * voxel_size
    return P @ np.asarray(T_true, np.float64)


# ------------------------------------------------------------------------------------------------
# The kernel's cases
def case_seed(sshape, count):
    return 7919 * sshape[0] + 131 * sshape[1] + sshape[2] + 1000003 * count


def dst_shape_of(sshape):
    """The box THIS map's entries are drawn from: the source's, two voxels larger, so that identity and shifts leave entries outside."""
    return tuple(s + 2 for s in sshape)


@functools.lru_cache(maxsize=None)
def case_maps(sshape):
    """name -> seeded maps [6, 12, 2] from THIS map's box dst_shape_of(sshape) into a source of sshape."""
    rng = np.random.default_rng(case_seed(sshape, 0) + 11)
    D, S = np.array(dst_shape_of(sshape)), np.array(sshape)
    vs = 0.0625

    def rigid(angle):
        R = rotation(rng.normal(size=3), angle)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, 0.5 * S * vs - R @ (0.5 * D * vs) + rng.uniform(-0.4, 0.4, 3) * vs
        return T

    out = {
        "identity": real_maps(xform()),
        "shift_whole": real_maps(xform(offset=(-1, -1, -1))),
        "shift_mixed": real_maps(xform(offset=(1, -2, 0))),
        "half_x": real_maps(xform(offset=(-0.5, -1, -1))),
        "half_xyz": real_maps(xform(offset=(-1.5, -0.5, -1.5))),
        "far_face": real_maps(xform(offset=S - D)),                  # the last entry of the box lands exactly on S - 1: dropped
        "rotation_2": seeded_maps(rigid(np.radians(2.0)), vs, vs),
        "rotation_7": seeded_maps(rigid(np.radians(7.0)), vs, vs),
        "ratio_2": seeded_maps(np.eye(4), 2 * vs, vs),
        "ratio_half": seeded_maps(np.eye(4), 0.5 * vs, vs),
        "miss": real_maps(xform(offset=S + 5)),
    }
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(sshape, count, built=False):
    """(xyz, gt, src, dense): an index of `count` fabricated entries (built: the band of a dense volume of dst_shape_of(sshape), `count`
    ignored), a source, and the seed bumped until (a) no map and min_weight leaves an entry near the residual threshold and (b), for the
    cases large enough to be held to it (FULL_CASE_COUNT entries or more, or a built index over a source wider than 3 voxels), every one of
    the three gates drops an entry and an entry is kept, over the case's maps and min_weights together."""
    full = count >= FULL_CASE_COUNT or (built and min(sshape) > 3)
    for bump in range(400):
        rng = np.random.default_rng(case_seed(sshape, count) + 7 * bump + (3 if built else 0))
        src = source(rng, sshape)
        dense = dense_this(rng, dst_shape_of(sshape)) if built else None
        xyz, gt = band_of(dense) if built else fabricated_index(rng, count, dst_shape_of(sshape))
        evs = [evaluate(xyz, gt, src, m, mw) for m in case_maps(sshape).values() for mw in MIN_WEIGHTS]
        if any(ev["near_threshold"] for ev in evs):
            continue
        if full and not all(sum(ev[k] if k != "kept" else int(ev[k].sum()) for ev in evs) > 0 for k in ("outside", "weight", "residual", "kept")):
            continue
        for a in (xyz, gt) + src + ((dense,) if built else ()):
            a.setflags(write=False)
        return xyz, gt, src, dense
    raise AssertionError("no seed that meets the conditions on the cases")


@functools.lru_cache(maxsize=None)
def expected(sshape, count, built, name, min_weight):
    xyz, gt, src, _ = case(sshape, count, built)
    return evaluate(xyz, gt, src, case_maps(sshape)[name], min_weight)


def sphere_scene(n=24, shift=(2, -1, 1), voxel_size=0.05, trunc_voxels=3.0):
    """THIS map and the other map of the loop tests: a sphere's truncated signed distance on n^3 voxels, the other map the same field
    shifted by whole voxels (other voxel d holds this map's voxel d + shift: the same float32 numbers, so the residual at the truth is 0
    exactly), weights 5.  Returns (this value [n, n, n], (other value, other weight), T_true: this map's frame -> the other's)."""
    pad = 4
    N = n + 2 * pad
    ax = (np.arange(N, dtype=np.float64) - pad + 0.5) * voxel_size
    zz, yy, xx = np.meshgrid(ax, ax, ax, indexing="ij")
    c = 0.5 * n * voxel_size
    d = np.sqrt((xx - c * 1.05) ** 2 + (yy - c * 0.95) ** 2 + (zz - c) ** 2) - 0.33 * n * voxel_size
    big = np.clip(d / (trunc_voxels * voxel_size), -1.0, 1.0).astype(F32)
    this = big[pad:pad + n, pad:pad + n, pad:pad + n].copy()
    s = shift
    other = big[pad + s[2]:pad + s[2] + n, pad + s[1]:pad + s[1] + n, pad + s[0]:pad + s[0] + n].copy()
    T = np.eye(4)
    T[:3, 3] = -np.asarray(s, np.float64) * voxel_size
    return this, (other, np.full(other.shape, 5, np.int32)), T


# ------------------------------------------------------------------------------------------------
# Device helpers (torch and capi are handed in by the GPU tests)
class DevSource:
    """The value and weight arrays of a source on the device, one pitch and base offset, each an extract_cases.DevVolume with guard planes
    and padding that any kernel that read them as a weight or a value would show."""

    def __init__(self, torch, src, pitch, offset=0):
        from extract_cases import DevVolume
        v, w = src
        self.shape, self.pitch = v.shape, int(pitch)
        self.value = DevVolume(torch, np.ascontiguousarray(v, F32), pitch, offset)
        self.weight = DevVolume(torch, np.ascontiguousarray(w, np.int32).view(F32), pitch, offset)

    def untouched(self):
        return self.value.untouched() and self.weight.untouched()


def fabricated_band_index(torch, capi, xyz, gt):
    """A capi.BandIndex over hand-made entries (nblocks 1: the field the alignment does not use but checks)."""
    n = len(gt)
    idx = capi.BandIndex()
    idx.keys_t = torch.from_numpy(np.array(keys_of(xyz) if n else np.zeros(1, np.int64))).cuda()
    idx.values_t = torch.from_numpy(np.array(gt if n else np.zeros(1, F32))).cuda()
    idx.keys, idx.values, idx.capacity, idx.count, idx.nblocks = idx.keys_t.data_ptr(), idx.values_t.data_ptr(), n, n, 1
    return idx


class AlignRunner:
    """A workspace (tickets zeroed once) and an output buffer with guards for xs_tsdf_align_terms."""

    def __init__(self, torch, capi, transforms=32):
        self.torch, self.capi = torch, capi
        self.ws = torch.full((capi.tsdf_align_workspace_bytes(transforms),), 0x5A, dtype=torch.uint8, device="cuda")
        capi.tsdf_reduce_workspace_init(self.ws)
        self.out = torch.full((29 * 32 + 16,), -7.0, dtype=torch.float64, device="cuda")

    def run(self, index, dev, sshape, maps, min_weight, max_residual=MAX_RESIDUAL):
        """maps [N, 6, 12, 2]: the N x 29 raw sums."""
        maps = np.ascontiguousarray(maps, F32).reshape(-1, 6, 12, 2)
        N = maps.shape[0]
        self.out.fill_(-7.0)
        self.capi.tsdf_align_terms(index, dev.value.addr, dev.weight.addr, dev.pitch, list(sshape), maps, min_weight, max_residual, self.ws, self.out)
        self.torch.cuda.synchronize()
        host = self.out.cpu().numpy()
        assert (host[29 * N:] == -7.0).all(), "wrote past its transforms' sums"
        return host[:29 * N].reshape(N, 29).copy()

    def tickets_zero(self):
        return not self.ws[:256].any().item()
