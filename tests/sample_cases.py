"""Cases and models for xs_tsdf_sample_points / xs_tsdf_sample_depth (x-slam_amd/csrc/xs_sample.hip), shared by
tests/test_sample_cases_cpu.py, tests/test_sample_gpu.py and tests/test_sample_pipeline_gpu.py.

sample_points() and sample_depth() are the contract of include/xslam_amd.h written out in numpy, one array operation per IEEE operation of the
contract, in the contract's order, written from the header and not from the kernel.  With dtype=np.float32 every operation is one correctly
rounded float32 operation (numpy does not contract), so the GPU tests ask for equal bits.  With dtype=np.float64 the same text is the float64
twin (the inputs are the float32 inputs, converted exactly).  F is trilinear() below, which the CPU tests hold equal to render_cases._trilinear
(the contract declares them one function); it is restated here because it reports WHY it refuses, interpolates a second array, and carries the
switches of the mutants (MUTANTS): mistakes a kernel could make, each of which must change an expected byte of some case.

The bound between the two precisions (bounds) is derived operation by operation, u = 2^-24:
  P, points       without a transform P = p exactly: Ep = 0.  With one, P[c] = ((R0 p0 + R1 p1) + R2 p2) + t: a product rounds once and then passes
                  through at most three sums: Ep = 4u A,  A = max over the points of |R0 p0| + |R1 p1| + |R2 p2| + |t|.
  P, depth        z = float(D) / 1000 rounds once (D is exact).  dx, dy two roundings each; d[c] = (R0 dx + R1 dy) + R2: |err d| <= 5u A,
                  A = max (|R0 dx| + |R1 dy| + |R2|), as render_cases derives it.  P[c] = t + z d: |err| <= zmax 5u A + 2u zmax Dm + u L =: Ep,
                  zmax = 5, Dm = max |d[c]|, L = max |t[c]| + zmax Dm >= |P[c]|.
  g = P / vs - 0.5   |err g| <= Ep / vs + u L / vs + u (L / vs + 0.5) =: Eg   (in voxels; L = max |P[c]| over the points compared)
  F               continuous across cells, its slope along an axis at most Delta = max |v - v'| over face neighbours; the stages round 12 times
                  (render_cases): |err F| <= 3 Delta Eg + 12u vmax =: EF.  The same for dvalue with the grad array's Delta and vmax.
  gradient        h = 0.5 vs is exact; P +- h rounds once more: Ep' = Ep + u (L + h), Eg' and EF' from it with L + h for L.
                  G = Fp - Fm: |err G| <= 2 EF' + u |G| <= 2 EF' + 2u vmax;  G / vs rounds once more: |err| <= (2 EF' + 4u vmax) / vs.
The bounds are global per case and hold where both precisions give the same status; ALLOW covers the second-order terms."""
import functools

import numpy as np

import render_cases as rc

U, ALLOW, NAN_BITS, F32 = rc.U, rc.ALLOW, rc.NAN_BITS, np.float32
OUTSIDE, UNSEEN, OK, NO_DEPTH = 0, 1, 2, 3
DEPTH_MIN, DEPTH_MAX = 200, 5000
OUTPUTS = ("status", "value", "dvalue", "gradient", "counts")
# "<" for "<=" at the upper limit; x and y exchanged in the row index; the unneeded corners' weights read; h = voxel_size; g without the - 0.5; the
# depth limits off by one; a row offset taken modulo 2^32
MUTANTS = ("upper_lt", "row_xy", "all_weights", "h_full", "no_half", "depth_limits", "row_wrap32")


# ------------------------------------------------------------------------------------------------
# The models
def trilinear(arrays, weight, vs, min_weight, p, T, mutant=None, pitch=None):
    """F(P) of the contract at the points p = [p0, p1, p2] (arrays of T) on each of `arrays` ([Z, Y, X] of T): (status, [values]).  Every voxel is
    read through its row (z Y + y) and column x; `pitch` (bytes per row) matters to the row_wrap32 mutant alone."""
    Z, Y, X = weight.shape
    S = (X, Y, Z)
    half = T(0) if mutant == "no_half" else T(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        g = [p[c] / vs - half for c in range(3)]
        inb = np.ones(g[0].shape, bool)
        for c in range(3):
            inb &= (g[c] >= 0) & ((g[c] < T(S[c] - 1)) if mutant == "upper_lt" else (g[c] <= T(S[c] - 1)))
        b, f, need = [], [], []
        for c in range(3):
            gc = np.where(inb, g[c], T(0))
            bc = np.floor(gc)
            f.append(gc - bc)
            b.append(bc.astype(np.int64))
            need.append(f[c] > 0)

    def read(a, ix, iy, iz):
        row, col = (iz * Y + np.minimum(ix, Y - 1), np.minimum(iy, X - 1)) if mutant == "row_xy" else (iz * Y + iy, ix)
        if mutant == "row_wrap32" and (row * pitch >= 1 << 32).any():
            assert pitch & (pitch - 1) == 0      # (a power of two: the wrapped offset is a whole row again)
            row = (row * pitch) % (1 << 32) // pitch
        return a.reshape(Z * Y, X)[row, col]

    ws = np.full(g[0].shape, 0x7FFFFFFF, np.int64)
    v = [[None] * 8 for _ in arrays]
    for d in range(8):
        used = np.ones(g[0].shape, bool)
        idx = []
        for c in range(3):
            bit = d >> c & 1
            if bit:
                used &= need[c]
            idx.append(np.minimum(b[c] + bit, S[c] - 1))   # (an unused corner may lie outside: it is not read)
        w = read(weight, *idx)
        ws = np.minimum(ws, w) if mutant == "all_weights" else np.where(used, np.minimum(ws, w), ws)
        for k, a in enumerate(arrays):
            v[k][d] = np.where(used, read(a, *idx), T(0))
    status = np.where(inb, np.where(ws >= min_weight, OK, UNSEEN), OUTSIDE).astype(np.uint8)
    for k in range(3):
        stride = 1 << k
        fk = f[k]
        gk = T(1) - fk
        for vv in v:
            for d in range(0, 8, 2 * stride):
                vv[d] = np.where(need[k], vv[d] * gk + vv[d + stride] * fk, vv[d])
    return status, [vv[0] for vv in v]


def _with_nans(a, bad, T):
    a = np.array(a, T)
    if T is np.float32:
        a.view(np.uint32)[bad] = NAN_BITS
    else:
        a[bad] = np.nan
    return a


def _sample(vol, vs, P, min_weight, grad, T, mutant, pitch, no_depth=None):
    """Every output at the points P = [P0, P1, P2] (arrays of T): status, value, dvalue (None without grad), G (a list of three), counts."""
    value, weight = vol
    val = value.astype(T)
    vs = T(F32(vs))
    mw = max(1, int(min_weight))
    arrays = [val] if grad is None else [val, grad.astype(T)]
    status, out = trilinear(arrays, weight, vs, mw, P, T, mutant, pitch)
    if no_depth is not None:
        status = np.where(no_depth, np.uint8(NO_DEPTH), status)
    ok = status == OK
    h = (T(1) if mutant == "h_full" else T(0.5)) * vs
    G, gok = [], ok.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            sp, Fp = trilinear([val], weight, vs, mw, [P[a] + h if a == c else P[a] for a in range(3)], T, mutant, pitch)
            sm, Fm = trilinear([val], weight, vs, mw, [P[a] - h if a == c else P[a] for a in range(3)], T, mutant, pitch)
            gok &= (sp == OK) & (sm == OK)
            G.append((Fp[0] - Fm[0]) / vs)
    res = dict(status=status, value=_with_nans(out[0], ~ok, T), dvalue=None if grad is None else _with_nans(out[1], ~ok, T),
               G=[_with_nans(G[c], ~gok, T) for c in range(3)], gok=gok, counts=np.bincount(status.reshape(-1), minlength=4).astype(np.uint64), P=P)
    return res


def sample_points(vol, vs, pts, xform=None, min_weight=1, grad=None, dtype=np.float32, mutant=None, pitch=None):
    """The contract of xs_tsdf_sample_points.  vol = (value [Z, Y, X] float32, weight [Z, Y, X] int32), pts float32 [N, 3], xform float32 [12] or None.
    Returns a dict: status uint8 [N], value, dvalue (None without grad) [N], gradient [N, 3], counts uint64 [4], and for the tests gok and P."""
    T = dtype
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    p = [pts[:, c].astype(T) for c in range(3)]
    if xform is None:
        P = p
    else:
        m = np.asarray(xform, np.float32).reshape(12).astype(T)
        with np.errstate(invalid="ignore", over="ignore"):
            P = [((m[3 * c] * p[0] + m[3 * c + 1] * p[1]) + m[3 * c + 2] * p[2]) + m[9 + c] for c in range(3)]
    r = _sample(vol, vs, P, min_weight, grad, T, mutant, pitch)
    r["gradient"] = np.stack(r.pop("G"), axis=1)
    return r


def sample_depth(vol, vs, depth, intr, R, t, min_weight=1, grad=None, dtype=np.float32, mutant=None, pitch=None):
    """The contract of xs_tsdf_sample_depth.  depth uint16 [rows, cols], intr (fx, fy, cx, cy), R [3, 3], t [3] camera to volume.  The outputs are
    images [rows, cols], gradient [3, rows, cols]."""
    T = dtype
    depth = np.asarray(depth, np.uint16)
    rows, cols = depth.shape
    lo, hi = (DEPTH_MIN + 1, DEPTH_MAX - 1) if mutant == "depth_limits" else (DEPTH_MIN, DEPTH_MAX)
    D = depth.astype(np.int64)
    no_depth = (D < lo) | (D > hi)
    fx, fy, cx, cy = (T(F32(a)) for a in intr)
    R = np.asarray(R, np.float32).reshape(3, 3).astype(T)
    t = np.asarray(t, np.float32).reshape(3).astype(T)
    z = D.astype(T) / T(1000)
    dx = ((np.arange(cols, dtype=T) - cx) / fx)[None, :]
    dy = ((np.arange(rows, dtype=T) - cy) / fy)[:, None]
    d = [(R[c, 0] * dx + R[c, 1] * dy) + R[c, 2] for c in range(3)]
    P = [t[c] + z * d[c] for c in range(3)]
    r = _sample(vol, vs, P, min_weight, grad, T, mutant, pitch, no_depth=no_depth)
    bad = np.broadcast_to(no_depth, r["value"].shape)
    r["value"] = _with_nans(r["value"], bad, T)
    if r["dvalue"] is not None:
        r["dvalue"] = _with_nans(r["dvalue"], bad, T)
    r["gok"] = r["gok"] & ~no_depth
    r["gradient"] = np.stack([_with_nans(g, bad, T) for g in r.pop("G")], axis=0)
    r["d"] = d
    return r


def _field_terms(a):
    a = np.asarray(a, np.float64)
    delta = max(float(np.abs(np.diff(a, axis=k)).max()) if a.shape[k] > 1 else 0.0 for k in range(3))
    return delta, float(np.abs(a).max())


def bounds_from(Ep, L, vs, value, grad=None, storage=0.0):
    """(value bound, dvalue bound, gradient bound) from the error Ep of P and L >= |P[c]|: the derivation at the top.  storage: an error of every
    stored value against the field it stands for, in units of u vmax (the linear field's rounding)."""
    vs = float(vs)

    def EF(Ep, L, a):
        delta, vmax = _field_terms(a)
        Eg = Ep / vs + U * L / vs + U * (L / vs + 0.5)
        return 3 * delta * Eg + (12 + storage) * U * vmax, vmax
    h = 0.5 * vs
    EFv, _ = EF(Ep, L, value)
    EFg, vmax = EF(Ep + U * (L + h), L + h, value)
    Ed = EF(Ep, L, grad)[0] if grad is not None else None
    return ALLOW * EFv, None if Ed is None else ALLOW * Ed, ALLOW * (2 * EFg + 4 * U * vmax) / vs


def bounds(case, m64):
    """The bounds of `case` between the float32 model and its float64 twin m64."""
    sel = m64["status"] == OK
    L = max((float(np.abs(m64["P"][c][sel]).max()) for c in range(3)), default=0.0) if sel.any() else 0.0
    if case["kind"] == "points":
        Ep = 0.0
        if case["xform"] is not None:
            m = np.abs(case["xform"].astype(np.float64))
            p = np.abs(case["pts"].astype(np.float64))
            p = p[np.isfinite(p).all(axis=1)]
            Ep = 4 * U * max(float((m[3 * c] * p[:, 0] + m[3 * c + 1] * p[:, 1] + m[3 * c + 2] * p[:, 2] + m[9 + c]).max()) for c in range(3))
    else:
        R = np.abs(case["R"].astype(np.float64))
        intr = [float(a) for a in case["intr"]]
        rows, cols = case["depth"].shape
        dxm = max(abs((0 - intr[2]) / intr[0]), abs((cols - 1 - intr[2]) / intr[0]))
        dym = max(abs((0 - intr[3]) / intr[1]), abs((rows - 1 - intr[3]) / intr[1]))
        A = float((R[:, 0] * dxm + R[:, 1] * dym + R[:, 2]).max())
        Dm = max(float(np.abs(a).max()) for a in m64["d"])
        zmax = DEPTH_MAX / 1000.0
        L = float(np.abs(case["t"]).max()) + zmax * Dm
        Ep = zmax * 5 * U * A + 2 * U * zmax * Dm + U * L
    return bounds_from(Ep, L, case["vs"], case["vol"][0], case["grad"])


# ------------------------------------------------------------------------------------------------
# Volumes and point sets
VS2 = F32(0.0625)      # a power of two: (i + 0.5) vs, the limits and the points built on a 1/64 voxel lattice are exact, and so are their g


def random_volume(shape, seed, low_weight=0):
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    return rng.uniform(-1, 1, (Z, Y, X)).astype(np.float32), rng.integers(low_weight, 4, size=(Z, Y, X)).astype(np.int32)


def linear_volume(shape, vs, a, b):
    """value = a . centre + b, every weight 2: (volume, the field in float64)."""
    c = rc.centres(shape, float(vs))
    field = a[0] * c[0] + a[1] * c[1] + a[2] * c[2] + b
    return (field.astype(np.float32), np.full(field.shape, 2, np.int32)), field


def lattice_points(shape, vs, g):
    """Points at the continuous voxel indices g [N, 3] (multiples of 1/64): exact in float32 for a power-of-two vs."""
    return ((np.asarray(g, np.float64) + 0.5) * float(vs)).astype(np.float32)


def structured_points(vol, shape, vs, min_weight, seed, max_centres=3000):
    """The point set of the issue's list on one volume (vs a power of two): every voxel centre (a random max_centres of them on a large volume); points
    on cell faces and edges; g == 0 and g == S - 1 exactly and nextafter on either side of both; -0.0, NaN and +-Inf coordinates; centres whose
    neighbour along +x, +y or +z is unseen while they are seen (OK, with a refused gradient sample); random points reaching a voxel past every face."""
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    S = np.array(shape)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    cen = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float64)
    if len(cen) > max_centres:
        cen = cen[rng.choice(len(cen), max_centres, replace=False)]
    out = [lattice_points(shape, vs, cen)]
    g = rng.integers(0, (S - 1) * 64 + 1, size=(240, 3)) / 64.0                 # on the 1/64 lattice, inside
    snap = rng.integers(1, 7, size=240)                                         # bit c: axis c is snapped to a centre; 1 .. 6: one or two axes
    for c in range(3):
        g[:, c] = np.where(snap >> c & 1, np.floor(g[:, c]), g[:, c])
    out.append(lattice_points(shape, vs, g))
    base = lattice_points(shape, vs, [np.minimum(S - 1, S // 2) + np.array([0.25, 0.5, 0.75]) * (S > 1)])[0]
    edge = []
    for c in range(3):
        lo, hi = F32((0 + 0.5) * float(vs)), F32((S[c] - 1 + 0.5) * float(vs))
        for v in (lo, hi, np.nextafter(lo, F32(-np.inf)), np.nextafter(lo, F32(np.inf)), np.nextafter(hi, F32(-np.inf)), np.nextafter(hi, F32(np.inf)),
                  F32(-0.0), F32(np.nan), F32(np.inf), F32(-np.inf)):
            for start in (base, lattice_points(shape, vs, [np.zeros(3)])[0]):
                p = start.copy()
                p[c] = v
                edge.append(p)
    out.append(np.array(edge, np.float32))
    w = vol[1]
    for axis, sl_a, sl_b in ((2, np.s_[:, :, :-1], np.s_[:, :, 1:]), (1, np.s_[:, :-1, :], np.s_[:, 1:, :]), (0, np.s_[:-1], np.s_[1:])):
        if w.shape[axis] < 2:
            continue
        zz, yy, xx = np.nonzero((w[sl_a] >= min_weight) & (w[sl_b] < min_weight))
        if len(zz):
            pick = rng.choice(len(zz), min(len(zz), 24), replace=False)
            out.append(lattice_points(shape, vs, np.stack([xx[pick], yy[pick], zz[pick]], axis=1)))
    out.append(((rng.uniform(-1.0, 1.0, (300, 3)) * ((S - 1) / 2 + 1) + S / 2) * float(vs)).astype(np.float32))
    return np.concatenate(out).astype(np.float32)


def random_points(shape, vs, n, seed, margin=1.0):
    """n points uniform in the box that reaches `margin` voxels past the first and last voxel centres."""
    rng = np.random.default_rng(seed)
    S = np.array(shape, np.float64)
    return ((rng.uniform(-1.0, 1.0, (n, 3)) * ((S - 1) / 2 + margin) + S / 2) * float(vs)).astype(np.float32)


def rigid(seed, angle, shift):
    """xform12 (row-major R, then t, float32) and its float64 4 x 4."""
    import merge_cases as mc
    rng = np.random.default_rng(seed)
    T = np.eye(4)
    T[:3, :3] = mc.rotation(rng.normal(size=3), angle)
    T[:3, 3] = shift
    return np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]]).astype(np.float32), T


def points_for(xform, T, pts_volume):
    """Points of a frame A that the transform takes (up to rounding) to pts_volume."""
    inv = np.linalg.inv(T)
    return (pts_volume.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)


LINEAR_SHAPE, LINEAR_A, LINEAR_B = (9, 5, 6), (0.9, -0.6, 1.3), 0.1
IDENTITY12 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)


# ------------------------------------------------------------------------------------------------
# The cases
def _points_case(name, vol, vs, pts, xform=None, min_weight=1, grad=None, pitch_extra=0, offset=0):
    shape = vol[0].shape[::-1]
    for a in vol + ((grad,) if grad is not None else ()):
        a.setflags(write=False)
    pts = np.ascontiguousarray(pts, np.float32)
    pts.setflags(write=False)
    return dict(kind="points", name=name, vol=vol, vs=F32(vs), shape=shape, pts=pts, xform=xform, min_weight=min_weight, grad=grad, pitch=shape[0] * 4 + pitch_extra,
                offset=offset)


def _depth_case(name, vol, vs, depth, intr, R, t, min_weight=1, grad=None, pitch_extra=0, offset=0, depth_pitch_extra=0):
    shape = vol[0].shape[::-1]
    depth = np.ascontiguousarray(depth, np.uint16)
    depth.setflags(write=False)
    return dict(kind="depth", name=name, vol=vol, vs=F32(vs), shape=shape, depth=depth, intr=np.asarray(intr, np.float32), R=np.asarray(R, np.float32),
                t=np.asarray(t, np.float32), min_weight=min_weight, grad=grad, pitch=shape[0] * 4 + pitch_extra, offset=offset,
                depth_pitch=depth.shape[1] * 2 + depth_pitch_extra)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # one voxel, one cell, a ragged handful: random values, weights 0 .. 3 (1 .. 3 for the single voxel)
    for shape, seed in (((1, 1, 1), 1), ((2, 2, 2), 2), ((3, 4, 5), 3)):
        vol = random_volume(shape, seed, low_weight=1 if shape == (1, 1, 1) else 0)
        out.append(_points_case("v%d%d%d" % shape, vol, VS2, structured_points(vol, shape, VS2, 1, 10 + seed), pitch_extra=4 * (seed - 1)))
    # 33 x 17 x 20, pitched with an offset (the guard planes are the GPU test's): a sphere with a shell and a hole in the weights, and a grad array
    sphere = rc.sphere_volume((33, 17, 20), float(VS2), (0.45, 0.5, 0.55), 0.3, seed=4)
    grad = np.random.default_rng(40).normal(0.0, 0.5, sphere[0].shape).astype(np.float32)
    out.append(_points_case("s33_structured", sphere, VS2, structured_points(sphere, (33, 17, 20), VS2, 1, 14), grad=grad, pitch_extra=12, offset=8))
    out.append(_points_case("s33_structured_mw3", sphere, VS2, structured_points(sphere, (33, 17, 20), VS2, 3, 15), min_weight=3, pitch_extra=20, offset=4))
    # 100 003 random points of a frame that a rotation with a translation takes into a sphere at vs = 0.05
    sphere5 = rc.sphere_volume((33, 17, 20), 0.05, (0.5, 0.45, 0.5), 0.3, seed=5)
    x12, T = rigid(50, 0.7, (0.3, -0.2, 0.5))
    out.append(_points_case("s33_n100003_rigid", sphere5, 0.05, points_for(x12, T, random_points((33, 17, 20), 0.05, 100003, 51)), xform=x12, min_weight=3,
                            pitch_extra=4))
    # a plane at vs = 0.05: the explicit identity and no transform on the same finite points
    plane = rc.plane_volume((33, 17, 20), 0.05, (0.2, 0.3, 1.0), 0.55, seed=6)
    pts = random_points((33, 17, 20), 0.05, 257, 61)
    out.append(_points_case("plane_n257_null", plane, 0.05, pts, pitch_extra=8))
    out.append(_points_case("plane_n257_identity", plane, 0.05, pts, xform=IDENTITY12, pitch_extra=8))
    # the linear field
    lin, _ = linear_volume(LINEAR_SHAPE, VS2, LINEAR_A, LINEAR_B)
    out.append(_points_case("linear", lin, VS2, np.concatenate([structured_points(lin, LINEAR_SHAPE, VS2, 1, 17), random_points(LINEAR_SHAPE, VS2, 400, 71, margin=-0.5)])))
    # n = 1, 63, 64, 65: the ragged last wave, under a transform
    v345 = random_volume((3, 4, 5), 8, low_weight=1)
    x12, T = rigid(80, -0.4, (0.05, 0.1, -0.03))
    for n in (1, 63, 64, 65):
        out.append(_points_case("v345_n%d" % n, v345, VS2, points_for(x12, T, random_points((3, 4, 5), VS2, n, 80 + n, margin=0.3)), xform=x12, pitch_extra=4))
    # depth images in pitched buffers: the six entries at the limits, then 17 x 9 with pixels whose points leave the volume
    ctr = np.array((33, 17, 20)) * float(VS2) / 2
    pos = ctr + np.array([0.05, -0.03, -0.5])
    R = rc.look_at(pos, ctr + np.array([0.1, 0.05, 0.0]))
    out.append(_depth_case("depth_2x3", sphere, VS2, np.array([[0, 199, 200], [5000, 5001, 65535]]), rc.intrinsics(2, 3, zoom=3.0), R, pos, grad=grad, pitch_extra=12,
                           offset=8, depth_pitch_extra=6))
    rng = np.random.default_rng(90)
    depth = rng.integers(300, 2400, size=(9, 17))
    depth.reshape(-1)[rng.choice(9 * 17, 12, replace=False)] = [0, 199, 200, 5000, 5001, 65535, 201, 4999, 1000, 1, 65534, 2500]
    out.append(_depth_case("depth_17x9", sphere, VS2, depth, rc.intrinsics(9, 17, zoom=0.9), R, pos, grad=grad, pitch_extra=12, offset=8, depth_pitch_extra=2))
    out.append(_depth_case("depth_17x9_mw3", sphere, VS2, depth, rc.intrinsics(9, 17, zoom=0.9), R, pos, min_weight=3, pitch_extra=4, depth_pitch_extra=10))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def big_case():
    """The (65, 33, 64) volume the GPU test lays out in rows of 1 MiB, so that row offsets pass 2^31 bytes (from row 2048 on: plane 62, y >= 2): the centres of the last
    plane, and random points between the last two planes, every one of which reads rows of the last plane."""
    vol = rc.sphere_volume(rc.BIG_SHAPE, float(VS2), (0.5, 0.5, 0.8), 0.25, seed=6)
    X, Y, Z = rc.BIG_SHAPE
    y, x = np.meshgrid(np.arange(Y), np.arange(X), indexing="ij")
    cen = np.concatenate([np.stack([x.ravel(), y.ravel(), np.full(x.size, z)], axis=1) for z in (Z - 1,)])
    rng = np.random.default_rng(7)
    g = np.stack([rng.uniform(0, X - 1, 3000), rng.uniform(0, Y - 1, 3000), rng.uniform(Z - 1.9, Z - 1, 3000)], axis=1)
    pts = np.concatenate([lattice_points(rc.BIG_SHAPE, VS2, cen), ((g + 0.5) * float(VS2)).astype(np.float32)])
    return _points_case("big_rows", vol, VS2, pts)


def wrap_case():
    """For the model alone: the (3, 4, 5) volume behind a synthetic address map with rows of 2^28 bytes, whose rows 16 .. 19 lie past 2^32 bytes."""
    c = dict(next(c for c in cases() if c["name"] == "v345"))
    c.update(name="v345_pitch_2_28", pitch=1 << 28)
    return c


def run_model(case, dtype=np.float32, mutant=None):
    if case["kind"] == "points":
        return sample_points(case["vol"], case["vs"], case["pts"], case["xform"], case["min_weight"], case["grad"], dtype, mutant, case["pitch"])
    return sample_depth(case["vol"], case["vs"], case["depth"], case["intr"], case["R"], case["t"], case["min_weight"], case["grad"], dtype, mutant, case["pitch"])


@functools.lru_cache(maxsize=None)
def expected(name, f64=False):
    """The model's result for a case, computed once and shared: never modified."""
    case = {c["name"]: c for c in cases() + (big_case(),)}[name]
    out = run_model(case, np.float64 if f64 else np.float32)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def same_output(a, b):
    """Equal bits (the NaNs included)."""
    return rc.same_output("", a, b)
