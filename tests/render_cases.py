"""Cases and models for xs_render_views / xs_render_mask_build (x-slam_amd/csrc/xs_render.hip), shared by
tests/test_render_cases_cpu.py, tests/test_render_gpu.py and tests/test_render_pipeline_gpu.py.

render() is the contract of include/xslam_amd.h written out in numpy, one array operation per IEEE operation of the contract, in the contract's
order.  It is written from the header, not from the kernel: where the kernel is organised differently (it keeps the previous sample in
registers, defers reads with the cull, refines after the loop) the model simply evaluates every sample.  With dtype=np.float32 every
operation is one correctly rounded float32 operation (numpy does not contract), so the GPU tests ask for equal bits.  With dtype=np.float64 the
same text is the float64 twin (the inputs are the float32 inputs, converted exactly; the sample count is the float32 count: it is an input).

The bound between the two (depth_bound, normal_bound) is derived below operation by operation, u = 2^-24:
  dx, dy             two roundings each.  d[c] = (R0 dx + R1 dy) + R2: each product carries 3u relative, each sum one more u:
                     |err d[c]| <= 5u A,  A = max (|R0 dx| + |R1 dy| + |R2|).
  t_k                one product, one sum:  |err t| <= 2u tmax,  tmax = max(|t_near|, |t_far|).
  p[c] = tc + t d    |err p| <= tmax 5u A + 2u tmax Dm + u tmax Dm + u L =: Ep,  Dm = max |d[c]|,  L = max |tc[c]| + tmax Dm >= |p[c]|.
  g = p / vs - 0.5   |err g| <= Ep / vs + u L / vs + u (L / vs + 0.5) =: Eg   (in voxels)
  F                  the trilinear value is continuous across cells and its slope along an axis is a blend of differences of neighbouring
                     voxels, at most Delta = max |v - v'| over face neighbours; g - floor(g) is exact, 1 - f rounds once, a stage
                     lo (1 - f) + hi f rounds three more times, three stages: 12u vmax (merge_cases.MODEL_BOUND_U), so
                     |err F| <= 3 Delta Eg + 12u vmax =: EF.
  ts = ta - step (F0 / (F1 - F0))   with F0 >= 0 >= F1 the quotient r has |r| <= 1 and |den| = F0 + |F1|:
                     |err den| <= 2 EF + u |den|,  |err r| <= (EF + |err den|) / (|den| - 2 EF) + u  <=  3 EF / (|den| - 2 EF) + 2u,
                     |err ts| <= 2u tmax + step (|err r| + u) + u tmax  =  3u tmax + step (3 EF / (|den| - 2 EF) + 3u) =: Ets   (per pixel: den varies)
  Q = tc + ts d      |err Q| <= Ets Dm + Ep;  Q +- h rounds once more (u L);  the index: Eg' = (Ets Dm + Ep + u L) / vs + u L / vs + u (L / vs + 0.5),
                     EF' = 3 Delta Eg' + 12u vmax,  |err G[c]| <= 2 EF' + 2u vmax,  as a vector sqrt(3) times that =: EG.
  N = G / |G|        |a / |a| - b / |b|| <= 2 |a - b| / |b|, and the sum of squares, the root and the divide round 4 times:
                     |err N[c]| <= 2 EG / (|G| - EG) + 4u.
Both bounds are infinite where their denominator is not positive (an ill-conditioned crossing says nothing).  ALLOW covers the second-order terms."""
import functools
import math

import numpy as np

U = 2.0 ** -24
ALLOW = 1.01
NAN_BITS = 0x7FFFFFFF
HIT, BACKFACE, REJECTED, NONE, _REFINE = 0, 1, 2, 3, 4
MAX_SAMPLES, MAX_VIEWS = 4096, 64
F32 = np.float32


# ------------------------------------------------------------------------------------------------
# The models
def samples(t_near, t_far, step):
    """The number of k with t_near + float(k) * step < t_far in float32, counted to MAX_SAMPLES + 1 (host/render_host.hpp: render_samples)."""
    t_near, t_far, step = F32(t_near), F32(t_far), F32(step)
    n = 0
    while n <= MAX_SAMPLES and t_near + F32(n) * step < t_far:
        n += 1
    return n


def defaults(vs, t_near=0.0, t_far=0.0, step=0.0, min_weight=1):
    """The options with the contract's defaults applied."""
    t_near, t_far, step = F32(t_near), F32(t_far), F32(step)
    if t_near == 0 and t_far == 0:
        t_near, t_far = F32(0.2), F32(5.0)
    return t_near, t_far, (F32(vs) if step == 0 else step), max(1, int(min_weight))


def mask_dims(res):
    BX, BY, BZ = (-(-int(r) // 8) for r in res)
    return BX, BY, BZ, -(-BX // 32)


def brick_bits(vol, min_weight):
    """bool [BZ, BY, BX]: the brick holds a voxel with value < 0 and weight >= min_weight."""
    value, weight = vol
    Z, Y, X = value.shape
    BX, BY, BZ, _ = mask_dims((X, Y, Z))
    neg = np.zeros((BZ * 8, BY * 8, BX * 8), bool)
    neg[:Z, :Y, :X] = (value < 0) & (weight >= max(1, min_weight))
    return neg.reshape(BZ, 8, BY, 8, BX, 8).any(axis=(1, 3, 5))


def mask_words(vol, min_weight):
    """The brick mask as xs_render_mask_build leaves it: uint32 [BZ * BY * WX], bit bx & 31 of word (bz BY + by) WX + (bx >> 5)."""
    bits = brick_bits(vol, min_weight)
    BZ, BY, BX = bits.shape
    WX = -(-BX // 32)
    padded = np.zeros((BZ, BY, WX * 32), np.uint64)
    padded[:, :, :BX] = bits
    words = (padded.reshape(BZ, BY, WX, 32) << np.arange(32, dtype=np.uint64)).sum(axis=3)
    return words.astype(np.uint32).reshape(-1)


def workspace_bytes(res):
    BX, BY, BZ, WX = mask_dims(res)
    return 256 + MAX_VIEWS * 12 * 4 + -(-(WX * BY * BZ * 4) // 256) * 256


def _trilinear(val, weight, vs, min_weight, p, T):
    """F(P) of the contract at the points p = [p0, p1, p2] (arrays): (ok, value)."""
    Z, Y, X = val.shape
    S = (X, Y, Z)
    with np.errstate(invalid="ignore", over="ignore"):
        g = [p[c] / vs - T(0.5) for c in range(3)]
        inb = np.ones(g[0].shape, bool)
        for c in range(3):
            inb &= (g[c] >= 0) & (g[c] <= T(S[c] - 1))
        b, f, need = [], [], []
        for c in range(3):
            gc = np.where(inb, g[c], T(0))
            bc = np.floor(gc)
            f.append(gc - bc)
            b.append(bc.astype(np.int64))
            need.append(f[c] > 0)
    ws = np.full(g[0].shape, 0x7FFFFFFF, np.int64)
    v = [None] * 8
    for d in range(8):
        used = np.ones(g[0].shape, bool)
        idx = []
        for c in range(3):
            bit = d >> c & 1
            if bit:
                used &= need[c]
            idx.append(np.minimum(b[c] + bit, S[c] - 1))   # (an unused corner may lie outside: it is not read)
        ws = np.where(used, np.minimum(ws, weight[idx[2], idx[1], idx[0]]), ws)
        v[d] = np.where(used, val[idx[2], idx[1], idx[0]], T(0))
    ok = inb & (ws >= min_weight)
    for k in range(3):
        stride = 1 << k
        fk = f[k]
        gk = T(1) - fk
        for d in range(0, 8, 2 * stride):
            v[d] = np.where(need[k], v[d] * gk + v[d + stride] * fk, v[d])
    return ok, v[0]


def render(vol, vs, R, t, intr, rows, cols, t_near=0.0, t_far=0.0, step=0.0, min_weight=1, cull=False, dtype=np.float32):
    """The contract of xs_render_views.  vol = (value [Z, Y, X] float32, weight [Z, Y, X] int32), R [P, 3, 3], t [P, 3], intr (fx, fy, cx, cy).
    Returns a dict: depth [P, rows, cols], depth_u16, normal [P, 3, rows, cols] (float32: NaN bits NAN_BITS), shade uint8, counts uint32 [P, 4],
    and for the tests cls, kh (the crossing step), den (F1 - F0) and gnorm (|G|) per pixel."""
    T = dtype
    value, weight = vol
    Z, Y, X = value.shape
    val = value.astype(T)
    t_near, t_far, step, mw = defaults(vs, t_near, t_far, step, min_weight)
    n = samples(t_near, t_far, step)
    assert n <= MAX_SAMPLES
    vs, t_near, step = T(F32(vs)), T(t_near), T(step)
    fx, fy, cx, cy = (T(F32(a)) for a in intr)
    R = np.asarray(R, np.float32).reshape(-1, 3, 3).astype(T)
    tc = np.asarray(t, np.float32).reshape(-1, 3).astype(T)
    P = R.shape[0]
    shape = (P, rows, cols)
    dx = ((np.arange(cols, dtype=T) - cx) / fx)[None, None, :]
    dy = ((np.arange(rows, dtype=T) - cy) / fy)[None, :, None]
    d = [np.ascontiguousarray(np.broadcast_to((R[:, c, 0, None, None] * dx + R[:, c, 1, None, None] * dy) + R[:, c, 2, None, None], shape)) for c in range(3)]
    t3 = [tc[:, c, None, None] for c in range(3)]
    bricks = brick_bits(vol, mw) if cull else None
    S = (X, Y, Z)

    def point(tt):
        return [t3[c] + tt * d[c] for c in range(3)]

    cls = np.full(shape, NONE, np.int32)
    kh = np.zeros(shape, np.int64)
    alive = np.ones(shape, bool)
    pk = np.zeros(shape, np.int8)          # 0 NONE, 1 a value, 2 deferred by the cull
    pv = np.zeros(shape, T)
    ptk, ptv = pk.copy(), pv.copy()        # what reading the previous sample gives
    reads = 0
    for k in range(n):
        if not alive.any():
            break
        tk = t_near + T(k) * step
        p = point(tk)
        with np.errstate(invalid="ignore", over="ignore"):
            q = [p[c] / vs for c in range(3)]
            inside = np.ones(shape, bool)
            for c in range(3):
                inside &= (q[c] >= 0) & (q[c] < T(S[c]))
            ix = [np.where(inside, np.floor(np.where(inside, q[c], T(0))), 0).astype(np.int64) for c in range(3)]
        w = weight[ix[2], ix[1], ix[0]]
        tkind = (inside & (w >= mw)).astype(np.int8)
        tv = np.where(tkind == 1, val[ix[2], ix[1], ix[0]], T(0))
        if cull:
            deferred = inside & ~bricks[ix[2] >> 3, ix[1] >> 3, ix[0] >> 3]
            ck = np.where(deferred, np.int8(2), tkind)
            cv = np.where(deferred, T(0), tv)
            # a deferred sample is read when its neighbour turns out to be a negative value
            m = (ck == 1) & (cv < 0) & (pk == 2)
            pk, pv = np.where(m, ptk, pk), np.where(m, ptv, pv)
            m = (pk == 1) & (pv < 0) & (ck == 2)
            ck, cv = np.where(m, tkind, ck), np.where(m, tv, cv)
            reads += int((alive & inside & (ck != 2)).sum())
        else:
            ck, cv = tkind, tv
            reads += int((alive & inside).sum())
        both = alive & (pk == 1) & (ck == 1)
        back = both & (pv < 0) & (cv > 0)
        front = both & (pv > 0) & (cv < 0)
        cls[back] = BACKFACE
        cls[front] = _REFINE
        kh[front] = k - 1
        alive &= ~(back | front)
        pk, pv, ptk, ptv = ck, cv, tkind, tv

    sel = cls == _REFINE
    ta, tb = t_near + kh.astype(T) * step, t_near + (kh + 1).astype(T) * step
    ok0, F0 = _trilinear(val, weight, vs, mw, point(ta), T)
    ok1, F1 = _trilinear(val, weight, vs, mw, point(tb), T)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        den = F1 - F0
        hit = sel & ok0 & ok1 & (F0 >= 0) & (F1 <= 0) & ~(den == 0)
        ts = np.where(hit, ta - step * (F0 / den), T(0))
    cls[sel & ~hit] = REJECTED
    cls[hit] = HIT

    Q = point(ts)
    h = T(0.5) * vs
    G, allok = [], hit.copy()
    for c in range(3):
        okp, Fp = _trilinear(val, weight, vs, mw, [Q[a] + h if a == c else Q[a] for a in range(3)], T)
        okm, Fm = _trilinear(val, weight, vs, mw, [Q[a] - h if a == c else Q[a] for a in range(3)], T)
        allok &= okp & okm
        G.append(Fp - Fm)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        gg = (G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]
        have = allok & (gg > 0)
        length = np.sqrt(gg)
        N = [np.where(have, G[c] / length, T(0)) for c in range(3)]
        nd = (N[0] * d[0] + N[1] * d[1]) + N[2] * d[2]
        dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        shade = np.where(have, np.rint(T(255) * np.minimum(T(1), np.abs(nd) / np.sqrt(dd))), T(0)).astype(np.uint8)
        r = np.rint(ts * T(1000))
        d16 = np.where(hit & (r >= 1) & (r <= 65535), r, T(0)).astype(np.uint16)
    normal = np.stack(N, axis=1)
    if T is np.float32:
        normal.view(np.uint32)[np.broadcast_to(~have[:, None], normal.shape)] = NAN_BITS
    else:
        normal[np.broadcast_to(~have[:, None], normal.shape)] = np.nan
    counts = np.stack([(cls == c).sum(axis=(1, 2)) for c in (HIT, BACKFACE, REJECTED, NONE)], axis=1).astype(np.uint32)
    return dict(depth=ts, depth_u16=d16, normal=normal, shade=shade, counts=counts, cls=cls, kh=kh, den=np.where(hit, den, T(0)), gnorm=np.where(have, length, T(0)),
                have=have, reads=reads, d=d)


def bounds(case, m64):
    """(depth bound, normal bound) per pixel between the float32 model and the float64 twin m64 of `case`: the derivation at the top."""
    value = case["vol"][0].astype(np.float64)
    vs = float(case["vs"])
    t_near, t_far, step, _ = defaults(vs, case["t_near"], case["t_far"], case["step"], case["min_weight"])
    tmax, step = max(abs(float(t_near)), abs(float(t_far))), float(step)
    R = np.abs(case["R"].astype(np.float64))
    intr = [float(a) for a in case["intr"]]
    dxm = max(abs((0 - intr[2]) / intr[0]), abs((case["cols"] - 1 - intr[2]) / intr[0]))
    dym = max(abs((0 - intr[3]) / intr[1]), abs((case["rows"] - 1 - intr[3]) / intr[1]))
    A = float((R[:, :, 0] * dxm + R[:, :, 1] * dym + R[:, :, 2]).max())
    Dm = max(float(np.abs(a).max()) for a in m64["d"])
    L = float(np.abs(case["t"]).max()) + tmax * Dm
    vmax = float(np.abs(value).max())
    Delta = max(float(np.abs(np.diff(value, axis=a)).max()) if value.shape[a] > 1 else 0.0 for a in range(3))
    Ep = tmax * 5 * U * A + 3 * U * tmax * Dm + U * L
    Eg = Ep / vs + U * L / vs + U * (L / vs + 0.5)
    EF = 3 * Delta * Eg + 12 * U * vmax
    den = np.abs(m64["den"]) - 2 * EF
    with np.errstate(divide="ignore", invalid="ignore"):
        Ets = np.where(den > 0, 3 * U * tmax + step * (3 * EF / den + 3 * U), np.inf)
        Eg2 = (Ets * Dm + Ep + U * L) / vs + U * L / vs + U * (L / vs + 0.5)
        EG = math.sqrt(3.0) * (2 * (3 * Delta * Eg2 + 12 * U * vmax) + 2 * U * vmax)
        gn = m64["gnorm"] - EG
        En = np.where(gn > 0, 2 * EG / gn + 4 * U, np.inf)
    return ALLOW * Ets, ALLOW * En


# ------------------------------------------------------------------------------------------------
# Volumes
def centres(shape, vs):
    X, Y, Z = shape
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return [(a + 0.5) * vs for a in (x, y, z)]


def tsdf_of(dist, trunc):
    return np.clip(dist / trunc, -1.0, 1.0).astype(np.float32)


def weights_of(rng, value, dist, trunc, shell=True):
    """Weights 3 .. 5, one voxel in thirty 1 or 2 (so that min_weight 3 sees less than min_weight 1), 0 in a shell deep behind the surface, as
    fusion leaves it."""
    w = np.where(rng.random(value.shape) < 1 / 30, rng.integers(1, 3, size=value.shape), rng.integers(3, 6, size=value.shape)).astype(np.int32)
    if shell:
        w[dist < -0.95 * trunc] = 0
    return w


def plane_volume(shape, vs, normal, offset, trunc_vox=4.0, seed=0, holes=True, zeros=False):
    """dist = n . c - offset: free space where it is positive."""
    rng = np.random.default_rng(seed)
    c = centres(shape, vs)
    nrm = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    dist = nrm[0] * c[0] + nrm[1] * c[1] + nrm[2] * c[2] - offset
    trunc = trunc_vox * vs
    value = tsdf_of(dist, trunc)
    weight = weights_of(rng, value, dist, trunc)
    if holes and min(shape) > 4:
        centre = [rng.uniform(0.3, 0.7) * s * vs for s in shape]
        weight[sum((c[a] - centre[a]) ** 2 for a in range(3)) < (0.12 * max(shape) * vs) ** 2] = 0
    if zeros:
        near = np.argwhere(np.abs(dist) < 0.6 * vs)
        for i, (z, y, x) in enumerate(near[::3]):
            value[z, y, x] = np.float32(0.0) if i % 2 == 0 else np.float32(-0.0)
    return value, weight


def sphere_volume(shape, vs, centre_frac, radius_frac, trunc_vox=4.0, seed=0, holes=True):
    rng = np.random.default_rng(seed)
    c = centres(shape, vs)
    centre = [centre_frac[a] * shape[a] * vs for a in range(3)]
    dist = np.sqrt(sum((c[a] - centre[a]) ** 2 for a in range(3))) - radius_frac * min(shape) * vs
    trunc = trunc_vox * vs
    value = tsdf_of(dist, trunc)
    weight = weights_of(rng, value, dist, trunc)
    if holes:
        hole = [centre[0] + radius_frac * min(shape) * vs * 0.7, centre[1], centre[2] - radius_frac * min(shape) * vs * 0.7]
        weight[sum((c[a] - hole[a]) ** 2 for a in range(3)) < (0.12 * min(shape) * vs) ** 2] = 0
    return value, weight


# ------------------------------------------------------------------------------------------------
# Views
def look_at(pos, target, down=(0.0, 1.0, 0.0)):
    """Camera-to-volume rotation (columns: the camera's x, y, z axes in the volume frame) looking from pos at target, float64."""
    z = np.asarray(target, np.float64) - np.asarray(pos, np.float64)
    z /= np.linalg.norm(z)
    dn = np.asarray(down, np.float64)
    if abs(dn @ z) > 0.95:
        dn = np.array([1.0, 0.0, 0.0])
    x = np.cross(dn, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z], axis=1)


def views_around(shape, vs, count, seed, distance=1.6, inside=True, away=True):
    """`count` views of the volume: from outside at `distance` extents from its centre in Halton-like directions, then (if asked and there is
    room) one from inside it and one outside looking away from it."""
    rng = np.random.default_rng(seed)
    ext = np.array(shape, np.float64) * vs
    ctr = ext / 2
    R, t = [], []
    for i in range(count):
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        kind = "outside"
        if inside and count >= 3 and i == 1:
            kind = "inside"
        if away and count >= 3 and i == 2:
            kind = "away"
        if kind == "inside":
            pos = ctr + 0.42 * ext * np.sign(v)                  # inside the volume, near a corner, looking across it
            tgt = ctr
        elif kind == "away":
            pos = ctr + distance * np.linalg.norm(ext) / 2 * v
            tgt = pos + v
        else:
            pos = ctr + distance * np.linalg.norm(ext) / 2 * v
            tgt = ctr + 0.15 * ext * rng.uniform(-1, 1, 3)
        R.append(look_at(pos, tgt))
        t.append(pos)
    return np.array(R, np.float32), np.array(t, np.float32)


def intrinsics(rows, cols, zoom=1.3):
    f = zoom * max(rows, cols, 4)
    return np.array([f, -1.1 * f, (cols - 1) / 2 + 0.25, (rows - 1) / 2 - 0.25], np.float32)   # (fy < 0, as the ICL configuration has it)


# ------------------------------------------------------------------------------------------------
# The cases
def _case(name, vol, vs, R, t, rows, cols, step_vox, min_weight, t_near=None, t_far=None, pitch_extra=0, offset=0, zoom=1.3):
    shape = vol[0].shape[::-1]
    ext = float(np.linalg.norm(np.array(shape) * vs))
    reach = float(max(np.linalg.norm(np.asarray(t, np.float64) - np.array(shape) * vs / 2, axis=1))) + ext
    for a in vol:
        a.setflags(write=False)
    return dict(name=name, vol=vol, vs=F32(vs), shape=shape, R=np.asarray(R, np.float32), t=np.asarray(t, np.float32), intr=intrinsics(rows, cols, zoom), rows=rows, cols=cols,
                step=F32(step_vox * vs), min_weight=min_weight, t_near=F32(0.25 * vs if t_near is None else t_near), t_far=F32(reach if t_far is None else t_far),
                pitch=shape[0] * 4 + pitch_extra, offset=offset)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    vs = 0.05
    # 2 x 2 x 2: one trilinear cell; mostly rejected or none
    vol = plane_volume((2, 2, 2), vs, (0.2, 0.3, 1.0), 0.05, trunc_vox=2.0, seed=1, holes=False)
    vol[1][...] = 2
    R, t = views_around((2, 2, 2), vs, 2, 11, distance=2.5)
    out.append(_case("cube2_1x1", vol, vs, R[:1], t[:1], 1, 1, 0.5, 1))
    out.append(_case("cube2_17x9", vol, vs, R, t, 9, 17, 0.5, 1, pitch_extra=4))
    # 3 x 4 x 5: a sphere cut by every face
    vol = sphere_volume((3, 4, 5), vs, (0.5, 0.5, 0.5), 0.35, trunc_vox=2.0, seed=2, holes=False)
    R, t = views_around((3, 4, 5), vs, 3, 12, distance=2.0)
    out.append(_case("s345_2x3", vol, vs, R, t, 2, 3, 1.0, 1, pitch_extra=8))
    out.append(_case("s345_17x9_half", vol, vs, R, t, 9, 17, 0.5, 3, offset=4))
    # 9 x 5 x 6: a plane with zeros of both signs on the surface, seen from both sides (the second view from behind)
    vol = plane_volume((9, 5, 6), vs, (0.3, -0.2, 1.0), 0.14, trunc_vox=3.0, seed=3, holes=False, zeros=True)
    ctr = np.array((9, 5, 6)) * vs / 2
    front, behind = ctr + np.array([0.1, -0.05, 0.6]), ctr + np.array([-0.05, 0.1, -0.6])
    R = np.array([look_at(front, ctr), look_at(behind, ctr)], np.float32)
    t = np.array([front, behind], np.float32)
    out.append(_case("plane956_17x9", vol, vs, R, t, 9, 17, 1.0, 1, pitch_extra=4))
    out.append(_case("plane956_big_step", vol, vs, R, t, 9, 17, 2.5, 1))
    # 33 x 17 x 20 with a pitch that is no multiple of 16: a sphere with a shell and a hole, outside, inside and away; both min_weights
    vol = sphere_volume((33, 17, 20), vs, (0.45, 0.5, 0.55), 0.3, seed=4)
    R, t = views_around((33, 17, 20), vs, 3, 14)
    out.append(_case("s33_80x60", vol, vs, R, t, 60, 80, 1.0, 1, pitch_extra=4 * 3, zoom=2.2))
    out.append(_case("s33_80x60_mw3", vol, vs, R, t, 60, 80, 1.0, 3, pitch_extra=4 * 3, zoom=2.2))
    out.append(_case("s33_17x9_half", vol, vs, R, t, 9, 17, 0.5, 1, pitch_extra=4 * 5, offset=8))
    R, t = views_around((33, 17, 20), vs, 64, 15, inside=False, away=False)
    out.append(_case("s33_64views", vol, vs, R, t, 9, 17, 1.0, 1, pitch_extra=4, zoom=2.0))
    # a slab of matter seen from behind: the first crossing is from inside to outside
    vol = plane_volume((33, 17, 20), vs, (0.1, 0.2, 1.0), 0.45, trunc_vox=4.0, seed=5, holes=True)
    vol[1][vol[1] == 0] = 1                                        # (the shell behind the surface is weighted here: the camera stands in it)
    ctr = np.array((33, 17, 20)) * vs / 2
    behind = ctr + np.array([0.1, 0.05, -0.45])
    R = np.array([look_at(behind, ctr + np.array([0.0, 0.0, 0.3]))], np.float32)
    out.append(_case("slab_behind", vol, vs, R, np.array([behind], np.float32), 9, 17, 1.0, 1, pitch_extra=4))
    return tuple(out)


def analytic_plane():
    """A plane whose truncation band holds a whole march step and a trilinear cell around every crossing: (case, normal, offset).  Every
    weight is 2: nothing is refused."""
    vs, shape = 0.05, (33, 17, 20)
    normal, offset = np.array([0.15, -0.1, 1.0]) / np.linalg.norm([0.15, -0.1, 1.0]), 0.4
    c = centres(shape, vs)
    dist = normal[0] * c[0] + normal[1] * c[1] + normal[2] * c[2] - offset
    trunc = 20 * vs
    assert np.abs(dist / trunc).max() < 1      # the whole volume lies inside the band: the stored field is linear up to its float32 rounding
    value = (dist / trunc).astype(np.float32)
    weight = np.full(value.shape, 2, np.int32)
    ctr = np.array(shape) * vs / 2
    pos = ctr + np.array([0.05, -0.1, 0.8])
    R = np.array([look_at(pos, ctr)], np.float32)
    case = _case("analytic_plane", (value, weight), vs, R, np.array([pos], np.float32), 9, 17, 1.0, 1)
    return case, normal, offset, trunc


BIG_SHAPE, BIG_PITCH = (65, 33, 64), 1 << 20


@functools.lru_cache(maxsize=None)
def big_case():
    """The (65, 33, 64) volume the GPU test lays out in rows of 1 MiB, so that row offsets pass 2^31 bytes; the camera stands beyond the last
    planes and looks at them."""
    vs = 0.05
    vol = sphere_volume(BIG_SHAPE, vs, (0.5, 0.5, 0.8), 0.25, seed=6)
    ctr = np.array(BIG_SHAPE) * vs * np.array([0.5, 0.5, 0.8])
    pos = ctr + np.array([0.2, -0.1, 2.0])
    R = np.array([look_at(pos, ctr)], np.float32)
    return _case("big_rows", vol, vs, R, np.array([pos], np.float32), 60, 80, 1.0, 1, zoom=2.2)


@functools.lru_cache(maxsize=None)
def expected(name, cull=False, f64=False):
    """The model's result for a case, computed once and shared: never modified."""
    case = {c["name"]: c for c in cases() + (big_case(),)}[name]
    out = render(case["vol"], case["vs"], case["R"], case["t"], case["intr"], case["rows"], case["cols"], case["t_near"], case["t_far"], case["step"],
                 case["min_weight"], cull=cull, dtype=np.float64 if f64 else np.float32)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


OUTPUTS = ("depth", "depth_u16", "normal", "shade", "counts")


def same_output(name, a, b):
    """Equal bits (the normal's NaNs included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        return a.shape == b.shape and b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)
