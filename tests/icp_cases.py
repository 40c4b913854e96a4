"""The cases that hold the ICP reduction (k_icp and its launchers, x-slam_amd/csrc/xs_icp.hip; oracle/oc_kernels.hpp: icp_combined)
against the float64 model of tests/independent_f64.py, on the smallest images that reach each kernel instance and each of its edges,
in pitched buffers with guard rows.  The four maps are built here in numpy and rounded once to float32, so no other kernel is
involved.  Backend-neutral: tests/test_icp_windows_cpu.py runs the cases on the CPU oracle, tests/test_icp_windows_gpu.py on the HIP
kernels.  Test infrastructure."""
import functools

import numpy as np

import independent_f64 as ind
import map_cases as mc
from independent_cases import FD, Hs

DIST = 0.10
ANGLE = float(np.sin(np.float32(15.0) / np.float32(180.0) * np.pi))
U = ind.U32

# rows, cols, tiles = ceil(cols / 64) * rows, records (= workgroups), row groups G of the last workgroup's gather, what the case holds
GEOMETRIES = [
    (2, 3, 2, 1, 18, "<8,1>: six idle waves, three lanes"),
    (1, 640, 10, 2, 18, "<8,1>: one row"),
    (480, 1, 480, 60, 18, "<8,1>: one lane per tile"),
    (37, 70, 74, 10, 18, "<8,1>: six-lane tail tile, half-empty last workgroup"),
    (13, 131, 39, 5, 18, "<8,1>: three-lane tail tile"),
    (1024, 70, 2048, 256, 18, "<8,1>: last one-pass launch"),
    (683, 130, 2049, 257, 18, "<8,2>: first two-pass launch, the last workgroup holds one tile"),
    (1024, 200, 4096, 512, 18, "<8,2>: last two-pass launch"),
    (241, 1030, 4097, 256, 36, "<16,2,BAL>: base 16, rem 1 - exactly one second tile in the launch"),
    (1500, 130, 4500, 256, 36, "<16,2,BAL>: base 17, rem 148"),
    (256, 1220, 5120, 256, 36, "<16,2,BAL>: 20 tiles everywhere - every second-tile slot used"),
    (1707, 130, 5121, 641, 18, "<8,3>: first three-pass launch"),
    (1024, 330, 6144, 768, 18, "<8,3>: XS_ICP_MAX_BLOCKS"),
    (1229, 260, 6145, 512, 9, "<4,2>: first striding launch"),
]
SHAPES = [(g[0], g[1]) for g in GEOMETRIES]
ALL_PITCHES = SHAPES[:5]           # tight, the host's and tight plus one element; the larger images run at the host's pitch
# three ranges that tile the image, y0 > 0 in two; of 1500 x 130, rows [0, 1400) are 4 200 tiles — a balanced launch — the others are not
# (the camera motion empties the first five rows of 37 x 70 and the first two of 13 x 131: the first range reaches past them)
RANGES = {(37, 70): [(0, 12), (12, 25), (25, 37)], (13, 131): [(0, 4), (4, 12), (12, 13)], (1500, 130): [(0, 1400), (1400, 1450), (1450, 1500)]}
EMPTY_SHAPE, EMPTY_RANGES = (37, 70), [(0, 0), (17, 17), (37, 37)]
POSTED_SHAPES = [(37, 70), (1707, 130)]
# current pixels made inliers on purpose besides (0, y0): the only second tile of 241 x 1030 (workgroup 0's seventeenth tile) is the six
# columns past 1024 of row 0, which the camera motion would otherwise carry out of the model image
EXTRA_INLIERS = {(241, 1030): [(0, x) for x in range(1024, 1030)]}
BRANCHES = ("nan_normal", "hole", "left", "right", "top", "bottom", "behind", "far", "tilted")
PUNCH_CAP = 0.05                   # fragile pixels punched out, as a share of the current pixels with a valid normal (a condition on the inputs)

# Tolerance of a sum of row_i * row_j, in units of 2^-24 * sum_p m_i(p) m_j(p) (ind.icp_normal_equations: m, dm).  Derived, not tuned:
# the rounded float32 operations on the longest path to a product.  A row entry is at most the pose transform (ICP_OPS_TRANSFORM = 5)
# followed by the dot product n . (d - s) (ICP_OPS_DOT = 5; the cross product is 3), i.e. within 10 * 2^-24 of m_i; a product of two
# such entries carries both factors' errors and its own two roundings: 10 + 10 + 2.  The conversion to double is exact and the double
# accumulation adds 2^-53 per addition: nothing at this scale.  The imaginary parts go through the same operations on operands that
# are first-order parts, so got / h lies within the same count times 2^-24 * sum_p (m_i dm_j + dm_i m_j) of the derivative; the rows
# are polynomials of degree <= 3 in the seeds with tangents of the size of the values, so the truncation error of the model's central
# difference (FD^2 / 6 times a third derivative, 2e-11 relative) is far below that, and so is its float64 round-off (1e-16 / FD).
# Worst ratio of error to bound over all cases and ranges, CPU oracle (complex<float>, the reference's operation order): real parts
# 0.040, imaginary parts 0.054, both on the two inliers of 2 x 3; from 1 x 640 up, where the errors of hundreds of pixels average out,
# below 0.02 and 0.012 (per case: test_icp_windows_cpu.py prints them with -s; the HIP kernels': profiles/icp_windows_f64.json).
C_ICP = 2 * (ind.ICP_OPS_TRANSFORM + ind.ICP_OPS_DOT) + ind.ICP_OPS_PRODUCT


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _surface(a, b):
    """Depth z over the previous camera's normalised image coordinates (a plane and three low sinusoids: 1.1 .. 2.9 m over the widest
    image here) and its two partial derivatives."""
    z = 2.0 + 0.25 * a - 0.2 * b + 0.08 * np.sin(3 * a + 0.5) + 0.06 * np.cos(2.5 * b - 0.3) + 0.04 * np.sin(2 * a + 3 * b)
    za = 0.25 + 0.24 * np.cos(3 * a + 0.5) + 0.08 * np.cos(2 * a + 3 * b)
    zb = -0.2 - 0.15 * np.sin(2.5 * b - 0.3) + 0.12 * np.cos(2 * a + 3 * b)
    return z, za, zb


def _gradient(p):
    """Gradient of g(p) = p_z - z(p_x / p_z, p_y / p_z), whose zero set is the surface, at points p [3, n] of the previous camera's frame."""
    a, b = p[0] / p[2], p[1] / p[2]
    z, za, zb = _surface(a, b)
    return p[2] - z, np.stack([-za / p[2], -zb / p[2], 1 + (za * a + zb * b) / p[2]])


def _at(a, b):
    """Surface point and unit normal (towards the camera) at normalised coordinates (a, b), previous camera's frame: [3, n] each."""
    z = _surface(a, b)[0]
    p = np.stack([z * a, z * b, z])
    g = _gradient(p)[1]
    return p, -g / np.linalg.norm(g, axis=0)


def _pack(re, im, rows, cols):
    """[3, rows * cols] real and imaginary planes -> [3 * rows, cols, 2] float32; a NaN in the x plane is the sentinel (NaN, 0)."""
    m = np.stack([re, im], -1).reshape(3 * rows, cols, 2).astype(np.float32)
    m[:rows, :, 1][np.isnan(m[:rows, :, 0])] = 0.0
    return m


def _inputs(rows, cols, protect_rows, extra=()):
    """The crafted maps of one geometry, before any pixel is punched: a dict of float32 arrays and poses."""
    rng = np.random.default_rng(1000 * rows + cols)
    intr = mc.intr_for(rows, cols)
    fx, fy, cx, cy = (float(v) for v in intr)
    N = rows * cols
    yy, xx = (g.reshape(-1).astype(np.float64) for g in np.mgrid[0:rows, 0:cols])
    # previous camera in the world; the current camera seen from the previous one (what the current maps are made with) and the pose
    # estimate the kernel is given, a little off.  The motion moves a pixel by 0.15 of the image's smaller side, 6 pixels at the most
    # (0.7 degrees and 1.2 cm; the estimate 0.85 degrees and 1.5 cm: within 2 degrees and 3 cm), so a one-row image keeps its inliers.
    Rp, tp = _rot([0.4, -0.8, 0.3], 0.2), np.array([0.3, -0.2, 0.1])
    ang = min(6.0, 0.15 * min(rows, cols)) / fx
    Dr, Dt = _rot([0.5, 0.6, 0.25], ang), ang * np.array([0.7, -0.5, 0.4])
    Er, Et = _rot([0.45, 0.65, 0.3], 1.25 * ang), 1.2 * ang * np.array([0.75, -0.45, 0.5])
    Rc, tc = Rp @ Er, Rp @ Et + tp
    # model maps: the surface at the previous camera's pixels, in the world
    P, n = _at((xx - cx) / fx, (yy - cy) / fy)
    pv, pn = Rp @ P + tp[:, None], Rp @ n
    # current maps: the current camera's rays cut with the surface (Newton along the ray), in the current camera's frame
    ray = np.stack([(xx - cx) / fx, (yy - cy) / fy, np.ones(N)])
    rp, t = Dr @ ray, np.full(N, 2.0)
    for _ in range(8):
        g, grad = _gradient(Dt[:, None] + t * rp)
        t = t - g / (grad * rp).sum(0)
    grad = _gradient(Dt[:, None] + t * rp)[1]
    cv, cn = t * ray, Dr.T @ (-grad / np.linalg.norm(grad, axis=0))
    # (displacements go along the previous camera's ray through the point, as the estimate sees it: the projection stays where it is)
    along = lambda v: Er.T @ ((Er @ v + Et[:, None]) / np.linalg.norm(Er @ v + Et[:, None], axis=0))
    cv = cv + along(cv) * 0.004 * np.sin(5 * ray[0] + 2 * ray[1] + 1.0)  # a few millimetres of residual everywhere

    def match(u, v, flip=False):
        """Current vertex and normal that the estimate maps onto the surface point of model coordinates (u, v) — behind the previous
        camera, with flip, where the projection is the same pixel and only cpz < 0 rejects."""
        p, nn = _at((u - cx) / fx, (v - cy) / fy)
        return Er.T @ ((-p if flip else p) - Et[:, None]), Er.T @ nn

    xn, yn = (xx + 0.5) / cols, (yy + 0.5) / rows
    block = lambda x0, x1, y0, y1: (xn >= x0) & (xn < x1) & (yn >= y0) & (yn < y1)
    prot = np.array(sorted({y * cols for y in protect_rows} | {y * cols + x for y, x in extra}), np.int64)
    pool = rng.permutation(np.setdiff1d(np.arange(N), prot))[:N // 2]    # at most half the pixels are crafted one by one
    k = min(16, max(1, N // 40))
    taken = [0]

    def take(count):
        out = pool[taken[0]:taken[0] + count]
        taken[0] += count
        return out

    # a region displaced by 0.25 m (distThres 0.1) and one tilted by 30 degrees (gate 15), a sprinkle of each
    far = block(0.55, 0.8, 0.3, 0.7)
    far[take(k)] = True
    cv[:, far] += 0.25 * along(cv[:, far])
    tilt = block(0.15, 0.4, 0.3, 0.7)
    tilt[take(k)] = True
    tang = np.cross(cn[:, tilt].T, np.array([0.0, 0.6, 0.8])).T
    cn[:, tilt] = np.cos(np.pi / 6) * cn[:, tilt] + np.sin(np.pi / 6) * tang / np.linalg.norm(tang, axis=0)
    # pixels that project 0.8 .. 2.3 pixels outside the image on each of the four sides, and a few behind the previous camera
    for side in range(4):
        i = take(k)
        off = 0.8 + 1.5 * rng.random(i.size)
        u = [-off, cols - 1 + off, xx[i] + 0.25, xx[i] + 0.25][side]
        v = [yy[i] + 0.25, yy[i] + 0.25, -off, rows - 1 + off][side]
        cv[:, i], cn[:, i] = match(np.clip(u, -3, cols + 2), np.clip(v, -3, rows + 2))
    i = take(k)
    cv[:, i], cn[:, i] = match(xx[i] + 0.2, yy[i] - 0.2, flip=True)
    # the pixels that idle lanes and rejected pixels read — current (0, y0) of every range, model (0, 0) — are valid and well matched
    cv[:, prot], cn[:, prot] = match(xx[prot] + 0.25, yy[prot] + 0.25)
    keep = np.union1d(prot, [0])
    # sentinels: current pixels with a NaN normal and the other five values left as they are (the pixel would be an inlier), a few
    # with a NaN vertex as well (what the map kernels write for a hole); model holes likewise
    cn[0, take(max(k, N // 33))] = np.nan
    i = take(max(1, k // 3))
    cn[0, i], cv[0, i] = np.nan, np.nan
    hole = block(0.42, 0.52, 0.75, 0.9)
    hole[rng.choice(N, max(1, N // 33) if N >= 12 else 1, replace=False)] = True
    hole[keep] = False
    pn[0, hole] = np.nan
    # first-order parts: random tangents times h, on every map and on the pose
    im = lambda shape: Hs * rng.uniform(-1.0, 1.0, shape)
    cplx = lambda a: np.stack([a, im(a.shape)], -1).astype(np.float32)
    out = dict(rows=rows, cols=cols, intr=intr, Rcurr=cplx(Rc), tcurr=cplx(tc), Rprev_inv=np.stack([Rp.T, np.zeros((3, 3))], -1).astype(np.float32),
               tprev=np.stack([tp, np.zeros(3)], -1).astype(np.float32),
               cv=_pack(cv, im(cv.shape), rows, cols), cn=_pack(cn, im(cn.shape), rows, cols),
               pv=_pack(pv, im(pv.shape), rows, cols), pn=_pack(pn, im(pn.shape), rows, cols), protected=prot)
    return out


def _model(c, y0, y1, dec=None, margins=False):
    args = (c["Rcurr"], c["tcurr"], c["cv"], c["cn"], c["Rprev_inv"], c["tprev"], c["intr"], c["pv"], c["pn"], DIST, ANGLE)
    s0, inl, dec = ind.icp_normal_equations(0.0, Hs, *args, dec=dec, y0=y0, y1=y1, margins=margins)
    sp = ind.icp_normal_equations(+FD, Hs, *args, dec=dec, y0=y0, y1=y1)[0]
    sm = ind.icp_normal_equations(-FD, Hs, *args, dec=dec, y0=y0, y1=y1)[0]
    B, dB = ind.icp_bounds(dec, c["cols"], y0, y1)
    return dict(s0=s0, ds=(sp - sm) / (2 * FD), inliers=inl, B=B, dB=dB), dec


@functools.lru_cache(maxsize=None)
def case(rows, cols):
    """The inputs of one geometry with their model, computed once and shared: never modified.  The model is evaluated once, every
    fragile pixel's current normal sentinel is set to NaN — which removes that pixel and nothing else — and the model is evaluated
    again: no fragile pixel is left, so the implementation's decisions are the model's, pixel for pixel."""
    ranges = RANGES.get((rows, cols), []) + (EMPTY_RANGES if (rows, cols) == EMPTY_SHAPE else [])
    c = _inputs(rows, cols, {0} | {min(y0, rows - 1) for y0, _ in ranges}, EXTRA_INLIERS.get((rows, cols), ()))
    args = (c["Rcurr"], c["tcurr"], c["cv"], c["cn"], c["Rprev_inv"], c["tprev"], c["intr"], c["pv"], c["pn"], DIST, ANGLE)
    dec = ind.icp_normal_equations(0.0, Hs, *args, margins=True)[2]
    valid = int((~np.isnan(c["cn"][:rows, :, 0])).sum())
    punched = dec["fragile"].reshape(rows, cols)
    c["cn"][:rows][punched] = (np.nan, 0.0)
    c["whole"], dec = _model(c, 0, rows, margins=True)
    c["ranges"] = {r: _model(c, *r, dec=dec)[0] for r in ranges}
    c["ranges"][(0, rows)] = c["whole"]
    c["dec"] = dec
    c["stats"] = dict(pixels=rows * cols, valid_normals=valid, punched=int(punched.sum()), punched_share=float(punched.sum() / max(valid, 1)),
                      fragile_left=int(dec["fragile"].sum()), inliers=c["whole"]["inliers"],
                      protected_inliers=int(dec["ok"][c["protected"]].sum()), protected=int(c["protected"].size),
                      model_00_valid=bool(not np.isnan(c["pn"][0, 0, 0])), **{b: int(dec["branch"][b].sum()) for b in BRANCHES})
    # the same inputs with real current maps: what the _real entry points take (float planes, zero imaginary parts)
    for k in ("cv", "cn"):
        z = c[k].copy()
        z[..., 1] = 0.0
        c[k + "0"] = z
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def check_inputs(rows, cols):
    """What the generator has to deliver for the assertions below to mean something (no backend)."""
    s = case(rows, cols)["stats"]
    assert s["fragile_left"] == 0, s
    assert s["punched_share"] <= PUNCH_CAP, s
    assert s["protected_inliers"] == s["protected"] and s["model_00_valid"], s
    if s["pixels"] >= 1000:
        assert all(s[b] >= 10 for b in BRANCHES) and s["inliers"] >= 0.3 * s["pixels"], s
    elif s["pixels"] >= 400:                                             # one row, one column: every branch, fewer members
        assert all(s[b] >= 5 for b in BRANCHES) and s["inliers"] >= 0.3 * s["pixels"], s
    else:                                                                # 2 x 3: six pixels
        assert s["inliers"] >= 2 and s["inliers"] < s["pixels"], s
    return s


def _plausible_real(v):
    v[np.isnan(v)] = 0.75
    return v


def buffers(c, pitch_kind, real=False, zero=False):
    """The four maps in pitched buffers with a guard row before and after the stacked planes, padding and guards filled with mirrored
    image data (finite: a read past an edge is taken for data); with zero, the current maps have zero imaginary parts; with real, they
    come with their float planes (vertex, normal) at the matching pitch as well."""
    rows, cols = c["rows"], c["cols"]
    p8, p4 = mc.pitches(cols, 8)[pitch_kind], mc.pitches(cols, 4)[pitch_kind]
    maps = [mc.Pitched.source(c[k], p8, mc.plausible_map) for k in (("cv0", "cn0") if real or zero else ("cv", "cn")) + ("pv", "pn")]
    planes = [mc.Pitched.source(np.ascontiguousarray(c[k][..., 0]), p4, _plausible_real) for k in ("cv0", "cn0")] if real else None
    for b in maps + (planes or []):
        assert not np.isnan(b.typed[0]).any() and not np.isnan(b.typed[-1]).any() and not np.isnan(b.typed[:, b.width:]).any()
    return maps, planes


def run(be, c, pitch_kind, y0=0, y1=None, real=False, zero=False, **kw):
    maps, planes = buffers(c, pitch_kind, real, zero)
    return be.icp_p(c["Rcurr"], c["tcurr"], maps[0], maps[1], c["Rprev_inv"], c["tprev"], c["intr"], maps[2], maps[3], c["rows"], c["cols"],
                    DIST, ANGLE, y0=y0, y1=c["rows"] if y1 is None else y1, real=tuple(planes) if real else None, **kw)


def ratios(got, ref):
    """(worst |error| / bound of the real parts, of the imaginary parts) of 55 doubles against the model of their range; a bound of
    zero (no inlier) asks for equality."""
    re, im = got[0:54:2], got[1:54:2] / Hs
    def worst(err, bound):
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        return float(r.max())
    return worst(np.abs(re - ref["s0"]), C_ICP * U * ref["B"]), worst(np.abs(im - ref["ds"]), C_ICP * U * ref["dB"])


def assert_sums(got, ref, what=""):
    r = ratios(got, ref)
    print(f"icp {what}: inliers {int(got[54])} (model {ref['inliers']}), error / bound: real {r[0]:.4f}, imaginary {r[1]:.4f}")
    assert got[54] == ref["inliers"], (what, got[54], ref["inliers"])     # no fragile pixel is left: exact
    assert r[0] <= 1.0 and r[1] <= 1.0, (what, r)
    return r


def check_case(be, rows, cols):
    """The whole image on every pitch the geometry runs at: the count, the 54 sums, and the same bits whatever the pitch."""
    c = case(rows, cols)
    first, worst = None, (0.0, 0.0)
    for kind in ((0, 1, 2) if (rows, cols) in ALL_PITCHES else (1,)):
        got = run(be, c, kind)
        r = assert_sums(got, c["whole"], f"{rows}x{cols} pitch {kind}")
        worst = tuple(max(a, b) for a, b in zip(worst, r))
        first = got if first is None else first
        assert np.array_equal(got.view(np.uint64), first.view(np.uint64)), "the result must not depend on the pitch"
    return dict(real=worst[0], imag=worst[1], inliers=int(first[54]), punched_share=c["stats"]["punched_share"]), first


def check_ranges(be, rows, cols):
    """Three row ranges that tile the image, each against the model of that range, and their sum against the whole image's launch:
    every launch adds its n products in some fixed association of double additions, each within n * 2^-53 of sum |product| <= B."""
    c = case(rows, cols)
    whole = run(be, c, 1)
    parts, worst = np.zeros(55), (0.0, 0.0)
    for y0, y1 in RANGES[(rows, cols)]:
        got = run(be, c, 1, y0, y1)
        r = assert_sums(got, c["ranges"][(y0, y1)], f"{rows}x{cols} rows [{y0}, {y1})")
        worst = tuple(max(a, b) for a, b in zip(worst, r))
        parts = parts + got
    assert parts[54] == whole[54]
    slack = 2 * whole[54] * 2.0 ** -53
    assert np.all(np.abs(parts[0:54:2] - whole[0:54:2]) <= slack * c["whole"]["B"])
    assert np.all(np.abs(parts[1:54:2] - whole[1:54:2]) <= slack * Hs * c["whole"]["dB"])
    return dict(real=worst[0], imag=worst[1])


def check_empty(be, **kw):
    """Empty ranges at the start, inside and at the end of the image: 55 zeros."""
    c = case(*EMPTY_SHAPE)
    for y0, y1 in EMPTY_RANGES:
        got = run(be, c, 1, y0, y1, **kw)
        assert got.shape == (55,) and not got.any(), (y0, y1, got)
