"""The cases that hold the map-preparation kernels (bilateral filter, depth pyramid, vertex / normal maps, the two resizes and the
fused launches; x-slam_amd/csrc/xs_map.hip, oracle/oc_kernels.hpp) against the float64 model of tests/independent_f64.py, on small
ragged images in pitched buffers with guard rows.  Backend-neutral: tests/test_maps_cpu.py runs them on the CPU oracle,
tests/test_maps_gpu.py on the HIP kernels.  Test infrastructure."""
import functools

import numpy as np

import independent_f64 as ind
from independent_cases import Hs

# rows x cols: one full wave row plus 6 lanes and nine 4-row blocks plus one row (halves to 18 x 35 and 9 x 17, both odd); exactly one
# 13-tap window high and two 64-column tiles plus 3; smaller than the window both ways; two taps in all; several blocks each way
SHAPES = [(37, 70), (13, 131), (5, 9), (2, 3), (66, 200)]
PATTERN = 0xA5                     # guard rows, pitch padding and unwritten outputs: float 0xA5A5A5A5 = -2.87e-16, finite and not a value
U = 2.0 ** -24                     # float32 unit round-off

# Bilateral tie zone.  A float32 evaluation of sum1 / sum2 lies within a relative TAU of the float64 quotient q, so the kernel's
# integer may be either neighbour only where q is within TAU * q of a half-integer.  Measured: the float32 emulation
# ind.bilateral_f32 (every operation rounded, taps in the reference's order) deviates from q by at most 1.01e-6 over the five test
# images (worst on 66 x 200; at most 7.9e-7 on the others); times 2, because the GPU's exp and fma are not the emulation's: 2.1e-6.
TAU = 2.1e-6
TIE_CAP = 0.03                     # at most this share of the live pixels may lie in the tie zone (a condition on the inputs)
# Normal map and resizes.  An output component may be off by C_MAP * 2^-24 * kappa.  Measured: the float32 evaluation of the model
# itself differs from its float64 evaluation by at most 1.99 * 2^-24 on the scale of each case over the test inputs (normal map 1.92,
# resize of vertices 1.98, resize of normals 1.66, the fused launches' inputs 1.97); times 4: 8.
C_MAP = 8.0
C_VERTEX = 4.0                     # vertex map: three rounded operations and the rounded reciprocal of the focal length


def pitches(cols, elem):
    """Tight, the C++ host's (rounded up to 256 B, device_array.hpp), and the smallest the ABI allows above tight (the header asks for
    a pitch in bytes as PtrStep's and nothing more: one element)."""
    tight = cols * elem
    return [tight, -(-tight // 256) * 256, tight + elem]


def pitch_pairs(scols, selem, dcols, delem):
    return [(s, d) for s in pitches(scols, selem) for d in pitches(dcols, delem)]


class Pitched:
    """rows x cols elements of comp values of dtype in a byte buffer of (rows + 2) rows of pitch bytes: one guard row before and one
    after the image.  A fresh buffer holds PATTERN everywhere; addr is the address of image row 0 (what a kernel is given)."""
    def __init__(self, rows, cols, dtype, comp, pitch):
        self.rows, self.cols, self.dtype, self.comp, self.pitch = rows, cols, np.dtype(dtype), comp, int(pitch)
        self.width = cols * comp
        assert pitch >= self.width * self.dtype.itemsize and pitch % (comp * self.dtype.itemsize) == 0
        self.a = np.full((rows + 2, self.pitch), PATTERN, np.uint8)

    @property
    def addr(self):
        return self.a.ctypes.data + self.pitch

    @property
    def typed(self):
        return self.a.view(self.dtype)                                   # [rows + 2, pitch / itemsize], guards and padding included

    @property
    def image(self):
        v = self.typed[1:-1, :self.width]
        return v.reshape(self.rows, self.cols, 2) if self.comp == 2 else v

    def outside_untouched(self):
        return bool((self.a[0] == PATTERN).all() and (self.a[-1] == PATTERN).all()
                    and (self.a[1:-1, self.width * self.dtype.itemsize:] == PATTERN).all())

    def untouched(self, mask):
        """Image elements under mask ([rows, cols]) still hold the pattern."""
        b = self.a[1:-1, :self.width * self.dtype.itemsize].reshape(self.rows, self.cols, -1)
        return bool((b[mask] == PATTERN).all())

    @classmethod
    def out(cls, rows, cols, comp, pitch):
        return cls(rows, cols, np.float32, comp, pitch)

    @classmethod
    def source(cls, img, pitch, plausible):
        """img ([rows, cols] or [rows, cols, 2]) with the padding and the guard rows filled from the image itself (columns mirrored
        about the last column but one, the first row above, the last row but one below) — values a read past the edge would mistake
        for data, so that such a read changes the result.  plausible(values) replaces what would hide a read (holes, outliers, NaN)."""
        img = np.asarray(img)
        comp = 2 if img.ndim == 3 else 1
        rows, cols = img.shape[:2]
        b = cls(rows, cols, img.dtype, comp, pitch)
        ncol = b.pitch // (comp * b.dtype.itemsize)
        ic = np.concatenate([np.arange(cols), (cols - 2 - np.arange(ncol - cols)) % cols])
        ir = np.concatenate([[0], np.arange(rows), [max(rows - 2, 0)]])
        ext = img[ir][:, ic]
        fixed = plausible(ext.copy())
        inside = np.zeros(ext.shape[:2], bool)
        inside[1:-1, :cols] = True
        ext = np.where(inside if comp == 1 else inside[..., None], ext, fixed)
        b.typed[...] = ext.reshape(rows + 2, ncol * comp)
        return b


def plausible_depth(level):
    def f(v):
        v[(v == 0) | (v >= 60000)] = level
        return v
    return f


def plausible_map(v):
    """finite complex values: a NaN becomes a vertex-sized number (never the sentinel)"""
    v[np.isnan(v[..., 0]), 0] = 0.75
    return v


# ------------------------------------------------------------------------------------------------
# Bilateral filter
def bilateral_depth(rows, cols, seed):
    """Depth in which float32 underflow is never ambiguous: any two pixels of one window differ by <= 300 mm (weight >= e^-52, a normal
    float) or by >= 560 mm (exponent >= 174: zero in float32 however it is evaluated).  9 x 11 blocks of plateau levels 700 mm apart
    (700 .. 5600), a plateau at 140 mm (so that values cross the 200 mm flush; its neighbours are >= 1400), a ramp of <= 100 mm across
    the image plus integer noise +-20 (the 4900 plateau crosses 5000), 3 % speckle of {0, 60000, 65535}, and the reference's blind spot:
    30 % of the last column set to 0 and 30 % of the last row to 65535 (no window visits those, not even their own)."""
    rng = np.random.default_rng(seed)
    by, bx = -(-rows // 9), -(-cols // 11)
    lv = rng.integers(1, 9, (by, bx)) * 700
    lv.flat[rng.integers(0, lv.size)] = 4900
    lv.flat[rng.integers(0, lv.size)] = 700
    if lv.size >= 4:
        j, i = rng.integers(0, by), rng.integers(0, bx)
        lv[max(j - 1, 0):j + 2, max(i - 1, 0):i + 2] = np.maximum(lv[max(j - 1, 0):j + 2, max(i - 1, 0):i + 2], 1400)
        lv[j, i] = 140
    d = np.kron(lv, np.ones((9, 11), np.int64))[:rows, :cols]
    yy, xx = np.mgrid[0:rows, 0:cols]
    d = d + np.rint(100.0 * (xx + yy) / max(rows + cols - 2, 1)).astype(np.int64) + rng.integers(-20, 21, (rows, cols))
    sp = rng.random((rows, cols)) < 0.03
    d[sp] = rng.choice([0, 60000, 65535], int(sp.sum()))
    d[rng.random(rows) < 0.3, cols - 1] = 0
    d[rows - 1, rng.random(cols) < 0.3] = 65535
    if rows * cols < 64:
        d[0, 0] = 60000                                                  # (too few pixels to leave a flushed one to chance)
    return d.astype(np.uint16)


@functools.lru_cache(maxsize=None)
def bilateral_reference(rows, cols):
    """The input of one shape with its model, computed once and shared: never modified."""
    d = bilateral_depth(rows, cols, 1000 * rows + cols)
    q, amin, nband = ind.bilateral(d, band=(60.0, 170.0))
    q32 = ind.bilateral_f32(d)
    dead = amin > 150
    live = ~dead
    lo = np.where(live, np.floor(np.where(live, q, 0)), 0)
    tie = live & (np.abs(q - (lo + 0.5)) <= TAU * q)
    want = ind.bilateral_post(np.where(live, np.rint(q), 0))
    with np.errstate(invalid="ignore", divide="ignore"):
        dev = np.abs(q32[live] - q[live]) / np.maximum(q[live], 0.5)      # (below the first half-integer only the size matters)
    for a in (d, q, amin, dead, tie, want):
        a.setflags(write=False)
    return dict(depth=d, q=q, amin=amin, dead=dead, live=live, tie=tie, want=want, lo=lo, ambiguous_taps=int(nband.sum()),
                ambiguous_pixels=int(((amin > 80) & (amin <= 150)).sum()), f32_dev=float(dev.max()) if dev.size else 0.0,
                q32_dead_not_nan=int((~np.isnan(q32[dead])).sum()),
                n_dead=int(dead.sum()), n_live=int(live.sum()), n_inrange=int((live & (want > 0)).sum()),
                n_flushed=int((live & (want == 0)).sum()), tie_share=float(tie.sum() / max(live.sum(), 1)))


def check_bilateral_inputs(rows, cols):
    """What the generator has to deliver for the assertions below to mean something (CPU only, no backend)."""
    r = bilateral_reference(rows, cols)
    assert r["ambiguous_taps"] == 0 and r["ambiguous_pixels"] == 0, r      # no weight whose underflow depends on the exp at hand
    assert r["q32_dead_not_nan"] == 0                                       # a dead pixel is 0 / 0 in float32
    assert r["n_dead"] > 0 and r["n_inrange"] > 0 and r["n_flushed"] > 0, r
    assert 2 * r["f32_dev"] <= TAU, r["f32_dev"]
    assert r["tie_share"] <= TIE_CAP, r["tie_share"]
    return {k: r[k] for k in ("n_dead", "n_live", "n_inrange", "n_flushed", "tie_share", "f32_dev")}


def assert_bilateral(out, r):
    """out: [rows, cols, 2] of the implementation; r: bilateral_reference.  Returns (tie pixels that took the other neighbour,
    largest |out - q| over the in-range pixels)."""
    re, im = out[..., 0].astype(np.float64), out[..., 1]
    assert np.array_equal(im.view(np.uint32), np.zeros(im.shape, np.uint32)), "imaginary part must be +0 everywhere"
    assert (re[r["dead"]] == 0).all(), "0 / 0 converts to 0"
    # a live pixel is post(rint(q)); within TAU * q of a half-integer (see TAU above: measured 1.01e-6, doubled) either neighbour's
    lo_ok = re == ind.bilateral_post(r["lo"])
    hi_ok = re == ind.bilateral_post(r["lo"] + 1)
    ok = np.where(r["tie"], lo_ok | hi_ok, re == r["want"])
    bad = r["live"] & ~ok
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist(), re[bad][:5].tolist(), r["q"][bad][:5].tolist())
    inr = r["live"] & (r["want"] > 0)
    return int((r["tie"] & (re != r["want"])).sum()), float(np.abs(re - r["q"])[inr].max())


def check_bilateral(be, rows, cols):
    r = bilateral_reference(rows, cols)
    other, dist, outs = 0, 0.0, None
    for sp, dp in pitch_pairs(cols, 2, cols, 8):
        src = Pitched.source(r["depth"], sp, plausible_depth(1400))
        dst = Pitched.out(rows, cols, 2, dp)
        be.bilateral_p(src, dst, rows, cols)
        assert dst.outside_untouched(), (sp, dp)
        o, d = assert_bilateral(dst.image, r)
        other, dist = max(other, o), max(dist, d)
        outs = dst.image.copy() if outs is None else outs
        assert np.array_equal(outs, dst.image), "the result must not depend on the pitches"
    return dict(tie_other_neighbour=other, max_dist_to_q=dist, n_dead=r["n_dead"], n_inrange=r["n_inrange"], n_flushed=r["n_flushed"],
                tie_share=r["tie_share"]), outs


# ------------------------------------------------------------------------------------------------
# Depth pyramid
def pyr_crafted(rows, cols, seed):
    """A complex map for pyrDown's gate and rounding: real parts 1000 .. 1003 plus an offset of 0, +-1, +-89, +-90, +-91 (so that
    differences between a tap and its centre sit at 88 .. 92 either side of the 90 mm gate) plus a fraction of 0, +-1/4, +-1/2 or 3/4
    (x.5 rounds to even, not down and not away); imaginary parts non-zero everywhere (they must not reach the output)."""
    rng = np.random.default_rng(seed)
    re = (1000 + rng.integers(0, 4, (rows, cols)) + rng.choice([-91, -90, -89, -1, 0, 0, 0, 1, 89, 90, 91], (rows, cols))
          + rng.choice([0.0, 0.5, -0.5, 0.25, -0.25, 0.75], (rows, cols)))
    im = rng.choice([-1.0, 1.0], (rows, cols)) * rng.uniform(0.5, 50.0, (rows, cols))
    return np.stack([re, im], -1).astype(np.float32)


def check_pyr_down(be, src_img):
    """One halving of the complex image src_img on every pitch pair: exact equality with the integer model.  Returns the output."""
    srows, scols = src_img.shape[:2]
    drows, dcols = srows // 2, scols // 2
    want = ind.pyr_down(src_img[..., 0])
    nz = src_img[..., 0][src_img[..., 0] != 0]
    level = float(np.rint(np.median(nz))) if nz.size else 1000.0
    first = None
    for sp, dp in pitch_pairs(scols, 8, dcols, 8):
        src = Pitched.source(src_img, sp, lambda v: np.where(np.isfinite(v) & (v != 0), v, level).astype(np.float32))
        dst = Pitched.out(drows, dcols, 2, dp)
        be.pyr_down_p(src, dst, srows, scols)
        assert dst.outside_untouched(), (sp, dp)
        got = dst.image
        assert np.array_equal(got[..., 0].astype(np.float64), want.astype(np.float64)), (sp, dp, np.argwhere(got[..., 0] != want)[:5].tolist())
        assert np.array_equal(got[..., 1].view(np.uint32), np.zeros((drows, dcols), np.uint32)), "imaginary part must be +0"
        first = got.copy() if first is None else first
    return first


def check_pyramid_of_bilateral(be, level0):
    """Two halvings of a bilateral output (level0: what check_bilateral returned), each against the model on the implementation's own
    input.  An image too small to halve twice stops where the reference's would be empty."""
    img, n = level0, 0
    while img.shape[0] >= 2 and img.shape[1] >= 2 and n < 2:
        img, n = check_pyr_down(be, img), n + 1
    return n


# ------------------------------------------------------------------------------------------------
# Vertex and normal maps
def intr_for(rows, cols):
    """fx, fy arbitrary floats; cx, cy multiples of 1/2, so that float(u) - cx is exact and three rounded operations remain."""
    return np.array([517.3, 516.5, (cols - 1) / 2, (rows - 1) / 2], np.float32)


def scene_depth(rows, cols, seed, step_blocks=True):
    """Complex depth (mm) for the vertex / normal cases: a gentle ramp near 1 m with 4 x 5 blocks raised by 500 mm (at a block's
    corner both neighbours of a pixel are 0.5 m away: the two edges are nearly parallel, kappa in the hundreds), isolated holes — one
    per parity class of (y, x), each touching the three taps of the normal and the four positions of the resize — and a dense imaginary
    part of Hs * (1 .. 100) of either sign, holes included (Re = 0, Im != 0 must still be a hole)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    re = 1000.0 + 3.0 * xx + 2.0 * yy + rng.integers(-2, 3, (rows, cols))
    if step_blocks:
        re = re + 500.0 * (((yy // 4) + (xx // 5)) % 2)
    hole = rng.random((rows, cols)) < 0.04
    for py in (0, 1):
        for px in (0, 1):
            ys, xs = np.arange(py, rows, 2), np.arange(px, cols, 2)
            if ys.size and xs.size:
                hole[rng.choice(ys), rng.choice(xs)] = True
    if hole.all():
        hole[0, 0] = False
    re[hole] = 0.0
    im = Hs * rng.uniform(1.0, 100.0, (rows, cols)) * rng.choice([-1.0, 1.0], (rows, cols))
    return np.stack([re, im], -1).astype(np.float32)


def planes(img, rows):
    """[3 * rows, cols, 2] -> ([3, rows, cols] real, [3, rows, cols] imaginary)"""
    m = np.asarray(img).reshape(3, rows, img.shape[1], 2)
    return m[..., 0], m[..., 1]


def assert_vertex(vm, depth, intr, rows, cols, real=None):
    """vm: Pitched vertex map written by the implementation for depth [rows, cols, 2].  Returns the worst relative errors in units of 2^-24."""
    val, d1, hole = ind.vertex_map(intr, depth)
    re, im = planes(vm.image, rows)
    assert vm.outside_untouched()
    assert np.array_equal(np.isnan(re[0]), hole), "sentinel sets differ"
    assert (im[0][hole] == 0).all()                                      # the sentinel is (NaN, 0)
    under = np.zeros((3 * rows, cols), bool)
    under[rows:] = np.tile(hole, (2, 1))
    assert vm.untouched(under), "y / z planes under a sentinel must not be written"
    ok = ~hole
    e_re = np.abs(re[:, ok] - val[:, ok]) / np.abs(val[:, ok]).clip(1e-300)
    e_im = np.abs(im[:, ok] - d1[:, ok]) / np.abs(d1[:, ok]).clip(1e-300)
    e_re[val[:, ok] == re[:, ok]] = 0
    e_im[d1[:, ok] == im[:, ok]] = 0
    assert e_re.max() <= C_VERTEX * U and e_im.max() <= C_VERTEX * U, (e_re.max() / U, e_im.max() / U)
    if real is not None:
        assert real.outside_untouched() and real.untouched(under)
        r = real.image.reshape(3, rows, cols)
        assert np.array_equal(np.isnan(r[0]), hole)
        assert np.array_equal(r[:, ok].view(np.uint32), re[:, ok].view(np.uint32)), "real planes must carry the same values"
    return float(e_re.max() / U), float(e_im.max() / U)


def normal_reference(vimg, rows):
    """Model of the normal map of the vertex map vimg as given: values, sentinel, tolerances and the derivative from the fourth-order
    central difference with one step per pixel, 5e-3 / (kappa * dscale): truncation (5e-3)^4 and float64 round-off ~1e-11 * kappa,
    both relative and far below 2^-24."""
    n, sent, kappa, dscale = ind.normal_map(vimg, 0.0, Hs)
    n32 = ind.normal_map(vimg, dtype=np.float32)[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        step = np.where(sent | ~(kappa * dscale > 0), 1.0, 5e-3 / (kappa * dscale))
        dn = ind.central4(lambda d: ind.normal_map(vimg, d, Hs)[0], step)
        spread = np.abs(n32.astype(np.float64) - n)[:, ~sent] / (U * kappa[~sent])
    return dict(n=n, sent=sent, kappa=kappa, dscale=dscale, dn=dn, spread=float(spread.max()) if spread.size else 0.0)


def assert_normal(nm, vimg, rows, cols, real=None):
    """nm: Pitched normal map written for the vertex map image vimg.  Returns figures (errors in units of their tolerance scale)."""
    m = normal_reference(vimg, rows)
    re, im = planes(nm.image, rows)
    sent, ok = m["sent"], ~m["sent"]
    assert nm.outside_untouched()
    assert np.array_equal(np.isnan(re[0]), sent), "sentinel sets differ"
    assert (im[0][sent] == 0).all()
    under = np.zeros((3 * rows, cols), bool)
    under[rows:] = np.tile(sent, (2, 1))
    assert nm.untouched(under)
    fig = dict(n_valid=int(ok.sum()), kappa_max=float(m["kappa"][ok].max()) if ok.any() else 0.0, model_f32_spread=m["spread"], value_err=0.0, deriv_err=0.0)
    if ok.any():
        k, ds = m["kappa"][ok], m["dscale"][ok]
        e_v = np.abs(re[:, ok] - m["n"][:, ok]) / (U * k)
        dnorm = np.sqrt((m["dn"][:, ok] ** 2).sum(0))
        e_d = np.abs(im[:, ok].astype(np.float64) / Hs - m["dn"][:, ok]) / (U * k * (ds + dnorm))
        fig.update(value_err=float(e_v.max()), deriv_err=float(e_d.max()))
        assert dnorm.max() > 0
        # C_MAP: four times the float32-vs-float64 spread of the model itself on these inputs (measured 1.99, see above)
        assert e_v.max() <= C_MAP and e_d.max() <= C_MAP, fig
    if real is not None:
        assert real.outside_untouched() and real.untouched(under)
        r = real.image.reshape(3, rows, cols)
        assert np.array_equal(np.isnan(r[0]), sent)
        assert np.array_equal(r[:, ok].view(np.uint32), re[:, ok].view(np.uint32)), "real planes must carry the same values"
    return fig


def maps_of(be, depth, rows, cols, pitch, intr=None):
    """The implementation's vertex and normal map of a complex depth at one map pitch (the depth itself at the host's pitch)."""
    intr = intr_for(rows, cols) if intr is None else intr
    dsrc = Pitched.source(depth, pitches(cols, 8)[1], lambda v: np.where(v == 0, np.float32(1234.0), v))
    vm, nm = Pitched.out(3 * rows, cols, 2, pitch), Pitched.out(3 * rows, cols, 2, pitch)
    be.create_vmap_p(intr, dsrc, vm, rows, cols)
    vsrc = Pitched.source(vm.image, pitch, plausible_map)
    be.create_nmap_p(vsrc, nm, rows, cols)
    return vm, nm


def check_vertex(be, rows, cols):
    depth, intr = scene_depth(rows, cols, 7 * rows + cols), intr_for(rows, cols)
    worst = (0.0, 0.0)
    for sp, dp in pitch_pairs(cols, 8, cols, 8):
        dsrc = Pitched.source(depth, sp, lambda v: np.where(v == 0, np.float32(1234.0), v))
        vm = Pitched.out(3 * rows, cols, 2, dp)
        be.create_vmap_p(intr, dsrc, vm, rows, cols)
        worst = tuple(max(a, b) for a, b in zip(worst, assert_vertex(vm, depth, intr, rows, cols)))
    return dict(value_err_ulp=worst[0], deriv_err_ulp=worst[1], holes=int((depth[..., 0] == 0).sum()))


def check_normal(be, rows, cols):
    depth = scene_depth(rows, cols, 7 * rows + cols)
    figs = []
    for p in pitches(cols, 8):
        vm, nm = maps_of(be, depth, rows, cols, p)
        figs.append(assert_normal(nm, vm.image, rows, cols))
    return {k: max(f[k] for f in figs) for k in figs[0]}


# ------------------------------------------------------------------------------------------------
# The two resizes
def resize_reference(img, srows, normalize):
    """Model of one halving of the map image img as given, with its tolerance scales.  Vertices: per component, sum |x_i| / 4 (value)
    and sum |Im_i| / 4 / Hs (derivative; the function is linear, so any step serves: one that moves the value by its own size).
    Normals: kappa = |mean of |n_i|| / |mean n_i| and the derivative as for the normal map."""
    out, sent, mag, dmag = ind.resize(img, normalize, 0.0, Hs)
    o32 = ind.resize(img, normalize, dtype=np.float32)[0].astype(np.float64)
    nrm = lambda v: np.sqrt((v * v).sum(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        if normalize:
            mean = ind.resize(img, False)[0]
            kappa = nrm(mag) / nrm(mean)
            ds = nrm(dmag) / nrm(mean)
            step = np.where(sent | ~(kappa * ds > 0), 1.0, 5e-3 / (kappa * ds))
            vscale, unit = kappa[None], ds
        else:
            ratio = np.where(dmag > 0, mag / dmag, np.inf).min(0)
            step = np.where(sent | ~np.isfinite(ratio) | ~(ratio > 0), 1.0, ratio)
            vscale, unit = mag, None
        dout = ind.central4(lambda d: ind.resize(img, normalize, d, Hs)[0], step)
        dscale = (unit + nrm(dout))[None] * kappa[None] if normalize else dmag
        spread = (np.abs(o32 - out) / (U * vscale))[:, ~sent]
    return dict(out=out, sent=sent, vscale=np.broadcast_to(vscale, out.shape), dout=dout, dscale=np.broadcast_to(dscale, out.shape),
                spread=float(np.nanmax(spread)) if spread.size else 0.0)


def assert_resize(dst, img, srows, normalize):
    drows, dcols = srows // 2, img.shape[1] // 2
    m = resize_reference(img, srows, normalize)
    re, im = planes(dst.image, drows)
    sent, ok = m["sent"], ~m["sent"]
    assert dst.outside_untouched()
    assert np.array_equal(np.isnan(re[0]), sent), "sentinel sets differ"
    assert (im[0][sent] == 0).all()
    under = np.zeros((3 * drows, dcols), bool)
    under[drows:] = np.tile(sent, (2, 1))
    assert dst.untouched(under)
    fig = dict(n_valid=int(ok.sum()), n_sentinel=int(sent.sum()), model_f32_spread=m["spread"], value_err=0.0, deriv_err=0.0)
    if ok.any():
        with np.errstate(invalid="ignore", divide="ignore"):
            e_v = np.abs(re[:, ok] - m["out"][:, ok]) / (U * m["vscale"][:, ok])
            e_d = np.abs(im[:, ok].astype(np.float64) / Hs - m["dout"][:, ok]) / (U * m["dscale"][:, ok])
        e_v[re[:, ok] == m["out"][:, ok]] = 0
        e_d[~np.isfinite(e_d) & (np.abs(im[:, ok].astype(np.float64) / Hs - m["dout"][:, ok]) == 0)] = 0
        fig.update(value_err=float(e_v.max()), deriv_err=float(e_d.max()))
        assert e_v.max() <= C_MAP and e_d.max() <= C_MAP, fig               # C_MAP as for the normal map
    return fig


def check_resize(be, rows, cols):
    """Both maps of the scene at rows x cols halved twice (vertices plain, normals renormalised), every level on every pitch pair,
    each against the model on the implementation's own input.  With the holes of scene_depth a NaN sits in each of the four positions."""
    depth = scene_depth(rows, cols, 7 * rows + cols, step_blocks=False)
    vm, nm = maps_of(be, depth, rows, cols, pitches(cols, 8)[0])
    figs, positions = {}, set()
    for name, buf, normalize in (("vmap", vm, False), ("nmap", nm, True)):
        img, srows = buf.image.copy(), rows
        for level in (1, 2):
            scols = img.shape[1]
            drows, dcols = srows // 2, scols // 2
            if drows == 0 or dcols == 0:
                break
            x = np.isnan(img[:srows, :, 0])
            positions |= {(i, j) for i in (0, 1) for j in (0, 1) if x[i:2 * drows:2, j:2 * dcols:2].any()}
            first = None
            for sp, dp in pitch_pairs(scols, 8, dcols, 8):
                src = Pitched.source(img, sp, plausible_map)
                dst = Pitched.out(3 * drows, dcols, 2, dp)
                be.resize_p(src, dst, srows, scols, normalize)
                f = assert_resize(dst, img, srows, normalize)
                key = f"{name}_level{level}"
                figs[key] = f if key not in figs else {k: max(f[k], figs[key][k]) for k in f}
                first = dst.image.copy() if first is None else first
            valid = ~np.isnan(first[:drows, :, 0])
            first[drows:][np.tile(~valid, (2, 1))] = 0.5                  # (unwritten y / z under a sentinel: any finite filler)
            img, srows = first, drows
    figs["nan_positions"] = len(positions)
    return figs


# ------------------------------------------------------------------------------------------------
# Fused launches, at 37 x 70 with a different pitch kind on every level
FUSED = (37, 70)


def check_vnmaps(be, real):
    """xs_create_vnmaps(_real): three levels in one launch, each level's vertex map against the model of its depth and its normal
    map against the model on that vertex map; with real, the float planes carry the same values and sentinels."""
    rows0, cols0 = FUSED
    depths, intrs, ds, vs, ns, vr, nr = [], [], [], [], [], [], []
    for l in range(3):
        rows, cols = rows0 >> l, cols0 >> l
        depths.append(scene_depth(rows, cols, 31 * l + 5))
        intrs.append(intr_for(rows, cols))
        ds.append(Pitched.source(depths[l], pitches(cols, 8)[(l + 2) % 3], lambda v: np.where(v == 0, np.float32(1234.0), v)))
        mp = pitches(cols, 8)[(l + 1) % 3]
        vs.append(Pitched.out(3 * rows, cols, 2, mp))
        ns.append(Pitched.out(3 * rows, cols, 2, mp))
        rp = pitches(cols, 4)[(l + 1) % 3]
        vr.append(Pitched.out(3 * rows, cols, 1, rp))
        nr.append(Pitched.out(3 * rows, cols, 1, rp))
    be.create_vnmaps_p(intrs, ds, vs, ns, rows0, cols0, vreal=vr if real else None, nreal=nr if real else None)
    figs = {}
    for l in range(3):
        rows, cols = rows0 >> l, cols0 >> l
        ev = assert_vertex(vs[l], depths[l], intrs[l], rows, cols, real=vr[l] if real else None)
        f = assert_normal(ns[l], vs[l].image, rows, cols, real=nr[l] if real else None)
        f.update(vertex_value_err_ulp=ev[0], vertex_deriv_err_ulp=ev[1])
        figs[f"level{l}"] = f
    return figs


def check_resize_pyramid(be):
    """xs_resize_pyramid: both halvings of both maps in one launch; level 1 against the model on level 0, level 2 against the model on
    the implementation's own level 1."""
    rows0, cols0 = FUSED
    depth = scene_depth(rows0, cols0, 77, step_blocks=False)
    p0, p1, p2 = pitches(cols0, 8)[1], pitches(cols0 // 2, 8)[2], pitches(cols0 // 4, 8)[0]
    vm, nm = maps_of(be, depth, rows0, cols0, p0)
    v0, n0 = Pitched.source(vm.image, p0, plausible_map), Pitched.source(nm.image, p0, plausible_map)
    r1, c1, r2, c2 = rows0 // 2, cols0 // 2, rows0 // 4, cols0 // 4
    v1, n1 = Pitched.out(3 * r1, c1, 2, p1), Pitched.out(3 * r1, c1, 2, p1)
    v2, n2 = Pitched.out(3 * r2, c2, 2, p2), Pitched.out(3 * r2, c2, 2, p2)
    be.resize_pyramid_p(v0, n0, rows0, cols0, v1, n1, v2, n2)
    figs = {}
    for name, m0, m1, m2, nrm in (("vmap", vm, v1, v2, False), ("nmap", nm, n1, n2, True)):
        figs[f"{name}_level1"] = assert_resize(m1, m0.image, rows0, nrm)
        mid = m1.image.copy()
        mid[r1:][np.tile(np.isnan(mid[:r1, :, 0]), (2, 1))] = 0.5
        figs[f"{name}_level2"] = assert_resize(m2, mid, r1, nrm)
    return figs
