"""A second, independently written checker for the hot-path kernels — TEST INFRASTRUCTURE ONLY.

Everything the parity tests otherwise rest on (oracle/, the fixtures under tests/golden/pipeline_*) is one
restatement of the reference's kernels in complex<float>, i.e. the same formulas in the same arithmetic as the
HIP kernels.  This module shares no text with it.  It was written from the reference's kernel sources alone
(file:line cited per function), in real float64 numpy, vectorised over voxels / pixels, and it never evaluates a
complex number: a quantity carried as (re, im) by the CSFD kernels is taken here as the real function
x(d) = re + d * im / h of the seed offset d, and derivatives come from central differences
(f(+d) - f(-d)) / 2d  (second order: (f(+d) - 2 f(0) + f(-d)) / d^2) of that real function, with every discrete
decision of the kernel — pixel picks, bounds and truncation tests, the zero-crossing step, trilinear cells, ICP
gates — taken once at d = 0 and held (the complex-step kernels decide on real parts only, so that is the function
they differentiate).  What the GPU tests assert with it:
  values       GPU real parts == this model in float64, to float32 rounding of the formula at hand;
  derivatives  GPU imaginary parts / h == the central difference, i.e. "gradients (and Hessians) fall out of the
               imaginary parts" is checked against a method that is not complex-step differentiation.
"""
import numpy as np

F32 = np.float32


def lin(c, d, h):
    """(..., 2) packed (re, im) float32 -> float64 value of the real function at seed offset d."""
    c = np.asarray(c, np.float64)
    return c[..., 0] + (d / h) * c[..., 1]


def _gather2d(img, y, x):
    return img[np.clip(y, 0, img.shape[0] - 1), np.clip(x, 0, img.shape[1] - 1)]


# ------------------------------------------------------------------------------------------------
# TSDF integrate — tsdfFusionKernal, XKinectFusion/src/TsdfFusion.cu:85-171
def integrate(d, h, Rv2c, tv2c, xyz, depth_m, intr, voxel_size, trunc, threshold, prev_value, prev_grad, prev_weight, dec=None):
    """One voxel update for the voxels xyz [n, 3] (integer coordinates).  Returns (new_value, dec); dec holds the
    decisions (taken when dec is None, which needs d == 0) incl. dec['update'] = voxels the kernel writes."""
    R = lin(np.asarray(Rv2c).reshape(3, 3, 2), d, h)
    t = lin(np.asarray(tv2c).reshape(3, 2), d, h)
    fx, fy, cx, cy = (float(F32(v)) for v in intr)
    vs, tr = float(F32(voxel_size)), float(F32(trunc))
    rows, cols = depth_m.shape
    vg = (np.asarray(xyz, np.float64) + 0.5) * vs                       # :108-111 voxel centre
    vc = vg @ R.T + t                                                    # :112
    inv_z = 1.0 / vc[:, 2]                                               # :113
    ix = vc[:, 0] * fx * inv_z + cx                                      # :116-117
    iy = vc[:, 1] * fy * inv_z + cy
    if dec is None:
        assert d == 0.0
        front = ~(inv_z < 0)                                             # :114-115
        with np.errstate(invalid="ignore"):
            coox = np.floor(ix - 0.5).astype(np.int64)                   # :118-119 __float2int_rd
            cooy = np.floor(iy - 0.5).astype(np.int64)
        inside = front & (coox > 1) & (cooy > 1) & (coox < cols - 1) & (cooy < rows - 1)   # :121-122
        nx, ny = np.rint(ix).astype(np.int64), np.rint(iy).astype(np.int64)                 # :123-124 __float2int_rn
        dd = [_gather2d(depth_m, cooy + j, coox + i).astype(np.float64) for j in (0, 1) for i in (0, 1)]  # d00 d10 d01 d11
        gmax, gmin = np.maximum.reduce(dd), np.minimum.reduce(dd)
        bil = (gmax - gmin < float(F32(threshold))) & (dd[0] != 0) & (dd[1] != 0) & (dd[2] != 0) & (dd[3] != 0)  # :133
        dec = dict(inside=inside, coox=coox, cooy=cooy, nx=nx, ny=ny, bil=bil)
    coox, cooy = dec["coox"], dec["cooy"]
    d00, d10 = _gather2d(depth_m, cooy, coox).astype(np.float64), _gather2d(depth_m, cooy, coox + 1).astype(np.float64)
    d01, d11 = _gather2d(depth_m, cooy + 1, coox).astype(np.float64), _gather2d(depth_m, cooy + 1, coox + 1).astype(np.float64)
    a, b = ix - (coox + 0.5), iy - (cooy + 0.5)                          # :135-136
    inter = d00 * (1 - a) * (1 - b) + d10 * a * (1 - b) + d01 * (1 - a) * b + d11 * a * b   # :137
    Dp = np.where(dec["bil"], inter, _gather2d(depth_m, dec["ny"], dec["nx"]).astype(np.float64))
    xl, yl = (ix - cx) / fx, (iy - cy) / fy                              # :142-143
    sdf = np.sqrt((Dp * xl) ** 2 + (Dp * yl) ** 2 + Dp ** 2) - np.sqrt((vc ** 2).sum(-1))  # :144-147
    if "update" not in dec:
        dec["update"] = dec["inside"] & (Dp > 0) & (sdf >= -tr)          # :148
        dec["far"] = sdf > tr                                            # :152
    tsdf = np.where(dec["far"], 1.0, sdf / tr)                           # :151-156 (the constant carries no derivative)
    w = np.asarray(prev_weight, np.float64)
    prev = np.asarray(prev_value, np.float64) + (d / h) * np.asarray(prev_grad, np.float64)
    return (prev * w + tsdf) / (w + 1.0), dec                            # :163


# ------------------------------------------------------------------------------------------------
# Raycast — RayCaster::operator(), XKinectFusion/src/RayCaster.cu:197-310 (+ :57-141 helpers)
def _cells(p, vs, res):
    """interpolateTrilineary's cell pick (:96-117) for points p [n, 3]: (lower cell [n, 3], on_border [n])."""
    with np.errstate(invalid="ignore"):
        g = np.floor(p / vs).astype(np.int64)                            # getVoxel :82-88
    r = np.asarray(res, np.int64)[None, :]
    border = ((g <= 0) | (g >= r - 1)).any(-1) | ~np.isfinite(p).all(-1)
    centre = (g + 0.5) * vs
    g = g - (p <= centre)                                                # :110-115: -(sgn(v - p) + 1) >> 1 is -1 for p <= v
    return g, border


def _trilinear(p, vol, cells, vs):
    """:117-136 on the (already offset) volume vol[z, y, x] for fixed lower cells."""
    gx, gy, gz = (np.clip(cells[:, i], 0, vol.shape[2 - i] - 2) for i in range(3))
    a0 = (p[:, 0] - (cells[:, 0] + 0.5) * vs) / vs
    b0 = (p[:, 1] - (cells[:, 1] + 0.5) * vs) / vs
    c0 = (p[:, 2] - (cells[:, 2] + 0.5) * vs) / vs
    a1, b1, c1 = 1 - a0, 1 - b0, 1 - c0
    V = lambda i, j, k: vol[gz + k, gy + j, gx + i]
    return (V(0, 0, 0) * a1 * b1 * c1 + V(0, 0, 1) * a1 * b1 * c0 + V(0, 1, 0) * a1 * b0 * c1 + V(0, 1, 1) * a1 * b0 * c0 +
            V(1, 0, 0) * a0 * b1 * c1 + V(1, 0, 1) * a0 * b1 * c0 + V(1, 1, 0) * a0 * b0 * c1 + V(1, 1, 1) * a0 * b0 * c0)


def raycast(d, h, intr, Rc2v, tc2v, Rv2w, tv2w, trunc, res, voxel_size, value, grad, px, py, dec=None):
    """Rays through pixels (px, py).  value / grad: [Z, Y, X] float arrays.  Returns (vertex_w [n, 3], normal_w [n, 3], dec);
    rows of pixels without a vertex (dec['hit'] False) / without a normal (dec['has_normal'] False) are NaN."""
    fx, fy, cx, cy = (float(F32(v)) for v in intr)
    vs = float(F32(voxel_size))
    step = float(F32(trunc) * F32(0.8))                                  # raycast() :350
    Rc = lin(np.asarray(Rc2v).reshape(3, 3, 2), d, h)
    tc = lin(np.asarray(tc2v).reshape(3, 2), d, h)
    Rw = lin(np.asarray(Rv2w).reshape(3, 3, 2), d, h)
    tw = lin(np.asarray(tv2w).reshape(3, 2), d, h)
    n = len(px)
    # readTsdf :69-78: stored value (+ i grad) + 1e-5
    vol = np.asarray(value, np.float64) + (d / h) * np.asarray(grad, np.float64) + float(F32(1e-5))
    cam = np.stack([(np.asarray(px, np.float64) - cx) / fx, (np.asarray(py, np.float64) - cy) / fy, np.ones(n)], -1)  # :57-63
    nxt = cam @ Rc.T + tc                                                # :207
    dirv = nxt - tc
    dirv = dirv / np.sqrt((dirv ** 2).sum(-1, keepdims=True))            # :208 normalized
    dirv = np.where(dirv == 0, 1e-15, dirv)                              # :210-212
    r = np.asarray(res, np.int64)
    if dec is None:
        assert d == 0.0
        t_curr = F32(0.2)                                                # :222-226
        g = np.floor((tc + dirv * float(t_curr)) / vs).astype(np.int64)
        g = np.clip(g, 0, r[None, :] - 1)                                # :227-230
        tsdf = vol[g[:, 2], g[:, 1], g[:, 0]]
        alive = np.ones(n, bool)
        cross_t = np.full(n, np.nan)
        cross_tn = np.full(n, np.nan)
        while t_curr < F32(5.0):                                         # :236, times accumulate in float
            t_next = F32(t_curr + F32(step))
            p = tc + dirv * float(t_next)                                # :238
            g = np.floor(p / vs).astype(np.int64)
            inside = ((g >= 0) & (g < r[None, :])).all(-1)               # checkInds :65-68
            alive &= inside                                              # :240-241
            gc = np.clip(g, 0, r[None, :] - 1)
            new = vol[gc[:, 2], gc[:, 1], gc[:, 0]]
            back = alive & (tsdf < 0) & (new > 0)                        # :245-246
            front = alive & (tsdf > 0) & (new < 0)                       # :247
            cross_t[front], cross_tn[front] = float(t_curr), float(t_next)
            alive &= ~(back | front)
            tsdf = np.where(alive, new, tsdf)
            t_curr = F32(t_curr + F32(step))
            if not alive.any():
                break
        cand = ~np.isnan(cross_t)
        p1, p0 = tc + dirv * cross_tn[:, None], tc + dirv * cross_t[:, None]
        c1, b1 = _cells(p1, vs, r)
        c0, b0 = _cells(p0, vs, r)
        dec = dict(cand=cand, t=cross_t, tn=cross_tn, c1=c1, c0=c0)
        ok = cand & ~b1 & ~b0                                            # :251-252, :256-257 (NaN from the border test)
        Ftdt, Ft = _trilinear(p1, vol, c1, vs), _trilinear(p0, vol, c0, vs)
        ok &= ~((Ft < 0) | (Ftdt > 0))                                   # :259-260
        dec["hit"] = ok
    hit = dec["hit"]
    t0 = np.where(hit, dec["t"], 0.0)
    tn = np.where(hit, dec["tn"], 0.0)
    Ftdt = _trilinear(tc + dirv * tn[:, None], vol, dec["c1"], vs)
    Ft = _trilinear(tc + dirv * t0[:, None], vol, dec["c0"], vs)
    with np.errstate(invalid="ignore", divide="ignore"):
        Ts = t0 - step * (Ft / (Ftdt - Ft))                              # :258, :261
    vertex = tc + dirv * Ts[:, None]                                     # :263
    vertex_w = vertex @ Rw.T + tw                                        # :264
    half = float(F32(voxel_size) * F32(0.5))                             # :274
    if "ncells" not in dec:
        with np.errstate(invalid="ignore"):
            g = np.floor(vertex / vs)
        okn = hit & ((g > 1) & (g < r[None, :] - 2)).all(-1)             # :269-271
        ncells, nb = [], np.zeros(n, bool)
        for axis in range(3):
            for sgn in (+1, -1):
                q = vertex.copy(); q[:, axis] += sgn * half
                c, b = _cells(q, vs, r)
                ncells.append(c); nb |= b
        dec["ncells"], dec["has_normal"] = ncells, okn & ~nb              # a NaN tap makes the normal NaN (:276-304)
    nrm = np.zeros((n, 3))
    k = 0
    for axis in range(3):
        taps = []
        for sgn in (+1, -1):
            q = vertex.copy(); q[:, axis] += sgn * half
            taps.append(_trilinear(q, vol, dec["ncells"][k], vs)); k += 1
        nrm[:, axis] = taps[0] - taps[1]                                 # :278, :286, :294
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm = nrm / np.sqrt((nrm ** 2).sum(-1, keepdims=True))           # :301 normalized
    normal_w = nrm @ Rw.T                                                # :301
    vertex_w = np.where(hit[:, None], vertex_w, np.nan)
    normal_w = np.where(dec["has_normal"][:, None], normal_w, np.nan)
    return vertex_w, normal_w, dec


# ------------------------------------------------------------------------------------------------
# ICP rows and normal equations — Combined::search_newton / operator(), XKinectFusion/src/ICP.cu:196-281
U32 = 2.0 ** -24                  # float32 unit round-off
# Rounded float32 operations on the path to the REAL part of a complex expression (complex<float>, the reference's operation order).  A
# running error bound: an expression whose longest path holds n rounded operations is evaluated within n * U32 of the same expression
# with every operand replaced by its absolute value (first order; the second-order terms are 1e-7 of that).
ICP_OPS_ROTATE = 4                # R * v, per component: a product, minus the product of the imaginary parts, two additions
ICP_OPS_TRANSFORM = 5             # R * v + t: the translation on top
ICP_OPS_CROSS = 3                 # a_y b_z - a_z b_y: a complex product (two roundings) and the difference
ICP_OPS_DOT = 5                   # n . (d - s): the difference, a complex product, two additions
ICP_OPS_PRODUCT = 2               # row_i * row_j: the product and the product of the imaginary parts taken off it
ICP_DEVICE = 2                    # a division or square root that the device may round one ulp away from the reference's counts twice
# The gates compare Re sqrt(sum of three complex squares): each square is two roundings, two additions follow — four relative
# roundings of the square, two of its root — and the complex square root is five library operations (hypot, sqrt, atan2, cos, a
# product: oc_complex.hpp / xs_complex.h), each of which may differ by an ulp between host and device: 2 + 5 * ICP_DEVICE.
ICP_OPS_NORM = 2 + 5 * ICP_DEVICE


def _abs_cross(a, b):
    """|a x b| with every operation replaced by the sum of its operands' absolute values (a, b >= 0, [3, n])."""
    return np.stack([a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]])


def icp_bounds(dec, cols, y0, y1):
    """(sum_p m_i m_j [27], sum_p (m_i dm_j + dm_i m_j) [27]) over the inliers of rows [y0, y1) from the per-pixel magnitude bounds of an
    evaluation with margins=True, in the order of the sums."""
    pr = np.arange(dec["ok"].size) // cols
    sel = dec["ok"] & (pr >= y0) & (pr < y1)
    m, dm = dec["m"][:, sel], dec["dm"][:, sel]
    pairs = [(i, j) for i in range(6) for j in range(i, 7)]
    return (np.array([np.dot(m[i], m[j]) for i, j in pairs]), np.array([np.dot(m[i], dm[j]) + np.dot(dm[i], m[j]) for i, j in pairs]))


def icp_normal_equations(d, h, Rcurr, tcurr, vmap_curr, nmap_curr, Rprev_inv, tprev, intr, vmap_prev, nmap_prev, dist_thres,
                         angle_thres, dec=None, y0=0, y1=None, margins=False):
    """The current pixels of rows [y0, y1) of one pyramid level (association ranges over the whole model map).  Maps: [3 * rows, cols, 2].
    Returns (sums[27] in the kernel's order i = 0..5, j = i..6 of row_i * row_j, inliers, dec).  dec (whole image, whatever the range):
    'ok' the inliers, 'branch' the pixels each rejection test removes (in the kernel's order, each among those that reached it), and with
    margins=True
      'fragile'  current pixels with a valid normal of which one decision — the two roundings rint(u), rint(v) (the four image bounds are
                 among their half-integers), cpz < 0, the distance gate, the angle gate — lies within the float32 evaluation error of its
                 boundary (derivations at the statements below; sized for the reference's float32 evaluation, ICP_DEVICE for the device);
      'm', 'dm'  [7, pixels]: m_i >= |row_i| formed with every operation replaced by the sum of its operands' absolute values (so the
                 cancellation in d - s and in the cross products does not shrink it), and the same bound of the tangent d row_i / d seed."""
    fx, fy, cx, cy = (float(F32(v)) for v in intr)
    rows, cols = vmap_curr.shape[0] // 3, vmap_curr.shape[1]
    y1 = rows if y1 is None else y1
    planes = lambda m: lin(np.asarray(m).reshape(3, rows, cols, 2), d, h).reshape(3, -1)
    vc, nc, vp, npv = planes(vmap_curr), planes(nmap_curr), planes(vmap_prev), planes(nmap_prev)
    Rc = lin(np.asarray(Rcurr).reshape(3, 3, 2), d, h)
    tc = lin(np.asarray(tcurr).reshape(3, 2), d, h)
    Rpi = lin(np.asarray(Rprev_inv).reshape(3, 3, 2), d, h)
    tp = lin(np.asarray(tprev).reshape(3, 2), d, h)
    with np.errstate(invalid="ignore", divide="ignore"):
        vg = Rc @ vc + tc[:, None]                                       # :212
        vcp = Rpi @ (vg - tp[:, None])                                   # :213
        if dec is None:
            assert d == 0.0
            valid = ~np.isnan(nc[0])                                     # :202-204
            fu, fv = vcp[0] * fx / vcp[2] + cx, vcp[1] * fy / vcp[2] + cy
            ux, uy = np.rint(fu), np.rint(fv)                            # :216-217 __float2int_rn
            fin = np.isfinite(ux) & np.isfinite(uy)
            sides = dict(left=ux < 0, right=ux >= cols, top=uy < 0, bottom=uy >= rows, behind=vcp[2] < 0)
            ok = valid & fin & ~np.logical_or.reduce(list(sides.values()))   # :218-220
            idx = (np.where(ok, uy, 0).astype(np.int64) * cols + np.where(ok, ux, 0).astype(np.int64))
            inb = ok.copy()
            ok &= ~np.isnan(npv[0][idx])                                 # :222-224
            dec = dict(idx=idx, branch=dict(nan_normal=~valid, hole=inb & ~ok, **{k: valid & fin & v for k, v in sides.items()}))
        idx = dec["idx"]
        n_prev, v_prev = npv[:, idx], vp[:, idx]
        if "ok" not in dec:
            thr_d, thr_a = float(F32(dist_thres)), float(F32(angle_thres))
            dist = np.sqrt(((v_prev - vg) ** 2).sum(0))                  # :232-234
            far = dist > thr_d
            ncg = Rc @ nc                                                # :235
            sine = np.sqrt((np.cross(ncg.T, n_prev.T) ** 2).sum(-1))     # :236-238
            tilted = sine >= thr_a
            dec["branch"].update(far=ok & far, tilted=ok & ~far & tilted)
            dec["ok"] = ok & ~far & ~tilted & np.isfinite(dist) & np.isfinite(sine)
            if margins:
                A = np.abs
                tan = lambda m, shape: A(np.asarray(m, np.float64).reshape(*shape, 2)[..., 1] / h).reshape(shape[0], -1)
                aR, aRp = A(Rc), A(Rpi)
                # s = Rcurr * v + t: ICP_OPS_TRANSFORM roundings on mag_g; cp = Rprev_inv * (s - tprev): one more for the difference and
                # ICP_OPS_ROTATE for the rotation, on mag_cp
                mag_g = aR @ A(vc) + A(tc)[:, None]
                e_g = ICP_OPS_TRANSFORM * U32 * mag_g
                mag_cp = aRp @ (mag_g + A(tp)[:, None])
                e_cp = (ICP_OPS_TRANSFORM + 1 + ICP_OPS_ROTATE) * U32 * mag_cp
                az = A(vcp[2])
                # u = cpx * fx / cpz + cx: the errors of cpx and cpz through the quotient q, the product and the division
                # ((1 + ICP_DEVICE) roundings of q), and the addition (one rounding of |q| + |cx|).  rint flips where u lies this
                # close to a half-integer; -1/2 and cols - 1/2 (rows - 1/2) are the image bounds.
                def pix_err(k, f, c0):
                    q = A(vcp[k] * f / vcp[2])
                    return f / az * e_cp[k] + q / az * e_cp[2] + (1 + ICP_DEVICE) * U32 * q + U32 * (q + abs(c0))
                near_half = lambda f, e: A(f - (np.floor(f) + 0.5)) <= e
                frag = ~fin | near_half(fu, pix_err(0, fx, cx)) | near_half(fv, pix_err(1, fy, cy))
                frag |= az <= e_cp[2]                                    # cpz < 0
                # |d - s|: each component of the difference carries s's error and one rounding of |d| + mag_g; the root of the sum
                # of squares moves by at most the length of that error vector (Cauchy-Schwarz, whatever the cancellation), plus
                # ICP_OPS_NORM roundings of the root itself
                e_d = e_g + U32 * (A(v_prev) + mag_g)
                frag_gate = A(dist - thr_d) <= np.sqrt((e_d ** 2).sum(0)) + ICP_OPS_NORM * U32 * dist
                # |Rcurr n x n_prev|: ICP_OPS_ROTATE roundings on mag_n, through the cross product (n_prev is exact) plus its own
                # ICP_OPS_CROSS roundings
                mag_n = aR @ A(nc)
                e_c = _abs_cross(ICP_OPS_ROTATE * U32 * mag_n, A(n_prev)) + ICP_OPS_CROSS * U32 * _abs_cross(mag_n, A(n_prev))
                frag_gate |= A(sine - thr_a) <= np.sqrt((e_c ** 2).sum(0)) + ICP_OPS_NORM * U32 * sine
                dec["fragile"] = valid & (frag | (ok & frag_gate))
                # magnitude bounds of the rows: row[0:3] = s x n, row[3:6] = n, row[6] = n . (d - s); tangents by the product rule
                dmag_g = tan(Rcurr, (3, 3)).reshape(3, 3) @ A(vc) + aR @ tan(vmap_curr, (3, rows, cols)) + tan(tcurr, (3,)).reshape(3)[:, None]
                an, ad = A(n_prev), A(v_prev)
                dn, dd_ = tan(nmap_prev, (3, rows, cols))[:, idx], tan(vmap_prev, (3, rows, cols))[:, idx]
                dec["m"] = np.concatenate([_abs_cross(mag_g, an), an, (an * (ad + mag_g)).sum(0)[None]])
                dec["dm"] = np.concatenate([_abs_cross(dmag_g, an) + _abs_cross(mag_g, dn), dn,
                                            (dn * (ad + mag_g) + an * (dd_ + dmag_g)).sum(0)[None]])
        pr = np.arange(rows * cols) // cols
        ok = dec["ok"] & (pr >= y0) & (pr < y1)
        s, nn, dd = vg[:, ok], n_prev[:, ok], v_prev[:, ok]              # :239-242: n = n_prev_g, d = p_prev_g, s = p_curr_g
        row = np.empty((7, s.shape[1]))
        row[0:3] = np.cross(s.T, nn.T).T                                 # :256
        row[3:6] = nn                                                    # :257
        row[6] = (nn * (dd - s)).sum(0)                                  # :258
    sums = np.array([np.dot(row[i], row[j]) for i in range(6) for j in range(i, 7)])   # :266-279
    return sums, int(ok.sum()), dec


# ------------------------------------------------------------------------------------------------
# Dual-complex local-TSDF residual — ComputeLocalTsdfHessianKernel, XKinectFusion/src/TsdfFusion.cu:204-283
def seeded_pose(p, h, Rv2c, tv2c):
    """The real pose at seed offsets p = (p1, p2) of packed groups Rv2c [3, 3, k], tv2c [3, k]: k = 4 dual-complex (re.re, re.im, im.re,
    im.im): x = re.re + p1 * re.im / h + p2 * im.re / h + p1 * p2 * im.im / h^2; k = 2 complex (re, im): x = re + p1 * im / h.  A scalar p
    is (p, 0)."""
    p1, p2 = (p, 0.0) if np.ndim(p) == 0 else p
    out = []
    for a, shape in ((Rv2c, (3, 3)), (tv2c, (3,))):
        q = np.asarray(a, np.float64).reshape(*shape, -1)
        x = q[..., 0] + (p1 / h) * q[..., 1]
        if q.shape[-1] == 4:
            x = x + (p2 / h) * q[..., 2] + (p1 * p2 / h / h) * q[..., 3]
        else:
            assert q.shape[-1] == 2 and p2 == 0.0
        out.append(x)
    return out


def tsdf_residuals(p, h, Rv2c, tv2c, gt_planes, depth_m, intr, voxel_size, trunc, z0=0, dec=None):
    """Per-voxel form of tsdf_residual_loss: (error [n], use [n], dec) over the band voxels dec['xyz'] [n, 3] of gt_planes; error is
    meaningful where use holds (the voxels the kernel sums)."""
    R, t = seeded_pose(p, h, Rv2c, tv2c)
    fx, fy, cx, cy = (float(F32(v)) for v in intr)
    vs, tr = float(F32(voxel_size)), float(F32(trunc))
    rows, cols = depth_m.shape
    if dec is None:
        assert np.all(np.asarray(p) == 0.0)
        g = np.asarray(gt_planes, np.float64)
        band = (g != 0) & ~(np.abs(g) > 0.95)                            # :221-223
        zz, yy, xx = np.nonzero(band)
        dec = dict(xyz=np.stack([xx, yy, zz + z0], -1), gt=g[band])
    xyz, g = dec["xyz"], dec["gt"]
    vg = (xyz.astype(np.float64) + 0.5) * vs                             # :224-227
    vc = vg @ R.T + t                                                    # :228
    inv_z = 1.0 / vc[:, 2]                                               # :229
    ix = vc[:, 0] * inv_z * fx + cx                                      # :232-233
    iy = vc[:, 1] * inv_z * fy + cy
    if "keep" not in dec:
        keep = ~(inv_z < 0)                                              # :230-231
        coox, cooy = np.floor(ix - 0.5).astype(np.int64), np.floor(iy - 0.5).astype(np.int64)    # :234-235
        keep &= (coox > 1) & (cooy > 1) & (coox < cols - 1) & (cooy < rows - 1)                  # :236-237
        dec.update(coox=coox, cooy=cooy, nx=np.rint(ix).astype(np.int64), ny=np.rint(iy).astype(np.int64))
        dd = [_gather2d(depth_m, cooy + j, coox + i) for j in (0, 1) for i in (0, 1)]
        dec["bil"] = (dd[0] != 0) & (dd[1] != 0) & (dd[2] != 0) & (dd[3] != 0)                  # :248-251 (threshold unused)
        dec["keep"] = keep
    coox, cooy = dec["coox"], dec["cooy"]
    d00, d10 = _gather2d(depth_m, cooy, coox).astype(np.float64), _gather2d(depth_m, cooy, coox + 1).astype(np.float64)
    d01, d11 = _gather2d(depth_m, cooy + 1, coox).astype(np.float64), _gather2d(depth_m, cooy + 1, coox + 1).astype(np.float64)
    a, b = ix - (coox + 0.5), iy - (cooy + 0.5)                          # :253-254
    inter = d00 * (1 - a) * (1 - b) + d10 * a * (1 - b) + d01 * (1 - a) * b + d11 * a * b
    Dp = np.where(dec["bil"], inter, _gather2d(depth_m, dec["ny"], dec["nx"]).astype(np.float64))
    xl, yl = (ix - cx) / fx, (iy - cy) / fy                              # :262-263
    dist = np.sqrt((Dp * xl) ** 2 + (Dp * yl) ** 2 + Dp ** 2) - np.sqrt((vc ** 2).sum(-1))    # :264-267
    err = (dist - g * tr) / tr                                           # :268-269
    if "use" not in dec:
        dec["use"] = dec["keep"] & ~((Dp > 5) | (Dp < 0.2)) & ~(np.abs(err) > 1)                # :260, :271
    return err, dec["use"], dec


def tsdf_residual_loss(p, h, Rv2c, tv2c, gt_planes, depth_m, intr, voxel_size, trunc, z0=0, dec=None):
    """sum over the voxels of gt_planes ([nz, Y, X]: planes z0 .. z0 + nz of the map, as the C ABI takes a slab) of error(p)^2,
    error = (|Dp (xl, yl, 1)| - |v_c| - gt * trunc) / trunc, for the pose seeded_pose(p, h, Rv2c, tv2c) (Rv2c [3, 3, 4], tv2c [3, 4]
    dual-complex groups; p a scalar or the two offsets (p1, p2)).  Returns (loss, count, dec)."""
    err, use, dec = tsdf_residuals(p, h, Rv2c, tv2c, gt_planes, depth_m, intr, voxel_size, trunc, z0, dec)
    return float((err[use] ** 2).sum()), int(use.sum()), dec             # :274-280 + the four reductions :317-324


def gn_terms(Rv2c6, tv2c6, gt_planes, depth_m, intr, voxel_size, trunc, z0=0, h=1e-7, fd=1e-6):
    """The 29 Gauss-Newton sums of the same residual for six complex poses (Rv2c6 [6, 3, 3, 2], tv2c6 [6, 3, 2]) that share one real
    part: d_k = h * (r_k(+fd) - r_k(-fd)) / 2 fd, the central difference of pose k's real residual along its imaginary part; out =
    sum d_j d_k (j <= k, row-major: 21), sum d_k r (6), sum r^2, count, over the voxels that pass the gates at the shared real pose."""
    Rs = np.asarray(Rv2c6, np.float32).reshape(6, 3, 3, 2)
    ts = np.asarray(tv2c6, np.float32).reshape(6, 3, 2)
    assert np.all(Rs[..., 0] == Rs[0, ..., 0]) and np.all(ts[..., 0] == ts[0, ..., 0])
    args = (gt_planes, depth_m, intr, voxel_size, trunc, z0)
    e0, use, dec = tsdf_residuals(0.0, h, Rs[0], ts[0], *args)
    D = np.empty((6, int(use.sum())))
    for k in range(6):
        ep = tsdf_residuals(+fd, h, Rs[k], ts[k], *args, dec=dec)[0]
        em = tsdf_residuals(-fd, h, Rs[k], ts[k], *args, dec=dec)[0]
        D[k] = (h * (ep - em) / (2 * fd))[use]
    r = e0[use]
    return np.array([D[j] @ D[k] for j in range(6) for k in range(j, 6)] + [D[k] @ r for k in range(6)] + [r @ r, float(use.sum())])


def central(f, step):
    """(value at 0, first, second central difference) of a scalar- or array-valued f(d, dec) -> (value, dec)."""
    f0, dec = f(0.0, None)
    fp, _ = f(+step, dec)
    fm, _ = f(-step, dec)
    return f0, (fp - fm) / (2 * step), (fp - 2 * f0 + fm) / (step * step), dec


# ------------------------------------------------------------------------------------------------
# Map preparation — XKinectFusion/src/Map.cu.  Images are [rows, cols]; vertex / normal maps [3, rows, cols] (x, y, z planes).
SIGMA_SPACE2_INV_HALF = F32(0.5) / (F32(4.5) * F32(4.5))                 # :5, :267 (float32 constants, as the launcher forms them)
SIGMA_COLOR2_INV_HALF = F32(0.5) / (F32(30) * F32(30))                   # :4, :268


def _window(img, r, fill=0):
    """For every shift (dy, dx) in [-r, r]^2, rows outer as the kernels' loops run: (dy, dx, tap, visited).  tap[y, x] = img[y + dy, x + dx];
    visited where the clipped loops of bilateralKernel / pyrDownKernel reach it: 0 <= cy < rows - 1 and 0 <= cx < cols - 1 (the upper
    bound min(y - D/2 + D, rows - 1) is exclusive, :172-179 and :213-221: the last row and column are never read)."""
    rows, cols = img.shape
    pad = np.full((rows + 2 * r, cols + 2 * r), fill, img.dtype)
    pad[r:r + rows, r:r + cols] = img
    yy, xx = np.mgrid[0:rows, 0:cols]
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            cy, cx = yy + dy, xx + dx
            yield dy, dx, pad[r + dy:r + dy + rows, r + dx:r + dx + cols], (cy >= 0) & (cy < rows - 1) & (cx >= 0) & (cx < cols - 1)


def bilateral(depth_u16, band=None):
    """bilateralKernel :155-191 before the conversion to an integer: (q, amin), q = sum tmp * w / sum w in float64 over the taps visited,
    w = exp(-(space2 * sigma_space2_inv_half + color2 * sigma_color2_inv_half)), amin = the smallest exponent argument over those taps
    (where it is large every float32 weight is 0 and the kernel divides 0 by 0).  band = (lo, hi): also the number of visited taps
    per pixel whose argument lies in (lo, hi).  The colour distance is taken as the number (value - tmp)^2."""
    v = np.asarray(depth_u16).astype(np.float64)
    s1, s2 = np.zeros(v.shape), np.zeros(v.shape)
    amin = np.full(v.shape, np.inf)
    nband = np.zeros(v.shape, np.int64)
    for dy, dx, tmp, vis in _window(v, 6):
        arg = (dx * dx + dy * dy) * float(SIGMA_SPACE2_INV_HALF) + (v - tmp) ** 2 * float(SIGMA_COLOR2_INV_HALF)   # :182-186
        w = np.where(vis, np.exp(-arg), 0.0)
        s1 += tmp * w                                                    # :188-189
        s2 += w
        amin = np.where(vis, np.minimum(amin, arg), amin)
        if band is not None:
            nband += vis & (arg > band[0]) & (arg < band[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        q = s1 / s2
    return (q, amin) if band is None else (q, amin, nband)


def bilateral_f32(depth_u16):
    """The same quotient with every operation of :180-192 rounded to float32 and the taps added in the kernel's order (rows outer,
    columns inner) — one legitimate float32 evaluation, the measure of how far such evaluations may lie from bilateral()'s q."""
    v = np.asarray(depth_u16).astype(np.int64)
    s1, s2 = np.zeros(v.shape, F32), np.zeros(v.shape, F32)
    with np.errstate(under="ignore"):
        for dy, dx, tmp, vis in _window(v, 6):
            space2 = F32(dx * dx + dy * dy)
            color2 = ((v - tmp) ** 2).astype(F32)
            w = np.exp(-(space2 * SIGMA_SPACE2_INV_HALF + color2 * SIGMA_COLOR2_INV_HALF))
            assert w.dtype == F32
            s1 = np.where(vis, s1 + tmp.astype(F32) * w, s1)
            s2 = np.where(vis, s2 + w, s2)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (s1 / s2).astype(np.float64)


def bilateral_post(r):
    """:192-196 on an integer candidate r = __float2int_rn(sum1 / sum2): 0 outside [200, 5000] mm, then the clamp to a short."""
    r = np.asarray(r, np.int64)
    r = np.where((r > 5000) | (r < 200), 0, r)
    return np.clip(r, 0, 32767)


def pyr_down(depth_re):
    """pyrDownKernel :202-230, exact: int64 [rows // 2, cols // 2] from the real parts of the source (any float values)."""
    r = np.rint(np.asarray(depth_re, np.float64)).astype(np.int64)      # :211, :222 __float2int_rn, ties to even
    srows, scols = r.shape
    drows, dcols = srows // 2, scols // 2                                # :275
    sel = (slice(0, 2 * drows, 2), slice(0, 2 * dcols, 2))               # the window of (y, x) is centred on source pixel (2y, 2x)
    center = r[sel]
    s, n = np.zeros((drows, dcols), np.int64), np.zeros((drows, dcols), np.int64)
    for dy, dx, val, vis in _window(r, 2):
        use = vis[sel] & (np.abs(val[sel] - center) < 90)               # :223 |val - center| < 3 * sigma_color
        s += np.where(use, val[sel], 0)
        n += use
    return np.sign(s) * (np.abs(s) // n)                                 # :228 C integer division


def vertex_map(intr, depth_c):
    """computeVmapKernel :8-29 for a complex depth [rows, cols, 2] in mm: (value [3, rows, cols], first-order part [3, rows, cols],
    sentinel [rows, cols]).  Every operation is linear in z, so the imaginary part passes through the same factors."""
    fx, fy, cx, cy = (float(F32(v)) for v in intr)
    d = np.asarray(depth_c, np.float64)
    rows, cols = d.shape[:2]
    z, dz = d[..., 0] / 1000.0, d[..., 1] / 1000.0                       # :16
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    kx, ky = (u - cx) / fx, (v - cy) / fy                                # :19-20
    return np.stack([z * kx, z * ky, z]), np.stack([dz * kx, dz * ky, dz]), z == 0   # :18 tests the real part only


def _at(m, dtype):
    m = np.asarray(m)
    rows = m.shape[0] // 3
    m = m.reshape(3, rows, m.shape[1], 2).astype(dtype)
    return m[..., 0], m[..., 1]


def _norm3(v):
    return np.sqrt((v * v).sum(0))


def normal_map(vmap, d=0.0, h=1.0, dtype=np.float64):
    """computeNmapKernel :32-70 on the vertex map as given ([3 * rows, cols, 2] float32): (normal [3, rows, cols], sentinel [rows, cols],
    kappa [rows, cols], dscale [rows, cols]).  The three taps are taken at Re + d * Im / h; d is a scalar or one offset per output
    pixel [rows, cols].  kappa = |a| |b| / |a x b| (a = v01 - v00, b = v10 - v00) is the condition number of the direction; dscale =
    (|v01'| + |v00'|) / |a| + (|v10'| + |v00'|) / |b| with v' = Im / h is the size of the relative change of the two edges per unit seed."""
    re, im = _at(vmap, dtype)
    rows, cols = re.shape[1:]
    sh = lambda a, dy, dx: np.pad(a, ((0, 0), (0, dy), (0, dx)), constant_values=np.nan)[:, dy:dy + rows, dx:dx + cols]
    k = np.asarray(d, dtype) / dtype(h)
    tap = lambda dy, dx: sh(re, dy, dx) + k * sh(im, dy, dx)
    v00, v01, v10 = tap(0, 0), tap(0, 1), tap(1, 0)                      # :47-58
    nan = lambda dy, dx: np.isnan(sh(re, dy, dx)[0])
    sentinel = nan(0, 0) | nan(0, 1) | nan(1, 0)                         # :51 (x plane only), and :41 the last row / column (padded NaN)
    with np.errstate(invalid="ignore", divide="ignore"):
        a, b = v01 - v00, v10 - v00
        m = np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])   # :60 cross
        n = m / _norm3(m)                                                # :60 normalized
        kappa = _norm3(a) * _norm3(b) / _norm3(m)
        dn = lambda dy, dx: _norm3(sh(im, dy, dx)) / abs(dtype(h))
        dscale = (dn(0, 1) + dn(0, 0)) / _norm3(a) + (dn(1, 0) + dn(0, 0)) / _norm3(b)
    return n, sentinel, kappa, dscale


def resize(m, normalize, d=0.0, h=1.0, dtype=np.float64):
    """resizeMapKernel<normalize> :105-152 on a map [3 * srows, cols, 2]: (out [3, srows // 2, scols // 2], sentinel, mag, dmag).
    out = the mean of the 2 x 2 block of each plane (then normalized); the sentinel is set if any of the four x-plane entries is NaN
    (:124-127).  mag [3, ...] = sum |x_i| / 4 per component and dmag the same of the first-order parts Im / h: the sizes the
    rounding of the three additions is relative to.  d: a scalar or one offset per output pixel."""
    re, im = _at(m, dtype)
    drows, dcols = re.shape[1] // 2, re.shape[2] // 2                    # :238-239: an odd source drops its last row / column
    blk = lambda a: [a[:, i:2 * drows:2, j:2 * dcols:2] for i in (0, 1) for j in (0, 1)]   # x00 x01 x10 x11
    k = np.asarray(d, dtype) / dtype(h)
    taps = [r + k * i for r, i in zip(blk(re), blk(im))]
    sentinel = np.isnan(np.stack([t[0] for t in blk(re)])).any(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (taps[0] + taps[1] + taps[2] + taps[3]) / dtype(4)         # :131, :138, :145
        mag = sum(np.abs(t) for t in blk(re)) / dtype(4)
        dmag = sum(np.abs(t) for t in blk(im)) / dtype(4) / abs(dtype(h))
        if normalize:
            out = out / _norm3(out)                                      # :146-147
    return out, sentinel, mag, dmag


def central4(f, step):
    """Fourth-order central difference (-f(2s) + 8 f(s) - 8 f(-s) + f(-2s)) / 12 s of an array-valued f(d); s may hold one step per
    element.  The map kernels' derivatives are checked to a few float32 ulps times the condition number: the second-order stencil
    cannot be both that exact and above float64 round-off where kappa reaches the hundreds."""
    return (-f(2 * step) + 8 * f(step) - 8 * f(-step) + f(-2 * step)) / (12 * step)
