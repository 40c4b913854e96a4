"""Cases and models for xs_tsdf_register_terms (x-slam_amd/csrc/xs_register.hip), shared by
tests/test_register_cases_cpu.py, tests/test_register_gpu.py and tests/test_register_pipeline_gpu.py.

THE MODEL is the contract of include/xslam_amd.h in numpy float32, written from the header and not from the kernel.  The transformed point P,
the status, the residual r and the gradient g are sample_cases.sample_points' (imported, not restated: the contract declares them the bytes
xs_tsdf_sample_points writes); J[3..5] = P x g is two float32 products and one float32 subtraction each; the 29 terms of a kept point are
exact double products of float32 factors.  The sums are formed two ways: chunk_sums() in the kernel's own order in float64 (lane l of wave w
of workgroup b adds the points 64 c + l of its chunks c = 4 b + w, + 4 nblocks, ... in that order; the 64 lanes by wave_sum_f64's shuffle-down
tree; the four waves in wave order; the workgroups' records g, g + 8, ... per group and then the eight groups in order:
block_fold_and_finish_of<29>), and fsum_sums() with math.fsum, which knows no order.  A correct kernel produces the model's float32 r and J
bit for bit, so its count is the model's and its other sums differ from chunk_sums' by the association of at most n double additions.

THE TWIN redoes the same operations in float64 on the float32 inputs, on the model's own keep / drop decisions.

THE BOUND between the two (bound()): sample_cases.bounds gives, per case, Ep >= |P32 - P64|, bv >= |r32 - r64| and bg >= |g32 - g64| (per
component) wherever both precisions give the same status, which the cases require of every kept point.  On top of it, by the running error
analysis of align_cases (u = 2^-24; z = x y: e_z = (|x| e_y + |y| e_x + e_x e_y)(1 + u) + u |z|; z = x - y: e_z = (e_x + e_y)(1 + u) + u |z|):
J[0..2] carry bg, J[3..5] the two products and the difference of their own magnitudes, r carries bv; a term p q formed exactly in double
differs by at most |p| e_q + |q| e_p + e_p e_q; the double additions of either side add n 2^-52 sum |terms|.  Nothing is fitted.

Conditions on the cases (test_register_cases_cpu.py asserts them; the seed of a case's points is bumped until they hold): in every case with
n >= 255 each of the three gates drops at least one point and at least one point is kept; every kept point is OK with an accepted gradient in
the twin too; no point has |r| within 2^-22 of max_residual without being EQUAL to it.  Points whose |r| equals max_residual bit for bit are
wanted, not forbidden: the identity cases plant voxels holding exactly +-max_residual with seen neighbours and put points on their centres,
where F returns the stored word and P = p exactly, so the gate "fabsf(r) > max_residual" keeps them and a gate written ">=" drops them.  Both
precisions and the kernel decide such a point alike; a point a rounding away from the threshold is what the condition excludes.

MUTANTS: mistakes a kernel could make, each of which must change a sum of some case beyond the GPU test's tolerance."""
import functools
import math

import numpy as np

import render_cases as rc
import sample_cases as sc

U, ALLOW, F32 = sc.U, sc.ALLOW, np.float32
NEAR = 2.0 ** -22
# J[3..5] from p instead of P; a sign of the cross product flipped; rotation slots before translation slots; the residual gate as >=; a point with a
# refused gradient kept with g = 0; the last chunk's tail counted (its lanes read the last point again); a row offset taken modulo 2^32
MUTANTS = ("J_from_p", "cross_sign", "rot_first", "gate_ge", "grad_zero", "tail", "row_wrap32")
MAX_BLOCKS = 4096
BIG_N = 1064960           # 16640 chunks: 4160 workgroups' worth, past one round of the 4096-workgroup grid
# The model's loop and the twin's loop on loop_scene() (ten iterations) ended 1.38e-07 m apart at the worst corner of the 24^3 volume when this
# was written (printed by test_register_cases_cpu.py::test_twin_loop; 2.8e-6 voxel edges).  The bound is four times that: it rests on the
# conditioning of this scene's normal equations, which nothing else measures.  A sphere does not constrain the rotation about its centre: the
# damping alone holds those three directions, and they are where the two loops drift apart.  The GPU's loop
# (tests/test_register_pipeline_gpu.py), whose sums differ from the model's by association only, is held to the same figure against the model's.
LOOP_AGREEMENT_M = 5.6e-7


# ------------------------------------------------------------------------------------------------
# The per-point contract
def point_terms(case, dtype=np.float32, mutant=None, keep=None, pts=None, xform=None):
    """r, J [6] and the keep / drop decisions of every point of `case` (or of pts under xform on its volume).  keep: decisions to use instead
    of this precision's own (the twin)."""
    T = dtype
    pts = case["pts"] if pts is None else pts
    xform = case["xform"] if xform is None else xform
    s = sc.sample_points(case["vol"], case["vs"], pts, xform, case["min_weight"], None, T, "row_wrap32" if mutant == "row_wrap32" else None, case["pitch"])
    P, r = s["P"], s["value"]
    ok, gok = s["status"] == sc.OK, s["gok"]
    g = [s["gradient"][:, c] for c in range(3)]
    mr = T(F32(case["max_residual"]))
    with np.errstate(invalid="ignore", over="ignore"):
        over = (np.abs(r) >= mr) if mutant == "gate_ge" else (np.abs(r) > mr)
        if mutant == "grad_zero":
            g = [np.where(gok, gc, T(0)) for gc in g]
        refused = np.zeros_like(ok) if mutant == "grad_zero" else ok & ~gok
        kept = ok & ~refused & ~over
        if keep is not None:
            kept = keep
        Q = [np.asarray(pts, np.float32).reshape(-1, 3)[:, c].astype(T) for c in range(3)] if mutant == "J_from_p" else P
        J3 = Q[1] * g[2] - Q[2] * g[1]
        J4 = (Q[0] * g[2] - Q[2] * g[0]) if mutant == "cross_sign" else (Q[2] * g[0] - Q[0] * g[2])
        J5 = Q[0] * g[1] - Q[1] * g[0]
    J = [J3, J4, J5] + g if mutant == "rot_first" else g + [J3, J4, J5]
    return dict(r=r, J=J, P=P, kept=kept, status_drop=~ok, gradient_drop=ok & ~gok, residual_drop=ok & gok & over, ok=ok, gok=gok, sample=s)


def terms29(pt):
    """The 29 double terms of every point [n, 29]; zero rows for dropped points (adding +0.0 changes no bit of a sum that is never -0.0)."""
    kept = pt["kept"]
    J = [np.where(kept, j, 0).astype(np.float64) for j in pt["J"]]
    r = np.where(kept, pt["r"], 0).astype(np.float64)
    cols = [J[j] * J[k] for j in range(6) for k in range(j, 6)] + [J[k] * r for k in range(6)] + [r * r, kept.astype(np.float64)]
    return np.stack(cols, axis=1)


def nblocks_of(n):
    nchunks = (n + 63) // 64
    return int(min(max((nchunks + 3) // 4, 1), MAX_BLOCKS))


def chunk_sums(terms, tail=False):
    """The 29 sums in the kernel's order, float64.  tail: the last chunk's missing lanes add the last point's terms again (the tail mutant)."""
    n = len(terms)
    nchunks = (n + 63) // 64
    nb = nblocks_of(n)
    rounds = -(-nchunks // (4 * nb))
    a = np.zeros((rounds * 4 * nb * 64, 29), np.float64)
    a[:n] = terms
    if tail:
        a[n:nchunks * 64] = terms[n - 1]
    a = a.reshape(rounds, 4 * nb, 64, 29)
    acc = np.zeros((4 * nb, 64, 29), np.float64)
    for k in range(rounds):                      # a lane's chunks, in order
        acc = acc + a[k]
    for half in (32, 16, 8, 4, 2, 1):            # wave_sum_f64: v[l] += v[l + off], lane 0's result
        acc = acc[:, :half] + acc[:, half:2 * half]
    w = acc.reshape(nb, 4, 29)
    rec = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    G = 8                                        # 256 threads / 32 doubles per record
    pad = np.zeros((-(-nb // G) * G, 29), np.float64)
    pad[:nb] = rec
    pad = pad.reshape(-1, G, 29)
    s = np.zeros((G, 29), np.float64)
    for k in range(pad.shape[0]):                # thread (g, c): records g, g + G, ... in order
        s = s + pad[k]
    out = s[0]
    for gidx in range(1, G):
        out = out + s[gidx]
    return out


def fsum_sums(terms):
    return np.array([math.fsum(terms[:, k]) for k in range(29)])


def tolerance(terms):
    """What the association of at most n double additions can change: n 2^-52 sum |terms| per sum (0 for the count, which is exact)."""
    t = len(terms) * 2.0 ** -52 * np.abs(terms).sum(axis=0)
    t[28] = 0.0
    return t


def _ep_of(case):
    if case["xform"] is None:
        return 0.0
    m = np.abs(case["xform"].astype(np.float64))
    p = np.abs(case["base_pts"].astype(np.float64))
    return 4 * U * max(float((m[3 * c] * p[:, 0] + m[3 * c + 1] * p[:, 1] + m[3 * c + 2] * p[:, 2] + m[9 + c]).max()) for c in range(3))


def bound(case, m32, m64):
    """The bound on |model sums - twin sums| of the module docstring, per sum (0 for the count)."""
    kept = m32["kept"]
    bcase = dict(case, pts=case["base_pts"])
    bv, _, bg = sc.bounds(bcase, m64["sample"])
    Ep = _ep_of(case)

    def mag(a, b):
        return np.maximum(np.abs(np.where(kept, a, 0).astype(np.float64)), np.abs(np.where(kept, b, 0).astype(np.float64)))
    P = [mag(m32["P"][c], m64["P"][c]) + Ep for c in range(3)]
    g = [mag(m32["J"][c], m64["J"][c]) + bg for c in range(3)]

    def prod_e(x, ex, y, ey):
        return (x * ey + y * ex + ex * ey) * (1 + U) + U * x * y

    def cross_e(a, b, jmag):     # P[a] g[b] - P[b] g[a]
        return (prod_e(P[a], Ep, g[b], bg) + prod_e(P[b], Ep, g[a], bg)) * (1 + U) + U * jmag
    Jm = [mag(m32["J"][k], m64["J"][k]) for k in range(6)]
    eJ = [np.full(len(kept), bg)] * 3 + [cross_e(1, 2, Jm[3] + 1), cross_e(2, 0, Jm[4] + 1), cross_e(0, 1, Jm[5] + 1)]
    rm, er = mag(m32["r"], m64["r"]), np.full(len(kept), bv)
    k = kept.astype(np.float64)

    def term_e(p, ep, q, eq):
        return float(((p * eq + q * ep + ep * eq) * k).sum())
    out = [term_e(Jm[j], eJ[j], Jm[i], eJ[i]) for j in range(6) for i in range(j, 6)] + [term_e(Jm[i], eJ[i], rm, er) for i in range(6)] + [term_e(rm, er, rm, er), 0.0]
    t64 = terms29(m64)
    return ALLOW * (np.array(out) + 2 * tolerance(t64))


# ------------------------------------------------------------------------------------------------
# The cases
def _plant(vol, mr, min_weight, rng, count=6):
    """Copies of (value, weight) with `count` interior voxels holding exactly +-mr among neighbours of weight 5: (vol, their indices [count, 3])."""
    value, weight = vol[0].copy(), vol[1].copy()
    Z, Y, X = value.shape
    idx = []
    while len(idx) < count:
        x, y, z = (int(rng.integers(2, s - 2)) for s in (X, Y, Z))
        if any(max(abs(x - a), abs(y - b), abs(z - c)) <= 2 for a, b, c in idx):
            continue
        weight[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2] = 5
        value[z, y, x] = F32(mr) if len(idx) % 2 == 0 else -F32(mr)
        idx.append((x, y, z))
    return (value, weight), np.array(idx)


def _conditions(case, m):
    """(the three gates' drop counts, kept, near-threshold points)"""
    r = np.abs(m["r"][m["ok"] & m["gok"]].astype(np.float64))
    d = np.abs(r - float(F32(case["max_residual"])))
    return (int(m["status_drop"].sum()), int(m["gradient_drop"].sum()), int(m["residual_drop"].sum())), int(m["kept"].sum()), int(((d > 0) & (d < NEAR)).sum())


def _case(name, vol, vs, n, seed, rigid_seed=None, min_weight=1, max_residual=0.9, pitch_extra=0, offset=0, plant=False, tile=1, extra_pts=None, margin=1.0):
    shape = vol[0].shape[::-1]
    base_n = n // tile
    assert base_n * tile == n
    for attempt in range(40):
        rng = np.random.default_rng(1000 * seed + attempt)
        v, planted = (vol, None)
        if plant:
            v, planted = _plant(vol, max_residual, min_weight, rng)
        pts = sc.random_points(shape, vs, base_n, 7000 * seed + attempt, margin=margin)
        if extra_pts is not None:
            k = min(len(extra_pts), base_n // 2)
            pts[:k] = extra_pts[rng.choice(len(extra_pts), k, replace=False)]
        if planted is not None and base_n >= 255:
            pts[base_n - 1 - len(planted):base_n - 1] = sc.lattice_points(shape, vs, planted)      # (the last point stays random)
        xform, T = (None, np.eye(4))
        if rigid_seed is not None:
            xform, T = sc.rigid(rigid_seed, 0.35, (0.11, -0.07, 0.05))
            pts = sc.points_for(xform, T, pts)
        else:
            xform = sc.IDENTITY12.copy()
        case = dict(kind="points", name=name, vol=v, vs=F32(vs), shape=shape, pts=pts, base_pts=pts, xform=xform, T=T, min_weight=min_weight, grad=None,
                    max_residual=float(F32(max_residual)), pitch=shape[0] * 4 + pitch_extra, offset=offset, tile=tile, n=n, planted=planted)
        m = point_terms(case)
        drops, kept, near = _conditions(case, m)
        m64 = point_terms(case, np.float64, keep=m["kept"])
        twin_ok = bool((m64["ok"] & m64["gok"])[m["kept"]].all())
        if near == 0 and twin_ok and (base_n < 255 or (min(drops) > 0 and kept > 0)):
            break
    else:
        raise AssertionError("no seed gives case %s its conditions" % name)
    for a in v:
        a.setflags(write=False)
    pts = np.ascontiguousarray(pts, np.float32)
    pts.setflags(write=False)
    case["pts"] = case["base_pts"] = pts
    return case


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    v222 = sc.random_volume((2, 2, 2), 2, low_weight=1)
    v345 = sc.random_volume((3, 4, 5), 8, low_weight=1)
    out.append(_case("v222_n5_identity", v222, sc.VS2, 5, 1, margin=0.2))
    out.append(_case("v222_n64_rigid_mr03", v222, sc.VS2, 64, 2, rigid_seed=21, max_residual=0.3, margin=0.2))
    out.append(_case("v345_n1_rigid", v345, sc.VS2, 1, 3, rigid_seed=22, margin=-0.6, pitch_extra=4))
    out.append(_case("v345_n6_identity_mw3", v345, sc.VS2, 6, 4, min_weight=3, margin=0.0, pitch_extra=4))
    out.append(_case("v345_n63_rigid", v345, sc.VS2, 63, 5, rigid_seed=23, margin=0.3, pitch_extra=8))
    out.append(_case("v345_n65_identity_mr03", v345, sc.VS2, 65, 6, max_residual=0.3, margin=0.3))
    # 33 x 17 x 20, pitched with an offset: a sphere and a plane with weight-0 shells and holes
    sphere = rc.sphere_volume((33, 17, 20), float(sc.VS2), (0.45, 0.5, 0.55), 0.3, seed=4)
    plane = rc.plane_volume((33, 17, 20), float(sc.VS2), (0.2, 0.3, 1.0), 0.55, seed=6)
    out.append(_case("sphere_n255_identity", sphere, sc.VS2, 255, 7, plant=True, pitch_extra=12, offset=8))
    out.append(_case("sphere_n257_rigid_mw3_mr03", sphere, sc.VS2, 257, 8, rigid_seed=24, min_weight=3, max_residual=0.3, pitch_extra=20, offset=4))
    out.append(_case("plane_n255_rigid_mr03", plane, sc.VS2, 255, 9, rigid_seed=25, max_residual=0.3, pitch_extra=12, offset=8))
    out.append(_case("plane_n257_identity_mw3", plane, sc.VS2, 257, 10, min_weight=3, plant=True, pitch_extra=8, offset=4))
    out.append(_case("sphere_n1064960_rigid", sphere, sc.VS2, BIG_N, 11, rigid_seed=26, pitch_extra=12, offset=8, tile=256))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def big_case():
    """The (65, 33, 64) volume the GPU test lays out in rows of 1 MiB (row offsets past 2^31 bytes from row 2048 on: plane 62, y >= 2): half of
    the points lie between planes 62.0 and 62.3 over the sphere's cap, so that their seven samples read planes 61 to 63, the gradient's +- half a
    voxel stays inside and most of them are kept, the others are random over the whole box and a voxel past it."""
    b = sc.big_case()
    X, Y, Z = rc.BIG_SHAPE
    rng = np.random.default_rng(70)
    # (the sphere's cap: its axis passes through voxel (32, 16), and within three voxels of it plane 62 lies inside the band)
    g = np.stack([rng.uniform(32.0 - 2.2, 32.0 + 2.2, 4000), rng.uniform(16.0 - 2.2, 16.0 + 2.2, 4000), rng.uniform(Z - 2.0, Z - 1.7, 4000)], axis=1)
    return _case("big_rows", tuple(np.array(a) for a in b["vol"]), sc.VS2, 1000, 12, extra_pts=((g + 0.5) * float(sc.VS2)).astype(np.float32))


def high_rows_kept(case, m):
    """The kept points of big_case() whose centre sample reads a row at or past 2^31 bytes in rows of rc.BIG_PITCH."""
    Y = case["shape"][1]
    g = [m["P"][c].astype(np.float64) / float(case["vs"]) - 0.5 for c in range(3)]
    row = np.floor(np.where(m["kept"], g[2], 0)) * Y + np.floor(np.where(m["kept"], g[1], 0))
    return m["kept"] & (row * rc.BIG_PITCH >= 2 ** 31)


def wrap_case():
    """For the model alone: the (3, 4, 5) volume behind a synthetic address map with rows of 2^28 bytes, whose rows 16 .. 19 lie past 2^32 bytes."""
    c = dict(next(c for c in cases() if c["name"] == "v345_n63_rigid"))
    c.update(name="v345_pitch_2_28", pitch=1 << 28)
    return c


def all_points(case):
    """The case's n points: the base points tiled."""
    return np.ascontiguousarray(np.tile(case["base_pts"], (case["tile"], 1)))


def evaluate(case, dtype=np.float32, mutant=None, keep=None):
    """The per-point results on the base points and the sums over all n points: dict(point=..., terms [n, 29], sums (kernel order), fsum)."""
    pt = point_terms(case, dtype, mutant, keep)
    terms = np.tile(terms29(pt), (case["tile"], 1))
    return dict(point=pt, terms=terms, sums=chunk_sums(terms, tail=mutant == "tail"), kept=pt["kept"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """The model's result for a case, computed once and shared: never modified."""
    case = {c["name"]: c for c in cases() + (big_case(),)}[name]
    out = evaluate(case)
    out["fsum"] = fsum_sums(out["terms"])
    out["tolerance"] = tolerance(out["terms"])
    for a in (out["terms"], out["sums"], out["fsum"], out["tolerance"]):
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------
# The loop, restated (gn_batch_loop's shape for one start; the step is align_cases.step: register_step is align_step)
def xform12_of(T):
    """register_xform12 restated: one rounding per entry; None where an entry is not finite in float32."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    with np.errstate(over="ignore"):
        m = np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]]).astype(F32)
    return m if np.isfinite(m).all() and np.isfinite(T[:3]).all() else None


MISS12 = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, -1, -1, -1], F32)     # what the orchestrator launches for a T outside float32's range


def loop(case, pts, T0, iterations, damping=1e-3, twin=False):
    """The whole registration loop of one start on the CPU: `iterations` steps and a final loss pass, the sums in the kernel's order.  Returns
    (ok, T, loss history, the last pass's sums)."""
    import align_cases as ac
    T = np.array(T0, np.float64).reshape(4, 4).copy()
    hist, s = [], None
    for p in range(iterations + 1):
        m = xform12_of(T)
        pt = point_terms(case, np.float32, pts=pts, xform=MISS12 if m is None else m)
        if twin:
            pt = point_terms(case, np.float64, keep=pt["kept"], pts=pts, xform=MISS12 if m is None else m)
        s = chunk_sums(terms29(pt))
        hist.append(s[27] / s[28] if s[28] > 0 else 0.0)
        if p == iterations:
            return bool(s[28] >= 6), T, np.array(hist), s
        taken, T = ac.step(s, damping, T)
        if not taken:
            return False, T, np.array(hist), s
    return True, T, np.array(hist), s


def loop_scene(n=24, vs=0.05, count=1500, seed=5):
    """An analytic sphere's TSDF at n^3, `count` points on its surface plus 20 % far outliers, given in a frame that T_true takes to the volume, and
    a start 1.5 voxels and 2 degrees off: (case, pts, T_true, T0)."""
    import align_cases as ac
    rng = np.random.default_rng(seed)
    vol = rc.sphere_volume((n, n, n), vs, (0.5, 0.5, 0.5), 0.3, seed=seed, holes=False)
    centre, radius = 0.5 * n * vs * np.ones(3), 0.3 * n * vs
    d = rng.normal(size=(count, 3))
    surf = centre + radius * d / np.linalg.norm(d, axis=1, keepdims=True)
    far = rng.uniform(-0.5, 1.5, (count // 5, 3)) * n * vs
    far = far[np.abs(np.linalg.norm(far - centre, axis=1) - radius) > 6 * vs]
    _, T_true = sc.rigid(77, 0.4, (0.2, -0.1, 0.15))
    pts = sc.points_for(None, T_true, np.concatenate([surf, far]).astype(np.float32))
    T0 = ac.perturbed(T_true, (n, n, n), vs, shift_voxels=(0.9, -0.8, 0.9), degrees=2.0)
    case = dict(kind="points", name="loop", vol=vol, vs=F32(vs), shape=(n, n, n), pts=pts, base_pts=pts, xform=None, T=T_true, min_weight=1, grad=None,
                max_residual=float(F32(0.9)), pitch=n * 4, offset=0, tile=1, n=len(pts))
    return case, pts, T_true, T0
