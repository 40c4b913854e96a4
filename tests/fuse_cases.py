"""Cases and models for xs_tsdf_fuse_points_accumulate and xs_tsdf_fuse_points_fold (x-slam_amd/csrc/xs_fuse.hip), shared by
tests/test_fuse_cases_cpu.py, tests/test_fuse_gpu.py and tests/test_fuse_pipeline_gpu.py.

THE MODEL is the contract of include/xslam_amd.h in numpy, written from the header and not from the kernel.  walk() takes the rays of a case
through steps 1 to 7 one float32 operation at a time (every array is float32 and every constant np.float32, so numpy rounds where the contract
does) and returns one record per ray sample; accumulate() adds (1 << 40) | q to uint64 words with np.add.at, which knows no order; fold() is the
per-voxel rule, its two double operations in float64.  The same walk() in float64 with decisions of its own is the whole pipeline "done in
double" (the accuracy test's yardstick).

THE TWIN AND THE BOUND.  replay() redoes steps 1 to 6 (and the product of step 7) on the model's own decisions in a number type V that carries
three things per value: a, the model's float32 value; b, the float64 twin's value; and e >= |a - b|, by running error analysis with LOCAL
ERRORS THAT ARE COMPUTED, not assumed: for z = x op y the model's rounding is |fl32(x.a op y.a) - (x.a op y.a)| evaluated in float64 (exact for
+, -, x of float32 operands, and within 2^-52 relative for / and sqrt, which is added), the twin's own rounding is 2^-52 |z.b|, and the
operands' errors propagate by
    x + y, x - y:  e_x + e_y                      x * y:  |x.a| e_y + (|y.a| + e_y) e_x
    x / y:  (e_x + |x.a / y.a| e_y) / (|y.a| - e_y)        sqrt(x):  e_x / (sqrt(x.a) + sqrt(x.b)).
Nothing is fitted.  test_fuse_cases_cpu.py asserts V.a equal to walk()'s float32 values bit for bit, V.b equal to the float64 values, and
|a - b| <= e.

FORBIDDEN NEAR MISSES (near_misses()): a ray is not admitted to a case if a value of it lies within e of a decision without sitting ON it in both
precisions: L against min_range and max_range; a g[c] against an integer in 0 .. res[c] (the floorf boundaries and the two range tests); u
against -1; (u + 1) * 32768 against a half integer (the tie of rintf).  Equality that is meant is allowed, as in register_cases: the cases without
a transform put origins and points on the half-voxel lattice of a power-of-two voxel size, where rays along the axes give every other sample a g
that IS an integer, a voxel centre exactly tranc_dist behind the point (u == -1.0f, q == 0: kept by "u < -1", dropped by "u <= -1"), and sums that
are exact in float32 and float64 alike.  Candidate rays are drawn until enough admitted ones are found: rays are independent of each other, so
leaving one out changes no other ray's record.

MUTANTS: mistakes a kernel could make, each of which must change an expected byte of some case."""
import functools

import numpy as np

import render_cases as rc
import sample_cases as sc

F32, F64 = np.float32, np.float64
VS = sc.VS2                                  # 0.0625: a power of two
COUNT_SHIFT, SUM_MASK = np.uint64(40), np.uint64((1 << 40) - 1)
MAX_POINTS, MAX_HALF_STEPS = (1 << 24) - 1, 256
# accumulate: every sample deduped against nothing; (int) conversion before the range test; the centre without its half voxel; "u <= -1" as the skip
# rule; u not clamped at 1; q truncated; the ray started K half steps in front of the point even behind the sensor.  fold: grad left as it was; the
# weight not capped.
WALK_MUTANTS = ("no_dedupe", "trunc_int", "no_half", "skip_le", "no_clamp", "trunc_q", "klo_K")
FOLD_MUTANTS = ("grad_unscaled", "no_cap")
MUTANTS = WALK_MUTANTS + FOLD_MUTANTS


# ------------------------------------------------------------------------------------------------
# Arithmetic: plain numpy in one precision, or V
class V:
    """(a, b, e): the float32 model's value, the float64 twin's, and a bound on their distance (module docstring)."""
    __slots__ = ("a", "b", "e")

    def __init__(self, a, b=None, e=None):
        self.a = np.asarray(a, F32)
        self.b = self.a.astype(F64) if b is None else b
        self.e = np.zeros(self.a.shape) if e is None else e

    @staticmethod
    def _of(a, b, prop, exact):
        with np.errstate(invalid="ignore"):
            local = np.abs(a.astype(F64) - exact) + 2.0 ** -52 * np.abs(exact)
            return V(a, b, prop + local + 2.0 ** -52 * np.abs(b))

    def __add__(self, o):
        return V._of(self.a + o.a, self.b + o.b, self.e + o.e, self.a.astype(F64) + o.a.astype(F64))

    def __sub__(self, o):
        return V._of(self.a - o.a, self.b - o.b, self.e + o.e, self.a.astype(F64) - o.a.astype(F64))

    def __mul__(self, o):
        return V._of(self.a * o.a, self.b * o.b, np.abs(self.a.astype(F64)) * o.e + (np.abs(o.a.astype(F64)) + o.e) * self.e, self.a.astype(F64) * o.a.astype(F64))

    def __truediv__(self, o):
        with np.errstate(invalid="ignore", divide="ignore"):
            exact = self.a.astype(F64) / o.a.astype(F64)
            room = np.abs(o.a.astype(F64)) - o.e
            prop = np.where(room > 0, (self.e + np.abs(exact) * o.e) / np.where(room > 0, room, 1.0), np.inf)
            return V._of(self.a / o.a, self.b / o.b, prop, exact)

    def sqrt(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            ra, rb = np.sqrt(self.a), np.sqrt(self.b)
            den = ra.astype(F64) + rb
            prop = np.where(den > 0, self.e / np.where(den > 0, den, 1.0), np.sqrt(self.e))
            return V._of(ra, rb, prop, np.sqrt(self.a.astype(F64)))

    def take(self, idx):
        return V(self.a[idx], self.b[idx], self.e[idx])

    def minimum1(self):
        """fminf(x, 1.0f): 1-Lipschitz, no rounding."""
        return V(np.minimum(self.a, F32(1)), np.minimum(self.b, 1.0), self.e)


class Plain:
    """numpy in one precision: lift() takes float32 data to it."""

    def __init__(self, dtype):
        self.T = dtype

    def lift(self, x):
        return np.asarray(x, F32).astype(self.T)

    @staticmethod
    def sqrt(x):
        return np.sqrt(x)

    @staticmethod
    def take(x, idx):
        return x[idx]

    def minimum1(self, x):
        return np.minimum(x, self.T(1))


class Tracked:
    @staticmethod
    def lift(x):
        return V(x)

    @staticmethod
    def sqrt(x):
        return x.sqrt()

    @staticmethod
    def take(x, idx):
        return x.take(idx)

    @staticmethod
    def minimum1(x):
        return x.minimum1()


# ------------------------------------------------------------------------------------------------
# Steps 1 to 7, written once for the three arithmetics
def _transform(A, xform, p):
    """xs_tsdf_sample_points' formula; the bits as they are without a transform."""
    if xform is None:
        return [A.lift(p[:, c]) for c in range(3)]
    m = [A.lift(np.full(len(p), xform[i], F32)) for i in range(12)]
    q = [A.lift(p[:, c]) for c in range(3)]
    return [((m[3 * c] * q[0] + m[3 * c + 1] * q[1]) + m[3 * c + 2] * q[2]) + m[9 + c] for c in range(3)]


def _ray(A, case, pts):
    """Steps 1 and 2: P, L, d and the half step, per point."""
    n = len(pts)
    P = _transform(A, case["xform"], pts)
    O = _transform(A, case["xform"], np.tile(np.asarray(case["origin"], F32), (n, 1)))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = [P[c] - O[c] for c in range(3)]
        L = A.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        d = [v[c] / L for c in range(3)]
    return P, L, d


def _consts(A, case, n):
    vs, tranc = A.lift(np.full(n, case["vs"], F32)), A.lift(np.full(n, case["tranc"], F32))
    return vs, tranc, A.lift(np.full(n, 0.5, F32)) * vs


def _g(A, P, d, kf, step, vs):
    """Step 4's g for samples: P, d, kf (float(k)), step and vs one entry per sample."""
    return [(P[c] + (kf * step) * d[c]) / vs for c in range(3)]


def _u(A, P, d, i_f, vs, tranc, half):
    """Step 6's u before the skip and the clamp; i_f: the voxel indices as floats; half: 0.5 (0 in the no_half mutant)."""
    C = [(i_f[c] + half) * vs for c in range(3)]
    sd = ((P[0] - C[0]) * d[0] + (P[1] - C[1]) * d[1]) + (P[2] - C[2]) * d[2]
    return sd / tranc


def half_steps(case):
    """K, in the host's float32 operations."""
    return int(np.ceil(F32(case["tranc"]) / (F32(0.5) * F32(case["vs"]))))


def _quiet(f):
    """NaN and infinite coordinates are among the inputs: their arithmetic is meant, numpy's warnings about it are not."""
    @functools.wraps(f)
    def g(*a, **k):
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            return f(*a, **k)
    return g


@_quiet
def walk(case, dtype=np.float32, mutant=None, pts=None):
    """Steps 1 to 7 for the points `pts` (default: the case's base points) in one precision, with that precision's own decisions.  Returns per point
    used, L; and per ray SAMPLE, in (k, point) order: pt, k, inside, i [m, 3], g [m, 3], reached (step 6 was evaluated), u (before the clamp; NaN
    where not reached), qf = (min(u, 1) + 1) * 32768, visit (a word is added) and q."""
    A = Plain(dtype)
    T = dtype
    pts = case["pts"] if pts is None else pts
    n = len(pts)
    res = np.array(case["shape"])
    P, L, d = _ray(A, case, pts)
    vs, tranc, step = _consts(A, case, n)
    K = half_steps(case)
    with np.errstate(invalid="ignore"):
        used = (L >= T(F32(case["min_range"]))) & (L <= T(F32(case["max_range"])))
        k_far = np.where(used, np.floor(np.where(used, L / step, 0)), 0).astype(np.int64)
    k_lo = -k_far if case["carve"] else -np.minimum(K, k_far)
    if mutant == "klo_K" and not case["carve"]:
        k_lo = np.full(n, -K, np.int64)
    half = A.lift(np.full(n, 0.0 if mutant == "no_half" else 0.5, F32))
    prev = np.full((n, 3), -1, np.int64)
    rec = {k: [] for k in ("pt", "k", "inside", "i", "g", "reached", "u", "qf", "visit", "q")}
    for k in (range(int(k_lo[used].min()), K + 1) if used.any() else ()):
        act = np.nonzero(used & (k_lo <= k))[0]
        if not len(act):
            continue
        Pa, da = [x[act] for x in P], [x[act] for x in d]
        g = np.stack(_g(A, Pa, da, A.lift(np.full(len(act), k, F32)), step[act], vs[act]), axis=1)
        if mutant == "trunc_int":
            i = np.trunc(np.clip(g, -1e6, 1e6)).astype(np.int64)
            inside = ((i >= 0) & (i < res)).all(axis=1)
        else:
            inside = ((g >= 0) & (g < res.astype(T))).all(axis=1)
            i = np.where(inside[:, None], np.floor(np.where(inside[:, None], g, 0)), -1).astype(np.int64)
        dup = inside & (i == prev[act]).all(axis=1)
        if mutant == "no_dedupe":
            dup[:] = False
        prev[act[inside]] = i[inside]
        reached = inside & ~dup
        r = np.nonzero(reached)[0]
        u = np.full(len(act), np.nan, T)
        u[r] = _u(A, [x[r] for x in Pa], [x[r] for x in da], [A.lift(i[r, c].astype(F32)) for c in range(3)], vs[act][r], tranc[act][r], half[act][r])
        with np.errstate(invalid="ignore"):
            skip = (u <= T(-1)) if mutant == "skip_le" else (u < T(-1))
            visit = reached & ~skip
            uc = u if mutant == "no_clamp" else np.minimum(u, T(1))
            qf = (uc + T(1)) * T(32768)
            q = np.where(visit, np.trunc(qf) if mutant == "trunc_q" else np.rint(qf), 0).astype(np.int64)
        for name, val in (("pt", act), ("k", np.full(len(act), k)), ("inside", inside), ("i", i), ("g", g), ("reached", reached), ("u", u), ("qf", qf),
                          ("visit", visit), ("q", q)):
            rec[name].append(val)
    out = {k: (np.concatenate(v) if v else np.zeros((0, 3) if k in ("i", "g") else 0, np.int64 if k in ("pt", "k", "i", "q") else (bool if k in ("inside", "reached", "visit") else T)))
           for k, v in rec.items()}
    out.update(used=used, L=L, n=n)
    return out


def counts4(case, w):
    """{points used, points dropped, visits, samples outside} of the case's n points (the base points tiled)."""
    t = case["tile"]
    return np.array([int(w["used"].sum()) * t, (w["n"] - int(w["used"].sum())) * t, int(w["visit"].sum()) * t, int((~w["inside"]).sum()) * t], np.uint64)


def accumulate(case, w, acc=None):
    """The accumulator [Z, Y, X] uint64 after the case's n points: np.add.at of every visit's word, the base points' visits `tile` times over."""
    X, Y, Z = case["shape"]
    acc = np.zeros((Z, Y, X), np.uint64) if acc is None else acc
    v = w["visit"]
    idx = (w["i"][v, 2] * Y + w["i"][v, 1]) * X + w["i"][v, 0]
    word = (np.uint64(1) << COUNT_SHIFT) | w["q"][v].astype(np.uint64)
    np.add.at(acc.reshape(-1), np.tile(idx, case["tile"]), np.tile(word, case["tile"]))
    return acc


def fold(vol, acc, obs_weight, max_weight, z0=0, z1=None, mutant=None):
    """The per-voxel rule of xs_tsdf_fuse_points_fold on copies: ((value, weight, grad), accumulator after, voxels written)."""
    value, weight, grad = (np.array(a) for a in vol)
    acc = acc.copy()
    z1 = value.shape[0] if z1 is None else z1
    sl = np.s_[z0:z1]
    a = acc[sl]
    cnt, s = a >> COUNT_SHIFT, a & SUM_MASK
    t = cnt > 0
    m = s.astype(F64) / np.where(t, cnt, 1).astype(F64)
    o = (m * 2.0 ** -15 - 1.0).astype(F32)
    wp = weight[sl]
    fp, fs, ft = wp.astype(F32), F32(obs_weight), (wp + obs_weight).astype(F32)
    nv = np.where(wp == 0, o, (value[sl] * fp + o * fs) / ft)
    ng = np.where(wp == 0, F32(0), grad[sl] if mutant == "grad_unscaled" else (grad[sl] * fp) / ft)
    nw = wp + obs_weight if mutant == "no_cap" else np.minimum(wp + obs_weight, max_weight)
    value[sl], grad[sl], weight[sl] = np.where(t, nv, value[sl]), np.where(t, ng, grad[sl]), np.where(t, nw, wp).astype(np.int32)
    acc[sl] = np.where(t, np.uint64(0), a)
    return (value, weight, grad), acc, int(t.sum())


# ------------------------------------------------------------------------------------------------
# The twin and the bound
@_quiet
def replay(case, w, pts=None):
    """Steps 1 to 6 and step 7's product in V arithmetic on the decisions of the float32 walk `w`: dict(L [n], g [m] x 3, u, qf [reached samples])
    of V, and `reached`, the indices of those samples."""
    A = Tracked
    pts = case["pts"] if pts is None else pts
    n = len(pts)
    P, L, d = _ray(A, case, pts)
    vs, tranc, step = _consts(A, case, n)
    pt = w["pt"]
    g = _g(A, [x.take(pt) for x in P], [x.take(pt) for x in d], V(w["k"].astype(F32)), step.take(pt), vs.take(pt))
    r = np.nonzero(w["reached"])[0]
    pr = pt[r]
    u = _u(A, [x.take(pr) for x in P], [x.take(pr) for x in d], [V(w["i"][r, c].astype(F32)) for c in range(3)], vs.take(pr), tranc.take(pr), V(np.full(len(r), 0.5, F32)))
    qf = (u.minimum1() + V(np.full(len(r), 1, F32))) * V(np.full(len(r), 32768, F32))
    return dict(L=L, g=g, u=u, qf=qf, reached=r)


def _near(dist, e, on_it):
    """within e of a decision without sitting on it in both precisions"""
    with np.errstate(invalid="ignore"):
        return (dist <= e) & ~((dist == 0) & on_it)


def near_misses(case, w, rp):
    """Per point: does any of its values lie within its bound of a decision (module docstring)?  Returns (bad [n], counts per kind)."""
    n = w["n"]
    bad = np.zeros(n, bool)
    kinds = {}
    L = rp["L"]
    fin = np.isfinite(L.a)
    for name in ("min_range", "max_range"):
        lim = float(F32(case[name]))
        hit = fin & _near(np.abs(L.a.astype(F64) - lim), L.e, L.b == lim)
        kinds[name] = int(hit.sum())
        bad |= hit
    res = np.array(case["shape"], F64)
    hit_g = np.zeros(len(w["pt"]), bool)
    for c in range(3):
        g = rp["g"][c]
        ga = g.a.astype(F64)
        with np.errstate(invalid="ignore"):
            near_int = np.rint(ga)
            relevant = np.isfinite(ga) & (near_int >= 0) & (near_int <= res[c])
        hit_g |= relevant & _near(np.abs(ga - near_int), g.e, g.b == near_int)
    kinds["floor"] = int(hit_g.sum())
    bad[w["pt"][hit_g]] = True
    r = rp["reached"]
    u, qf = rp["u"], rp["qf"]
    hit_u = _near(np.abs(u.a.astype(F64) + 1.0), u.e, u.b == -1.0)
    kinds["u_minus_1"] = int(hit_u.sum())
    bad[w["pt"][r][hit_u]] = True
    qa = qf.a.astype(F64)
    visit = w["visit"][r]
    hit_q = visit & _near(np.abs(qa - np.floor(qa) - 0.5), qf.e, qf.b == qa)
    kinds["tie"] = int(hit_q.sum())
    bad[w["pt"][r][hit_q]] = True
    return bad, kinds


# ------------------------------------------------------------------------------------------------
# The cases
def random_volume(shape, seed):
    """(value, weight, grad) [Z, Y, X]: values and derivatives in (-1, 1), weights 0 .. 3 (a quarter of the voxels empty)."""
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    return (rng.uniform(-1, 1, (Z, Y, X)).astype(F32), rng.integers(0, 4, size=(Z, Y, X)).astype(np.int32), rng.uniform(-1, 1, (Z, Y, X)).astype(F32))


def _candidates(shape, origin_v, rng, count, lattice):
    """Candidate points in the volume frame, the ones the issue lists first: NaN and infinite coordinates, the origin itself, far points, rays
    along each axis in both directions, short rays (shorter than the band), then `count` random points reaching three voxels past every face."""
    S = np.array(shape, F64)
    vs = float(VS)
    o = np.asarray(origin_v, F64)
    out = [[np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, -np.inf], list(o), [40.0, 0.2, 0.2], [-9.0, -9.0, 0.3]]
    for c in range(3):
        for sgn in (1.0, -1.0):
            for r in ((8, 19) if lattice else (8.3, 19.6)):       # voxels
                p = o.copy()
                p[c] += sgn * r * vs
                out.append(list(p))
    for _ in range(8):                                             # shorter than the band: k_far < K
        dvec = rng.normal(size=3)
        out.append(list(o + dvec / np.linalg.norm(dvec) * rng.uniform(1.2, 3.2) * vs))
    special = np.array(out)
    rnd = (rng.uniform(-1.0, 1.0, (count, 3)) * (S / 2 + 3) + S / 2) * vs
    return np.concatenate([special, rnd]), len(special)


def _case(name, shape, seed, carve, rigid_seed, obs_weight, n_random, origin_vox, pitch_extra=0, offset=0, tile=1, launches=1):
    vs = float(VS)
    lattice = rigid_seed is None
    xform, T = (None, np.eye(4)) if lattice else sc.rigid(rigid_seed, 0.4, (0.15, -0.08, 0.06))
    tranc = F32(0.25) if lattice else F32(0.2)
    o_v = (np.array(origin_vox, F64) + 0.5) * vs + (0.0 if lattice else np.array([0.013, 0.021, 0.017]))
    rng = np.random.default_rng(seed)
    cand_v, n_special = _candidates(shape, o_v, rng, 12 * n_random + 40, lattice)
    to_frame = (lambda p: np.asarray(p, F32)) if lattice else (lambda p: sc.points_for(xform, T, np.asarray(p, F64)))
    origin = to_frame(o_v[None, :])[0]
    cand = to_frame(cand_v)
    cand[3] = origin                                               # the point at the origin: L == 0 in either precision, under any transform
    case = dict(name=name, shape=tuple(shape), vol=random_volume(shape, seed + 500), vs=VS, tranc=tranc, xform=xform, T=T, origin=origin, carve=bool(carve),
                min_range=float(F32(0.05)), max_range=float(F32(3.0)), obs_weight=obs_weight, max_weight=4, pitch=shape[0] * 4 + pitch_extra, offset=offset,
                tile=tile, launches=launches, lattice=lattice, degenerate=shape[0] * shape[1] * shape[2] < 200)
    w = walk(case, pts=cand)
    bad, _ = near_misses(case, w, replay(case, w, pts=cand))
    good = ~bad
    keep = np.concatenate([np.nonzero(good[:n_special])[0], n_special + np.nonzero(good[n_special:])[0][:n_random]])
    assert len(keep) - int(good[:n_special].sum()) == n_random, "case %s: too few admitted rays" % name
    pts = np.ascontiguousarray(cand[keep], F32)
    pts.setflags(write=False)
    for a in case["vol"]:
        a.setflags(write=False)
    case.update(pts=pts, n=len(pts) * tile, n_special=int(good[:n_special].sum()))
    return case


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    seed = 0
    for shape, n_random, inside, outside, pe in (((2, 2, 2), 12, (0, 1, 0), (-3, 0, 1), 4), ((5, 3, 2), 24, (2, 1, 0), (-4, 1, 0), 8), ((70, 9, 11), 640, (30, 4, 5), (-5, 3, 6), 20)):
        for carve in (False, True):
            for rigid in (False, True):
                for ws in (1, 3):
                    seed += 1
                    nm = "v%dx%dx%d_%s_%s_w%d" % (shape + ("carve" if carve else "band", "rigid" if rigid else "lattice", ws))
                    out.append(_case(nm, shape, seed, carve, 40 + seed if rigid else None, ws, n_random, inside if ws == 1 else outside, pitch_extra=pe,
                                     offset=(8 if rigid else 0)))
    # accumulated by two launches (the first 150 points, then the rest) before one fold
    out.append(_case("v70x9x11_two_launches", (70, 9, 11), 101, True, 77, 1, 640, (40, 4, 5), pitch_extra=12, launches=2))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def hot_case():
    """70 000 identical points: the ray along +x from outside the 5 x 3 x 2 volume to the centre of voxel (4, 1, 1), carving: five voxels whose count
    passes 2^16, and the first, four voxels in front of the point (u == 1, q == 65536), whose sum of q passes 2^32."""
    c = _case("hot_voxel", (5, 3, 2), 201, True, None, 1, 0, (-4, 1, 1), tile=70000)
    p = np.array([[(4 + 0.5) * float(VS), (1 + 0.5) * float(VS), (1 + 0.5) * float(VS)]], F32)
    p.setflags(write=False)
    c.update(pts=p, n=70000, n_special=1)
    return c


@functools.lru_cache(maxsize=None)
def big_case():
    """The (65, 33, 64) volume the GPU test lays out in rows of 1 MiB (row offsets past 2^31 bytes from row 2048 on: plane 62, y >= 2), for the fold: a
    sensor above the last plane whose rays end around planes 60 to 63."""
    shape = rc.BIG_SHAPE
    c = _case("big_rows", shape, 301, False, None, 3, 0, (32, 16, 70))
    rng = np.random.default_rng(302)
    vs = float(VS)
    cand = np.stack([rng.uniform(20, 45, 4000), rng.uniform(6, 27, 4000), rng.uniform(60.5, 63.5, 4000)], axis=1) * vs
    cand = cand.astype(F32)
    w = walk(c, pts=cand)
    bad, _ = near_misses(c, w, replay(c, w, pts=cand))
    pts = np.ascontiguousarray(cand[~bad][:600])
    assert len(pts) == 600
    pts.setflags(write=False)
    c.update(pts=pts, n=600, n_special=0)
    return c


def all_cases():
    return cases() + (hot_case(), big_case())


def all_points(case):
    """The case's n points: the base points tiled."""
    return np.ascontiguousarray(np.tile(case["pts"], (case["tile"], 1)))


def launch_split(case):
    """Where the points are cut for the launches of a case: [0, ..., n]."""
    return [0, case["n"]] if case["launches"] == 1 else [0, 150, case["n"]]


def evaluate(case, mutant=None):
    """The model on a case: dict(walk, acc (after accumulate), counts, vol (after the fold: value, weight, grad), acc_after, written)."""
    w = walk(case, mutant=mutant if mutant in WALK_MUTANTS else None)
    acc = accumulate(case, w)
    vol, after, written = fold(case["vol"], acc, case["obs_weight"], case["max_weight"], mutant=mutant if mutant in FOLD_MUTANTS else None)
    return dict(walk=w, acc=acc, counts=counts4(case, w), vol=vol, acc_after=after, written=written)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The model's result for a case, computed once and shared: never modified."""
    case = {c["name"]: c for c in all_cases()}[name]
    out = evaluate(case)
    for a in (out["acc"], out["counts"], out["acc_after"]) + tuple(out["vol"]):
        a.setflags(write=False)
    return out


def same_bytes(a, b):
    """Equal bit for bit: (value, weight, grad) triples or single arrays."""
    if isinstance(a, tuple):
        return all(same_bytes(x, y) for x, y in zip(a, b))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def high_rows_written(case, ev, pitch=rc.BIG_PITCH):
    """The voxels the fold writes in rows at or past 2^31 bytes, in rows of `pitch` bytes."""
    X, Y, Z = case["shape"]
    t = (ev["acc"] >> COUNT_SHIFT) > 0
    rows = (np.arange(Z)[:, None] * Y + np.arange(Y)[None, :]) * pitch >= 2 ** 31
    return int((t & rows[:, :, None]).sum())


# ------------------------------------------------------------------------------------------------
# The analytic scene of the accuracy test
def analytic_scene(n=48, rays=60000, seed=9):
    """A plane and a sphere in front of it at n^3, seen from one origin, fused into an EMPTY volume: (case, hits [m, 3] float64: the true surface
    points of the rays with incidence up to 45 degrees, their unit directions, incidence cosines)."""
    vs = float(VS)
    ext = n * vs
    o = np.array([0.5 * ext + 0.011, 0.5 * ext - 0.007, 0.06 * ext + 0.003])
    zp = 0.8 * ext + 0.004                                           # the plane z = zp, normal -z towards the sensor
    cs, rs = np.array([0.55 * ext, 0.45 * ext, 0.55 * ext]), 0.14 * ext   # the sphere
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(rays, 3))
    d[:, 2] = np.abs(d[:, 2]) + 0.9
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t_plane = (zp - o[2]) / d[:, 2]
    oc = o - cs
    b = d @ oc
    disc = b * b - (oc @ oc - rs * rs)
    t_sph = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), np.inf)
    t_sph = np.where(t_sph > 0, t_sph, np.inf)
    t = np.minimum(t_plane, t_sph)
    hit = o + t[:, None] * d
    normal = np.where((t_sph < t_plane)[:, None], (hit - cs) / rs, np.array([0.0, 0.0, -1.0]))
    cosi = -(normal * d).sum(axis=1)
    inside = ((hit > 2 * vs) & (hit < ext - 2 * vs)).all(axis=1)
    ok = inside & (cosi >= np.cos(np.pi / 4))
    empty = (np.zeros((n, n, n), F32), np.zeros((n, n, n), np.int32), np.zeros((n, n, n), F32))
    case = dict(name="analytic", shape=(n, n, n), vol=empty, vs=VS, tranc=F32(0.25), xform=None, T=np.eye(4), origin=o.astype(F32), carve=False,
                min_range=float(F32(0.05)), max_range=float(F32(5.0)), obs_weight=1, max_weight=4, pitch=n * 4, offset=0, tile=1, launches=1, lattice=False,
                degenerate=False, pts=hit[ok].astype(F32), n=int(ok.sum()), n_special=0)
    return case, hit[ok], d[ok], cosi[ok]


def fused_field(case, dtype):
    """The value and weight volumes after fusing the case's points into its (empty) volume with the whole pipeline in one precision: walk in
    `dtype` with its own decisions, the integer accumulator, the fold."""
    w = walk(case, dtype)
    vol, _, _ = fold(case["vol"], accumulate(case, w), case["obs_weight"], case["max_weight"])
    return vol[0], vol[1]


def crossing_error(case, value, weight, hits, dirs, span_vox=3.0, sub=16):
    """Along every ray, the distance in metres between the true surface point and the zero crossing of the fused field's trilinear interpolation
    (sample_cases.trilinear: the library's F), searched within span_vox voxels of the hit in steps of 1 / sub voxel and refined linearly; NaN where
    the field has no crossing there.  Float64."""
    vs = float(case["vs"])
    ts = np.arange(-span_vox * sub, span_vox * sub + 1) / sub * vs
    out = np.full(len(hits), np.nan)
    vol = (value, weight)
    pts = (hits[:, None, :] + ts[None, :, None] * dirs[:, None, :]).reshape(-1, 3)
    s = sc.sample_points(vol, case["vs"], pts.astype(F32), None, 1, None, np.float64)
    f = np.where(s["status"] == sc.OK, s["value"], np.nan).reshape(len(hits), len(ts))
    for r in range(len(hits)):
        row = f[r]
        sgn = np.nonzero((row[:-1] > 0) & (row[1:] <= 0))[0]
        if len(sgn):
            j = sgn[np.argmin(np.abs(ts[sgn]))]
            out[r] = abs(ts[j] + (ts[j + 1] - ts[j]) * row[j] / (row[j] - row[j + 1]))
    return out
