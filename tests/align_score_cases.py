"""The cases that hold the transform score (xs_tsdf_score_transforms, x-slam_amd/csrc/xs_align.hip: k_align_score) and the alignment with no
guess built on it (align_search_host.hpp; KinectFusion.align_map_global) to a model written from the per-entry contract in
include/xslam_amd.h and not from the kernel, nor from align_cases.evaluate.  Test infrastructure; backend-neutral parts first
(tests/test_align_score_cpu.py), the device helpers after them (the GPU tests hand torch in).

THE MODEL is the contract in numpy float32, operation by operation.  The library is built with -ffp-contract=off, so a correct kernel
forms the model's float32 products r * r bit for bit; it differs from the model's double sum of them only by the six-level float tree
that adds each 64-entry chunk first.  All terms are >= 0: a pairwise float tree of depth 6 is off by at most 6 u (1 + 6 u) of its sum
(u = 2^-24) and the double additions after it by n 2^-53 of theirs, so |sum_gpu - sum_model| <= 8 u sum_model (DESIGN.md section 4.17's
derivation; 8 leaves the second order and the doubles room).

Case data: align_cases' generators (source volumes with a quarter of the weights zero in blocks, fabricated indices), its shapes, index
counts, pitches, min_weights and transforms (the real parts of its seeded maps).  CONDITION on every case of FULL_CASE_COUNT entries or more,
over its transforms and min_weights together: each of the three gates drops an entry, an entry is kept, and no entry's |r| lies within
4 * 2^-24 * (|F| + |gt|) of max_residual (F carries at most three stages of three roundings on magnitudes <= max |corner|, so the model's own
F - gt is within that of any other association; inside the margin a count could differ for reasons that are no error).  The seed is bumped
until this holds; tests/test_align_score_cpu.py asserts it.

THE SEARCH FIXTURE: an analytic scene on 48^3 voxels of 0.1 m, truncation 0.3 m — three spheres, a floor and a wall — as this map, and the
same scene under T_true (a rotation about an axis through the volume's centre, plus a shift) as the other map, both generated here."""
import functools

import numpy as np

import align_cases as ac

U = 2.0 ** -24
F32 = np.float32
MAX_RESIDUAL = 1.0
MIN_WEIGHTS = ac.MIN_WEIGHTS
SOURCE_SHAPES = ac.SOURCE_SHAPES
INDEX_COUNTS = ac.INDEX_COUNTS
FULL_CASE_COUNT = 255
SUM_BOUND_U = 8       # |sum_gpu - sum_model| <= SUM_BOUND_U u sum_model
STRIDES = (1, 2, 3, 7)
MAX_TRANSFORMS = 4096


# ------------------------------------------------------------------------------------------------
# The model
def score_model(xyz, gt, src, m12, min_weight=1, max_residual=MAX_RESIDUAL):
    """The per-entry contract on index entries (xyz [n, 3], gt [n]) against src = (value, weight) [Z, Y, X] under the real index map m12.
    Returns a dict: kept [n] bool, terms [n] float32 (r * r where kept, else 0), sum (the terms added in float64), count, the entries
    dropped at each gate (outside, weight, residual) and near (entries inside the margin of the condition on the cases)."""
    sv, sw = src
    SZ, SY, SX = sv.shape
    S = (SX, SY, SZ)
    n = len(gt)
    m = np.asarray(m12, F32).reshape(12)
    gt = np.asarray(gt, F32)
    c = [np.asarray(xyz)[:, a].astype(F32) for a in range(3)]
    # 1. the index under the map
    with np.errstate(over="ignore", invalid="ignore"):
        g = [((m[3 * a] * c[0] + m[3 * a + 1] * c[1]) + m[3 * a + 2] * c[2]) + m[9 + a] for a in range(3)]
        # 2. the cell rule
        inside = np.ones(n, bool)
        for a in range(3):
            inside &= (g[a] >= F32(0)) & (g[a] < F32(S[a] - 1))
    sel = np.flatnonzero(inside)
    b = [np.floor(g[a][sel]).astype(np.int64) for a in range(3)]
    f = [g[a][sel] - b[a].astype(F32) for a in range(3)]
    cm = [F32(1.0) - f[a] for a in range(3)]
    assert all(x.dtype == F32 for x in f + cm)
    # 3. the weight gate: all eight corners
    corner = [(b[0] + (d & 1), b[1] + (d >> 1 & 1), b[2] + (d >> 2 & 1)) for d in range(8)]
    wmin = np.full(len(sel), np.iinfo(np.int64).max, np.int64)
    for d in range(8):
        wmin = np.minimum(wmin, sw[corner[d][2], corner[d][1], corner[d][0]])
    heavy = wmin >= min_weight
    hs = np.flatnonzero(heavy)
    v = [sv[corner[d][2][hs], corner[d][1][hs], corner[d][0][hs]].astype(F32) for d in range(8)]
    f, cm = [x[hs] for x in f], [x[hs] for x in cm]
    # 4. x, then y, then z
    x00, x10 = v[0] * cm[0] + v[1] * f[0], v[2] * cm[0] + v[3] * f[0]
    x01, x11 = v[4] * cm[0] + v[5] * f[0], v[6] * cm[0] + v[7] * f[0]
    y0, y1 = x00 * cm[1] + x10 * f[1], x01 * cm[1] + x11 * f[1]
    F = y0 * cm[2] + y1 * f[2]
    # 5. the residual gate
    r = F - gt[sel][hs]
    assert r.dtype == F32
    ok = np.abs(r) <= F32(max_residual)
    near = np.abs(np.abs(r).astype(np.float64) - max_residual) <= 4 * U * (np.abs(F).astype(np.float64) + np.abs(gt[sel][hs]).astype(np.float64))
    # 6. the terms
    kept = np.zeros(n, bool)
    kept[sel[hs[ok]]] = True
    terms = np.zeros(n, F32)
    terms[sel[hs[ok]]] = (r * r)[ok]
    return dict(kept=kept, terms=terms, sum=float(terms.astype(np.float64).sum()), count=int(ok.sum()), outside=int(n - len(sel)),
                weight=int(len(sel) - len(hs)), residual=int(len(hs) - ok.sum()), near=int(near.sum()))


def strided(xyz, gt, stride):
    """The scored entries of the contract: index entries 0, stride, 2 stride, ..."""
    return xyz[::stride], gt[::stride]


# ------------------------------------------------------------------------------------------------
# The kernel's cases
@functools.lru_cache(maxsize=None)
def case_xforms(sshape):
    """name -> xform12 float32 [12]: the real parts of align_cases' seeded maps (every seed's are the same)."""
    out = {k: np.ascontiguousarray(v[0, :, 0], F32) for k, v in ac.case_maps(sshape).items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def condition(xyz, gt, src, sshape):
    """(holds for a full case, near-threshold entries) over the case's transforms and min_weights together."""
    evs = [score_model(xyz, gt, src, m, mw) for m in case_xforms(sshape).values() for mw in MIN_WEIGHTS]
    near = sum(ev["near"] for ev in evs)
    full = all(sum(ev[k] for ev in evs) > 0 for k in ("outside", "weight", "residual", "count"))
    return full, near


@functools.lru_cache(maxsize=None)
def case(sshape, count):
    """(xyz, gt, src): `count` fabricated entries over dst_shape_of(sshape) and a source, align_cases' generators and seeds, the seed bumped
    until the condition on the cases holds."""
    for bump in range(400):
        rng = np.random.default_rng(ac.case_seed(sshape, count) + 7 * bump)
        src = ac.source(rng, sshape)
        xyz, gt = ac.fabricated_index(rng, count, ac.dst_shape_of(sshape))
        full, near = condition(xyz, gt, src, sshape)
        if near or (count >= FULL_CASE_COUNT and not full):
            continue
        for a in (xyz, gt) + src:
            a.setflags(write=False)
        return xyz, gt, src
    raise AssertionError("no seed that meets the condition on the cases")


@functools.lru_cache(maxsize=None)
def expected(sshape, count, name, min_weight, stride=1):
    xyz, gt, src = case(sshape, count)
    return score_model(*strided(xyz, gt, stride), src, case_xforms(sshape)[name], min_weight)


@functools.lru_cache(maxsize=None)
def large_case(count=300000, sshape=(9, 10, 13)):
    """More scored entries than one round of the grid (1024 workgroups x 4 waves x 64 lanes): fabricated entries, repeats allowed."""
    for bump in range(50):
        rng = np.random.default_rng(300007 + bump)
        src = ac.source(rng, sshape)
        xyz, gt = ac.fabricated_index(rng, count, ac.dst_shape_of(sshape))
        full, near = condition(xyz, gt, src, sshape)
        if full and not near:
            return xyz, gt, src
    raise AssertionError("no seed that meets the condition on the cases")


# ------------------------------------------------------------------------------------------------
# The search fixture
SCENE_N, SCENE_VS, SCENE_TRUNC = 48, 0.1, 0.3
SCENE_SPHERES = (((1.6, 2.0, 2.6), 0.7), ((3.2, 2.4, 2.0), 0.45), ((2.4, 3.4, 3.0), 0.3))
SCENE_FLOOR_Z, SCENE_WALL_X = 3.9, 4.3
SCENE_AXIS, SCENE_SHIFT = (0.5, -0.3, 1.0), (0.23, -0.17, 0.11)
SCENE_BAND_VOXELS = 29816


def scene_sdf(p):
    """The signed distance of the scene at points p [..., 3] (metres, THIS map's frame), float64."""
    d = np.minimum(SCENE_FLOOR_Z - p[..., 2], SCENE_WALL_X - p[..., 0])
    for c, r in SCENE_SPHERES:
        d = np.minimum(d, np.linalg.norm(p - np.asarray(c, np.float64), axis=-1) - r)
    return d


def scene_truth(degrees):
    """T_true: this map's frame -> the other's: a rotation by `degrees` about SCENE_AXIS through the volume's centre, plus SCENE_SHIFT."""
    c = 0.5 * SCENE_N * SCENE_VS * np.ones(3)
    T = np.eye(4)
    T[:3, :3] = ac.rotation(SCENE_AXIS, np.radians(degrees))
    T[:3, 3] = c - T[:3, :3] @ c + np.asarray(SCENE_SHIFT, np.float64)
    return T


@functools.lru_cache(maxsize=None)
def scene_volume(degrees=None):
    """(value float32, weight int32) [Z, Y, X]: this map (degrees None) or the other map under scene_truth(degrees).  value = clip(sdf / trunc,
    -1, 1); weight 1 where sdf > -trunc and the point lies inside this map's cube, else weight 0 and value 0."""
    ax = (np.arange(SCENE_N, dtype=np.float64) + 0.5) * SCENE_VS
    zz, yy, xx = np.meshgrid(ax, ax, ax, indexing="ij")
    p = np.stack([xx, yy, zz], axis=-1)
    if degrees is not None:
        Ti = np.linalg.inv(scene_truth(degrees))
        p = p @ Ti[:3, :3].T + Ti[:3, 3]
    d = scene_sdf(p)
    ext = SCENE_N * SCENE_VS
    seen = (d > -SCENE_TRUNC) & (p >= 0).all(axis=-1) & (p <= ext).all(axis=-1)
    value = np.where(seen, np.clip(d / SCENE_TRUNC, -1.0, 1.0), 0.0).astype(F32)
    weight = seen.astype(np.int32)
    value.setflags(write=False)
    weight.setflags(write=False)
    return value, weight


def search_on_the_model(this_value, other, vs, candidates, keep, rounds, stride, box_t, refine_t, refine_r, pl, min_weight=1, log=None):
    """The search of align_map_global with the model as the scorer and the library's host entries for everything else: the kept transforms
    [K, 4, 4] after the last round, best first, and their S on the strided band."""
    xyz, gt = ac.band_of(this_value)
    sx, sg = strided(xyz, gt, stride)
    c_this = pl.band_centroid(ac.keys_of(xyz), vs)
    c_other = pl.band_centroid(ac.keys_of(ac.band_of(other[0])[0]), vs)

    def score(Ts):
        out = np.zeros((len(Ts), 2))
        for i, T in enumerate(Ts):
            ev = score_model(sx, sg, other, pl.merge_affine(T, vs, vs), min_weight)
            out[i] = ev["sum"], ev["count"]
        return out

    cand = pl.transform_candidates_free(candidates, c_this, c_other, box_t)
    out = score(cand)
    idx = pl.transform_rank(out, keep)
    kept, S = cand[idx], out[idx, 1] - out[idx, 0]
    bt, br = refine_t, refine_r
    for r in range(rounds):
        if log is not None:
            log.append((r, S.copy()))
        cand = np.concatenate([pl.transform_candidates_around(T, c_this, bt, br, max(1, candidates // keep)) for T in kept])
        out = score(cand)
        idx = pl.transform_rank(out, keep)
        kept, S = cand[idx], out[idx, 1] - out[idx, 0]
        bt, br = 0.5 * bt, 0.5 * br
    return kept, S


# ------------------------------------------------------------------------------------------------
# Device helpers (torch and capi are handed in by the GPU tests)
class ScoreRunner:
    """A workspace (tickets zeroed once, the rest a pattern) and an output buffer with guards for xs_tsdf_score_transforms."""

    def __init__(self, torch, capi, transforms=MAX_TRANSFORMS):
        self.torch, self.capi = torch, capi
        self.ws = torch.full((capi.tsdf_score_transforms_workspace_bytes(transforms),), 0x5A, dtype=torch.uint8, device="cuda")
        capi.tsdf_reduce_workspace_init(self.ws)
        self.out = torch.full((2 * transforms + 16,), -7.0, dtype=torch.float64, device="cuda")

    def run(self, index, dev, sshape, xforms, min_weight=1, stride=1, max_residual=MAX_RESIDUAL):
        """xforms [P, 12]: [P, 2] = {sum r^2, count}."""
        xforms = np.ascontiguousarray(xforms, F32).reshape(-1, 12)
        P = xforms.shape[0]
        self.out.fill_(-7.0)
        self.capi.tsdf_score_transforms(index, stride, dev.value.addr, dev.weight.addr, dev.pitch, list(sshape), xforms, min_weight, max_residual, self.ws, self.out)
        self.torch.cuda.synchronize()
        host = self.out.cpu().numpy()
        assert (host[2 * P:] == -7.0).all(), "wrote past its transforms' pairs"
        return host[:2 * P].reshape(P, 2).copy()

    def tickets_zero(self):
        return not self.ws[:256].any().item()


def check(got, ev, what):
    """One transform's pair against the model."""
    assert got[1] == ev["count"], (what, got[1], ev["count"])
    assert abs(got[0] - ev["sum"]) <= SUM_BOUND_U * U * ev["sum"], (what, got[0], ev["sum"])
    if ev["count"] == 0:
        assert got[0] == 0.0 and not np.signbit(got[0]), what
