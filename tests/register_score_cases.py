"""Cases and the model for xs_tsdf_score_points (x-slam_amd/csrc/xs_register.hip: k_register_score) and the registration
with no starting guess built on it (register_search_host.hpp; KinectFusion.register_points_global), shared by tests/test_register_score_cpu.py,
tests/test_register_score_gpu.py and tests/test_register_global_pipeline_gpu.py.

THE MODEL is the contract of include/xslam_amd.h in numpy float32, written from the header and not from the kernel.  The scored points are
points 0, stride, 2 stride, ...; the transformed point P, the status and the residual r are sample_cases.sample_points' (imported, not
restated: the contract declares them the status and value xs_tsdf_sample_points writes); a point is kept iff its status is OK and
|r| <= max_residual; a kept point's term is the float32 product r * r.  The library is built with -ffp-contract=off, so a correct kernel forms
the model's terms bit for bit: its count EQUALS the model's, and its sum differs from the model's double sum of the terms only by the
six-level float tree that adds each 64-point chunk first.  All terms are >= 0, so |sum_gpu - sum_model| <= 8 u sum_model, u = 2^-24
(align_score_cases' bound and DESIGN.md section 4.17's derivation).  score_many() is the same model over many transforms at once through
sample_cases.trilinear, the function sample_points itself calls; the CPU test holds it to score_model bit for bit.

Cases: register_cases' volumes, clouds and transforms (ragged, pitched, rows past 2^31 bytes) at strides 1, 2, 3 and 7.  CONDITIONS on every
(case, stride) with 255 scored points or more, asserted by tests/test_register_score_cpu.py: each of the three gates (outside, unseen,
residual) drops a point, a point is kept, and no |r| lies within 2^-22 of max_residual without being EQUAL to it.  Points whose |r| equals
max_residual are wanted: register_cases' identity cases plant them, the gate "|r| <= max_residual" keeps them and a gate written "<" drops
them.  register_cases' own seeds meet the conditions at every stride except big_rows', whose seed is bumped here until they hold.

MUTANTS: mistakes a kernel could make, each of which must change a pair of some (case, stride) beyond the GPU test's tolerance.

THE SEARCH FIXTURE: align_score_cases' analytic scene (48^3 voxels of 0.1 m, truncation 0.3 m) as the map and a deterministic cloud on its
surface, handed over moved by scene_truth(degrees): the answer is that transform's inverse."""
import functools

import numpy as np

import align_cases as ac
import align_score_cases as asc
import register_cases as rg
import render_cases as rc
import sample_cases as sc

U, F32 = 2.0 ** -24, np.float32
NEAR = 2.0 ** -22
SUM_BOUND_U = 8        # |sum_gpu - sum_model| <= SUM_BOUND_U u sum_model
STRIDES = (1, 2, 3, 7)
FULL_CASE_COUNT = 255
MAX_TRANSFORMS = 4096
MAX_BLOCKS = 1024      # the grid's workgroup cap per tile: 4096 chunks a round
# the gate as <; scored points taken as stride i + stride - 1; the last chunk's tail counted (its lanes read the last scored point again); unseen
# points kept with the stored word; a row offset taken modulo 2^32; t added before the rotation sums; the stride ignored
MUTANTS = ("gate_lt", "stride_last", "tail", "unseen_kept", "row_wrap32", "t_first", "stride_ignored")


# ------------------------------------------------------------------------------------------------
# The model
def scored_points(pts, stride, mutant=None):
    pts = np.asarray(pts, F32).reshape(-1, 3)
    if mutant == "stride_ignored":
        return pts
    if mutant == "stride_last":
        return pts[stride - 1::stride]
    return pts[::stride]


def _keep(status, r, max_residual, mutant):
    ok = status == sc.OK
    mr = F32(max_residual)
    with np.errstate(invalid="ignore"):
        inside = (np.abs(r) < mr) if mutant == "gate_lt" else (np.abs(r) <= mr)
    return ok, ok & inside


def _unseen_kept(case, P, status, r, min_weight):
    """The unseen_kept mutant: an UNSEEN point's r is the interpolation of the stored words, and the point goes on to the residual gate."""
    st2, v2 = sc.trilinear([case["vol"][0].astype(F32)], case["vol"][1], F32(case["vs"]), -(1 << 40), P, F32, None, case["pitch"])
    unseen = status == sc.UNSEEN
    return np.where(unseen, np.uint8(sc.OK), status), np.where(unseen, v2[0], r)


def score_model(case, xform, stride=1, mutant=None, pts=None, min_weight=None, max_residual=None):
    """The contract for one transform xform [12] float32 over the case's cloud (or pts): dict(kept [scored] bool, terms [scored] float32
    (r * r where kept, else 0), sum (the terms added in float64), count, the scored points dropped at each gate (outside, unseen, residual),
    near (|r| within NEAR of max_residual without equalling it) and equal (|r| == max_residual))."""
    pts = rg.all_points(case) if pts is None else pts
    q = scored_points(pts, stride, mutant)
    mw = case["min_weight"] if min_weight is None else min_weight
    mr = case["max_residual"] if max_residual is None else max_residual
    m = np.asarray(xform, F32).reshape(12)
    if mutant == "t_first":
        p = [q[:, c] for c in range(3)]
        P = [((m[9 + c] + m[3 * c] * p[0]) + m[3 * c + 1] * p[1]) + m[3 * c + 2] * p[2] for c in range(3)]
        assert all(x.dtype == F32 for x in P)
        s = sc._sample(case["vol"], case["vs"], P, mw, None, F32, None, case["pitch"])
    else:
        s = sc.sample_points(case["vol"], case["vs"], q, m, mw, None, F32, "row_wrap32" if mutant == "row_wrap32" else None, case["pitch"])
    status, r = s["status"], s["value"]
    if mutant == "unseen_kept":
        status, r = _unseen_kept(case, s["P"], status, r, mw)
    ok, kept = _keep(status, r, mr, mutant)
    with np.errstate(invalid="ignore"):
        terms = np.where(kept, r * r, F32(0)).astype(F32)
    assert terms.dtype == F32
    total, count = float(terms.astype(np.float64).sum()), int(kept.sum())
    if mutant == "tail" and len(q) % 64:
        extra = 64 - len(q) % 64
        total, count = total + extra * float(terms[-1]), count + extra * int(kept[-1])
    d = np.abs(np.abs(r[ok].astype(np.float64)) - float(F32(mr)))
    return dict(kept=kept, terms=terms, sum=total, count=count, outside=int((status == sc.OUTSIDE).sum()), unseen=int((status == sc.UNSEEN).sum()),
                residual=int((ok & ~kept).sum()), near=int(((d > 0) & (d < NEAR)).sum()), equal=int((d == 0).sum()), scored=len(q))


def score_many(vol, vs, pts, xforms, stride=1, min_weight=1, max_residual=0.9, pitch=None, batch=256):
    """{sum, count} [P, 2] float64 of the model for xforms [P, 12] float32, many transforms per numpy call (sample_cases.trilinear on [B, scored]
    arrays): what the search fixture's scorer uses."""
    q = scored_points(pts, stride)
    p = [q[:, c][None, :] for c in range(3)]
    val, weight = vol[0].astype(F32), vol[1]
    xforms = np.ascontiguousarray(xforms, F32).reshape(-1, 12)
    out = np.zeros((len(xforms), 2))
    for b0 in range(0, len(xforms), batch):
        m = xforms[b0:b0 + batch]
        with np.errstate(invalid="ignore", over="ignore"):
            P = [((m[:, 3 * c, None] * p[0] + m[:, 3 * c + 1, None] * p[1]) + m[:, 3 * c + 2, None] * p[2]) + m[:, 9 + c, None] for c in range(3)]
            status, v = sc.trilinear([val], weight, F32(vs), max(1, int(min_weight)), P, F32, None, pitch)
            _, kept = _keep(status, v[0], max_residual, None)
            terms = np.where(kept, v[0] * v[0], F32(0)).astype(F32)
        out[b0:b0 + len(m), 0] = terms.astype(np.float64).sum(axis=1)
        out[b0:b0 + len(m), 1] = kept.sum(axis=1)
    return out


def nblocks_of(scored):
    return int(min(max(((scored + 63) // 64 + 3) // 4, 1), MAX_BLOCKS))


def differs(a, b):
    """Whether pair b lies outside the GPU test's tolerance about pair a (dicts with sum and count)."""
    return a["count"] != b["count"] or abs(a["sum"] - b["sum"]) > SUM_BOUND_U * U * a["sum"]


# ------------------------------------------------------------------------------------------------
# The cases
def conditions_hold(case, stride):
    ev = score_model(case, case["xform"], stride)
    if ev["scored"] < FULL_CASE_COUNT:
        return ev["near"] == 0
    return ev["near"] == 0 and min(ev["outside"], ev["unseen"], ev["residual"], ev["count"]) > 0


@functools.lru_cache(maxsize=None)
def big_case():
    """register_cases.big_case()'s recipe (the (65, 33, 64) volume of sample_cases.big_case, rows past 2^31 bytes in rows of 1 MiB, half of the
    points over the sphere's cap between planes 62.0 and 62.3), its seed bumped until the conditions hold at every stride."""
    b = sc.big_case()
    X, Y, Z = rc.BIG_SHAPE
    rng = np.random.default_rng(70)
    g = np.stack([rng.uniform(32.0 - 2.2, 32.0 + 2.2, 4000), rng.uniform(16.0 - 2.2, 16.0 + 2.2, 4000), rng.uniform(Z - 2.0, Z - 1.7, 4000)], axis=1)
    extra = ((g + 0.5) * float(sc.VS2)).astype(F32)
    for seed in range(12, 60):
        case = rg._case("big_rows", tuple(np.array(a) for a in b["vol"]), sc.VS2, 1000, seed, extra_pts=extra)
        if all(conditions_hold(case, s) for s in STRIDES):
            return case
    raise AssertionError("no seed gives big_rows its conditions at every stride")


@functools.lru_cache(maxsize=None)
def cases():
    return rg.cases()


def wrap_case():
    """For the model alone (the row_wrap32 mutant): register_cases.wrap_case(), rows of 2^28 bytes."""
    return rg.wrap_case()


@functools.lru_cache(maxsize=None)
def expected(name, stride=1):
    """The model's result for a case's own transform at a stride, computed once and shared: never modified."""
    case = {c["name"]: c for c in cases() + (big_case(),)}[name]
    ev = score_model(case, case["xform"], stride)
    for a in (ev["kept"], ev["terms"]):
        a.setflags(write=False)
    return ev


def transforms(case, count, seed=5):
    """`count` transforms [count, 12] float32: the case's own, one that maps every point outside, and small rigid motions in front of the case's."""
    rng = np.random.default_rng(seed)
    out = [np.asarray(case["xform"], F32).copy(), rg.MISS12.copy()]
    while len(out) < count:
        _, T = sc.rigid(int(rng.integers(1 << 30)), float(rng.uniform(-0.2, 0.2)), rng.uniform(-0.1, 0.1, 3))
        out.append(rg.xform12_of(T @ case["T"]))
    return np.stack(out[:count]).astype(F32)


# ------------------------------------------------------------------------------------------------
# The search fixture
SCENE_CLOUD_POINTS, SCENE_HALF_POINTS = 8443, 3912
# The bound of tests/test_align_global_pipeline_gpu.py, the project's own for a search that ends in a Gauss-Newton loop: the result lies within
# 0.01 voxel edges of worst-corner displacement of the loop started at the truth, and reaches 0.98 of its S.
SEARCH_AGREEMENT_VOXELS, SEARCH_S_FRACTION = 0.01, 0.98


@functools.lru_cache(maxsize=None)
def scene_cloud(half=False):
    """Points on the scene's surface in the MAP's frame, float64 [n, 3]: 1500 directions per sphere, 3000 floor points, 2000 wall points from
    default_rng(1), those kept that lie on the surface (|scene_sdf| < 1e-9: not inside another object) with every coordinate in (0.15, 4.65).
    half: the part with y < 2.4, whose centroid lies 0.84 m from the map's band centroid."""
    rng = np.random.default_rng(1)
    pts = []
    for c, r in asc.SCENE_SPHERES:
        d = rng.normal(size=(1500, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        pts.append(np.asarray(c, np.float64) + r * d)
    ext = asc.SCENE_N * asc.SCENE_VS
    xy = rng.uniform(0, ext, (3000, 2))
    pts.append(np.c_[xy, np.full(3000, asc.SCENE_FLOOR_Z)])
    yz = rng.uniform(0, ext, (2000, 2))
    pts.append(np.c_[np.full(2000, asc.SCENE_WALL_X), yz])
    pm = np.concatenate(pts)
    pm = pm[(np.abs(asc.scene_sdf(pm)) < 1e-9) & (pm > 0.15).all(axis=1) & (pm < 4.65).all(axis=1)]
    if half:
        pm = pm[pm[:, 1] < 2.4]
    pm.setflags(write=False)
    return pm


@functools.lru_cache(maxsize=None)
def handed_cloud(degrees, half=False):
    """(cloud float32 [n, 3] as the caller receives it: the scene's points moved by scene_truth(degrees); T_answer [4, 4]: cloud frame to map frame)."""
    Tt = asc.scene_truth(degrees)
    cloud = np.ascontiguousarray((scene_cloud(half) @ Tt[:3, :3].T + Tt[:3, 3]).astype(F32))
    cloud.setflags(write=False)
    return cloud, np.linalg.inv(Tt)


@functools.lru_cache(maxsize=None)
def scene_case():
    """The map of the fixture as a register_cases case (for point_terms and loop): dense rows, min_weight 1, max_residual 0.9."""
    n = asc.SCENE_N
    return dict(kind="points", name="scene", vol=asc.scene_volume(), vs=F32(asc.SCENE_VS), shape=(n, n, n), xform=None, T=np.eye(4), min_weight=1, grad=None,
                max_residual=float(F32(0.9)), pitch=n * 4, offset=0, tile=1)


def map_band_centroid(value, vs, pl):
    return pl.band_centroid(ac.keys_of(ac.band_of(value)[0]), vs)


def search_on_the_model(cloud, vol, vs, candidates, keep, rounds, stride, box_t, refine_t, refine_r, pl, min_weight=1, max_residual=0.9, log=None):
    """The search of register_points_global with the model as the scorer and the library's host entries for everything else (built like
    align_score_cases.search_on_the_model): the kept transforms [K, 4, 4] after the last round, best first, and their S on the strided cloud."""
    c_cloud = pl.points_centroid(cloud, stride)
    c_map = map_band_centroid(vol[0], vs, pl)

    def score(Ts):
        x = np.stack([rg.xform12_of(T) for T in Ts])
        return score_many(vol, vs, cloud, x, stride, min_weight, max_residual)

    cand = pl.transform_candidates_free(candidates, c_cloud, c_map, box_t)
    out = score(cand)
    idx = pl.transform_rank(out, keep)
    kept, S = cand[idx], out[idx, 1] - out[idx, 0]
    bt, br = refine_t, refine_r
    for r in range(rounds):
        if log is not None:
            log.append((r, S.copy()))
        cand = np.concatenate([pl.transform_candidates_around(T, c_cloud, bt, br, max(1, candidates // keep)) for T in kept])
        out = score(cand)
        idx = pl.transform_rank(out, keep)
        kept, S = cand[idx], out[idx, 1] - out[idx, 0]
        bt, br = 0.5 * bt, 0.5 * br
    return kept, S


# ------------------------------------------------------------------------------------------------
# Device helpers (torch and capi are handed in by the GPU tests)
class ScoreRunner:
    """A workspace (tickets zeroed once, the rest a pattern) and an output buffer with guards for xs_tsdf_score_points."""

    def __init__(self, torch, capi, transforms=MAX_TRANSFORMS):
        self.torch, self.capi = torch, capi
        self.ws = torch.full((capi.tsdf_score_points_workspace_bytes(transforms),), 0x5A, dtype=torch.uint8, device="cuda")
        capi.tsdf_reduce_workspace_init(self.ws)
        self.out = torch.full((2 * transforms + 16,), -7.0, dtype=torch.float64, device="cuda")

    def run(self, n, points, vol, case, xforms, stride=1, min_weight=None, max_residual=None):
        """xforms [P, 12] over n points at device address `points`: [P, 2] = {sum r^2, count}.  vol: value.addr, weight.addr, pitch, res."""
        xforms = np.ascontiguousarray(xforms, F32).reshape(-1, 12)
        P = xforms.shape[0]
        self.out.fill_(-7.0)
        self.capi.tsdf_score_points(n, points, xforms, vol.value.addr, vol.weight.addr, vol.pitch, vol.res, float(case["vs"]),
                                    case["min_weight"] if min_weight is None else min_weight, case["max_residual"] if max_residual is None else max_residual,
                                    self.ws, self.out, stride=stride)
        self.torch.cuda.synchronize()
        host = self.out.cpu().numpy()
        assert (host[2 * P:] == -7.0).all(), "wrote past its transforms' pairs"
        return host[:2 * P].reshape(P, 2).copy()

    def tickets_zero(self):
        return not self.ws[:256].any().item()

    def rest_is_pattern_or_written(self):
        """The workspace past the tickets: a launch writes its transforms and records there and nothing else; the bytes it never reaches keep
        the pattern (the last kilobyte of the full-size workspace belongs to tile 63's last record, which only a 1024-workgroup launch writes)."""
        return bool((self.ws[-1024:] == 0x5A).all().item())


def check(got, ev, what):
    """One transform's pair against the model."""
    assert got[1] == ev["count"], (what, got[1], ev["count"])
    assert abs(got[0] - ev["sum"]) <= SUM_BOUND_U * U * ev["sum"], (what, got[0], ev["sum"])
    if ev["count"] == 0:
        assert got[0] == 0.0 and not np.signbit(got[0]), what
