"""GPU: xs_tsdf_score_points (x-slam_amd/csrc/xs_register.hip: k_register_score) against the model of tests/register_score_cases.py.  The kernel's
float32 terms r * r are the model's bit for bit, so the count must EQUAL the model's and the sum may differ from the model's double sum only by
the six-level float tree per chunk: 8 * 2^-24 * sum (all terms are >= 0), and +0.0 where nothing is kept.  The volumes are pitched, with guard
planes and padding that must come back untouched; the points sit between guard bytes; the output's guards keep their sentinel; the tickets are
zero after every launch on a workspace otherwise filled with a pattern."""
import importlib

import numpy as np
import pytest

import register_cases as rg
import register_score_cases as rs
import render_cases as rc
from test_register_gpu import Guarded, Volume

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CASES = rs.cases()
BY_NAME = {c["name"]: c for c in CASES}
SMALL = [c for c in CASES if c["n"] < rg.BIG_N]


@pytest.fixture(scope="module")
def capi():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("x-slam_amd.capi")


@pytest.fixture(scope="module")
def runner(capi):
    return rs.ScoreRunner(torch, capi)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("case", SMALL, ids=[c["name"] for c in SMALL])
def test_pairs_equal_the_model(capi, runner, case):
    """n = 1, 5, 6, 63, 64, 65, 255, 257 at strides 1, 2, 3, 7 (n is a multiple of the stride only by accident): count equal, sum within the tree
    bound, +0.0 where nothing is kept; a second launch gives the same bytes; the points, the volume and its guard rows untouched; the tickets
    back at zero."""
    vol, pts = Volume(case), Guarded(case["n"] * 12, rg.all_points(case))
    for stride in rs.STRIDES:
        want = rs.expected(case["name"], stride)
        first = runner.run(case["n"], pts.addr, vol, case, case["xform"][None, :], stride)
        rs.check(first[0], want, (case["name"], stride))
        again = runner.run(case["n"], pts.addr, vol, case, case["xform"][None, :], stride)
        assert same(first, again) and runner.tickets_zero()
        print(case["name"], "stride", stride, "kept", int(first[0][1]), "of", want["scored"], "|kernel - model| / sum: %.3g" % (abs(first[0][0] - want["sum"]) / max(want["sum"], 1e-300)))
    assert pts.untouched() and vol.untouched()


def test_transform_counts_and_independence(capi, runner):
    """P = 1, 63, 64, 65, 130 and 4096 on the 65-point cloud (a partial last tile, several tiles, the cap), every pair against the model; and
    transform p's pair is the same bits scored alone, in another slot, or among others."""
    case = BY_NAME["v345_n65_identity_mr03"]
    vol, pts = Volume(case), Guarded(case["n"] * 12, rg.all_points(case))
    X = rs.transforms(case, rs.MAX_TRANSFORMS)
    X_before = X.copy()
    want = rs.score_many(case["vol"], case["vs"], rg.all_points(case), X, 1, case["min_weight"], case["max_residual"], case["pitch"])
    assert (want[:, 1] > 0).sum() > 3000 and want[1, 1] == 0
    full = runner.run(case["n"], pts.addr, vol, case, X)
    assert np.array_equal(X.view(np.uint32), X_before.view(np.uint32))          # the host's transforms are only read
    for p in range(rs.MAX_TRANSFORMS):
        rs.check(full[p], dict(sum=want[p, 0], count=want[p, 1]), p)
    assert full[1, 0] == 0.0 and not np.signbit(full[1, 0]) and full[1, 1] == 0
    for P in (1, 63, 64, 65, 130):
        got = runner.run(case["n"], pts.addr, vol, case, X[:P])
        assert same(got, full[:P]), P
    order = np.random.default_rng(6).permutation(130)
    assert same(runner.run(case["n"], pts.addr, vol, case, X[order]), full[order])
    for p in (0, 1, 64, 129, 4095):
        assert same(runner.run(case["n"], pts.addr, vol, case, X[p:p + 1]), full[p:p + 1]), p
    # strides on many transforms: a pair depends on the scored points alone
    for stride in (2, 7):
        got = runner.run(case["n"], pts.addr, vol, case, X[:130], stride)
        w = rs.score_many(case["vol"], case["vs"], rg.all_points(case), X[:130], stride, case["min_weight"], case["max_residual"], case["pitch"])
        for p in range(130):
            rs.check(got[p], dict(sum=w[p, 0], count=w[p, 1]), (stride, p))
    assert pts.untouched() and vol.untouched() and runner.tickets_zero() and runner.rest_is_pattern_or_written()


def test_more_chunks_than_one_round_of_the_grid(capi, runner):
    """register_cases.BIG_N points at stride 4: 266240 scored points in 4160 chunks, past the 4096 that 1024 workgroups of four waves take in one
    round; three transforms (the case's own, one that misses, a nearby one)."""
    case = next(c for c in CASES if c["n"] == rg.BIG_N)
    allp = rg.all_points(case)
    vol, pts = Volume(case), Guarded(case["n"] * 12, allp)
    X = rs.transforms(case, 3)
    got = runner.run(case["n"], pts.addr, vol, case, X, 4)
    rs.check(got[0], rs.expected(case["name"], 4), "big, own transform")
    for p in (1, 2):
        rs.check(got[p], rs.score_model(case, X[p], 4, pts=allp), ("big", p))
    assert got[0][1] > 40000 and got[1][1] == 0
    assert same(got, runner.run(case["n"], pts.addr, vol, case, X, 4)) and same(got[2:3], runner.run(case["n"], pts.addr, vol, case, X[2:3], 4))
    assert pts.untouched() and vol.untouched() and runner.tickets_zero()


def test_agrees_with_register_terms_where_every_gradient_is_accepted(capi, runner):
    """Stride 1 on a cloud none of whose OK points has a refused gradient: the count equals xs_tsdf_register_terms' slot 28 and sum r^2 its slot 27
    within the tree bound (that call adds the same float32 r, squared exactly in double)."""
    case = BY_NAME["plane_n257_identity_mw3"]
    pt = rg.expected(case["name"])["point"]
    sel = rg.all_points(case)[~(pt["ok"] & ~pt["gok"])]
    assert 150 < len(sel) < case["n"]
    vol, pts = Volume(case), Guarded(len(sel) * 12, sel)
    got = runner.run(len(sel), pts.addr, vol, case, case["xform"][None, :])
    ws = torch.zeros(capi.register_workspace_bytes(1), dtype=torch.uint8, device="cuda")
    out29 = torch.zeros(29, dtype=torch.float64, device="cuda")
    capi.register_terms(len(sel), pts.addr, case["xform"][None, :], vol.value.addr, vol.weight.addr, vol.pitch, vol.res, float(case["vs"]), case["min_weight"],
                        case["max_residual"], ws, out29)
    torch.cuda.synchronize()
    terms = out29.cpu().numpy()
    assert got[0][1] == terms[28] == pt["kept"].sum() > 20
    # r * r rounded to float32 against the exact square: u per term on top of the tree's bound
    assert abs(got[0][0] - terms[27]) <= (rs.SUM_BOUND_U + 1) * rs.U * terms[27], (got[0][0], terms[27])


def test_rows_past_2_31_bytes(capi, runner):
    """The (65, 33, 64) volume in rows of 1 MiB: 2112 rows, the last ones past 2^31 bytes, at every stride."""
    case = rs.big_case()
    X, Y, Z = case["shape"]
    pitch = rc.BIG_PITCH
    rows = Y * Z
    assert (rows - 1) * pitch > 2 ** 31
    buf = torch.full((rows * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
    words = buf.view(torch.int32)
    segs = [words.as_strided((Z, Y, X), (Y * (pitch // 4), pitch // 4, 1), k * 128) for k in range(2)]      # segments 512 bytes apart
    for seg, a in zip(segs, case["vol"]):
        seg.copy_(torch.from_numpy(np.array(a).view(np.int32)).cuda())

    class Vol:
        pass
    vol = Vol()
    vol.pitch, vol.res = pitch, [X, Y, Z]
    for name, k in (("value", 0), ("weight", 1)):
        seg = Vol()
        seg.addr = buf.data_ptr() + k * 512
        setattr(vol, name, seg)
    pts = Guarded(case["n"] * 12, rg.all_points(case))
    high = rg.high_rows_kept(case, rg.point_terms(case))
    assert high.sum() >= 50
    for stride in rs.STRIDES:
        want = rs.expected(case["name"], stride)
        assert (want["kept"] & high[::stride]).sum() >= 5
        rs.check(runner.run(case["n"], pts.addr, vol, case, case["xform"][None, :], stride)[0], want, ("big rows", stride))
    assert pts.untouched() and runner.tickets_zero()
    for seg, a in zip(segs, case["vol"]):
        assert np.array_equal(seg.cpu().numpy(), np.ascontiguousarray(a).view(np.int32))
        seg.fill_(-1515870811)                              # 0xA5A5A5A5
    assert bool((buf == 0xA5).all())                        # what lies between the segments kept the pattern


def with_entry(a, i, v):
    b = np.array(a, np.float32).copy()
    b.reshape(-1)[i] = v
    return b


def test_refusals(capi):
    """Each argument error: hipErrorInvalidValue with the call's name in the text, nothing launched: the output's sentinel, the points, the
    volume, the workspace's pattern and the tickets as they were.  The limits themselves are accepted."""
    case = BY_NAME["sphere_n257_rigid_mw3_mr03"]
    vol, pts = Volume(case), Guarded(case["n"] * 12, rg.all_points(case))
    X = rs.transforms(case, rs.MAX_TRANSFORMS)
    out = Guarded(rs.MAX_TRANSFORMS * 2 * 8)
    ws = torch.full((capi.tsdf_score_points_workspace_bytes(rs.MAX_TRANSFORMS),), 0x5A, dtype=torch.uint8, device="cuda")
    capi.tsdf_reduce_workspace_init(ws)
    ws_before = ws.clone()
    good = dict(n=case["n"], points=pts.addr, xforms=X[:3], value=vol.value.addr, weight=vol.weight.addr, vol_step=vol.pitch, res=vol.res, voxel_size=float(case["vs"]),
                min_weight=1, max_residual=0.9, workspace=ws, out2xP=out.addr, stride=1)
    nan, inf = float("nan"), float("inf")
    bad = [dict(transforms=0), dict(transforms=-1), dict(transforms=4097, xforms=np.concatenate([X, X[:1]])), dict(stride=0), dict(stride=-4),
           dict(n=0), dict(n=-1), dict(n=(1 << 30) + 1),
           dict(points=None), dict(xforms=None, transforms=3), dict(value=None), dict(weight=None), dict(res=None), dict(workspace=None), dict(out2xP=None),
           dict(xforms=with_entry(X[:3], 4, nan)), dict(xforms=with_entry(X[:3], 0, inf)), dict(xforms=with_entry(X[:3], 35, -inf)),
           dict(voxel_size=0.0), dict(voxel_size=-0.05), dict(voxel_size=nan), dict(voxel_size=inf),
           dict(res=[0, 17, 20]), dict(res=[33, 17, 65535 * 4 + 1]), dict(res=[33, 65536, 32768]), dict(vol_step=33 * 4 - 4), dict(vol_step=33 * 4 + 2),
           dict(min_weight=0), dict(min_weight=-3), dict(max_residual=0.0), dict(max_residual=-0.5), dict(max_residual=nan), dict(max_residual=inf)]
    for change in bad:
        with pytest.raises(capi.XsError) as e:
            capi.tsdf_score_points(**{**good, **change})
        assert "hip error 1:" in str(e.value) and "xs_tsdf_score_points" in str(e.value), (change, str(e.value))
    torch.cuda.synchronize()
    assert out.untouched() and pts.untouched() and vol.untouched() and torch.equal(ws, ws_before)
    # the limits themselves: one point, one transform and 4096, a stride past the cloud
    capi.tsdf_score_points(**{**good, "n": 1, "xforms": X[:1]})
    capi.tsdf_score_points(**{**good, "xforms": X})
    capi.tsdf_score_points(**{**good, "stride": 1 << 30})
    torch.cuda.synchronize()
    assert out.guards_ok() and not out.untouched() and not bool(ws[:256].any())
