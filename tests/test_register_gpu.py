"""GPU: xs_tsdf_register_terms (x-slam_amd/csrc/xs_register.hip) against the model of tests/register_cases.py.  The kernel's float32 r and J are
the model's bit for bit and every term is an exact double product of float32 factors, so the count must EQUAL the model's and each of the other
28 sums may differ from the model's own chunk-ordered sum only by the association of at most n double additions: n 2^-52 sum |terms|
(tests/test_align_gpu.py argues the same way).  The volumes are pitched, with guard planes and padding that must come back untouched; the
points and the output sit between guard bytes that must keep their pattern; the tickets are zero after every launch."""
import importlib

import numpy as np
import pytest

import register_cases as rg
import render_cases as rc
import sample_cases as sc
from extract_cases import DevVolume

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PATTERN, GUARD = 0xA7, 256
CASES = rg.cases()
BY_NAME = {c["name"]: c for c in CASES}


@pytest.fixture(scope="module")
def capi():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("x-slam_amd.capi")


class Guarded:
    """nbytes of device memory between GUARD bytes of PATTERN on either side, PATTERN inside too.  addr: the first of the nbytes."""

    def __init__(self, nbytes, content=None):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.addr = self.buf.data_ptr() + GUARD
        if content is not None:
            raw = np.ascontiguousarray(content).view(np.uint8).reshape(-1)
            self.buf[GUARD:GUARD + raw.size].copy_(torch.from_numpy(raw.copy()))
        self.before = self.buf.clone()

    def host(self, dtype, shape):
        return self.buf.cpu().numpy()[GUARD:GUARD + self.n].view(dtype).reshape(shape).copy()

    def guards_ok(self):
        a = self.buf.cpu().numpy()
        return bool((a[:GUARD] == PATTERN).all() and (a[GUARD + self.n:] == PATTERN).all())

    def untouched(self):
        return bool(torch.equal(self.buf, self.before))


class Volume:
    def __init__(self, case):
        value, weight = case["vol"]
        self.value = DevVolume(torch, np.ascontiguousarray(value), case["pitch"], case["offset"])
        self.weight = DevVolume(torch, np.ascontiguousarray(weight).view(np.float32), case["pitch"], case["offset"])
        self.pitch, self.res = case["pitch"], list(case["shape"])

    def untouched(self):
        return self.value.untouched() and self.weight.untouched()


_WS = []


def workspace(capi):
    """One workspace for the module: its tickets zeroed once, as the contract asks."""
    if not _WS:
        _WS.append(torch.zeros(capi.register_workspace_bytes(32), dtype=torch.uint8, device="cuda"))
    return _WS[0]


def tickets_zero(capi):
    return not bool(workspace(capi)[:256].any())


def launch(capi, case, vol, pts, xforms, **change):
    """One launch of N transforms [N, 12] over the points `pts` (a Guarded): ([N, 29] float64, the Guarded output)."""
    N = len(xforms)
    out = Guarded(N * 29 * 8)
    kw = dict(n=pts.n // 12, points=pts.addr, xforms=xforms, value=vol.value.addr, weight=vol.weight.addr, vol_step=vol.pitch, res=vol.res, voxel_size=float(case["vs"]),
              min_weight=case["min_weight"], max_residual=case["max_residual"], workspace=workspace(capi), out29xN=out.addr)
    kw.update(change)
    capi.register_terms(**kw)
    torch.cuda.synchronize()
    return out.host(np.float64, (N, 29)), out


def check(got, want, what):
    assert got[28] == want["sums"][28], (what, got[28], want["sums"][28])
    d = np.abs(got - want["sums"])
    assert (d[:28] <= want["tolerance"][:28]).all(), (what, d[:28], want["tolerance"][:28])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_sums_equal_the_model(capi, case):
    """The count equal, the 28 sums within the reassociation of n double additions of the model's chunk-ordered sums, and a second launch: the
    same bytes, guards included; the points, the volume and its guard rows untouched; the tickets back at zero."""
    want = rg.expected(case["name"])
    vol, pts = Volume(case), Guarded(case["n"] * 12, rg.all_points(case))
    runs = []
    for _ in range(2):
        got, out = launch(capi, case, vol, pts, case["xform"][None, :])
        check(got[0], want, case["name"])
        assert out.guards_ok() and pts.untouched() and vol.untouched() and tickets_zero(capi)
        runs.append(out)
    assert torch.equal(runs[0].buf, runs[1].buf)
    print(case["name"], "kept", int(got[0][28]), "of", case["n"], "largest |kernel - model| / tolerance: %.3g"
          % float((np.abs(got[0] - want["sums"])[:28] / np.maximum(want["tolerance"][:28], 1e-300)).max()))


def _transforms(case, count):
    """`count` transforms: the case's own, one that maps every point outside, and small rigid motions in front of the case's."""
    rng = np.random.default_rng(5)
    out = [case["xform"].copy(), rg.MISS12.copy()]
    while len(out) < count:
        x12, T = sc.rigid(int(rng.integers(1 << 30)), float(rng.uniform(-0.2, 0.2)), rng.uniform(-0.1, 0.1, 3))
        out.append(rg.xform12_of(T @ case["T"]))
    return np.stack(out).astype(np.float32)


def test_a_transforms_sums_do_not_depend_on_the_launch(capi):
    """N = 1, 5 and 32: transform m's 29 doubles are the same bits whatever N, its slot and the other transforms are; the transform that maps
    every point outside gives 29 zeros; the case's own transform gives the model's sums."""
    case = BY_NAME["sphere_n257_rigid_mw3_mr03"]
    vol, pts = Volume(case), Guarded(case["n"] * 12, rg.all_points(case))
    X = _transforms(case, 32)
    X_before = X.copy()
    full, _ = launch(capi, case, vol, pts, X)
    assert np.array_equal(X.view(np.uint32), X_before.view(np.uint32))          # the host's transforms are only read
    check(full[0], rg.expected(case["name"]), "slot 0 of 32")
    assert not full[1].any() and (np.signbit(full[1]) == 0).all()
    assert len({full[m].tobytes() for m in range(32)}) >= 30 and (full[2:, 28] > 0).sum() >= 25
    order = np.random.default_rng(6).permutation(32)
    shuffled, _ = launch(capi, case, vol, pts, X[order])
    assert all(shuffled[i].tobytes() == full[order[i]].tobytes() for i in range(32))
    five = [0, 1, 7, 19, 31]
    got5, _ = launch(capi, case, vol, pts, X[five])
    assert all(got5[i].tobytes() == full[m].tobytes() for i, m in enumerate(five))
    for m in (0, 1, 13, 31):
        got1, out = launch(capi, case, vol, pts, X[m:m + 1])
        assert got1[0].tobytes() == full[m].tobytes() and out.guards_ok()
    assert pts.untouched() and vol.untouched() and tickets_zero(capi)


@pytest.mark.parametrize("name", ["v345_n63_rigid", "sphere_n255_identity", "plane_n257_identity_mw3", "sphere_n1064960_rigid"])
def test_count_is_the_sample_kernels_kept_set(capi, name):
    """Against xs_tsdf_sample_points on the same inputs: the points whose status byte is OK, whose gradient words are not the refusal NaN and whose
    |value| is not above max_residual are exactly out[28] many; and the sums of the terms formed from that kernel's value and gradient bytes in
    the model's order are within the tolerance of the launch's."""
    case = BY_NAME[name]
    n = case["n"]
    vol, pts = Volume(case), Guarded(n * 12, rg.all_points(case))
    got, _ = launch(capi, case, vol, pts, case["xform"][None, :])
    status, value, grad = Guarded(n), Guarded(n * 4), Guarded(n * 12)
    capi.sample_points(n=n, points=pts.addr, xform12=case["xform"], value=vol.value.addr, weight=vol.weight.addr, vol_step=vol.pitch, res=vol.res,
                       voxel_size=float(case["vs"]), opts=capi.sample_opts(case["min_weight"]), status=status.addr, value_out=value.addr, gradient=grad.addr)
    torch.cuda.synchronize()
    st, r, g = status.host(np.uint8, (n,)), value.host(np.float32, (n,)), grad.host(np.float32, (n, 3))
    refused = (g.view(np.uint32) == sc.NAN_BITS).all(axis=1)
    with np.errstate(invalid="ignore"):
        kept = (st == sc.OK) & ~refused & ~(np.abs(r) > np.float32(case["max_residual"]))
    assert int(kept.sum()) == got[0][28] > 0
    m = rg.expected(name)["point"]
    assert np.array_equal(kept, np.tile(m["kept"], case["tile"]))
    assert np.array_equal(r[kept].view(np.uint32), np.tile(m["r"], case["tile"])[kept].view(np.uint32))


def test_rows_past_2_31_bytes(capi):
    """The (65, 33, 64) volume in rows of 1 MiB: 2112 rows, the last ones past 2^31 bytes.  The two arrays share one 2.2 GB buffer, each row holding
    a value and a weight segment; the rest of the buffer holds a pattern and must keep it."""
    case = rg.big_case()
    X, Y, Z = case["shape"]
    pitch = rc.BIG_PITCH
    rows = Y * Z
    assert (rows - 1) * pitch > 2 ** 31
    want = rg.expected(case["name"])
    assert rg.high_rows_kept(case, want["point"]).sum() >= 50
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
    for _ in range(2):
        got, out = launch(capi, case, vol, pts, case["xform"][None, :])
        check(got[0], want, "big rows")
        assert out.guards_ok() and pts.untouched()
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
    volume and the tickets as they were.  The limits themselves are accepted."""
    case = BY_NAME["sphere_n257_rigid_mw3_mr03"]
    vol, pts = Volume(case), Guarded(case["n"] * 12, rg.all_points(case))
    X = _transforms(case, 32)
    out = Guarded(32 * 29 * 8)
    good = dict(n=case["n"], points=pts.addr, xforms=X[:3], value=vol.value.addr, weight=vol.weight.addr, vol_step=vol.pitch, res=vol.res, voxel_size=float(case["vs"]),
                min_weight=1, max_residual=0.9, workspace=workspace(capi), out29xN=out.addr)
    nan, inf = float("nan"), float("inf")
    bad = [dict(transforms=0), dict(transforms=-1), dict(transforms=33, xforms=np.concatenate([X, X[:1]])), dict(n=0), dict(n=-1), dict(n=(1 << 30) + 1),
           dict(points=None), dict(xforms=None, transforms=3), dict(value=None), dict(weight=None), dict(res=None), dict(workspace=None), dict(out29xN=None),
           dict(xforms=with_entry(X[:3], 4, nan)), dict(xforms=with_entry(X[:3], 0, inf)), dict(xforms=with_entry(X[:3], 35, -inf)),
           dict(voxel_size=0.0), dict(voxel_size=-0.05), dict(voxel_size=nan), dict(voxel_size=inf),
           dict(res=[0, 17, 20]), dict(res=[33, 17, 65535 * 4 + 1]), dict(res=[33, 65536, 32768]), dict(vol_step=33 * 4 - 4), dict(vol_step=33 * 4 + 2),
           dict(min_weight=0), dict(min_weight=-3), dict(max_residual=0.0), dict(max_residual=-0.5), dict(max_residual=nan), dict(max_residual=inf)]
    for change in bad:
        with pytest.raises(capi.XsError) as e:
            capi.register_terms(**{**good, **change})
        assert "hip error 1:" in str(e.value) and "xs_tsdf_register_terms" in str(e.value), (change, str(e.value))
    torch.cuda.synchronize()
    assert out.untouched() and pts.untouched() and vol.untouched() and tickets_zero(capi)
    # the limits themselves: one point, one transform and 32
    capi.register_terms(**{**good, "n": 1, "xforms": X[:1]})
    capi.register_terms(**{**good, "xforms": X})
    torch.cuda.synchronize()
    assert out.guards_ok() and not out.untouched() and tickets_zero(capi)
