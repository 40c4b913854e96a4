"""GPU: xs_tsdf_sample_points and xs_tsdf_sample_depth (x-slam_amd/csrc/xs_sample.hip) against the float32 model of tests/sample_cases.py.  Every
comparison is for equal bits of every output (the NaNs included) and equal counts, with no share of exceptions; the volumes are pitched, with
guard planes and padding that must come back untouched, and the points, the depth image and every output sit between guard bytes that must
keep their pattern."""
import importlib

import numpy as np
import pytest

import render_cases as rc
import sample_cases as sc
from extract_cases import DevVolume

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PATTERN, GUARD = 0xA7, 256
CASES = sc.cases()
BY_NAME = {c["name"]: c for c in CASES}


@pytest.fixture(scope="module")
def capi():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("x-slam_amd.capi")


class Guarded:
    """nbytes of device memory between GUARD bytes of PATTERN on either side, PATTERN inside too.  addr: the first of the nbytes."""

    def __init__(self, nbytes, content=None, at=0):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.addr = self.buf.data_ptr() + GUARD
        if content is not None:
            raw = np.ascontiguousarray(content).view(np.uint8).reshape(-1)
            self.buf[GUARD + at:GUARD + at + raw.size].copy_(torch.from_numpy(raw.copy()))
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
        self.grad = DevVolume(torch, np.ascontiguousarray(case["grad"]), case["pitch"], case["offset"]) if case["grad"] is not None else None
        self.pitch, self.res = case["pitch"], list(case["shape"])

    def untouched(self):
        return self.value.untouched() and self.weight.untouched() and (self.grad is None or self.grad.untouched())


def outputs_of(case):
    return tuple(k for k in sc.OUTPUTS if k != "dvalue" or case["grad"] is not None)


def spec_of(case, n=None):
    if case["kind"] == "points":
        n = len(case["pts"]) if n is None else n
        return dict(status=(np.uint8, (n,)), value=(np.float32, (n,)), dvalue=(np.float32, (n,)), gradient=(np.float32, (n, 3)), counts=(np.uint64, (4,)))
    s = case["depth"].shape
    return dict(status=(np.uint8, s), value=(np.float32, s), dvalue=(np.float32, s), gradient=(np.float32, (3,) + s), counts=(np.uint64, (4,)))


class Input:
    """The points of a case (or the listed ones) between guard bytes, or its depth image in rows of depth_pitch bytes with a guard row either side."""

    def __init__(self, case, idx=None):
        if case["kind"] == "points":
            pts = case["pts"] if idx is None else case["pts"][idx]
            self.n = len(pts)
            self.mem = Guarded(pts.size * 4, pts)
            self.addr = self.mem.addr
        else:
            rows, cols = case["depth"].shape
            pitch = case["depth_pitch"]
            image = np.full((rows, pitch), PATTERN, np.uint8)
            image[:, :cols * 2] = case["depth"].view(np.uint8).reshape(rows, cols * 2)
            self.mem = Guarded((rows + 2) * pitch, image, at=pitch)
            self.addr = self.mem.addr + pitch


def launch(capi, case, vol, inp, outputs, **change):
    """One launch of `case` on the input `inp`: (dict of host arrays, the Guarded outputs)."""
    spec = spec_of(case, getattr(inp, "n", None))
    dev = {k: Guarded(int(np.prod(spec[k][1])) * np.dtype(spec[k][0]).itemsize) for k in outputs}
    names = dict(status="status", value="value_out", dvalue="dvalue", gradient="gradient", counts="counts")
    kw = dict(value=vol.value.addr, weight=vol.weight.addr, grad=None if vol.grad is None else vol.grad.addr, vol_step=vol.pitch, res=vol.res, voxel_size=float(case["vs"]),
              opts=capi.sample_opts(case["min_weight"]), **{names[k]: dev[k].addr for k in outputs})
    if case["kind"] == "points":
        kw.update(n=inp.n, points=inp.addr, xform12=case["xform"])
        kw.update(change)
        capi.sample_points(**kw)
    else:
        rows, cols = case["depth"].shape
        kw.update(depth=inp.addr, depth_step=case["depth_pitch"], rows=rows, cols=cols, intr=case["intr"], Rc2v=case["R"], tc2v=case["t"])
        kw.update(change)
        capi.sample_depth(**kw)
    torch.cuda.synchronize()
    return {k: dev[k].host(*spec[k]) for k in outputs}, dev


def assert_equal(got, want, idx=None, what=""):
    for k, a in got.items():
        if k == "counts" and idx is not None:
            w = np.bincount(want["status"][idx], minlength=4).astype(np.uint64)
        else:
            w = want[k] if idx is None else want[k][idx]
        assert sc.same_output(a, w), (what, k, int((np.ascontiguousarray(a).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)).sum()))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_equals_the_model(capi, case):
    """Every output and the counts, bit for bit, and a second time: the same bytes, guards included; the input and the volume untouched."""
    want = sc.expected(case["name"])
    vol, inp = Volume(case), Input(case)
    runs = []
    for _ in range(2):
        got, dev = launch(capi, case, vol, inp, outputs_of(case))
        assert_equal(got, want)
        assert all(d.guards_ok() for d in dev.values()) and inp.mem.untouched() and vol.untouched()
        runs.append(dev)
    for k in outputs_of(case):
        assert torch.equal(runs[0][k].buf, runs[1][k].buf), k
    print(case["name"], "outside, unseen, ok, no_depth:", want["counts"])


def test_a_subset_of_the_points_gives_the_same_bytes(capi):
    """Point i's outputs depend on nothing but point i: slices and a shuffled pick of the structured points equal those points of the full launch."""
    case = BY_NAME["s33_structured"]
    want = sc.expected(case["name"])
    vol = Volume(case)
    n = len(case["pts"])
    for idx in (np.arange(1), np.arange(5, 70), np.arange(n - 65, n), np.random.default_rng(3).permutation(n)[:1000]):
        got, dev = launch(capi, case, vol, Input(case, idx), outputs_of(case))
        assert_equal(got, want, idx=idx, what=len(idx))
        assert all(d.guards_ok() for d in dev.values())


@pytest.mark.parametrize("name", ["s33_structured", "depth_17x9"])
def test_a_null_output_changes_nothing_in_the_others(capi, name):
    case = BY_NAME[name]
    want = sc.expected(name)
    vol, inp = Volume(case), Input(case)
    for outputs in [(k,) for k in sc.OUTPUTS] + [("status", "gradient"), ("dvalue", "counts")]:
        got, dev = launch(capi, case, vol, inp, outputs)
        assert_equal(got, want, what=outputs)
        assert all(d.guards_ok() for d in dev.values())


def test_explicit_identity_equals_no_transform(capi):
    a, b = BY_NAME["plane_n257_null"], BY_NAME["plane_n257_identity"]
    vol, inp = Volume(a), Input(a)
    x, _ = launch(capi, a, vol, inp, outputs_of(a))
    y, _ = launch(capi, b, vol, inp, outputs_of(b))
    assert all(sc.same_output(x[k], y[k]) for k in x)


def refusal_table(capi, call, good, bad, dev, others):
    for change in bad:
        with pytest.raises(capi.XsError) as e:
            getattr(capi, call)(**{**good, **change})
        assert "hip error 1:" in str(e.value) and "xs_tsdf_" + call in str(e.value), (change, str(e.value))
    torch.cuda.synchronize()
    assert all(d.untouched() for d in dev.values()) and all(o.untouched() for o in others)


def with_entry(a, i, v):
    b = np.array(a, np.float32).copy()
    b.reshape(-1)[i] = v
    return b


def test_refusals_points(capi):
    """Each argument error: hipErrorInvalidValue with the call's name in the text, nothing launched, outputs, points and volume untouched."""
    case = BY_NAME["s33_structured"]
    vol, inp = Volume(case), Input(case)
    spec = spec_of(case)
    names = dict(status="status", value="value_out", dvalue="dvalue", gradient="gradient", counts="counts")
    dev = {k: Guarded(int(np.prod(spec[k][1])) * np.dtype(spec[k][0]).itemsize) for k in sc.OUTPUTS}
    x12 = sc.rigid(1, 0.3, (0.1, 0.0, 0.2))[0]
    good = dict(n=inp.n, points=inp.addr, xform12=x12, value=vol.value.addr, weight=vol.weight.addr, grad=vol.grad.addr, vol_step=vol.pitch, res=vol.res,
                voxel_size=float(case["vs"]), opts=capi.sample_opts(1), **{names[k]: dev[k].addr for k in sc.OUTPUTS})
    wrong_size = capi.sample_opts(1)
    wrong_size.struct_bytes += 4
    bad = [dict(n=0), dict(n=-1), dict(n=(1 << 30) + 1), dict(points=None), dict(res=None), dict(value=None), dict(weight=None),
           {names[k]: None for k in sc.OUTPUTS}, dict(grad=None),
           dict(status=inp.addr), dict(value_out=inp.addr), dict(dvalue=inp.addr), dict(gradient=inp.addr), dict(counts=inp.addr),
           dict(xform12=with_entry(x12, 4, np.nan)), dict(xform12=with_entry(x12, 0, np.inf)), dict(xform12=with_entry(x12, 11, -np.inf)),
           dict(voxel_size=0.0), dict(voxel_size=-0.05), dict(voxel_size=float("nan")), dict(voxel_size=float("inf")),
           dict(res=[0, 17, 20]), dict(res=[33, 17, 65535 * 4 + 1]), dict(res=[33, 65536, 32768]), dict(vol_step=33 * 4 - 4), dict(vol_step=33 * 4 + 2),
           dict(opts=wrong_size)]
    refusal_table(capi, "sample_points", good, bad, dev, [inp.mem])
    assert vol.untouched()
    # the limits themselves are accepted: one point, no transform, no opts, one output
    capi.sample_points(**{**good, "n": 1})
    capi.sample_points(**{**good, "xform12": None, "opts": None})
    capi.sample_points(**{**good, **{names[k]: None for k in sc.OUTPUTS if k != "counts"}, "grad": None})
    torch.cuda.synchronize()
    assert all(d.guards_ok() for d in dev.values()) and not dev["value"].untouched() and int(dev["counts"].host(np.uint64, (4,)).sum()) == inp.n


def test_refusals_depth(capi):
    case = BY_NAME["depth_17x9"]
    vol, inp = Volume(case), Input(case)
    names = dict(status="status", value="value_out", dvalue="dvalue", gradient="gradient", counts="counts")
    # outputs large enough for the accepted limit below: 4096 x 1 pixels
    sizes = dict(status=4096, value=4096 * 4, dvalue=4096 * 4, gradient=3 * 4096 * 4, counts=32)
    dev = {k: Guarded(sizes[k]) for k in sc.OUTPUTS}
    rows, cols = case["depth"].shape
    good = dict(depth=inp.addr, depth_step=case["depth_pitch"], rows=rows, cols=cols, intr=case["intr"], Rc2v=case["R"], tc2v=case["t"], value=vol.value.addr,
                weight=vol.weight.addr, grad=vol.grad.addr, vol_step=vol.pitch, res=vol.res, voxel_size=float(case["vs"]), opts=capi.sample_opts(1),
                **{names[k]: dev[k].addr for k in sc.OUTPUTS})
    wrong_size = capi.sample_opts(1)
    wrong_size.struct_bytes = 0
    bad = [dict(rows=0), dict(cols=0), dict(rows=4097), dict(cols=4097, depth_step=2 * 4097), dict(depth=None), dict(intr=None), dict(Rc2v=None), dict(tc2v=None),
           dict(res=None), dict(value=None), dict(weight=None), {names[k]: None for k in sc.OUTPUTS}, dict(grad=None),
           dict(status=inp.addr), dict(value_out=inp.addr), dict(dvalue=inp.addr), dict(gradient=inp.addr), dict(counts=inp.addr),
           dict(depth_step=cols * 2 - 2), dict(depth_step=cols * 2 + 1),
           dict(Rc2v=with_entry(case["R"], 4, np.nan)), dict(tc2v=with_entry(case["t"], 2, np.inf)), dict(intr=with_entry(case["intr"], 2, np.nan)),
           dict(intr=with_entry(case["intr"], 1, np.inf)), dict(intr=with_entry(case["intr"], 0, 0.0)), dict(intr=with_entry(case["intr"], 1, -0.0)),
           dict(voxel_size=0.0), dict(voxel_size=float("nan")), dict(res=[33, 0, 20]), dict(vol_step=33 * 4 - 4), dict(vol_step=33 * 4 + 2), dict(opts=wrong_size)]
    refusal_table(capi, "sample_depth", good, bad, dev, [inp.mem])
    assert vol.untouched()
    # 4096 x 1 pixels (a packed column of the same buffer, two bytes per row) and 1 x 17 are accepted
    tall = Guarded(4096 * 2, np.full(4096, 900, np.uint16))
    capi.sample_depth(**{**good, "depth": tall.addr, "depth_step": 2, "rows": 4096, "cols": 1})
    capi.sample_depth(**{**good, "rows": 1})
    torch.cuda.synchronize()
    assert all(d.guards_ok() for d in dev.values()) and tall.untouched() and inp.mem.untouched()


def test_rows_past_2_31_bytes(capi):
    """The (65, 33, 64) volume in rows of 1 MiB: 2112 rows, the last ones past 2^31 bytes, and every point reads those.  The two arrays share one
    2.2 GB buffer, each row holding a value and a weight segment; the rest of the buffer holds a pattern and must keep it."""
    case = sc.big_case()
    X, Y, Z = case["shape"]
    pitch = rc.BIG_PITCH
    rows = Y * Z
    assert (rows - 1) * pitch > 2 ** 31
    want = sc.expected(case["name"])
    assert want["counts"][sc.OK] == len(case["pts"]) and want["gok"].sum() > 1000
    buf = torch.full((rows * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
    words = buf.view(torch.int32)
    segs = [words.as_strided((Z, Y, X), (Y * (pitch // 4), pitch // 4, 1), k * 128) for k in range(2)]      # segments 512 bytes apart
    for seg, a in zip(segs, case["vol"]):
        seg.copy_(torch.from_numpy(np.array(a).view(np.int32)).cuda())

    class Vol:
        pass
    vol = Vol()
    vol.pitch, vol.res, vol.grad = pitch, [X, Y, Z], None
    for name, k in (("value", 0), ("weight", 1)):
        seg = Vol()
        seg.addr = buf.data_ptr() + k * 512
        setattr(vol, name, seg)
    inp = Input(case)
    for _ in range(2):
        got, dev = launch(capi, case, vol, inp, outputs_of(case))
        assert_equal(got, want)
        assert all(d.guards_ok() for d in dev.values())
    for seg, a in zip(segs, case["vol"]):
        assert np.array_equal(seg.cpu().numpy(), np.ascontiguousarray(a).view(np.int32))
        seg.fill_(-1515870811)                              # 0xA5A5A5A5
    assert bool((buf == 0xA5).all())                        # what lies between the segments kept the pattern
