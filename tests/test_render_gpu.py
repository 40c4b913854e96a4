"""GPU: xs_render_views and xs_render_mask_build (x-slam_amd/csrc/xs_render.hip) against the float32 model of tests/render_cases.py.  Every
comparison is for equal bits of every output (the normals' NaNs included) and equal counts; the volumes are pitched, with guard planes and
padding that must come back untouched, and every output and the workspace sit between guard bytes that must keep their pattern."""
import importlib

import numpy as np
import pytest

import render_cases as rc
from extract_cases import DevVolume

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PATTERN, GUARD = 0xA7, 256
CASES = rc.cases()


@pytest.fixture(scope="module")
def capi():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("x-slam_amd.capi")


class Guarded:
    """nbytes of device memory between GUARD bytes of PATTERN on either side, PATTERN inside too.  addr: the first of the nbytes."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.addr = self.buf.data_ptr() + GUARD

    def host(self, dtype, shape):
        return self.buf.cpu().numpy()[GUARD:GUARD + self.n].view(dtype).reshape(shape).copy()

    def guards_ok(self):
        a = self.buf.cpu().numpy()
        return bool((a[:GUARD] == PATTERN).all() and (a[GUARD + self.n:] == PATTERN).all())

    def untouched(self):
        return bool((self.buf == PATTERN).all())


class Volume:
    def __init__(self, case):
        value, weight = case["vol"]
        self.value = DevVolume(torch, np.ascontiguousarray(value), case["pitch"], case["offset"])
        self.weight = DevVolume(torch, np.ascontiguousarray(weight).view(np.float32), case["pitch"], case["offset"])
        self.pitch, self.res = case["pitch"], list(case["shape"])

    def untouched(self):
        return self.value.untouched() and self.weight.untouched()


def shapes_of(P, rows, cols):
    return dict(depth=(np.float32, (P, rows, cols)), depth_u16=(np.uint16, (P, rows, cols)), normal=(np.float32, (P, 3, rows, cols)),
                shade=(np.uint8, (P, rows, cols)), counts=(np.uint32, (P, 4)))


def workspace_for(capi, vol, min_weight, build=True):
    ws = Guarded(capi.render_workspace_bytes(vol.res))
    if build:
        capi.render_mask_build(vol.value.addr, vol.weight.addr, vol.pitch, vol.res, ws.addr, min_weight=min_weight)
    return ws


def launch(capi, case, vol, ws, cull, outputs=rc.OUTPUTS, views=None, **change):
    """One xs_render_views of `case` (its views, or the listed ones): (dict of host arrays, the Guarded outputs)."""
    idx = list(range(len(case["R"]))) if views is None else list(views)
    P, rows, cols = len(idx), case["rows"], case["cols"]
    spec = shapes_of(P, rows, cols)
    dev = {k: Guarded(int(np.prod(spec[k][1])) * np.dtype(spec[k][0]).itemsize) for k in outputs}
    opts = capi.render_opts(case["t_near"], case["t_far"], case["step"], case["min_weight"], cull)
    kw = dict(Rc2vxP=case["R"][idx], tc2vxP=case["t"][idx], intr=case["intr"], rows=rows, cols=cols, value=vol.value.addr, weight=vol.weight.addr, vol_step=vol.pitch,
              res=vol.res, voxel_size=float(case["vs"]), workspace=ws.addr, opts=opts, **{k: dev[k].addr for k in outputs})
    kw.update(change)
    capi.render_views(**kw)
    torch.cuda.synchronize()
    return {k: dev[k].host(*spec[k]) for k in outputs}, dev


def assert_equal(got, want, views=None, what=""):
    for k, a in got.items():
        w = want[k] if views is None else want[k][list(views)]
        assert rc.same_output(k, a, w), (what, k, int((np.ascontiguousarray(a).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)).sum()))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_equals_the_model(capi, case):
    """Every output and the counts, bit for bit; with the cull, without it and a second time: the same bytes, guards included."""
    want = rc.expected(case["name"])
    vol = Volume(case)
    ws = workspace_for(capi, vol, case["min_weight"])
    runs = []
    for cull in (False, True, True):
        got, dev = launch(capi, case, vol, ws, cull)
        assert_equal(got, want, what=("cull", cull))
        assert all(d.guards_ok() for d in dev.values()) and ws.guards_ok() and vol.untouched()
        runs.append(dev)
    for k in rc.OUTPUTS:
        assert torch.equal(runs[0][k].buf, runs[1][k].buf) and torch.equal(runs[1][k].buf, runs[2][k].buf), k
    print(case["name"], "hit, backface, rejected, none:", want["counts"].sum(axis=0))


@pytest.mark.parametrize("case", [c for c in CASES if c["name"] in ("cube2_17x9", "s345_2x3", "plane956_17x9", "s33_80x60_mw3")], ids=lambda c: c["name"])
def test_mask_is_the_models(capi, case):
    """The brick mask word for word at both min_weights, the header in front of it, and nothing written behind the workspace."""
    vol = Volume(case)
    for mw in (1, 3):
        ws = workspace_for(capi, vol, mw)
        torch.cuda.synchronize()
        words = rc.mask_words(case["vol"], mw)
        raw = ws.host(np.uint8, (-1,))
        off = capi.RENDER_HEADER_BYTES + capi.RENDER_STAGING_BYTES
        assert np.array_equal(raw[off:off + words.size * 4].view(np.uint32), words), mw
        assert (raw[off + words.size * 4:] == PATTERN).all() and (raw[256:off] == PATTERN).all()      # only the words and the header are written
        head = raw[:20].view(np.int32)
        assert head[1:4].tolist() == vol.res and head[4] == mw and (raw[20:256] == PATTERN).all()
        assert ws.guards_ok() and vol.untouched()


def test_mask_of_a_volume_wider_than_a_word_of_bricks(capi):
    """(300, 8, 9): 38 bricks along x, two words per brick row, the last segment of 64 voxels ragged."""
    rng = np.random.default_rng(300)
    value = np.where(rng.random((9, 8, 300)) < 0.004, -0.5, 0.5).astype(np.float32)
    weight = rng.integers(0, 4, size=(9, 8, 300)).astype(np.int32)
    value[8, 7, 299], weight[8, 7, 299] = -1.0, 3
    case = dict(vol=(value, weight), pitch=300 * 4 + 12, offset=4, shape=(300, 8, 9))
    vol = Volume(case)
    for mw in (1, 3):
        ws = workspace_for(capi, vol, mw)
        torch.cuda.synchronize()
        words = rc.mask_words(case["vol"], mw)
        assert words.size == 4 and 0 < sum(bin(int(w)).count("1") for w in words) < 76
        off = capi.RENDER_HEADER_BYTES + capi.RENDER_STAGING_BYTES
        assert np.array_equal(ws.host(np.uint8, (-1,))[off:off + 16].view(np.uint32), words), mw
        assert ws.guards_ok() and vol.untouched()


def test_a_view_of_64_equals_the_view_alone(capi):
    case = next(c for c in CASES if c["name"] == "s33_64views")
    want = rc.expected(case["name"])
    vol = Volume(case)
    ws = workspace_for(capi, vol, case["min_weight"])
    for views in ([0], [17], [63], [5, 40]):
        got, dev = launch(capi, case, vol, ws, True, views=views)
        assert_equal(got, want, views=views, what=views)
        assert all(d.guards_ok() for d in dev.values())


def test_a_null_output_changes_nothing_in_the_others(capi):
    case = next(c for c in CASES if c["name"] == "s33_17x9_half")
    want = rc.expected(case["name"])
    vol = Volume(case)
    ws = workspace_for(capi, vol, case["min_weight"])
    for outputs in [(k,) for k in rc.OUTPUTS] + [("depth_u16", "shade"), ("normal", "counts")]:
        for cull in (False, True):
            got, dev = launch(capi, case, vol, ws, cull, outputs=outputs)
            assert_equal(got, want, what=outputs)
            assert all(d.guards_ok() for d in dev.values())


def test_refusals(capi):
    """Each argument error: hipErrorInvalidValue with a text, nothing launched, outputs, workspace and volume untouched."""
    case = next(c for c in CASES if c["name"] == "s33_17x9_half")
    vol = Volume(case)
    P, rows, cols = len(case["R"]), case["rows"], case["cols"]
    spec = shapes_of(64, rows, cols)
    dev = {k: Guarded(int(np.prod(spec[k][1])) * np.dtype(spec[k][0]).itemsize) for k in rc.OUTPUTS}
    built = workspace_for(capi, vol, 1)
    torch.cuda.synchronize()
    built_before = built.buf.clone()
    never = Guarded(capi.render_workspace_bytes(vol.res))                      # never built: the pattern is no header
    other = Guarded(capi.render_workspace_bytes(vol.res))                      # built, but for another resolution
    small = Volume(dict(vol=(case["vol"][0][:9, :9, :9], case["vol"][1][:9, :9, :9]), pitch=9 * 4, offset=0, shape=(9, 9, 9)))
    capi.render_mask_build(small.value.addr, small.weight.addr, small.pitch, small.res, other.addr, min_weight=1)
    heavy = Guarded(capi.render_workspace_bytes(vol.res))                      # built for a min_weight above the call's
    capi.render_mask_build(vol.value.addr, vol.weight.addr, vol.pitch, vol.res, heavy.addr, min_weight=3)
    torch.cuda.synchronize()
    other_before, heavy_before = other.buf.clone(), heavy.buf.clone()

    def opts(**kw):
        return capi.render_opts(**{**dict(t_near=case["t_near"], t_far=case["t_far"], step=case["step"], min_weight=1, cull=True), **kw})
    good = dict(Rc2vxP=case["R"], tc2vxP=case["t"], intr=case["intr"], rows=rows, cols=cols, value=vol.value.addr, weight=vol.weight.addr, vol_step=vol.pitch,
                res=vol.res, voxel_size=float(case["vs"]), workspace=built.addr, opts=opts(), **{k: dev[k].addr for k in rc.OUTPUTS})

    def with_entry(a, i, v):
        b = np.array(a, np.float32).copy()
        b.reshape(-1)[i] = v
        return b
    wrong_size = opts()
    wrong_size.struct_bytes -= 4
    bad = [dict(views=0), dict(views=65), dict(views=-1), dict(rows=0), dict(cols=0), dict(rows=4097), dict(cols=4097),
           dict(Rc2vxP=None, views=P), dict(tc2vxP=None), dict(intr=None), dict(value=None), dict(weight=None), dict(workspace=None), dict(res=None),
           {k: None for k in rc.OUTPUTS},
           dict(Rc2vxP=with_entry(case["R"], 4, np.nan)), dict(Rc2vxP=with_entry(case["R"], 26, np.inf)), dict(tc2vxP=with_entry(case["t"], 8, -np.inf)),
           dict(intr=with_entry(case["intr"], 2, np.nan)), dict(intr=with_entry(case["intr"], 1, np.inf)),
           dict(intr=with_entry(case["intr"], 0, 0.0)), dict(intr=with_entry(case["intr"], 1, -0.0)),
           dict(voxel_size=0.0), dict(voxel_size=-0.05), dict(voxel_size=float("nan")),
           dict(opts=opts(step=-0.01)), dict(opts=opts(t_near=0.5, t_far=0.5)), dict(opts=opts(t_near=0.5, t_far=0.4)),
           dict(opts=opts(t_near=0.2, t_far=5.0, step=0.001)),                                                                        # 4800 samples
           dict(res=[0, 17, 20]), dict(res=[33, 17, 65535 * 4 + 1]), dict(res=[33, 65536, 32768]), dict(vol_step=33 * 4 - 4), dict(vol_step=33 * 4 + 2),
           dict(opts=wrong_size), dict(opts=opts(shade_mode=1)),
           dict(workspace=never.addr), dict(workspace=other.addr), dict(workspace=heavy.addr)]
    for change in bad:
        with pytest.raises(capi.XsError) as e:
            capi.render_views(**{**good, **change})
        assert "hip error 1:" in str(e.value) and "xs_render_views" in str(e.value), (change, str(e.value))
    torch.cuda.synchronize()
    assert all(d.untouched() for d in dev.values()) and vol.untouched() and never.untouched()
    assert torch.equal(built.buf, built_before) and torch.equal(other.buf, other_before) and torch.equal(heavy.buf, heavy_before)
    # the limits themselves are accepted: 64 views, a mask built below the call's min_weight, no cull over a workspace that was never built
    R64, t64 = np.repeat(case["R"][:1], 64, axis=0), np.repeat(case["t"][:1], 64, axis=0)
    capi.render_views(**{**good, "Rc2vxP": R64, "tc2vxP": t64})
    capi.render_views(**{**good, "opts": opts(min_weight=2)})
    capi.render_views(**{**good, "workspace": never.addr, "opts": opts(cull=False)})
    torch.cuda.synchronize()
    assert all(d.guards_ok() for d in dev.values()) and not dev["depth"].untouched()


def test_rows_past_2_31_bytes(capi):
    """The (65, 33, 64) volume in rows of 1 MiB: 2112 rows, the last ones past 2^31 bytes, and the camera looks at those.  The two arrays share
    one 2.2 GB buffer, each row holding a value and a weight segment; the rest of the buffer holds a pattern and must keep it."""
    case = rc.big_case()
    X, Y, Z = case["shape"]
    pitch = rc.BIG_PITCH
    rows = Y * Z
    assert (rows - 1) * pitch > 2 ** 31
    want = rc.expected(case["name"])
    hit_planes = (want["depth"] > 0).any()
    assert hit_planes and want["counts"][0, 0] > 1000
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
    ws = workspace_for(capi, vol, 1)
    torch.cuda.synchronize()
    off = capi.RENDER_HEADER_BYTES + capi.RENDER_STAGING_BYTES
    mask = rc.mask_words(case["vol"], 1)
    assert np.array_equal(ws.host(np.uint8, (-1,))[off:off + mask.size * 4].view(np.uint32), mask)
    for cull in (False, True):
        got, dev = launch(capi, case, vol, ws, cull)
        assert_equal(got, want, what=("cull", cull))
        assert all(d.guards_ok() for d in dev.values())
    for seg, a in zip(segs, case["vol"]):
        assert np.array_equal(seg.cpu().numpy(), np.ascontiguousarray(a).view(np.int32))
        seg.fill_(-1515870811)                              # 0xA5A5A5A5
    assert bool((buf == 0xA5).all())                        # what lies between the segments kept the pattern
