"""GPU: xs_tsdf_fuse_points_accumulate and xs_tsdf_fuse_points_fold (x-slam_amd/csrc/xs_fuse.hip) against the model of tests/fuse_cases.py, word
for word: the accumulator after the accumulate, the value, weight and grad words after the fold, the four counts and the voxels written.  The
volumes are pitched, with guard planes and padding that must come back untouched; the points, the accumulator and the counts sit between guard
bytes that must keep their pattern.  What is added is an integer, so nothing here has a tolerance."""
import importlib

import numpy as np
import pytest

import fuse_cases as fc
import render_cases as rc
from extract_cases import DevVolume

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PATTERN, GUARD = 0xA7, 256
CASES = fc.cases() + (fc.hot_case(),)
BY_NAME = {c["name"]: c for c in fc.all_cases()}


@pytest.fixture(scope="module")
def capi():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("x-slam_amd.capi")


class Guarded:
    """nbytes of device memory between GUARD bytes of PATTERN on either side; `content` (or zeros with zero=True, else PATTERN) inside."""

    def __init__(self, nbytes, content=None, zero=False):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.addr = self.buf.data_ptr() + GUARD
        if zero:
            self.buf[GUARD:GUARD + self.n] = 0
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
    """The case's three arrays, each a DevVolume of its own with the case's pitch and offset."""

    def __init__(self, case):
        self.arrays = [DevVolume(torch, np.ascontiguousarray(a).view(np.float32), case["pitch"], case["offset"]) for a in case["vol"]]
        self.value, self.weight, self.grad = self.arrays
        self.pitch, self.res = case["pitch"], list(case["shape"])

    def untouched(self):
        return all(a.untouched() for a in self.arrays)

    def holds(self, vol):
        """The three buffers, guards and padding included, hold what they held with the stored planes replaced by `vol`'s: (ok, the first difference)."""
        X, Y, Z = self.res
        for dv, want in zip(self.arrays, vol):
            host = dv.host.copy()
            g, w = dv.GUARD, dv.pitch // 4
            off = (dv.addr - dv.buf.data_ptr()) // 4 - g * Y * w
            host[off:off + (Z + 2 * g) * Y * w].reshape(Z + 2 * g, Y, w)[g:-g, :, :X] = np.ascontiguousarray(want).view(np.float32)
            got = dv.buf.cpu().numpy().view(np.uint32)
            if not np.array_equal(got, host.view(np.uint32)):
                return False, int(np.nonzero(got != host.view(np.uint32))[0][0])
        return True, -1

    def bytes(self):
        return b"".join(a.buf.cpu().numpy().tobytes() for a in self.arrays)


def accumulate(capi, case, pts, acc, counts, points=None, **change):
    """The case's launches over its points (a Guarded of all n points, or `points` [n, 3] uploaded here)."""
    cut = fc.launch_split(case)
    for a, b in zip(cut[:-1], cut[1:]):
        kw = dict(n=b - a, points=pts.addr + 12 * a, origin=case["origin"], res=list(case["shape"]), voxel_size=float(case["vs"]), tranc_dist=float(case["tranc"]),
                  opts=capi.fuse_opts(case["min_range"], case["max_range"], case["carve"]), accumulator=acc.addr, counts=counts.addr, xform12=case["xform"])
        kw.update(change)
        capi.fuse_points_accumulate(**kw)
    torch.cuda.synchronize()


def fold(capi, case, vol, acc, written, **change):
    kw = dict(value=vol.value.addr, weight=vol.weight.addr, grad=vol.grad.addr, step=vol.pitch, res=vol.res, accumulator=acc.addr, obs_weight=case["obs_weight"],
              max_weight=case["max_weight"], written=written.addr)
    kw.update(change)
    capi.fuse_points_fold(**kw)
    torch.cuda.synchronize()


def buffers(case, points=None):
    X, Y, Z = case["shape"]
    pts = Guarded(case["n"] * 12, fc.all_points(case) if points is None else points)
    return pts, Guarded(X * Y * Z * 8, zero=True), Guarded(32, zero=True), Guarded(8, zero=True)


def run(capi, case, points=None):
    """Accumulate and fold on fresh buffers: (volume, accumulator words after the accumulate, counts, written, the buffers)."""
    vol = Volume(case)
    pts, acc, counts, written = buffers(case, points)
    accumulate(capi, case, pts, acc, counts)
    X, Y, Z = case["shape"]
    words = acc.host(np.uint64, (Z, Y, X))
    assert vol.untouched() and pts.untouched() and acc.guards_ok() and counts.guards_ok()
    fold(capi, case, vol, acc, written)
    return vol, words, counts.host(np.uint64, (4,)), int(written.host(np.uint64, (1,))[0]), (pts, acc, counts, written)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_words_equal_the_model(capi, case):
    """The accumulator after the accumulate, the three arrays after the fold, the counts and the voxels written: the model's, word for word; guards
    and padding untouched; the accumulator all zero after the fold; a second run on fresh buffers gives equal bytes."""
    want = fc.expected(case["name"])
    runs = []
    for _ in range(2):
        vol, words, counts, written, (pts, acc, cnt, wr) = run(capi, case)
        assert np.array_equal(words, want["acc"]), (case["name"], int((words != want["acc"]).sum()))
        assert np.array_equal(counts, want["counts"]), (counts, want["counts"])
        ok, where = vol.holds(want["vol"])
        assert ok, (case["name"], where)
        assert written == want["written"]
        assert not acc.host(np.uint8, (acc.n,)).any() and acc.guards_ok() and pts.untouched() and cnt.guards_ok() and wr.guards_ok()
        runs.append(vol.bytes() + words.tobytes())
    assert runs[0] == runs[1]
    print(case["name"], "points", case["n"], "counts", counts.tolist(), "written", written)


@pytest.mark.parametrize("name", ["v70x9x11_band_rigid_w3", "v70x9x11_carve_lattice_w1", "v70x9x11_carve_rigid_w3", "v5x3x2_carve_rigid_w1"])
def test_the_order_of_the_points_does_not_matter(capi, name):
    """The points reversed and shuffled: equal accumulator words, equal counts, equal volumes.  A float-atomic implementation fails here: the
    voxels that several rays visit (at least 50 of them with a count of 2 or more in the large cases) would receive their sums in another order."""
    case = BY_NAME[name]
    want = fc.expected(name)
    p = fc.all_points(case)
    for order in (np.arange(len(p))[::-1], np.random.default_rng(8).permutation(len(p))):
        vol, words, counts, written, _ = run(capi, case, np.ascontiguousarray(p[order]))
        assert np.array_equal(words, want["acc"]) and np.array_equal(counts, want["counts"]) and written == want["written"]
        ok, where = vol.holds(want["vol"])
        assert ok, (name, where)


def test_hot_voxel(capi):
    """70 000 identical points: one word's count passes 2^16 and its sum of q 2^32; a 32-bit add or a narrower field loses them."""
    case = fc.hot_case()
    want = fc.expected(case["name"])
    vol, words, counts, written, _ = run(capi, case)
    assert int((words >> fc.COUNT_SHIFT).max()) == 70000 and int((words & fc.SUM_MASK).max()) == 70000 * 65536 > 2 ** 32
    assert np.array_equal(words, want["acc"]) and counts.tolist() == [70000, 0, 350000, 1050000] and written == 5
    assert vol.holds(want["vol"])[0]


def test_fold_of_a_plane_range(capi):
    """Planes outside [z0, z1) keep their voxels and their accumulator words; the remaining ranges afterwards complete the fold."""
    case = BY_NAME["v70x9x11_carve_rigid_w1"]
    want = fc.expected(case["name"])
    vol = Volume(case)
    pts, acc, counts, written = buffers(case)
    accumulate(capi, case, pts, acc, counts)
    fold(capi, case, vol, acc, written, z0=3, z1=7)
    mvol, macc, n1 = fc.fold(case["vol"], want["acc"], case["obs_weight"], case["max_weight"], 3, 7)
    assert vol.holds(mvol)[0] and np.array_equal(acc.host(np.uint64, macc.shape), macc) and int(written.host(np.uint64, (1,))[0]) == n1
    fold(capi, case, vol, acc, written, z0=0, z1=3)
    fold(capi, case, vol, acc, written, z0=7, z1=11)
    assert vol.holds(want["vol"])[0] and not acc.host(np.uint8, (acc.n,)).any() and int(written.host(np.uint64, (1,))[0]) == want["written"]


def test_rows_past_2_31_bytes(capi):
    """The (65, 33, 64) volume in rows of 1 MiB: 2112 rows, the last ones past 2^31 bytes.  The three arrays share one 2.2 GB buffer, each row
    holding a value, a weight and a grad segment; the rest of the buffer holds a pattern and must keep it."""
    case = fc.big_case()
    X, Y, Z = case["shape"]
    pitch = rc.BIG_PITCH
    rows = Y * Z
    assert (rows - 1) * pitch > 2 ** 31
    want = fc.expected(case["name"])
    assert fc.high_rows_written(case, want) >= 50
    buf = torch.full((rows * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
    words = buf.view(torch.int32)
    segs = [words.as_strided((Z, Y, X), (Y * (pitch // 4), pitch // 4, 1), k * 128) for k in range(3)]      # segments 512 bytes apart
    for seg, a in zip(segs, case["vol"]):
        seg.copy_(torch.from_numpy(np.array(a).view(np.int32)).cuda())
    pts, acc, counts, written = buffers(case)
    accumulate(capi, case, pts, acc, counts)
    assert np.array_equal(acc.host(np.uint64, (Z, Y, X)), want["acc"]) and np.array_equal(counts.host(np.uint64, (4,)), want["counts"])
    capi.fuse_points_fold(value=buf.data_ptr(), weight=buf.data_ptr() + 512, grad=buf.data_ptr() + 1024, step=pitch, res=[X, Y, Z], accumulator=acc.addr,
                          obs_weight=case["obs_weight"], max_weight=case["max_weight"], written=written.addr)
    torch.cuda.synchronize()
    assert int(written.host(np.uint64, (1,))[0]) == want["written"] and not acc.host(np.uint8, (acc.n,)).any() and acc.guards_ok()
    for seg, a in zip(segs, want["vol"]):
        assert np.array_equal(seg.cpu().numpy(), np.ascontiguousarray(a).view(np.int32))
        seg.fill_(-1515870811)                              # 0xA5A5A5A5
    assert bool((buf == 0xA5).all())                        # what lies between the segments kept the pattern


def with_entry(a, i, v):
    b = np.array(a, np.float32).copy()
    b.reshape(-1)[i] = v
    return b


def test_refusals(capi):
    """Each argument error: hipErrorInvalidValue with the call's name in the text, nothing launched: the points, the accumulator, the counts, the
    volume and the written word as they were.  The limits themselves are accepted."""
    case = BY_NAME["v70x9x11_band_rigid_w1"]
    X, Y, Z = case["shape"]
    vol = Volume(case)
    pts, acc, counts, written = buffers(case)
    o = capi.fuse_opts
    good = dict(n=case["n"], points=pts.addr, origin=case["origin"], res=[X, Y, Z], voxel_size=float(case["vs"]), tranc_dist=float(case["tranc"]), opts=o(0.05, 3.0, False),
                accumulator=acc.addr, counts=counts.addr, xform12=case["xform"])
    nan, inf = float("nan"), float("inf")
    short = o()
    short.struct_bytes = 12
    bad = [dict(n=0), dict(n=-1), dict(n=1 << 24), dict(points=None), dict(origin=None), dict(res=None), dict(opts=None), dict(accumulator=None), dict(counts=None),
           dict(opts=short), dict(res=[0, Y, Z]), dict(res=[X, 65535 * 4 + 1, Z]), dict(res=[4, 65536, 32768]),
           dict(voxel_size=0.0), dict(voxel_size=-0.05), dict(voxel_size=nan), dict(voxel_size=inf), dict(tranc_dist=0.0), dict(tranc_dist=-1.0), dict(tranc_dist=nan),
           dict(tranc_dist=inf), dict(tranc_dist=8.01), dict(xform12=with_entry(case["xform"], 4, nan)), dict(xform12=with_entry(case["xform"], 11, inf)),
           dict(origin=with_entry(case["origin"], 1, nan)), dict(origin=with_entry(case["origin"], 2, -inf)), dict(opts=o(nan, 3.0)), dict(opts=o(0.05, inf)),
           dict(opts=o(0.05, nan)), dict(opts=o(0.0, 3.0)), dict(opts=o(-0.1, 3.0)), dict(opts=o(0.5, 0.4)), dict(opts=o(0.05, 32769.0))]
    for change in bad:
        with pytest.raises(capi.XsError) as e:
            capi.fuse_points_accumulate(**{**good, **change})
        assert "hip error 1:" in str(e.value) and "xs_tsdf_fuse_points_accumulate" in str(e.value), (change, str(e.value))
    fgood = dict(value=vol.value.addr, weight=vol.weight.addr, grad=vol.grad.addr, step=vol.pitch, res=[X, Y, Z], accumulator=acc.addr, obs_weight=1, max_weight=4,
                 written=written.addr)
    fbad = [dict(value=None), dict(weight=None), dict(grad=None), dict(res=None), dict(accumulator=None), dict(res=[X, 0, Z]), dict(step=X * 4 - 4), dict(step=X * 4 + 2),
            dict(z0=-1), dict(z1=Z + 1), dict(z0=4, z1=4), dict(z0=5, z1=4), dict(max_weight=0), dict(max_weight=(1 << 24) + 1), dict(obs_weight=0), dict(obs_weight=5),
            dict(obs_weight=-2)]
    for change in fbad:
        with pytest.raises(capi.XsError) as e:
            capi.fuse_points_fold(**{**fgood, **change})
        assert "hip error 1:" in str(e.value) and "xs_tsdf_fuse_points_fold" in str(e.value), (change, str(e.value))
    torch.cuda.synchronize()
    assert pts.untouched() and acc.untouched() and counts.untouched() and written.untouched() and vol.untouched()
    # the call as it stands, then the limits themselves: one point; min_range == max_range; K == 256; obs_weight == max_weight; no written word
    capi.fuse_points_accumulate(**good)
    capi.fuse_points_accumulate(**{**good, "n": 1})
    capi.fuse_points_accumulate(**{**good, "opts": o(0.5, 0.5)})
    capi.fuse_points_accumulate(**{**good, "n": 4, "tranc_dist": 8.0})
    capi.fuse_points_fold(**{**fgood, "obs_weight": 4, "written": None})
    torch.cuda.synchronize()
    assert pts.untouched() and acc.guards_ok() and counts.guards_ok() and not counts.untouched() and written.untouched() and not vol.untouched()
    assert not acc.host(np.uint8, (acc.n,)).any()
