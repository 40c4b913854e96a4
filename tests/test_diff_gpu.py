"""GPU: xs_tsdf_diff (x-slam_amd/csrc/xs_diff.hip) against the model of tests/diff_cases.py.  Every comparison is for equality: both masks word
for word (the buffers are prefilled with 0xFF bytes, so an unwritten word or a set overhang bit shows), the three counts, with the cull and
with XS_DIFF_NO_CULL; the guards of the masks and counts, and both volumes whole (guard planes and padding included), must be untouched.
Every shape runs every map with both min_weights; the map's number picks the pitch pair, so the 17 maps of a shape cover its 16 pairs of
independently chosen pitches.  Then the masks go through xs_frontier_label and xs_frontier_clusters against the scipy model."""
import importlib

import numpy as np
import pytest

import diff_cases as dc
import merge_cases as mc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("x-slam_amd.capi")


@pytest.mark.parametrize("dshape,sshape", dc.SHAPES)
def test_diff_equals_the_model(capi, dshape, sshape):
    this_host, other_host = dc.volumes(dshape, sshape)
    pairs = dc.pitch_pairs(dshape, sshape)
    maps = dc.maps(dshape, sshape)
    assert len(maps) >= len(pairs)
    ran = 0
    for k, (name, m) in enumerate(maps.items()):
        (dp, doff), (sp, soff) = pairs[k % len(pairs)]
        this, other = dc.DevVolume3(torch, this_host, dp, doff), dc.DevVolume3(torch, other_host, sp, soff)
        for mw in dc.MIN_WEIGHTS:
            want = dc.expected(dshape, sshape, name, mw)
            results = []
            for flags in (0, capi.DIFF_NO_CULL):
                out = dc.DevMasks(torch, dshape)
                dc.gpu_diff(torch, capi, this, other, dshape, sshape, m, mw, out, flags=flags, workspace=(flags == 0))
                got = (out.words(0), out.words(1), out.counts())
                print(dshape, sshape, name, mw, flags, got[2], want[2])
                assert got[2] == want[2], (name, mw, flags, got[2], want[2])
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, mw, flags)
                assert out.guards_untouched(), (name, mw, flags)
                results.append(out)
                ran += 1
            # with and without the cull: the same bytes
            for c in range(2):
                assert torch.equal(results[0].bufs[c], results[1].bufs[c])
        # guards, padding and contents of both volumes
        assert this.untouched() and other.untouched(), name
    assert ran == len(maps) * 4


def planted(capi, v, s, lo, hi, wv=None, ws=None, min_weight=1):
    """One row of voxels under the identity: (only_this list, only_other list, counts) from the GPU, checked against the model."""
    n = len(v)
    v, s = np.asarray(v, np.float32).reshape(1, 1, n), np.asarray(s, np.float32).reshape(1, 1, n)
    wv = np.ones((1, 1, n), np.int32) if wv is None else np.asarray(wv, np.int32).reshape(1, 1, n)
    ws = np.ones((1, 1, n), np.int32) if ws is None else np.asarray(ws, np.int32).reshape(1, 1, n)
    shape = (n, 1, 1)
    this, other = dc.DevVolume3(torch, (v, wv, v), n * 4), dc.DevVolume3(torch, (s, ws, s), n * 4 + 4)
    out = dc.DevMasks(torch, shape)
    dc.gpu_diff(torch, capi, this, other, shape, shape, mc.xform(), min_weight, out, lo=lo, hi=hi)
    a, clear_a = dc.unpack(out.words(0), (1, 1, n))
    b, clear_b = dc.unpack(out.words(1), (1, 1, n))
    assert clear_a and clear_b and out.guards_untouched() and this.untouched() and other.untouched()
    ma, mb, counts = dc.diff((v, wv), (s, ws), mc.xform(), min_weight, lo, hi)
    assert np.array_equal(a, ma) and np.array_equal(b, mb) and out.counts() == counts
    return a.reshape(-1).tolist(), b.reshape(-1).tolist(), counts


def test_threshold_edges(capi):
    """Planted voxels, under the identity (s is the source's bits): a value exactly hi is `firmly free`, a value exactly lo is not below lo,
    -0.0 is not below lo = 0, and lo = hi splits at one value."""
    below, above = np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))
    tiny = np.float32(-1e-30)
    # v < lo against s at, just below and just above hi: only_this iff s >= hi
    t, o, c = planted(capi, [-1, -1, -1, tiny], [0.5, below, above, 0.5], 0.0, 0.5)
    assert t == [True, False, True, True] and not any(o) and c == (4, 3, 0)
    # the mirror image: v exactly hi
    t, o, c = planted(capi, [0.5, below, above, 0.5], [-1, -1, -1, tiny], 0.0, 0.5)
    assert o == [True, False, True, True] and not any(t) and c == (4, 0, 3)
    # s exactly lo is not below lo; v exactly lo neither; -0.0 against lo = 0 neither
    t, o, c = planted(capi, [1, 1, 1, 0.0, -0.0, tiny], [0.0, -0.0, tiny, 1, 1, 1], 0.0, 0.5)
    assert o == [False, False, True, False, False, False] and t == [False, False, False, False, False, True] and c == (6, 1, 1)
    # lo = hi = 0.25: every pair on opposite sides is classified, a pair on one side is not, and the value 0.25 itself counts as above
    t, o, c = planted(capi, [0.2, 0.25, 0.3, 0.2, 0.25], [0.25, 0.2, 0.2, 0.2, 0.25], 0.25, 0.25)
    assert t == [True, False, False, False, False] and o == [False, True, True, False, False] and c == (5, 1, 2)
    # a non-zero lo: exactly lo is not below it
    t, o, c = planted(capi, [-0.1, np.nextafter(np.float32(-0.1), np.float32(-1))], [1, 1], -0.1, 0.5)
    assert t == [False, True]
    # observed on both sides only: a weight below min_weight on either side takes the voxel out of the comparison
    t, o, c = planted(capi, [-1, -1, -1], [1, 1, 1], 0.0, 0.5, wv=[2, 1, 2], ws=[2, 2, 1], min_weight=2)
    assert t == [True, False, False] and c == (1, 1, 0)
    # a NaN on either side is in no class
    t, o, c = planted(capi, [np.nan, -1, 1], [1, np.nan, np.nan], 0.0, 0.5)
    assert not any(t) and not any(o) and c == (3, 0, 0)


def test_counts_are_incremented(capi):
    dshape, sshape = dc.SHAPES[3]
    this_host, other_host = dc.volumes(dshape, sshape)
    this, other = dc.DevVolume3(torch, this_host, dshape[0] * 4), dc.DevVolume3(torch, other_host, sshape[0] * 4)
    want = dc.expected(dshape, sshape, "identity", 1)[2]
    assert min(want) > 0
    out = dc.DevMasks(torch, dshape, counts=(5, 7 << 40, 11))
    dc.gpu_diff(torch, capi, this, other, dshape, sshape, mc.xform(), 1, out)
    assert out.counts() == (5 + want[0], (7 << 40) + want[1], 11 + want[2])
    first = [out.words(k).copy() for k in range(2)]
    dc.gpu_diff(torch, capi, this, other, dshape, sshape, mc.xform(), 1, out, flags=capi.DIFF_NO_CULL, workspace=False)
    assert out.counts() == (5 + 2 * want[0], (7 << 40) + 2 * want[1], 11 + 2 * want[2])
    assert all(np.array_equal(out.words(k), first[k]) for k in range(2)) and out.guards_untouched()


def test_refusals(capi):
    """Each argument error: hipErrorInvalidValue with a text, nothing launched, nothing written."""
    dshape, sshape = dc.SHAPES[1]
    this_host, other_host = dc.volumes(dshape, sshape)
    this, other = dc.DevVolume3(torch, this_host, dshape[0] * 4), dc.DevVolume3(torch, other_host, sshape[0] * 4)
    out = dc.DevMasks(torch, dshape, counts=(3, 4, 5))
    ws = torch.zeros(capi.tsdf_diff_workspace_bytes(dshape, sshape), dtype=torch.uint8, device="cuda")
    assert len(ws) == capi.tsdf_merge_workspace_bytes(dshape, sshape) > 0
    good = dict(value=this.value.addr, weight=this.weight.addr, step=this.pitch, res=list(dshape), src_value=other.value.addr, src_weight=other.weight.addr,
                src_step=other.pitch, src_res=list(sshape), xform12=mc.xform(), only_this=out.addr[0], only_other=out.addr[1], counts=out.counts_addr,
                min_weight=1, lo=0.0, hi=0.5, flags=0, workspace=ws)
    nan, inf = mc.xform(), mc.xform()
    nan[4], inf[10] = np.nan, np.inf
    bad = [dict(value=None), dict(weight=None), dict(src_value=None), dict(src_weight=None), dict(min_weight=0), dict(min_weight=-3), dict(xform12=nan),
           dict(xform12=inf), dict(src_value=this.value.addr), dict(src_weight=this.weight.addr), dict(workspace=None), dict(step=dshape[0] * 4 - 4),
           dict(src_step=sshape[0] * 4 + 2), dict(res=[0, 3, 2]), dict(src_res=[3, 7, 300000]),
           dict(lo=float("nan")), dict(hi=float("nan")), dict(lo=float("-inf")), dict(hi=float("inf")), dict(lo=0.5, hi=0.25),
           dict(only_this=None), dict(only_other=None), dict(counts=None), dict(only_other=out.addr[0]), dict(only_this=out.addr[0] + 4),
           dict(res=[5, 70000, 2]), dict(res=[2048, 2048, 1024])]          # resolutions the frontier calls cannot label
    for change in bad:
        with pytest.raises(capi.XsError) as e:
            capi.tsdf_diff(**{**good, **change})
        assert "hip error 1:" in str(e.value) and "xs_tsdf_diff" in str(e.value), (change, str(e.value))
    torch.cuda.synchronize()
    assert this.untouched() and other.untouched() and out.unwritten() and out.counts() == (3, 4, 5) and out.guards_untouched() and not ws.any()
    assert capi.tsdf_diff_workspace_bytes([5, 70000, 2], sshape) == 0 and capi.tsdf_diff_workspace_bytes([2048, 2048, 1024], sshape) == 0
    assert capi.tsdf_diff_workspace_bytes(dshape, [3, 7, 300000]) == 0
    capi.tsdf_diff(**{**good, "lo": 0.25, "hi": 0.25})               # the limits themselves are accepted
    capi.tsdf_diff(**{**good, "flags": capi.DIFF_NO_CULL, "workspace": None})
    torch.cuda.synchronize()
    assert not out.unwritten() and out.guards_untouched()


def test_source_rows_beyond_2_31_bytes(capi):
    """Row offsets past 2^31 bytes on the source side: a (1024, 1024, 513) source is 2.1 GiB per array, zero apart from a block of 9^3 at its
    far corner; an (8, 8, 8) map is compared with it half a voxel into that block (eight corners each, the far faces included).  The model
    runs on the block alone: the map is a half-voxel shift, so every index is exact in float32 and the block's own coordinates give the same
    fractions."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 10 ** 9:
        pytest.skip("needs about 6 GB of free device memory")
    big = (1024, 1024, 513)
    X, Y, Z = big
    rng = np.random.default_rng(2 ** 31 - 3)
    bv = torch.zeros((Z, Y, X), dtype=torch.float32, device="cuda")
    bw = torch.zeros((Z, Y, X), dtype=torch.int32, device="cuda")
    assert (Y * (Z - 1) + Y - 1) * X * 4 > 2 ** 31
    block = mc.volume(rng, (9, 9, 9))
    for t, a in zip((bv, bw), block[:2]):
        t[Z - 9:, Y - 9:, X - 9:] = torch.from_numpy(a).cuda()
    before = [int(torch.count_nonzero(t).item()) for t in (bv.view(torch.int32), bw)]
    small_host = mc.volume(rng, (8, 8, 8))
    m = mc.xform(offset=(X - 9 + 0.5, Y - 9 + 0.5, Z - 9 + 0.5))
    local = mc.xform(offset=(0.5, 0.5, 0.5))
    ws = torch.zeros(capi.tsdf_diff_workspace_bytes([8, 8, 8], big), dtype=torch.uint8, device="cuda")
    classified = 0
    for mw in dc.MIN_WEIGHTS:
        a, b, counts = dc.diff(small_host, block, local, mw, lo=0.0, hi=0.1)
        classified += counts[1] + counts[2]
        assert 0 < counts[0] < 8 ** 3          # (eight corners each, a quarter of the weights zero: about a tenth of the voxels pass)
        for flags in (0, capi.DIFF_NO_CULL):
            small = dc.DevVolume3(torch, small_host, 8 * 4 + 4)
            out = dc.DevMasks(torch, (8, 8, 8))
            capi.tsdf_diff(small.value.addr, small.weight.addr, small.pitch, [8, 8, 8], bv, bw, X * 4, list(big), m, out.addr[0], out.addr[1], out.counts_addr,
                           min_weight=mw, lo=0.0, hi=0.1, flags=flags, workspace=ws)
            torch.cuda.synchronize()
            print(mw, flags, out.counts(), counts)
            assert out.counts() == counts and np.array_equal(out.words(0), dc.pack(a)) and np.array_equal(out.words(1), dc.pack(b)), (mw, flags)
            assert out.guards_untouched() and small.untouched()
    assert classified > 0
    assert [int(torch.count_nonzero(t).item()) for t in (bv.view(torch.int32), bw)] == before
    for t, a in zip((bv, bw), block[:2]):
        assert np.array_equal(t[Z - 9:, Y - 9:, X - 9:].cpu().numpy().view(np.uint32), a.view(np.uint32))


@pytest.mark.parametrize("dshape,sshape", [dc.SHAPES[3], dc.SHAPES[6]])
@pytest.mark.parametrize("cell", [0, 8])
def test_masks_to_clusters(capi, dshape, sshape, cell):
    """xs_frontier_label and xs_frontier_clusters on the diff's masks, as they come: the records of the scipy model on the model's masks."""
    this_host, other_host = dc.volumes(dshape, sshape)
    this, other = dc.DevVolume3(torch, this_host, dshape[0] * 4), dc.DevVolume3(torch, other_host, sshape[0] * 4)
    X, Y, Z = dshape
    out = dc.DevMasks(torch, dshape)
    name = "identity" if cell == 0 else "perm_a"
    dc.gpu_diff(torch, capi, this, other, dshape, sshape, dc.maps(dshape, sshape)[name], 1, out)
    model = dc.diff(this_host, other_host, dc.maps(dshape, sshape)[name], 1)
    capacity = 4096
    labels = torch.empty((X * Y * Z,), dtype=torch.int32, device="cuda")
    ws = torch.zeros(capi.frontier_workspace_bytes(dshape, capacity), dtype=torch.uint8, device="cuda")
    rec = torch.zeros((capacity * 8,), dtype=torch.int64, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    for k in range(2):
        want = dc.clusters(model[k], cell)
        assert 0 < len(want) <= capacity
        mask = out.device_words(k).contiguous()
        assert capi.frontier_label(mask, dshape, cell, labels, ws) >= 1
        n = capi.frontier_clusters(mask, labels, dshape, capacity, rec, cnt, ws)
        torch.cuda.synchronize()
        got = rec[:n * 8].cpu().numpy().view(np.uint64).reshape(n, 8)
        assert n == len(want) and np.array_equal(got, want), (k, n, len(want))
        assert int(got[:, 1].sum()) == model[2][1 + k]
