"""GPU: xs_tsdf_merge (x-slam_amd/csrc/xs_merge.hip) against the float32 model of tests/merge_cases.py.  Every comparison is for equal bits of
value and grad, equal weights and an equal `written`; the destination's guard planes and padding and the whole source must be untouched
(the buffers are compared whole).  Every shape runs every map with both min_weights, into the empty and the populated destination, with the
cull and with XS_MERGE_NO_CULL; the map's number picks the pitch pair, so the 17 maps of a shape cover its 16 pairs of independently chosen
destination and source pitches."""
import importlib

import numpy as np
import pytest

import merge_cases as mc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("x-slam_amd.capi")


@pytest.mark.parametrize("dshape,sshape", mc.SHAPES)
def test_merge_equals_the_model(capi, dshape, sshape):
    dst_host, src_host = mc.volumes(dshape, sshape)
    pairs = mc.pitch_pairs(dshape, sshape)
    maps = mc.maps(dshape, sshape)
    assert len(maps) >= len(pairs)
    ran = 0
    for k, (name, m) in enumerate(maps.items()):
        (dp, doff), (sp, soff) = pairs[k % len(pairs)]
        src = mc.DevVolume3(torch, src_host, sp, soff)
        for mw in mc.MIN_WEIGHTS:
            for populated in (False, True):
                want = mc.expected(dshape, sshape, name, mw, populated)
                results = []
                for flags in (0, capi.MERGE_NO_CULL):
                    dst = mc.DevVolume3(torch, dst_host if populated else mc.empty_volume(dshape), dp, doff)
                    written = mc.gpu_merge(torch, capi, dst, src, dshape, sshape, m, mw, flags=flags, workspace=(flags == 0))
                    assert written == want[3], (name, mw, populated, flags, written, want[3])
                    assert dst.equals(want), (name, mw, populated, flags)
                    results.append(dst)
                    ran += 1
                # with and without the cull: the same bytes, guards and padding included
                for a, b in zip((results[0].value, results[0].weight, results[0].grad), (results[1].value, results[1].weight, results[1].grad)):
                    assert torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32))
        assert src.untouched(), name
    assert ran == len(maps) * 8


@pytest.mark.parametrize("dshape,sshape", [mc.SHAPES[3], mc.SHAPES[5]])
def test_plane_ranges(capi, dshape, sshape):
    """Disjoint plane ranges that cover the volume, in any order, give the whole-volume result; planes outside a range are untouched."""
    dst_host, src_host = mc.volumes(dshape, sshape)
    Z = dshape[2]
    (dp, doff), (sp, soff) = mc.pitch_pairs(dshape, sshape)[6]
    src = mc.DevVolume3(torch, src_host, sp, soff)
    for name in ("identity", "half_z", "rotation_33", "ratio_half"):
        m = mc.maps(dshape, sshape)[name]
        whole = mc.expected(dshape, sshape, name, 1, True)
        for flags in (0, capi.MERGE_NO_CULL):
            dst = mc.DevVolume3(torch, dst_host, dp, doff)
            total = 0
            ranges = [(Z - 1, Z), (0, 1), (1, Z - 1)] if Z > 2 else [(1, 2), (0, 1)]
            for i, (z0, z1) in enumerate(ranges):
                n = mc.gpu_merge(torch, capi, dst, src, dshape, sshape, m, 1, flags=flags, z0=z0, z1=z1)
                part = mc.merge(dst_host, src_host, m, 1, z0=z0, z1=z1)
                assert n == part[3], (name, z0, z1)
                total += n
                if i == 0:
                    assert dst.equals(part), (name, z0, z1)     # one range alone: the other planes keep their bits
            assert total == whole[3] and dst.equals(whole), (name, flags)
    assert src.untouched()


def test_refusals(capi):
    """Each argument error: hipErrorInvalidValue with a text, nothing launched, nothing written."""
    dshape, sshape = mc.SHAPES[1]
    dst_host, src_host = mc.volumes(dshape, sshape)
    dst = mc.DevVolume3(torch, dst_host, dshape[0] * 4)
    src = mc.DevVolume3(torch, src_host, sshape[0] * 4)
    written = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(capi.tsdf_merge_workspace_bytes(dshape, sshape), dtype=torch.uint8, device="cuda")
    good = dict(value=dst.value.addr, weight=dst.weight.addr, grad=dst.grad.addr, step=dst.pitch, res=list(dshape), src_value=src.value.addr,
                src_weight=src.weight.addr, src_grad=src.grad.addr, src_step=src.pitch, src_res=list(sshape), xform12=mc.xform(), min_weight=1,
                max_weight=mc.MAX_WEIGHT, flags=0, z0=0, z1=None, written=written, workspace=ws)
    nan, inf = mc.xform(), mc.xform()
    nan[4], inf[10] = np.nan, np.inf
    bad = [dict(value=None), dict(weight=None), dict(grad=None), dict(src_value=None), dict(src_weight=None), dict(src_grad=None),
           dict(min_weight=0), dict(min_weight=-3), dict(max_weight=0), dict(max_weight=(1 << 24) + 1), dict(xform12=nan), dict(xform12=inf),
           dict(z0=1, z1=1), dict(z0=2, z1=1), dict(z0=-1, z1=1), dict(z0=0, z1=dshape[2] + 1),
           dict(src_value=dst.value.addr), dict(src_weight=dst.weight.addr), dict(src_grad=dst.grad.addr), dict(workspace=None),
           dict(step=dshape[0] * 4 - 4), dict(src_step=sshape[0] * 4 + 2), dict(res=[0, 3, 2]), dict(src_res=[3, 7, 300000])]
    for change in bad:
        with pytest.raises(capi.XsError) as e:
            capi.tsdf_merge(**{**good, **change})
        assert "hip error 1:" in str(e.value) and "xs_tsdf_merge" in str(e.value), (change, str(e.value))
    torch.cuda.synchronize()
    assert dst.untouched() and src.untouched() and int(written.item()) == 0 and not ws.any()
    capi.tsdf_merge(**{**good, "max_weight": 1 << 24})     # the limits themselves are accepted
    capi.tsdf_merge(**{**good, "flags": capi.MERGE_NO_CULL, "workspace": None})
    torch.cuda.synchronize()


def test_beyond_2_31_bytes(capi):
    """Row offsets past 2^31 bytes on either side: a (1024, 1024, 513) volume is 2.1 GiB per array.  Part 1: such a source, zero apart from
    a block of 9^3 at its far corner, into an (8, 8, 8) destination mapped half a voxel into that block (eight corners each, the far faces
    included).  Part 2: an (8, 8, 8) source into the far corner of such a destination.  The model runs on the block alone: the maps are whole
    and half voxel shifts, so every index is exact in float32 and the block's own coordinates give the same fractions."""
    free, _ = torch.cuda.mem_get_info()
    if free < 14 * 10 ** 9:
        pytest.skip("needs about 14 GB of free device memory")
    big = (1024, 1024, 513)
    X, Y, Z = big
    rng = np.random.default_rng(2 ** 31 - 1)
    bv = torch.zeros((Z, Y, X), dtype=torch.float32, device="cuda")
    bw = torch.zeros((Z, Y, X), dtype=torch.int32, device="cuda")
    bg = torch.zeros((Z, Y, X), dtype=torch.float32, device="cuda")
    assert (Y * (Z - 1) + Y - 1) * X * 4 > 2 ** 31
    written = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(capi.tsdf_merge_workspace_bytes(big, big), dtype=torch.uint8, device="cuda")

    def nonzero():
        return [int(torch.count_nonzero(t).item()) for t in (bv.view(torch.int32), bw, bg.view(torch.int32))]

    # part 1: the big volume is the source
    block = mc.volume(rng, (9, 9, 9))
    for t, a in zip((bv, bw, bg), block):
        t[Z - 9:, Y - 9:, X - 9:] = torch.from_numpy(a).cuda()
    before = nonzero()
    small_host = mc.volume(rng, (8, 8, 8))
    m = mc.xform(offset=(X - 9 + 0.5, Y - 9 + 0.5, Z - 9 + 0.5))
    local = mc.xform(offset=(0.5, 0.5, 0.5))
    for mw in mc.MIN_WEIGHTS:
        want = mc.merge(small_host, block, local, mw)
        assert 0 < want[3] < 8 ** 3          # (eight corners each, a quarter of the weights zero: about a tenth of the voxels pass)
        for flags in (0, capi.MERGE_NO_CULL):
            small = mc.DevVolume3(torch, small_host, 8 * 4 + 4)
            written.zero_()
            capi.tsdf_merge(small.value.addr, small.weight.addr, small.grad.addr, small.pitch, [8, 8, 8], bv, bw, bg, X * 4, list(big), m, min_weight=mw,
                            max_weight=mc.MAX_WEIGHT, flags=flags, written=written, workspace=ws)
            torch.cuda.synchronize()
            assert int(written.item()) == want[3] and small.equals(want), (mw, flags)
    assert nonzero() == before
    for t, a in zip((bv, bw, bg), block):
        assert np.array_equal(t[Z - 9:, Y - 9:, X - 9:].cpu().numpy().view(np.uint32), a.view(np.uint32))

    # part 2: the big volume is the destination; its far block of 8^3 is populated, the source lands on it shifted by half a voxel along x
    for t in (bv, bw, bg):
        t[Z - 9:, Y - 9:, X - 9:] = 0
    dst_block = mc.volume(rng, (8, 8, 8))
    for t, a in zip((bv, bw, bg), dst_block):
        t[Z - 8:, Y - 8:, X - 8:] = torch.from_numpy(a).cuda()
    src_host = mc.volume(rng, (8, 8, 8))
    src = mc.DevVolume3(torch, src_host, 8 * 4)
    m = mc.xform(offset=(-(X - 8) + 0.5, -(Y - 8), -(Z - 8)))
    want = mc.merge(dst_block, src_host, mc.xform(offset=(0.5, 0, 0)), 1)
    assert 50 < want[3] < 8 * 8 * 7 + 1
    written.zero_()
    capi.tsdf_merge(bv, bw, bg, X * 4, list(big), src.value.addr, src.weight.addr, src.grad.addr, src.pitch, [8, 8, 8], m, min_weight=1,
                    max_weight=mc.MAX_WEIGHT, flags=0, written=written, workspace=ws)
    torch.cuda.synchronize()
    assert int(written.item()) == want[3] and src.untouched()
    got = [t[Z - 8:, Y - 8:, X - 8:].cpu().numpy() for t in (bv, bw, bg)]
    assert mc.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and mc.same_bits(got[2], want[2])
    # the rest of the big volume is unchanged (zero): all that is not zero is in the block
    assert nonzero() == [int(np.count_nonzero(a.view(np.uint32))) for a in got]
