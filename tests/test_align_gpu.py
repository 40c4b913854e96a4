"""GPU: xs_tsdf_align_terms (x-slam_amd/csrc/xs_align.hip) against the model of tests/align_cases.py.  Counts must equal the model's; each
of the 28 sums must lie within the derived bound of the float64 twin's and — the kernel's float32 residuals being the model's bit for bit,
the products exact in double — within the reassociation of n double additions of the model's own sums.  The source's guard planes and
padding, the whole source and the output's slack must be untouched and the tickets zero after every launch."""
import ctypes as C
import importlib

import numpy as np
import pytest

import align_cases as ac

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    assert torch.cuda.is_available()
    return importlib.import_module("x-slam_amd.capi")


_RUNNER = []


def the_runner(capi):
    """One workspace and output buffer for the module, made by the first test that runs."""
    if not _RUNNER:
        _RUNNER.append(ac.AlignRunner(torch, capi))
    return _RUNNER[0]


def check(got, ev, what):
    """One transform's 29 sums against the model's evaluate()."""
    n = ev["sums32"][28]
    assert got[28] == n, (what, got[28], n)
    d64 = np.abs(got - ev["sums64"])
    assert (d64[:28] <= ev["bound"][:28]).all(), (what, "twin", d64[:28] / np.maximum(ev["bound"][:28], 1e-300))
    reassociation = n * 2.0 ** -52 * (ev["terms"] + ev["bound"])
    d32 = np.abs(got - ev["sums32"])
    assert (d32[:28] <= reassociation[:28]).all(), (what, "model", d32[:28], reassociation[:28])


@pytest.mark.parametrize("sshape", ac.SOURCE_SHAPES)
def test_terms_equal_the_model(capi, sshape):
    """Every index count (fabricated) and the built index, every map in one launch, both min_weights, the map's number picking the pitch."""
    runner = the_runner(capi)
    names = list(ac.case_maps(sshape))
    maps = np.stack([ac.case_maps(sshape)[k] for k in names])
    pitch_list = ac.pitches(sshape[0])
    ran = 0
    for ci, count in enumerate(ac.INDEX_COUNTS + [None]):
        built = count is None
        xyz, gt, src, dense = ac.case(sshape, 0 if built else count, built)
        pitch, off = pitch_list[ci % len(pitch_list)]
        dev = ac.DevSource(torch, src, pitch, off)
        if built:
            D = ac.dst_shape_of(sshape)
            gtd = torch.from_numpy(np.array(dense)).cuda()
            index = capi.tsdf_band_build(gtd, list(D))
            assert index.count == len(gt) > 0
            keys = np.sort(index.keys_t[:index.count].cpu().numpy())
            assert np.array_equal(keys, np.sort(ac.keys_of(xyz)))
        else:
            index = ac.fabricated_band_index(torch, capi, xyz, gt)
        for mw in ac.MIN_WEIGHTS:
            got = runner.run(index, dev, sshape, maps, mw)
            again = runner.run(index, dev, sshape, maps, mw)
            assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
            for k, name in enumerate(names):
                check(got[k], ac.expected(sshape, 0 if built else count, built, name, mw), (sshape, count, name, mw))
                ran += 1
            if count == 0:
                assert not got.any()
        assert dev.untouched() and runner.tickets_zero(), count
    assert ran == 8 * 2 * len(names)


def test_a_transforms_sums_do_not_depend_on_the_launch(capi):
    """N = 1, 5 and 32: transform n's 29 sums are the same bits whatever N, its slot and the other transforms are."""
    runner = the_runner(capi)
    sshape = (9, 10, 13)
    xyz, gt, src, dense = ac.case(sshape, 0, True)
    index = capi.tsdf_band_build(torch.from_numpy(np.array(dense)).cuda(), list(ac.dst_shape_of(sshape)))
    dev = ac.DevSource(torch, src, *ac.pitches(sshape[0])[2])
    names = list(ac.case_maps(sshape))
    alone = {k: runner.run(index, dev, sshape, ac.case_maps(sshape)[k][None], 1)[0] for k in names}
    assert len({alone[k].tobytes() for k in names if k != "miss"}) == len(names) - 1
    rng = np.random.default_rng(5)
    for N in (5, 32):
        for _ in range(2):
            pick = [names[i] for i in rng.integers(0, len(names), N)]
            got = runner.run(index, dev, sshape, np.stack([ac.case_maps(sshape)[k] for k in pick]), 1)
            for slot, k in enumerate(pick):
                assert np.array_equal(got[slot].view(np.uint64), alone[k].view(np.uint64)), (N, slot, k)
    assert dev.untouched() and runner.tickets_zero()


def test_more_entries_than_one_round_of_the_grid(capi):
    """A 128 x 128 x 65 volume all of it band: 1 064 960 entries, more than 4096 workgroups x 256 lanes, so waves take a second chunk."""
    runner = the_runner(capi)
    D, sshape = (128, 128, 65), (70, 33, 5)
    rng = np.random.default_rng(109)       # (97 .. 107 leave an entry within its rounding bound of max_residual: the condition on the cases)
    dense = (rng.uniform(0.01, 0.95, (D[2], D[1], D[0])) * np.where(rng.random((D[2], D[1], D[0])) < 0.5, -1, 1)).astype(np.float32)
    index = capi.tsdf_band_build(torch.from_numpy(dense).cuda(), list(D))
    assert index.count == D[0] * D[1] * D[2] > 4096 * 256
    # the entries in the index's own order (the model's sums do not depend on it; which entries fall into the second round does)
    keys = index.keys_t[:index.count].cpu().numpy()
    xyz, gt = ac.xyz_of(keys), index.values_t[:index.count].cpu().numpy()
    assert np.array_equal(np.sort(keys), np.sort(ac.keys_of(ac.band_of(dense)[0]))) and np.array_equal(gt, dense[xyz[:, 2], xyz[:, 1], xyz[:, 0]])
    v, w = ac.source(rng, sshape)
    w[:, :, :58] = 0                     # (a sixth of the source carries weight: the model stays quick)
    src = (v, w)
    dev = ac.DevSource(torch, src, sshape[0] * 4 + 4)
    # the whole volume shrunk into the source: every entry is inside
    scale = (np.array(sshape) - 1.5) / np.array(D)
    m = ac.real_maps(ac.xform(np.diag(scale), (0.25, 0.25, 0.25)))
    ev = ac.evaluate(xyz, gt, src, m, 1)
    assert ev["near_threshold"] == 0 and ev["outside"] == 0 and ev["weight"] > 0 and ev["residual"] > 0
    assert ev["kept"][:4096 * 256].sum() > 1000 and ev["kept"][4096 * 256:].sum() > 10     # kept entries in the grid's second round
    got = runner.run(index, dev, sshape, m[None], 1)
    check(got[0], ev, "stride")
    assert dev.untouched() and runner.tickets_zero()


def test_source_rows_beyond_2_31_bytes(capi):
    """A (1024, 1024, 513) source is 2.1 GiB per array: a block of 9^3 at its far corner, a hand-made index of a few hundred entries mapped
    half a voxel into the block.  The model runs on the block alone with the same seeds and the block's own offsets: whole and half voxel
    shifts are exact in float32, so cells and fractions are the same bits."""
    runner = the_runner(capi)
    big = (1024, 1024, 513)
    X, Y, Z = big
    rng = np.random.default_rng(2 ** 31 - 1)
    bv = torch.zeros((Z, Y, X), dtype=torch.float32, device="cuda")
    bw = torch.zeros((Z, Y, X), dtype=torch.int32, device="cuda")
    assert (Y * (Z - 1) + 1) * X * 4 > 2 ** 31 >= Y * (Z - 1) * X * 4      # the last plane's rows, all but the first, start past 2^31 bytes
    block = ac.source(rng, (9, 9, 9))
    block[1][block[1] == 0] = 2          # (all corners valid: every entry reaches the far rows)
    bv[Z - 9:, Y - 9:, X - 9:] = torch.from_numpy(block[0]).cuda()
    bw[Z - 9:, Y - 9:, X - 9:] = torch.from_numpy(block[1]).cuda()
    before = (int(torch.count_nonzero(bv.view(torch.int32)).item()), int(torch.count_nonzero(bw).item()))
    xyz, gt = ac.fabricated_index(rng, 300, (8, 8, 8))
    index = ac.fabricated_band_index(torch, capi, xyz, gt)
    m_big = ac.real_maps(ac.xform(offset=(X - 9 + 0.5, Y - 9 + 0.5, Z - 9 + 0.5)))
    m_block = m_big.copy()
    m_block[:, 9:, 0] = np.float32(0.5)
    ev = ac.evaluate(xyz, gt, block, m_block, 1)
    assert ev["near_threshold"] == 0 and ev["sums32"][28] > 100 and ev["outside"] == 0
    assert ev["kept"][(xyz[:, 2] == 7) & (xyz[:, 1] >= 1)].sum() > 10       # entries whose upper corners lie in those rows

    class Dev:
        pass
    dev = Dev()
    dev.value, dev.weight, dev.pitch = Dev(), Dev(), X * 4
    dev.value.addr, dev.weight.addr = bv.data_ptr(), bw.data_ptr()
    got = runner.run(index, dev, big, m_big[None], 1)
    assert got[0][28] == ev["sums32"][28]
    n = got[0][28]
    assert (np.abs(got[0] - ev["sums32"])[:28] <= n * 2.0 ** -52 * (ev["terms"] + ev["bound"])[:28]).all()
    assert (np.abs(got[0] - ev["sums64"])[:28] <= ev["bound"][:28]).all()
    assert before == (int(torch.count_nonzero(bv.view(torch.int32)).item()), int(torch.count_nonzero(bw).item())) and runner.tickets_zero()


def test_refusals(capi):
    """Each argument error: hipErrorInvalidValue with a text, nothing launched, nothing written."""
    runner = the_runner(capi)
    sshape = (9, 10, 13)
    xyz, gt, src, _ = ac.case(sshape, 65, False)
    dev = ac.DevSource(torch, src, sshape[0] * 4)
    index = ac.fabricated_band_index(torch, capi, xyz, gt)
    maps = np.ascontiguousarray(ac.case_maps(sshape)["identity"][None], np.float32)
    out = torch.full((29 * 33,), -7.0, dtype=torch.float64, device="cuda")
    big_maps = np.ascontiguousarray(np.repeat(maps, 33, axis=0))
    _f32p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_int)

    def call(transforms=1, index=index, value=dev.value.addr, weight=dev.weight.addr, step=dev.pitch, res=sshape, maps=big_maps, min_weight=1,
             max_residual=1.0, ws=runner.ws.data_ptr(), out=out.data_ptr(), null_res=False, null_maps=False, null_index=False):
        r = np.ascontiguousarray(res, np.int32)
        m = np.ascontiguousarray(maps, np.float32)
        return capi._lib.xs_tsdf_align_terms(transforms, None if null_index else C.byref(index), value, weight, step, None if null_res else r.ctypes.data_as(_i32p),
                                             None if null_maps else m.ctypes.data_as(_f32p), min_weight, max_residual, ws, out, None)

    def unbuilt(**kw):
        i = capi.BandIndex()
        i.keys, i.values, i.capacity, i.count, i.nblocks = index.keys, index.values, index.capacity, index.count, index.nblocks
        for k, v in kw.items():
            setattr(i, k, v)
        return i

    nan, inf = big_maps.copy(), big_maps.copy()
    nan[0, 3, 5, 1], inf[0, 0, 11, 0] = np.nan, np.inf
    bad = [dict(transforms=0), dict(transforms=33), dict(transforms=-1), dict(null_index=True), dict(value=None), dict(weight=None), dict(null_res=True),
           dict(null_maps=True), dict(ws=None), dict(out=None), dict(index=unbuilt(nblocks=0)), dict(index=unbuilt(count=-1)),
           dict(index=unbuilt(count=index.capacity + 1)), dict(index=unbuilt(keys=None)), dict(index=unbuilt(values=None)),
           dict(res=(1, 10, 13)), dict(res=(9, 0, 13)), dict(res=(9, 10, 262141)), dict(res=(2, 262140, 262140), step=8), dict(step=sshape[0] * 4 - 4), dict(step=sshape[0] * 4 + 2),
           dict(min_weight=0), dict(min_weight=-2), dict(max_residual=0.0), dict(max_residual=-1.0), dict(max_residual=float("inf")),
           dict(max_residual=float("nan")), dict(maps=nan), dict(maps=inf)]
    for change in bad:
        assert call(**change) == 1, change
        text = capi._lib.xs_last_error().decode()
        assert "xs_tsdf_align_terms" in text, (change, text)
    torch.cuda.synchronize()
    assert (out == -7.0).all().item() and dev.untouched() and runner.tickets_zero()
    # the limits themselves are accepted
    assert call(transforms=32) == 0 and call(res=(9, 10, 13), min_weight=1, max_residual=1e-30) == 0
    torch.cuda.synchronize()
    assert runner.tickets_zero()
