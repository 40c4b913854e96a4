"""GPU: xs_tsdf_score_transforms (x-slam_amd/csrc/xs_align.hip: k_align_score) against the model of tests/align_score_cases.py.  Counts must
equal the model's; each sum must lie within 8 * 2^-24 of the model's (all terms >= 0, the float32 products bit-equal, a six-level float tree
per chunk, doubles after it).  A transform's pair must not depend on the launch it is in; the source's guard planes and padding, the output's
slack and — on a refusal — the whole workspace must be untouched, and the tickets zero after every launch."""
import ctypes as C
import importlib

import numpy as np
import pytest

import align_cases as ac
import align_score_cases as sc

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
        _RUNNER.append(sc.ScoreRunner(torch, capi))
    return _RUNNER[0]


@pytest.mark.parametrize("sshape", sc.SOURCE_SHAPES)
def test_pairs_equal_the_model(capi, sshape):
    """Every index count, every transform in one launch, both min_weights, the count's number picking the pitch."""
    runner = the_runner(capi)
    names = list(sc.case_xforms(sshape))
    xforms = np.stack([sc.case_xforms(sshape)[k] for k in names])
    pitch_list = ac.pitches(sshape[0])
    ran = 0
    for ci, count in enumerate(sc.INDEX_COUNTS):
        xyz, gt, src = sc.case(sshape, count)
        pitch, off = pitch_list[ci % len(pitch_list)]
        dev = ac.DevSource(torch, src, pitch, off)
        index = ac.fabricated_band_index(torch, capi, xyz, gt)
        for mw in sc.MIN_WEIGHTS:
            got = runner.run(index, dev, sshape, xforms, mw)
            for k, name in enumerate(names):
                sc.check(got[k], sc.expected(sshape, count, name, mw), (sshape, count, name, mw))
                ran += 1
            if count == 0:
                assert not got.any()
        assert dev.untouched() and runner.tickets_zero(), count
    assert ran == len(sc.INDEX_COUNTS) * 2 * len(names)


def test_tile_edges_and_independence(capi):
    """P = 1, 63, 64, 65, 129: transform p's two doubles are the same bits alone, in another slot and among others; two launches give equal
    bits; the tickets are zero after each launch."""
    runner = the_runner(capi)
    sshape = (9, 10, 13)
    xyz, gt, src = sc.case(sshape, 257)
    index = ac.fabricated_band_index(torch, capi, xyz, gt)
    dev = ac.DevSource(torch, src, *ac.pitches(sshape[0])[2])
    names = list(sc.case_xforms(sshape))
    alone = {}
    for k in names:
        alone[k] = runner.run(index, dev, sshape, sc.case_xforms(sshape)[k][None], 1)[0]
        assert runner.tickets_zero()
        sc.check(alone[k], sc.expected(sshape, 257, k, 1), k)
    assert len({alone[k].tobytes() for k in names if k != "miss"}) == len(names) - 1
    rng = np.random.default_rng(5)
    for P in (1, 63, 64, 65, 129):
        pick = [names[i] for i in rng.integers(0, len(names), P)]
        xf = np.stack([sc.case_xforms(sshape)[k] for k in pick])
        got = runner.run(index, dev, sshape, xf, 1)
        assert runner.tickets_zero()
        again = runner.run(index, dev, sshape, xf, 1)
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64)) and runner.tickets_zero()
        for slot, k in enumerate(pick):
            assert np.array_equal(got[slot].view(np.uint64), alone[k].view(np.uint64)), (P, slot, k)
    assert dev.untouched()


def test_strides(capi):
    """Strides 1, 2, 3, 7 on counts 1, 64, 65, 257: the model on xyz[::stride]; the last chunk is partial in all but one (64 entries at stride 1)."""
    runner = the_runner(capi)
    sshape = (9, 10, 13)
    names = list(sc.case_xforms(sshape))
    xforms = np.stack([sc.case_xforms(sshape)[k] for k in names])
    for count in (1, 64, 65, 257):
        xyz, gt, src = sc.case(sshape, count)
        index = ac.fabricated_band_index(torch, capi, xyz, gt)
        dev = ac.DevSource(torch, src, sshape[0] * 4 + 4)
        for stride in sc.STRIDES:
            got = runner.run(index, dev, sshape, xforms, 1, stride)
            for k, name in enumerate(names):
                sc.check(got[k], sc.expected(sshape, count, name, 1, stride), (count, stride, name))
        assert dev.untouched() and runner.tickets_zero()


def test_more_entries_than_one_round_of_the_grid(capi):
    """300 000 fabricated entries: more than 1024 workgroups x 4 waves x 64 lanes, so waves take a second chunk; P = 2."""
    runner = the_runner(capi)
    sshape = (9, 10, 13)
    xyz, gt, src = sc.large_case()
    index = ac.fabricated_band_index(torch, capi, xyz, gt)
    dev = ac.DevSource(torch, src, sshape[0] * 4 + 4)
    names = ["rotation_7", "half_xyz"]
    got = runner.run(index, dev, sshape, np.stack([sc.case_xforms(sshape)[k] for k in names]), 1)
    for k, name in enumerate(names):
        ev = sc.score_model(xyz, gt, src, sc.case_xforms(sshape)[name], 1)
        assert ev["kept"][:1024 * 256].sum() > 1000 and ev["kept"][1024 * 256:].sum() > 100      # kept entries in the grid's second round
        sc.check(got[k], ev, name)
    assert dev.untouched() and runner.tickets_zero()


def test_source_rows_beyond_2_31_bytes(capi):
    """A (1024, 1024, 513) source is 2.1 GiB per array: a block of 9^3 at its far corner, a hand-made index of a few hundred entries mapped
    half a voxel into the block (tests/test_align_gpu.py's case).  The model runs on the block alone with the block's own offsets: whole and
    half voxel shifts are exact in float32, so cells and fractions are the same bits."""
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
    m_big = ac.xform(offset=(X - 9 + 0.5, Y - 9 + 0.5, Z - 9 + 0.5))
    m_block = ac.xform(offset=(0.5, 0.5, 0.5))
    ev = sc.score_model(xyz, gt, block, m_block, 1)
    assert ev["near"] == 0 and ev["count"] > 100 and ev["outside"] == 0
    assert ev["kept"][(xyz[:, 2] == 7) & (xyz[:, 1] >= 1)].sum() > 10       # entries whose upper corners lie in those rows

    class Dev:
        pass
    dev = Dev()
    dev.value, dev.weight, dev.pitch = Dev(), Dev(), X * 4
    dev.value.addr, dev.weight.addr = bv.data_ptr(), bw.data_ptr()
    got = runner.run(index, dev, big, m_big[None], 1)
    sc.check(got[0], ev, "far rows")
    assert before == (int(torch.count_nonzero(bv.view(torch.int32)).item()), int(torch.count_nonzero(bw).item())) and runner.tickets_zero()


def test_early_out_adds_nothing(capi):
    """A transform that misses the source and one whose cells all fail the weight gate give exactly {+0, 0}; mixed into a launch with
    transforms that hit, they leave the others' bits as they are."""
    runner = the_runner(capi)
    sshape = (9, 10, 13)
    xyz, gt, src = sc.case(sshape, 257)
    index = ac.fabricated_band_index(torch, capi, xyz, gt)
    dev = ac.DevSource(torch, src, sshape[0] * 4)
    xf = sc.case_xforms(sshape)
    hits = ["identity", "rotation_7", "half_x"]
    alone = {k: runner.run(index, dev, sshape, xf[k][None], 1)[0] for k in hits}
    miss = runner.run(index, dev, sshape, xf["miss"][None], 1)[0]
    assert np.array_equal(miss.view(np.uint64), np.zeros(2, np.uint64))
    # min_weight 10: the source's weights end at 9, so every entry that is inside fails the weight gate
    ev = sc.score_model(xyz, gt, src, xf["identity"], 10)
    assert ev["weight"] > 50 and ev["count"] == 0
    light = runner.run(index, dev, sshape, xf["identity"][None], 10)[0]
    assert np.array_equal(light.view(np.uint64), np.zeros(2, np.uint64))
    order = ["miss", "identity", "miss", "rotation_7", "half_x", "miss"] * 11 + ["miss"]       # 67 transforms: two tiles
    got = runner.run(index, dev, sshape, np.stack([xf[k] for k in order]), 1)
    for slot, k in enumerate(order):
        want = miss if k == "miss" else alone[k]
        assert np.array_equal(got[slot].view(np.uint64), want.view(np.uint64)), (slot, k)
    # a source with no weight anywhere: every transform of a mixed launch fails the gate wave by wave
    empty = ac.DevSource(torch, (src[0], np.zeros_like(src[1])), sshape[0] * 4)
    got = runner.run(index, empty, sshape, np.stack([xf[k] for k in order]), 1)
    assert np.array_equal(got.view(np.uint64), np.zeros((len(order), 2), np.uint64))
    assert dev.untouched() and empty.untouched() and runner.tickets_zero()


def test_against_the_alignment_kernel(capi):
    """xs_tsdf_align_terms on the GPU for the same T: the count is equal and |sum r^2 - out29[27]| <= 8 * 2^-24 sum r^2 + the alignment
    model's bound on [27]."""
    runner = the_runner(capi)
    terms = ac.AlignRunner(torch, capi)
    sshape = (9, 10, 13)
    xyz, gt, src = sc.case(sshape, 257)
    index = ac.fabricated_band_index(torch, capi, xyz, gt)
    dev = ac.DevSource(torch, src, sshape[0] * 4 + 4)
    names = list(sc.case_xforms(sshape))
    for mw in sc.MIN_WEIGHTS:
        got = runner.run(index, dev, sshape, np.stack([sc.case_xforms(sshape)[k] for k in names]), mw)
        ref = terms.run(index, dev, sshape, np.stack([ac.case_maps(sshape)[k] for k in names]), mw)
        for k, name in enumerate(names):
            bound = ac.evaluate(xyz, gt, src, ac.case_maps(sshape)[name], mw)["bound"][27]
            assert got[k, 1] == ref[k, 28], (name, mw)
            assert abs(got[k, 0] - ref[k, 27]) <= sc.SUM_BOUND_U * sc.U * got[k, 0] + bound, (name, mw, got[k, 0], ref[k, 27], bound)
    assert dev.untouched() and runner.tickets_zero() and terms.tickets_zero()


def test_refusals(capi):
    """Each argument error: hipErrorInvalidValue with a text, nothing launched, nothing written — output, source and workspace."""
    runner = the_runner(capi)
    sshape = (9, 10, 13)
    xyz, gt, src = sc.case(sshape, 65)
    dev = ac.DevSource(torch, src, sshape[0] * 4)
    index = ac.fabricated_band_index(torch, capi, xyz, gt)
    one = np.ascontiguousarray(sc.case_xforms(sshape)["identity"][None], np.float32)
    many = np.ascontiguousarray(np.repeat(one, 4097, axis=0))
    out = torch.full((2 * 4097,), -7.0, dtype=torch.float64, device="cuda")
    ws_before = runner.ws.clone()
    _f32p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_int)

    def call(transforms=1, index=index, stride=1, value=dev.value.addr, weight=dev.weight.addr, step=dev.pitch, res=sshape, xforms=many, min_weight=1,
             max_residual=1.0, ws=runner.ws.data_ptr(), out=out.data_ptr(), null_res=False, null_xforms=False, null_index=False):
        r = np.ascontiguousarray(res, np.int32)
        m = np.ascontiguousarray(xforms, np.float32)
        return capi._lib.xs_tsdf_score_transforms(transforms, None if null_index else C.byref(index), stride, value, weight, step,
                                                  None if null_res else r.ctypes.data_as(_i32p), None if null_xforms else m.ctypes.data_as(_f32p), min_weight,
                                                  max_residual, ws, out, None)

    def unbuilt(**kw):
        i = capi.BandIndex()
        i.keys, i.values, i.capacity, i.count, i.nblocks = index.keys, index.values, index.capacity, index.count, index.nblocks
        for k, v in kw.items():
            setattr(i, k, v)
        return i

    nan, inf = many.copy(), many.copy()
    nan[0, 5], inf[0, 11] = np.nan, np.inf
    bad = [dict(transforms=0), dict(transforms=4097), dict(transforms=-1), dict(stride=0), dict(stride=-3), dict(null_index=True), dict(value=None),
           dict(weight=None), dict(null_res=True), dict(null_xforms=True), dict(ws=None), dict(out=None), dict(index=unbuilt(nblocks=0)),
           dict(index=unbuilt(count=-1)), dict(index=unbuilt(count=index.capacity + 1)), dict(index=unbuilt(keys=None)), dict(index=unbuilt(values=None)),
           dict(res=(1, 10, 13)), dict(res=(9, 0, 13)), dict(res=(9, 10, 262141)), dict(res=(2, 262140, 262140), step=8), dict(step=sshape[0] * 4 - 4),
           dict(step=sshape[0] * 4 + 2), dict(min_weight=0), dict(min_weight=-2), dict(max_residual=0.0), dict(max_residual=-1.0),
           dict(max_residual=float("inf")), dict(max_residual=float("nan")), dict(xforms=nan), dict(xforms=inf)]
    for change in bad:
        assert call(**change) == 1, change
        text = capi._lib.xs_last_error().decode()
        assert "xs_tsdf_score_transforms" in text, (change, text)
    torch.cuda.synchronize()
    assert (out == -7.0).all().item() and dev.untouched() and torch.equal(runner.ws, ws_before)
    # the limits themselves are accepted
    assert call(transforms=4096) == 0 and call(stride=2 ** 31 - 1, max_residual=1e-30) == 0
    torch.cuda.synchronize()
    assert runner.tickets_zero()
