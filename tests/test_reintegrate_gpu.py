"""GPU: xs_tsdf_reintegrate (x-slam_amd/csrc/xs_reintegrate.hip) against the float32 model of tests/reintegrate_cases.py.  The observations the
model applies are what the integrate kernel's exact walk writes into zeroed volumes (capi.integrate_scaled_ex with XS_INTEGRATE_NO_TILES), for
the nearest-pixel and the bilinear instance and for real and complex poses.  Values, weights and grads are compared with np.array_equal, counts
exactly; guard planes, padding and voxels no op sees must keep their bits."""
import importlib

import numpy as np
import pytest

import merge_cases as mc
import reintegrate_cases as rc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = rc.shapes()
_scenes = {}


@pytest.fixture(scope="module")
def capi():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("x-slam_amd.capi")


def scene_of(capi, shape, size):
    key = (tuple(shape), size)
    if key not in _scenes:
        _scenes[key] = rc.Scene(torch, capi, shape, size)
    return _scenes[key]


def check(vol, want, prior, touched, what):
    v, w, g, clean = rc.read_back(vol)
    assert not np.isnan(v).any() and not np.isnan(g).any(), what
    assert np.array_equal(w, want[1]), what
    assert np.array_equal(v, want[0]), (what, float(np.abs(v - want[0]).max()))
    assert np.array_equal(g, want[2]), (what, float(np.abs(g - want[2]).max()))
    assert clean, what
    keep = ~touched
    assert rc.same_words(v[keep], prior[0][keep]) and np.array_equal(w[keep], prior[1][keep]) and rc.same_words(g[keep], prior[2][keep]), what


@pytest.mark.parametrize("size", (0, 1))
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_model(capi, shape, size):
    """Op lists of length 1, 2, 3 and 8, mixed signs, repeated images, random prior states (weights 0, 1 and max_weight, values +-1); every
    list with the cull and without it, twice each; the list's number picks the pitch."""
    sc = scene_of(capi, shape, size)
    prior = rc.prior(shape)
    pitches = mc.pitches(shape[0])
    seen_any = 0
    for k, (name, ops) in enumerate(rc.OP_LISTS.items()):
        pitch, off = pitches[k % len(pitches)]
        model_ops = sc.model_ops(ops)
        want = rc.apply(prior, model_ops)
        touched = np.zeros(prior[0].shape, bool)
        for op in model_ops:
            touched |= op[1]
        seen_any += int(touched.sum())
        bufs = []
        for flags in (0, capi.REINTEGRATE_NO_CULL, 0):
            vol = mc.DevVolume3(torch, prior, pitch, off)
            counts = sc.run(vol, ops, flags=flags)
            assert counts == want[3], (name, flags, counts, want[3])
            check(vol, want, prior, touched, (name, flags))
            bufs.append(vol)
        for other in bufs[1:]:       # with and without the cull, and run to run: the same bytes, guards and padding included
            for a, b in zip((bufs[0].value, bufs[0].weight, bufs[0].grad), (other.value, other.weight, other.grad)):
                assert torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32)), name
    if max(shape) >= 33:             # the scenes see part of the volume: one side leaves the frustum, part lies behind the camera
        front = sc.observation(0, "front")[0]
        inside = sc.observation(1, "inside")[0]
        assert 0 < front.sum() < front.size and 0 < inside.sum() < inside.size
    assert not sc.observation(0, "away")[0].any() and seen_any > 0


@pytest.mark.parametrize("shape,size", [(SHAPES[3], 0), (SHAPES[4], 1), (SHAPES[6], 1)])
def test_one_addition_equals_integrate_scaled(capi, shape, size):
    """[+1] into any prior state is xs_integrate_scaled on a copy: weights and the count exactly, values with np.array_equal."""
    sc = scene_of(capi, shape, size)
    s = sc.s
    prior = rc.prior(shape)
    X, Y, Z = shape
    for k, pose in enumerate(("front", "inside", "seeded", "oblique")):
        pitch, off = mc.pitches(X)[k]
        a, b = mc.DevVolume3(torch, prior, pitch, off), mc.DevVolume3(torch, prior, pitch, off)
        counts = sc.run(a, [(1, k % 2, pose)])
        n = torch.zeros(1, dtype=torch.int64, device="cuda")
        R, t = sc.poses[pose]
        capi.integrate_scaled(sc.images[k % 2], s["cols"] * 4, s["rows"], s["cols"], s["intr"], rc.MAX_WEIGHT, [X, Y, Z], s["voxel_size"], R, t, s["tranc_dist"],
                              b.value.addr, b.weight.addr, b.grad.addr, pitch, threshold=s["threshold"], updated=n)
        torch.cuda.synchronize()
        va, wa, ga, clean_a = rc.read_back(a)
        vb, wb, gb, clean_b = rc.read_back(b)
        assert counts == [0, int(n.item()), 0, 0] and counts[1] == int(sc.observation(k % 2, pose)[0].sum()), pose
        assert np.array_equal(wa, wb) and np.array_equal(va, vb) and np.array_equal(ga, gb) and clean_a and clean_b, pose


@pytest.mark.parametrize("shape,size", [(SHAPES[3], 1), (SHAPES[5], 0)])
def test_plane_ranges_add_up(capi, shape, size):
    """Disjoint plane ranges that cover the volume, in any order, give the whole-volume result and counts; the pointers are at the range's
    first plane; planes outside a range keep their bits."""
    sc = scene_of(capi, shape, size)
    prior = rc.prior(shape)
    Z = shape[2]
    pitch, off = mc.pitches(shape[0])[2]
    for name in ("eight", "three"):
        ops = rc.OP_LISTS[name]
        want = rc.apply(prior, sc.model_ops(ops))
        for flags in (0, capi.REINTEGRATE_NO_CULL):
            vol = mc.DevVolume3(torch, prior, pitch, off)
            counts = torch.zeros(4, dtype=torch.int64, device="cuda")
            for i, (z0, z1) in enumerate([(Z - 1, Z), (0, 1), (1, Z - 1)]):
                got = sc.run(vol, ops, flags=flags, z0=z0, z1=z1, counts=counts)
                if i == 0:
                    v, w, g, clean = rc.read_back(vol)
                    assert clean and rc.same_words(v[:z0], prior[0][:z0]) and np.array_equal(w[:z0], prior[1][:z0]) and rc.same_words(g[:z0], prior[2][:z0])
                    assert np.array_equal(v[z0:], want[0][z0:]) and np.array_equal(w[z0:], want[1][z0:]) and np.array_equal(g[z0:], want[2][z0:])
            assert got == want[3], (name, flags)
            v, w, g, clean = rc.read_back(vol)
            assert clean and np.array_equal(v, want[0]) and np.array_equal(w, want[1]) and np.array_equal(g, want[2]), (name, flags)


@pytest.mark.parametrize("shape,size", [(SHAPES[3], 0), (SHAPES[6], 1)])
def test_two_launches_of_four_equal_one_of_eight(capi, shape, size):
    sc = scene_of(capi, shape, size)
    prior = rc.prior(shape)
    pitch, off = mc.pitches(shape[0])[1]
    for name in ("eight", "drain", "fill"):
        ops = rc.OP_LISTS[name]
        one, two = mc.DevVolume3(torch, prior, pitch, off), mc.DevVolume3(torch, prior, pitch, off)
        c1 = sc.run(one, ops)
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        sc.run(two, ops[:4], counts=counts)
        c2 = sc.run(two, ops[4:], counts=counts)
        assert c1 == c2 == rc.apply(prior, sc.model_ops(ops))[3], name
        for a, b in zip((one.value, one.weight, one.grad), (two.value, two.weight, two.grad)):
            assert torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32)), name


def test_refusals(capi):
    """Each argument error: hipErrorInvalidValue with a text, nothing launched, volume and counts untouched."""
    shape = SHAPES[1]
    X, Y, Z = shape
    sc = scene_of(capi, shape, 0)
    prior = rc.prior(shape)
    vol = mc.DevVolume3(torch, prior, X * 4 + 4)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    good = sc.device_ops(rc.OP_LISTS["move"])
    R, t = sc.poses["front"]
    nan_R, inf_t = R.copy(), t.copy()
    nan_R[1, 2, 1], inf_t[0, 0] = np.nan, np.inf
    bad = [dict(ops=[]), dict(ops=good * 5), dict(ops=[(0,) + good[0][1:]]), dict(ops=[(2,) + good[0][1:]]), dict(ops=[good[0], (-1, None) + good[0][2:]]),
           dict(ops=[(1, good[0][1], nan_R, t)]), dict(ops=[good[0], (1, good[0][1], R, inf_t)]),
           dict(value=None), dict(weight=None), dict(grad=None), dict(counts_arg=None), dict(vol_step=X * 4 - 4), dict(vol_step=X * 4 + 2),
           dict(z0=1, z1=1), dict(z0=2, z1=1), dict(z0=-1, z1=1), dict(z0=0, z1=Z + 1), dict(max_weight=0), dict(max_weight=(1 << 24) + 1),
           dict(res=[0, Y, Z]), dict(res=[X, 300000, Z]), dict(voxel_size=0.0), dict(tranc_dist=float("nan"))]
    for change in bad:
        with pytest.raises(capi.XsError) as e:
            sc.run(vol, rc.OP_LISTS["move"], counts=counts, **change)
        assert "hip error 1:" in str(e.value) and "xs_tsdf_reintegrate" in str(e.value), (change, str(e.value))
    torch.cuda.synchronize()
    assert vol.untouched() and not counts.any()
    sc.run(vol, rc.OP_LISTS["move"], counts=counts, max_weight=1 << 24)     # the limits themselves are accepted
    sc.run(vol, rc.OP_LISTS["eight"], counts=counts, max_weight=1)
    assert counts.any()


def test_rows_past_2_31_bytes(capi):
    """A (65, 33, 64) volume in rows of 1 MiB: 2112 rows, the last ones past 2^31 bytes.  The three arrays share one 2.2 GB buffer, each row
    holding a value, a weight and a grad segment; the rest of the buffer holds a pattern and must keep it."""
    shape = (65, 33, 64)
    X, Y, Z = shape
    pitch = 1 << 20
    rows = Y * Z
    assert (rows - 1) * pitch > 2 ** 31
    sc = scene_of(capi, shape, 1)
    prior = rc.prior(shape)
    ops = rc.OP_LISTS["far"]
    want = rc.apply(prior, sc.model_ops(ops))
    far = want[1][Z - 2:] != prior[1][Z - 2:]
    assert far.any()                                        # the last planes, past 2^31 bytes, are written
    buf = torch.full((rows * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
    words = buf.view(torch.int32)
    views = [words.as_strided((Z, Y, X), (Y * (pitch // 4), pitch // 4, 1), k * 128) for k in range(3)]      # segments 512 bytes apart
    for view, a in zip(views, prior):
        view.copy_(torch.from_numpy(np.array(a).view(np.int32)).cuda())

    class Vol:
        pass
    vol = Vol()
    vol.pitch = pitch
    for name, k in (("value", 0), ("weight", 1), ("grad", 2)):
        seg = Vol()
        seg.addr = buf.data_ptr() + k * 512
        setattr(vol, name, seg)
    results = []
    for flags in (0, capi.REINTEGRATE_NO_CULL):
        for view, a in zip(views, prior):
            view.copy_(torch.from_numpy(np.array(a).view(np.int32)).cuda())
        counts = sc.run(vol, ops, flags=flags)
        got = [view.cpu().numpy() for view in views]
        assert counts == want[3], flags
        assert np.array_equal(got[0].view(np.float32), want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2].view(np.float32), want[2]), flags
        results.append(got)
    assert all(np.array_equal(a, b) for a, b in zip(*results))
    for view in views:                                      # what lies between the segments kept the pattern
        view.fill_(-1515870811)                             # 0xA5A5A5A5
    assert bool((buf == 0xA5).all())
