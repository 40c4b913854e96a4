"""GPU parity: HIP TSDF integrate (through the C ABI) vs the CPU oracle on the same seeded
inputs.  Both sides evaluate the same float32 expressions without FMA contraction, so the
bar is bit-exact value / weight / grad with a small budget for voxels where a libm ulp flips
a discrete decision (pixel pick, truncation test)."""
import numpy as np
import pytest

from helpers import intr_of, mismatch_fraction, s1_transforms, synth, tranc_dist

pytestmark = pytest.mark.gpu

FLIP_BUDGET = 2e-5  # fraction of voxels allowed to differ at all (rounding flips)
REL_TOL = 1e-6      # relative tolerance on value; derivative (grad) relative to max|grad|


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    capi = __import__("importlib").import_module("x-slam_amd.capi")
    return torch, capi


def run_gpu(torch, capi, prm, frames, res, pitch_elems=None, threshold=0.0, slabs=1, max_weight=None, depth_fn=None, far_clip=False, bricks=False,
            always_store=False):
    X, Y, Z = res
    pitch = (pitch_elems or X)
    step = pitch * 4
    value = torch.full((Y * Z, pitch), 7.0, dtype=torch.float32, device="cuda")
    weight = torch.full((Y * Z, pitch), 7, dtype=torch.int32, device="cuda")
    grad = torch.full((Y * Z, pitch), 7.0, dtype=torch.float32, device="cuda")
    capi.init_volume(value, weight, grad, step, res)
    scaled = torch.empty((synth.HEIGHT, synth.WIDTH), dtype=torch.float32, device="cuda")
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    counts = []
    mw = max_weight or prm["max_integration_weight"]
    for k in frames:
        d = depth_fn(k) if depth_fn else synth.s1_frame(k)
        depth = torch.from_numpy(d.astype(np.int16)).cuda()  # same bits as u16
        T = s1_transforms(k, prm)
        counter.zero_()
        bounds = [Z * i // slabs for i in range(slabs + 1)]
        for s in range(slabs):
            z0, z1 = bounds[s], bounds[s + 1]
            off = z0 * Y
            if far_clip or bricks:  # the orchestrator's path: frame depth maximum -> far clip; brick work list
                dmax = torch.zeros(1, dtype=torch.float32, device="cuda")
                capi.scale_depth_max(depth, synth.WIDTH * 2, synth.HEIGHT, synth.WIDTH, scaled, synth.WIDTH * 4, dmax)
                ws = torch.zeros(capi.integrate_workspace_bytes(res, z1 - z0), dtype=torch.uint8, device="cuda") if bricks else None
                capi.integrate_scaled_ex(scaled, synth.WIDTH * 4, synth.HEIGHT, synth.WIDTH, intr_of(prm), mw, res, prm["tsdf_voxel_size"],
                                         T["Rv2c"], T["tv2c"], tranc_dist(prm), value[off:], weight[off:], grad[off:], step,
                                         8 if always_store else 0, threshold=threshold, z0=z0, z1=z1, updated=counter,
                                         depth_max=dmax if far_clip else None, workspace=ws)
            else:
                capi.integrate_tsdf_volume(depth, synth.WIDTH * 2, synth.HEIGHT, synth.WIDTH, intr_of(prm), mw, res,
                                           prm["tsdf_voxel_size"], T["Rv2c"], T["tv2c"], tranc_dist(prm),
                                           value[off:], weight[off:], grad[off:], step, scaled, synth.WIDTH * 4,
                                           threshold=threshold, z0=z0, z1=z1, updated=counter)
        torch.cuda.synchronize()
        counts.append(int(counter.item()))
    v = value[:, :X].contiguous().cpu().numpy().reshape(-1)
    w = weight[:, :X].contiguous().cpu().numpy().reshape(-1)
    g = grad[:, :X].contiguous().cpu().numpy().reshape(-1)
    return v, w, g, counts


def run_cpu(oracle, prm, frames, res, threshold=0.0, max_weight=None, depth_fn=None):
    v, w, g = oracle.new_volume(res)
    counts = []
    mw = max_weight or prm["max_integration_weight"]
    for k in frames:
        d = depth_fn(k) if depth_fn else synth.s1_frame(k)
        T = s1_transforms(k, prm)
        ds = oracle.scale_depth(d)
        counts.append(oracle.integrate(ds, v, w, g, res, tranc_dist(prm), mw, T["Rv2c"], T["tv2c"], intr_of(prm),
                                       prm["tsdf_voxel_size"], threshold))
    return v, w, g, counts


def compare(gpu, cpu):
    gv, gw, gg, gc = gpu
    cv, cw, cg, cc = cpu
    assert mismatch_fraction(gw, cw) <= FLIP_BUDGET
    assert mismatch_fraction(gv, cv) <= FLIP_BUDGET
    assert mismatch_fraction(gg, cg) <= FLIP_BUDGET
    same_w = gw == cw
    assert np.all(np.abs(gv[same_w] - cv[same_w]) <= REL_TOL * np.maximum(np.abs(cv[same_w]), 1e-3))
    gscale = max(np.abs(cg).max(), 1e-12)
    assert np.all(np.abs(gg[same_w] - cg[same_w]) <= REL_TOL * np.maximum(np.abs(cg[same_w]), gscale * 1e-2))
    for a, b in zip(gc, cc):
        assert abs(a - b) <= max(2, 1e-4 * b)
    assert np.abs(cg).max() > 0, "the CSFD seed must reach the volume"


@pytest.mark.parametrize("n", [64, 96, 128])
def test_integrate_s1_three_frames(dev, oracle, n):
    torch, capi = dev
    prm = synth.s1_params(n)
    res = [n, n, n]
    compare(run_gpu(torch, capi, prm, [0, 1, 2], res), run_cpu(oracle, prm, [0, 1, 2], res))


@pytest.mark.parametrize("n,threshold", [(96, 0.0), (128, 0.02)])
def test_integrate_far_clip_changes_nothing(dev, oracle, n, threshold):
    """Column clipping against the frame's largest depth skips only voxels the reference would
    not write: identical volumes with and without it, and both equal to the oracle."""
    torch, capi = dev
    prm = synth.s1_params(n, threshold=threshold)
    res = [n, n, n]
    a = run_gpu(torch, capi, prm, [0, 5, 9], res, threshold=threshold)
    for kw in (dict(far_clip=True), dict(bricks=True), dict(far_clip=True, bricks=True), dict(far_clip=True, bricks=True, slabs=3)):
        b = run_gpu(torch, capi, prm, [0, 5, 9], res, threshold=threshold, **kw)
        for u, v in zip(a[:3], b[:3]):
            assert np.array_equal(u, v), kw
        assert a[3] == b[3], kw
    compare(b, run_cpu(oracle, prm, [0, 5, 9], res, threshold=threshold))


def test_integrate_non_cubic_pitched_volume(dev, oracle):
    """A volume of 96 x 64 x 80 voxels in rows of 112 (a pitch wider than the row): the column walk, the brick list with
    the far clip, and the same over three z-slabs — against the oracle and against each other."""
    torch, capi = dev
    prm = synth.s1_params(96)
    res = [96, 64, 80]
    cpu = run_cpu(oracle, prm, [0, 3, 6], res)
    a = run_gpu(torch, capi, prm, [0, 3, 6], res, pitch_elems=112)
    compare(a, cpu)
    for kw in (dict(far_clip=True, bricks=True), dict(far_clip=True, bricks=True, slabs=3)):
        b = run_gpu(torch, capi, prm, [0, 3, 6], res, pitch_elems=112, **kw)
        for u, v in zip(a[:3], b[:3]):
            assert np.array_equal(u, v), kw
        assert a[3] == b[3], kw
    assert cpu[3][-1] > 1000


def test_integrate_with_the_brick_list_classified_ahead(dev):
    """xs_integrate_classify for the pose the last ICP launch starts from + xs_integrate_scaled_ex(LIST_IS_READY) for the final
    pose: the same volume and count, bit for bit, as the plain call — for a final pose a last ICP update away (covered) —, and
    xs_integrate_list_covers refuses a pose centimetres away."""
    torch, capi = dev
    n = 128
    prm = synth.s1_params(n)
    res = [n, n, n]
    Hh, Ww = synth.HEIGHT, synth.WIDTH
    scaled = torch.empty((Hh, Ww), dtype=torch.float32, device="cuda")
    dmax = torch.zeros(1, dtype=torch.float32, device="cuda")

    def fresh():
        v = torch.empty((n * n, n), dtype=torch.float32, device="cuda"); w = torch.empty((n * n, n), dtype=torch.int32, device="cuda")
        g = torch.empty((n * n, n), dtype=torch.float32, device="cuda")
        capi.init_volume(v, w, g, n * 4, res)
        return v, w, g
    a, b = fresh(), fresh()
    ws = torch.zeros(capi.integrate_workspace_bytes(res), dtype=torch.uint8, device="cuda")
    ca, cb = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    k4, vs, trunc = intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm)
    for k in (0, 4, 8):
        depth = torch.from_numpy(synth.s1_frame(k).astype(np.int16)).cuda()
        capi.scale_depth_max(depth, Ww * 2, Hh, Ww, scaled, Ww * 4, dmax)
        T = s1_transforms(k, prm)
        # the pose the classification sees: the final one moved by a last-iteration-sized update (0.3 mm, 2e-5 rad about y)
        Rl = np.array(T["Rv2c"], np.float32).reshape(3, 3, 2).copy(); tl = np.array(T["tv2c"], np.float32).reshape(3, 2).copy()
        c_, s_ = np.cos(2e-5), np.sin(2e-5)
        Ry = np.array([[c_, 0, s_], [0, 1, 0], [-s_, 0, c_]], np.float32)
        Rl[..., 0] = Ry @ Rl[..., 0]; tl[:, 0] = Ry @ tl[:, 0] + np.array([3e-4, -2e-4, 1e-4], np.float32)
        assert capi.integrate_list_covers(Hh, Ww, k4, res, vs, Rl, tl, 2.0, T["Rv2c"], T["tv2c"])
        capi.integrate_scaled(scaled, Ww * 4, Hh, Ww, k4, 100, res, vs, T["Rv2c"], T["tv2c"], trunc, *a, n * 4, updated=ca, depth_max=dmax, workspace=ws)
        capi.integrate_classify(Hh, Ww, k4, res, vs, Rl, tl, trunc, ws, slack_scale=2.0, depth_max=dmax)
        capi.integrate_scaled_ex(scaled, Ww * 4, Hh, Ww, k4, 100, res, vs, T["Rv2c"], T["tv2c"], trunc, *b, n * 4, 1 | 4, updated=cb, depth_max=dmax,
                                 workspace=ws)
        torch.cuda.synchronize()
        assert int(ca.item()) == int(cb.item()) > 1000
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        far_t = tl.copy(); far_t[0, 0] += 0.05
        assert not capi.integrate_list_covers(Hh, Ww, k4, res, vs, Rl, far_t, 2.0, T["Rv2c"], T["tv2c"])


def test_integrate_rotated_and_inside_out_views(dev, oracle):
    """Column clipping under strong rotations (every sign of the half-space slopes), a camera
    outside the volume and a view from the far side."""
    torch, capi = dev
    n = 96
    prm = synth.s1_params(n)
    res = [n, n, n]
    rng = np.random.default_rng(3)
    d = synth.s1_frame(0)
    ds = oracle.scale_depth(d)
    depth = torch.from_numpy(d.astype(np.int16)).cuda()
    scaled = torch.empty((synth.HEIGHT, synth.WIDTH), dtype=torch.float32, device="cuda")
    for trial in range(8):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        ang = rng.uniform(0.2, 3.0)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        tv = rng.uniform(-2.0, 9.0, 3)  # camera position in the volume frame, sometimes outside
        v2c = np.eye(4); v2c[:3, :3] = Rm.T; v2c[:3, 3] = -Rm.T @ tv
        R = np.zeros((3, 3, 2), np.float32); R[..., 0] = v2c[:3, :3]; R[..., 1] = rng.normal(size=(3, 3)) * 1e-7
        t = np.zeros((3, 2), np.float32); t[:, 0] = v2c[:3, 3]; t[:, 1] = rng.normal(size=3) * 1e-7
        value = torch.zeros((n * n, n), dtype=torch.float32, device="cuda")
        weight = torch.zeros((n * n, n), dtype=torch.int32, device="cuda")
        grad = torch.zeros((n * n, n), dtype=torch.float32, device="cuda")
        dmax = torch.zeros(1, dtype=torch.float32, device="cuda")
        counter = torch.zeros(1, dtype=torch.int64, device="cuda")
        capi.scale_depth_max(depth, synth.WIDTH * 2, synth.HEIGHT, synth.WIDTH, scaled, synth.WIDTH * 4, dmax)
        ws = torch.zeros(capi.integrate_workspace_bytes(res), dtype=torch.uint8, device="cuda") if trial % 2 else None
        capi.integrate_scaled(scaled, synth.WIDTH * 4, synth.HEIGHT, synth.WIDTH, intr_of(prm), 100, res, prm["tsdf_voxel_size"], R, t,
                              tranc_dist(prm), value, weight, grad, n * 4, updated=counter, depth_max=dmax, workspace=ws)
        torch.cuda.synchronize()
        assert abs(float(dmax.item()) - float(ds.max())) == 0.0
        v, w, g = oracle.new_volume(res)
        U = oracle.integrate(ds, v, w, g, res, tranc_dist(prm), 100, R, t, intr_of(prm), prm["tsdf_voxel_size"])
        gpu = (value.cpu().numpy().reshape(-1), weight.cpu().numpy().reshape(-1), grad.cpu().numpy().reshape(-1), [int(counter.item())])
        assert mismatch_fraction(gpu[1], w) <= FLIP_BUDGET and mismatch_fraction(gpu[0], v) <= FLIP_BUDGET, trial
        assert mismatch_fraction(gpu[2], g) <= FLIP_BUDGET, trial
        assert abs(gpu[3][0] - U) <= max(2, 1e-4 * U)


def test_integrate_bilinear_branch(dev, oracle):
    torch, capi = dev
    prm = synth.s1_params(96, threshold=0.02)
    res = [96, 96, 96]
    gpu = run_gpu(torch, capi, prm, [0, 3], res, threshold=0.02)
    cpu = run_cpu(oracle, prm, [0, 3], res, threshold=0.02)
    compare(gpu, cpu)
    near = run_cpu(oracle, prm, [0, 3], res, threshold=0.0)
    assert mismatch_fraction(cpu[0], near[0]) > 1e-4, "the bilinear branch must be exercised"


def test_integrate_ragged_pitched_volume(dev, oracle):
    """X, Y, Z all different, X not a multiple of the wave, pitch wider than a row."""
    torch, capi = dev
    prm = synth.s1_params(128)
    res = [100, 70, 90]
    cpu = run_cpu(oracle, prm, [0, 2], res)
    compare(run_gpu(torch, capi, prm, [0, 2], res, pitch_elems=128), cpu)
    compare(run_gpu(torch, capi, prm, [0, 2], res, pitch_elems=128, far_clip=True, bricks=True), cpu)


@pytest.mark.parametrize("slabs", [2, 3, 8])
def test_integrate_z_slabs_equal_whole(dev, oracle, slabs):
    """Sharding by z-slab (one launch per slab on its own storage) reproduces the whole volume."""
    torch, capi = dev
    prm = synth.s1_params(96)
    res = [96, 96, 96]
    whole = run_gpu(torch, capi, prm, [0, 1], res)
    parts = run_gpu(torch, capi, prm, [0, 1], res, slabs=slabs)
    for a, b in zip(whole[:3], parts[:3]):
        assert np.array_equal(a, b)
    assert whole[3] == parts[3]


def test_integrate_weight_saturation(dev, oracle):
    """Stored weight clamps at max_weight while the mean uses the unclamped one (TsdfFusion.cu:165-166)."""
    torch, capi = dev
    prm = synth.s1_params(64)
    res = [64, 64, 64]
    gpu = run_gpu(torch, capi, prm, [0, 0, 0, 0], res, max_weight=2)
    cpu = run_cpu(oracle, prm, [0, 0, 0, 0], res, max_weight=2)
    compare(gpu, cpu)
    assert gpu[1].max() == 2


@pytest.mark.parametrize("threshold", [0.0, 0.02])
def test_integrate_stores_only_words_that_change(dev, oracle, threshold):
    """The kernels store only the words of an updated voxel whose bits change (free space in front of a surface keeps
    (1, 0) from its second observation on; a saturated weight stays): the volume after six frames — the weight saturates
    at three — is identical to the one XS_INTEGRATE_ALWAYS_STORE writes, on the brick path and on the column walk, and
    equal to the oracle's."""
    torch, capi = dev
    prm = synth.s1_params(96, threshold=threshold)
    res = [96, 96, 96]
    frames = [0, 0, 1, 2, 2, 3]
    for kw in (dict(far_clip=True, bricks=True), dict(far_clip=True)):
        a = run_gpu(torch, capi, prm, frames, res, threshold=threshold, max_weight=3, always_store=True, **kw)
        b = run_gpu(torch, capi, prm, frames, res, threshold=threshold, max_weight=3, **kw)
        for u, v in zip(a[:3], b[:3]):
            assert np.array_equal(u, v), kw
        assert a[3] == b[3], kw
    compare(b, run_cpu(oracle, prm, frames, res, threshold=threshold, max_weight=3))
    assert b[1].max() == 3 and (b[0] == 1.0).sum() > 1000


def test_integrate_empty_inputs(dev, oracle):
    torch, capi = dev
    prm = synth.s1_params(64)
    res = [64, 64, 64]
    zero = lambda k: np.zeros((synth.HEIGHT, synth.WIDTH), np.uint16)
    v, w, g, c = run_gpu(torch, capi, prm, [0], res, depth_fn=zero)
    assert c == [0] and not v.any() and not w.any() and not g.any()
    far = lambda k: np.full((synth.HEIGHT, synth.WIDTH), 6000, np.uint16)  # beyond the 5 m gate
    v, w, g, c = run_gpu(torch, capi, prm, [0], res, depth_fn=far)
    assert c == [0] and not w.any()
    # empty slab: nothing launched, nothing touched
    value = torch.ones((8, 64), dtype=torch.float32, device="cuda")
    weight = torch.ones((8, 64), dtype=torch.int32, device="cuda")
    capi.init_volume(value, weight, value, 256, res, z0=5, z1=5)
    torch.cuda.synchronize()
    assert float(value.min()) == 1.0


def test_integrate_size_independent_properties_512(dev):
    """Full size (512^3, BASELINE config): weight == number of frames fused wherever touched,
    weights equal the update counter, untouched voxels stay exactly zero, and re-integrating
    the same frame leaves value unchanged where tsdf is the truncated constant 1."""
    torch, capi = dev
    n = 512
    prm = synth.s1_params(n)
    res = [n, n, n]
    v, w, g, c = run_gpu(torch, capi, prm, [0], res, far_clip=True, bricks=True)
    assert int(w.sum()) == c[0]
    assert abs(c[0] - 1930365) <= 200  # reference kernel, same scene
    assert not v[w == 0].any() and not g[w == 0].any()
    assert np.all(np.abs(v[w > 0]) <= 1.0 + 1e-6)
    v2, w2, g2, c2 = run_gpu(torch, capi, prm, [0, 0], res, far_clip=True, bricks=True)
    assert c2[1] == c2[0]
    assert np.array_equal(w2, 2 * w)
    free = v == 1.0
    assert np.all(v2[free] == 1.0)


def test_frustum_filling_scene_512_classes_and_order_against_the_walk_everywhere(dev):
    """Scene S2 (the frustum fills the volume: 23 000 listed bricks at 512^3 — the launch on which integrate is HBM-bound, and the one
    whose list is ordered with a reservation per 32 bricks): three launches with the boxes' classes and the ordered list against the
    per-voxel walk of every listed voxel (XS_INTEGRATE_NO_TILES), volumes and counts bit for bit; the ordered list holds the listed
    bricks once each, those with planes to walk in front."""
    torch, capi = dev
    n = 512
    prm = synth.s2_params(n)
    res = [n, n, n]
    Hh, Ww = synth.HEIGHT, synth.WIDTH
    vs, trunc = float(np.float32(prm["tsdf_voxel_size"])), synth.tranc_dist(prm)
    depth = torch.from_numpy(synth.render_s2().view(np.int16)).cuda()
    scaled = torch.empty((Hh, Ww), dtype=torch.float32, device="cuda")
    dmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    capi.scale_depth_max(depth, Ww * 2, Hh, Ww, scaled, Ww * 4, dmax)
    R = np.zeros((3, 3, 2), np.float32); R[[0, 1, 2], [0, 1, 2], 0] = 1
    t = np.zeros((3, 2), np.float32); t[:, 0] = [-prm["init_x"], -prm["init_y"], -prm["init_z"]]; t[0, 1] = 1e-7
    k4 = np.array([synth.FX, synth.FY, synth.CX, synth.CY], np.float32)
    ws = torch.zeros(capi.integrate_workspace_bytes(res), dtype=torch.uint8, device="cuda")
    vols, counts = [], []
    for flags in (64, 32):
        v = torch.empty((n * n, n), dtype=torch.float32, device="cuda"); w = torch.empty((n * n, n), dtype=torch.int32, device="cuda")
        g = torch.empty((n * n, n), dtype=torch.float32, device="cuda")
        capi.init_volume(v, w, g, n * 4, res)
        c = torch.zeros(1, dtype=torch.int64, device="cuda")
        for _ in range(3):
            capi.integrate_scaled_ex(scaled, Ww * 4, Hh, Ww, k4, 2, res, vs, R, t, trunc, v, w, g, n * 4, flags, updated=c, depth_max=dmax, workspace=ws)
        torch.cuda.synchronize()
        vols.append((v, w, g)); counts.append(int(c.item()))
        if flags == 64:
            host = ws.cpu().numpy()
            list_off, cap, class_off, second_off = capi.integrate_list_layout(res)
            count = int(host[:4].view(np.int32)[0])
            nwalk, nother = (int(x) for x in host[208:216].view(np.int32))
            assert count > 4096 and nwalk + nother == count and nwalk > 1000 and nother > 1000
            region = host[second_off:second_off + cap * 4].view(np.int32)
            ids = np.concatenate([region[:nwalk], region[cap - nother:]])
            assert np.array_equal(np.sort(ids), np.sort(host[list_off:list_off + 4 * count].view(np.int32)))
            words = host[class_off:class_off + cap * 16].view(np.uint32).reshape(cap, 4)
            walked = lambda wd: (8 - (wd & 0xff).astype(np.int64) - ((wd >> 8) & 0xff).astype(np.int64)).sum(axis=1)
            assert (walked(words[:nwalk]) > 0).all() and (walked(words[cap - nother:]) == 0).all()
            assert class_counts(ws)[0] > 10000     # wave-sized boxes wholly in free space
    assert counts[0] == counts[1] > 3 * 30_000_000
    for x, y in zip(*vols):
        assert torch.equal(x, y)


def test_full_size_properties_512(dev):
    """Size-independent properties at the benchmark's full size (512^3, scene S1): z-slab launches tile the
    whole-volume launch bit for bit and count the same voxels; integrating the same frame again leaves every
    written voxel's value within an ulp (running mean of equal samples) and raises its weight by one; the count
    of written voxels equals the figure recorded from the reference kernel body."""
    torch, capi = dev
    import json, os
    n = 512
    prm = synth.s1_params(n)
    res = [n, n, n]
    T = s1_transforms(0, prm)
    depth = torch.from_numpy(synth.s1_frame(0).view(np.int16)).cuda()
    scaled = torch.empty((synth.HEIGHT, synth.WIDTH), dtype=torch.float32, device="cuda")
    dmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    capi.scale_depth_max(depth, synth.WIDTH * 2, synth.HEIGHT, synth.WIDTH, scaled, synth.WIDTH * 4, dmax)
    def volume():
        return (torch.zeros((n * n, n), dtype=torch.float32, device="cuda"), torch.zeros((n * n, n), dtype=torch.int32, device="cuda"),
                torch.zeros((n * n, n), dtype=torch.float32, device="cuda"))
    def run(vol, z0, z1, counter):
        v, w, g = vol
        off = z0 * n
        ws = torch.zeros(capi.integrate_workspace_bytes(res, z1 - z0), dtype=torch.uint8, device="cuda")
        capi.integrate_scaled(scaled, synth.WIDTH * 4, synth.HEIGHT, synth.WIDTH, intr_of(prm), 100, res, prm["tsdf_voxel_size"], T["Rv2c"],
                              T["tv2c"], tranc_dist(prm), v[off:], w[off:], g[off:], n * 4, z0=z0, z1=z1, updated=counter, depth_max=dmax,
                              workspace=ws)
    whole, parts = volume(), volume()
    c_whole = torch.zeros(1, dtype=torch.int64, device="cuda"); c_parts = torch.zeros(1, dtype=torch.int64, device="cuda")
    run(whole, 0, n, c_whole)
    for z0, z1 in ((0, 100), (100, 301), (301, n)):
        run(parts, z0, z1, c_parts)
    torch.cuda.synchronize()
    U = int(c_whole.item())
    assert U == int(c_parts.item()) == int((whole[1] > 0).sum().item())
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)
    fig = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "survey_reference_kernel_figures.json")))
    assert abs(U - fig["integrate_U"]["512"]) <= 2
    # the same frame again
    v0, w0, g0 = whole[0].clone(), whole[1].clone(), whole[2].clone()
    run(whole, 0, n, c_whole)
    torch.cuda.synchronize()
    written = w0 > 0
    assert torch.equal(whole[1][written], w0[written] + 1) and torch.equal(whole[1][~written], w0[~written])
    dv = (whole[0][written] - v0[written]).abs()
    assert float(dv.max()) <= 1.2e-7 and float((dv > 0).float().mean()) < 0.5
    dg = (whole[2][written] - g0[written]).abs()
    assert float(dg.max()) <= 2.4e-7 * max(float(g0.abs().max()), 1e-30)


# ---- round 4: depth tiles and the brick classification (free space / nothing to write / exact walk) ----------------------------
def tiles_numpy(scaled, tw=8, th=8):
    """{lo, hi} per tw x th pixels of a scaled depth image over its VALID pixels, lo negated where the tile holds an invalid one (depth 0),
    {-inf, 0} where it holds no valid one (csrc/xs_scale_depth.hip, k_scale_depth)."""
    h, w = scaled.shape
    ty, tx = -(-h // th), -(-w // tw)
    out = np.zeros((ty, tx, 2), np.float32)
    for j in range(ty):
        for i in range(tx):
            blk = scaled[j * th:(j + 1) * th, i * tw:(i + 1) * tw]
            valid = blk[blk > 0]
            lo = np.float32(valid.min()) if valid.size else np.float32(np.inf)
            out[j, i] = (-lo if valid.size < blk.size else lo, blk.max())
    return out


holed = synth.holed   # (shared with bench.py's roofline_s2.noisy)


@pytest.mark.parametrize("shape", [(480, 640), (150, 200), (97, 131)])
def test_depth_tile_table(dev, oracle, shape):
    """xs_scale_depth_tiles: the scaled image and the frame maximum of xs_scale_depth_max, plus the per-tile depth range — against
    numpy on whole, ragged and holed images; xs_depth_tiles builds the same table from the scaled image."""
    torch, capi = dev
    rng = np.random.default_rng(11)
    h, w = shape
    d = holed(synth.s1_frame(3)[:h, :w], rng)
    d[0, 0] = 5000; d[h - 1, w - 1] = 200; d[5, 7] = 5001; d[6, 7] = 199
    depth = torch.from_numpy(np.ascontiguousarray(d).astype(np.int16)).cuda()
    scaled = torch.full((h, w), -1.0, dtype=torch.float32, device="cuda")
    dmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    nb = capi.depth_tiles_bytes(h, w)
    assert nb == (-(-h // 8) * -(-w // 8) + -(-h // 32) * -(-w // 64)) * 8     # 8 x 8 tiles, then 64 x 32 super tiles
    tiles = torch.full((nb // 4,), -1.0, dtype=torch.float32, device="cuda")
    capi.scale_depth_tiles(depth, w * 2, h, w, scaled, w * 4, dmax, tiles)
    torch.cuda.synchronize()
    ref = oracle.scale_depth(np.ascontiguousarray(d))
    got = scaled.cpu().numpy()
    assert np.array_equal(got, ref)
    assert float(dmax.item()) == float(ref.max())
    want = np.concatenate([tiles_numpy(ref).reshape(-1, 2), tiles_numpy(ref, 64, 32).reshape(-1, 2)])
    assert np.array_equal(tiles.cpu().numpy().reshape(-1, 2), want)
    again = torch.full_like(tiles, -1.0)
    capi.depth_tiles(scaled, w * 4, h, w, again)
    torch.cuda.synchronize()
    assert torch.equal(again, tiles)


def class_counts(ws):
    """boxes wholly free / wholly empty / with planes to walk (the workspace header's first three class counters)"""
    return [int(x) for x in ws[192:204].view(__import__("torch").int32).cpu().numpy()]


@pytest.mark.parametrize("n,threshold", [(128, 0.0), (256, 0.02), (256, 0.0)])
def test_brick_classification_is_invisible(dev, oracle, n, threshold):
    """The kernel's own classification of each wave-sized box from the depth tiles (free space: tsdf = (1, 0) streamed without a
    projection; nothing to write: skipped; else the per-voxel walk of TsdfFusion.cu:110-167) against XS_INTEGRATE_NO_TILES, which walks
    every voxel: the same volume and count bit for bit over frames with holes, out-of-range pixels and speckle, a saturating weight,
    the caller's tile table and the call's own, whole volume and slabs — and equal to the oracle.  The free and the skip class must
    both have been taken."""
    torch, capi = dev
    prm = synth.s1_params(n, threshold=threshold)
    res = [n, n, n]
    Hh, Ww = synth.HEIGHT, synth.WIDTH
    rng = np.random.default_rng(5)
    frames = [0, 2, 2, 5, 7]
    imgs = {k: holed(synth.s1_frame(k), rng, n_holes=25, speckle=0.0005 if n < 256 else 0.0) for k in sorted(set(frames))}
    for k in imgs:
        imgs[k][200:260, 300:420][rng.random((60, 120)) < 0.01] = 0      # speckle in one patch
    k4, vs, trunc = intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm)

    def run(flags, slabs=1, own_tiles=False):
        v = torch.empty((n * n, n), dtype=torch.float32, device="cuda"); w = torch.empty((n * n, n), dtype=torch.int32, device="cuda")
        g = torch.empty((n * n, n), dtype=torch.float32, device="cuda")
        capi.init_volume(v, w, g, n * 4, res)
        scaled = torch.empty((Hh, Ww), dtype=torch.float32, device="cuda")
        dmax = torch.zeros(1, dtype=torch.float32, device="cuda")
        tiles = torch.zeros(capi.depth_tiles_bytes(Hh, Ww) // 4, dtype=torch.float32, device="cuda")
        counter = torch.zeros(1, dtype=torch.int64, device="cuda")
        counts, classes = [], np.zeros(3, np.int64)
        bounds = [n * i // slabs for i in range(slabs + 1)]
        for k in frames:
            depth = torch.from_numpy(imgs[k].astype(np.int16)).cuda()
            dmax.zero_(); counter.zero_()
            capi.scale_depth_tiles(depth, Ww * 2, Hh, Ww, scaled, Ww * 4, dmax, tiles)
            T = s1_transforms(k, prm)
            for s in range(slabs):
                z0, z1 = bounds[s], bounds[s + 1]
                ws = torch.zeros(capi.integrate_workspace_bytes(res, z1 - z0), dtype=torch.uint8, device="cuda")
                capi.integrate_scaled_ex(scaled, Ww * 4, Hh, Ww, k4, 3, res, vs, T["Rv2c"], T["tv2c"], trunc, v[z0 * n:], w[z0 * n:], g[z0 * n:], n * 4,
                                         flags | 64, threshold=threshold, z0=z0, z1=z1, updated=counter, depth_max=dmax, workspace=ws,
                                         depth_tiles=None if own_tiles else tiles)
                torch.cuda.synchronize()
                classes += class_counts(ws)
            counts.append(int(counter.item()))
        return [t.cpu().numpy().reshape(-1) for t in (v, w, g)] + [counts], classes

    exact, c0 = run(32)
    assert c0.sum() == 0
    for kw in (dict(), dict(own_tiles=True), dict(slabs=3)):
        got, cls = run(0, **kw)
        for a, b in zip(exact[:3], got[:3]):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), kw
        assert exact[3] == got[3], kw
        assert (cls[0] > 20 or n < 256) and cls[1] > 0 and cls[2] > 20, (kw, cls)
    cv, cw, cg = oracle.new_volume(res)
    cc = []
    for k in frames:
        T = s1_transforms(k, prm)
        cc.append(oracle.integrate(oracle.scale_depth(imgs[k]), cv, cw, cg, res, trunc, 3, T["Rv2c"], T["tv2c"], k4, vs, threshold))
    compare(tuple(exact), (cv, cw, cg, cc))


@pytest.mark.parametrize("threshold", [0.0, 0.02])
def test_box_classes_decided_ahead_for_a_nearby_pose(dev, threshold):
    """xs_integrate_classify with a depth-tile table named decides the boxes' classes too, padded for every pose within the slack's
    allowances (sideways centimetres, a few millimetres along the viewing axis); xs_integrate_list_covers tells the three cases apart:
    3 — list and classes hold (a last-ICP-update-sized difference, and a 3 cm sideways slide like scene S1's): the call with
    LIST_IS_READY uses both; 1 — the list holds, the classes do not (12 mm along the viewing axis): RECLASSIFY_BOXES; 0 — neither.
    Every accepted combination gives the volume and count of the plain call, bit for bit, with free-space boxes taken."""
    torch, capi = dev
    n = 256
    prm = synth.s1_params(n, threshold=threshold)
    res = [n, n, n]
    Hh, Ww = synth.HEIGHT, synth.WIDTH
    k4, vs, trunc = intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm)
    scaled = torch.empty((Hh, Ww), dtype=torch.float32, device="cuda")
    dmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    tiles = torch.zeros(capi.depth_tiles_bytes(Hh, Ww) // 4, dtype=torch.float32, device="cuda")

    def fresh():
        v = torch.empty((n * n, n), dtype=torch.float32, device="cuda"); w = torch.empty((n * n, n), dtype=torch.int32, device="cuda")
        g = torch.empty((n * n, n), dtype=torch.float32, device="cuda")
        capi.init_volume(v, w, g, n * 4, res)
        return v, w, g

    def moved(T, dt, ang=0.0):
        R = np.array(T["Rv2c"], np.float32).reshape(3, 3, 2).copy(); t = np.array(T["tv2c"], np.float32).reshape(3, 2).copy()
        c_, s_ = np.cos(ang), np.sin(ang)
        Ry = np.array([[c_, 0, s_], [0, 1, 0], [-s_, 0, c_]], np.float32)
        R[..., 0] = Ry @ R[..., 0]; t[:, 0] = Ry @ t[:, 0] + np.asarray(dt, np.float32)
        return R, t
    cases = [("update", [3e-4, -2e-4, 1e-4], 2e-5, 3), ("slide", [0.03, -0.02, 0.001], 0.0, 3), ("along the axis", [0.0, 0.0, 0.012], 0.0, 1), ("far", [0.2, 0.0, 0.0], 0.0, 0)]
    vols = {name: fresh() for name, *_ in cases if _[-1]}
    plain = fresh()
    cp = torch.zeros(1, dtype=torch.int64, device="cuda")
    free_taken = 0
    for k in (0, 4, 8):
        depth = torch.from_numpy(synth.s1_frame(k).astype(np.int16)).cuda()
        dmax.zero_()
        capi.scale_depth_tiles(depth, Ww * 2, Hh, Ww, scaled, Ww * 4, dmax, tiles)
        T = s1_transforms(k, prm)
        ws = torch.zeros(capi.integrate_workspace_bytes(res), dtype=torch.uint8, device="cuda")
        cp.zero_()
        capi.integrate_scaled_ex(scaled, Ww * 4, Hh, Ww, k4, 100, res, vs, T["Rv2c"], T["tv2c"], trunc, *plain, n * 4, 32, threshold=threshold, updated=cp,
                                 depth_max=dmax, workspace=ws)      # every voxel through the per-voxel walk
        for name, dt, ang, want in cases:
            Rl, tl = moved(T, dt, ang)       # the pose the classification sees
            covers = capi.integrate_list_covers(Hh, Ww, k4, res, vs, Rl, tl, 2.0, T["Rv2c"], T["tv2c"])
            assert covers == want, (name, covers)
            if not covers:
                continue
            c = torch.zeros(1, dtype=torch.int64, device="cuda")
            capi.integrate_classify(Hh, Ww, k4, res, vs, Rl, tl, trunc, ws, slack_scale=2.0, flags=64, depth_max=dmax, depth_tiles=tiles)
            capi.integrate_scaled_ex(scaled, Ww * 4, Hh, Ww, k4, 100, res, vs, T["Rv2c"], T["tv2c"], trunc, *vols[name], n * 4,
                                     1 | 4 | 64 | (0 if covers & 2 else 128), threshold=threshold, updated=c, depth_max=dmax, workspace=ws, depth_tiles=tiles)
            torch.cuda.synchronize()
            free_taken += class_counts(ws)[0]
            assert int(c.item()) == int(cp.item()) > 1000, name
            for x, y in zip(plain, vols[name]):
                assert torch.equal(x, y), (name, k)
    assert free_taken > 100


def test_bricks_with_planes_to_walk_are_taken_first(dev):
    """k_classify_boxes leaves the list a second time, in the order the integrate kernel takes it: two runs of a region — the bricks that
    have a plane to walk voxel by voxel from the region's front, the others from its back, their counts in header words 52 / 53 — with
    each brick's four class words filed under its place.  The same set of bricks as the frustum test lists, every front brick with planes
    to walk, no back brick with any, the walked planes adding up to what the kernel counted.  Then a list classified ahead (slack 2)
    whose classes are decided again (XS_INTEGRATE_RECLASSIFY_BOXES): the second pair starts from zero again, the same bricks of the
    frustum have planes to walk."""
    torch, capi = dev
    n = 256
    prm = synth.s1_params(n)
    res = [n, n, n]
    Hh, Ww = synth.HEIGHT, synth.WIDTH
    k4, vs, trunc = intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm)
    scaled = torch.empty((Hh, Ww), dtype=torch.float32, device="cuda")
    dmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    tiles = torch.zeros(capi.depth_tiles_bytes(Hh, Ww) // 4, dtype=torch.float32, device="cuda")
    v = torch.empty((n * n, n), dtype=torch.float32, device="cuda"); w = torch.empty((n * n, n), dtype=torch.int32, device="cuda")
    g = torch.empty((n * n, n), dtype=torch.float32, device="cuda")
    capi.init_volume(v, w, g, n * 4, res)
    list_off, cap, class_off, second_off = capi.integrate_list_layout(res)
    assert second_off + (cap * 4 + 255) // 256 * 256 == capi.integrate_workspace_bytes(res)
    ws = torch.zeros(capi.integrate_workspace_bytes(res), dtype=torch.uint8, device="cuda")

    def listed(host):    # what k_classify_bricks listed: the front run of the first region
        count, other = (int(x) for x in host[:8].view(np.int32))
        assert other == 0 and count > 100
        ids = host[list_off:list_off + 4 * count].view(np.int32)
        assert len(np.unique(ids)) == count
        return ids

    def ordered(host):   # k_classify_boxes: the two runs of the second region and the planes walked per brick of each
        nwalk, nother = (int(x) for x in host[208:216].view(np.int32))
        region = host[second_off:second_off + cap * 4].view(np.int32)
        words = host[class_off:class_off + cap * 16].view(np.uint32).reshape(cap, 4)
        walked = lambda wd: (8 - (wd & 0xff).astype(np.int64) - ((wd >> 8) & 0xff).astype(np.int64)).sum(axis=1)
        check_two_entry_bricks(region[:nwalk], words[:nwalk], region[cap - nother:])
        return region[:nwalk], region[cap - nother:][::-1], walked(words[:nwalk]), walked(words[cap - nother:])

    def check_two_entry_bricks(front, wf, back):
        """A brick one of whose boxes walks six planes or more has two neighbouring entries in the front run (a launch this small lasts as
        long as its longest wave): the first streams the free planes and walks the half of each box's walked planes next to them, the second
        (bit 19 in its words: nothing to stream) the other half — together the box's own word; every other brick has one entry."""
        per_box = lambda wd: 8 - (wd & 0xff).astype(np.int64) - ((wd >> 8) & 0xff).astype(np.int64)
        assert len(np.unique(back)) == len(back) and not set(back.tolist()) & set(front.tolist())
        i, twice = 0, 0
        while i < len(front):
            if i + 1 < len(front) and front[i] == front[i + 1]:
                a_, b_ = wf[i], wf[i + 1]
                assert not (a_ >> 19 & 1).any() and (b_ >> 19 & 1).all()
                wa, wb = per_box(a_), per_box(b_)
                assert (wa + wb).max() >= 6 and (wb == (wa + wb) // 2).all()
                assert ((a_ & 0xff) == (b_ & 0xff) - wa).all() and (((a_ >> 8) & 0xff) - wb == ((b_ >> 8) & 0xff)).all()   # the halves tile the box's walked planes
                assert ((a_ >> 16 & 1) == (b_ >> 16 & 1)).all()
                twice += 1; i += 2
            else:
                assert not (wf[i] >> 19 & 1).any() and per_box(wf[i]).max() < 6
                i += 1
        assert len(np.unique(front)) == len(front) - twice and twice > 0

    for k in (0, 5):
        depth = torch.from_numpy(synth.s1_frame(k).astype(np.int16)).cuda()
        dmax.zero_()
        capi.scale_depth_tiles(depth, Ww * 2, Hh, Ww, scaled, Ww * 4, dmax, tiles)
        T = s1_transforms(k, prm)
        capi.integrate_scaled_ex(scaled, Ww * 4, Hh, Ww, k4, 100, res, vs, T["Rv2c"], T["tv2c"], trunc, v, w, g, n * 4, 64, depth_max=dmax, workspace=ws)
        torch.cuda.synchronize()
        assert capi.integrate_listed(ws)[1] == 0
        host = ws.cpu().numpy()
        ids = listed(host)
        front, back, w_front, w_back = ordered(host)
        assert len(front) > 0 and len(back) > 0
        assert np.array_equal(np.unique(np.concatenate([front, back])), np.sort(ids))
        assert (w_front > 0).all() and (w_back == 0).all()
        assert int(w_front.sum()) == int(host[204:208].view(np.int32)[0])        # header word 51: planes walked, counted as they were classified
        # a wider list classified ahead, its classes decided again for the pose itself
        capi.integrate_classify(Hh, Ww, k4, res, vs, T["Rv2c"], T["tv2c"], trunc, ws, slack_scale=2.0, depth_max=dmax, depth_tiles=tiles)
        capi.integrate_scaled_ex(scaled, Ww * 4, Hh, Ww, k4, 100, res, vs, T["Rv2c"], T["tv2c"], trunc, v, w, g, n * 4, 1 | 4 | 128, depth_max=dmax, workspace=ws,
                                 depth_tiles=tiles)
        torch.cuda.synchronize()
        host = ws.cpu().numpy()
        wide = listed(host)
        f2, b2, w2f, w2b = ordered(host)
        assert set(ids.tolist()) <= set(wide.tolist())
        assert np.array_equal(np.unique(np.concatenate([f2, b2])), np.sort(wide))
        assert (w2f > 0).all() and (w2b == 0).all()
        # the same bricks of the frustum have planes to walk (+ bricks of the wider list the tiles cannot decide)
        assert set(front.tolist()) <= set(f2.tolist()) and not (set(f2.tolist()) - set(front.tolist())) & set(ids.tolist())


@pytest.mark.parametrize("shape", [(960, 1280), (203, 333)])
def test_brick_classification_other_image_sizes(dev, shape):
    """A 1280 x 960 sensor (four times the tiles; boxes near the camera go through the super tiles) and a ragged 333 x 203 one (partial
    tiles and super tiles at the right and bottom edges): classified against the per-voxel walk everywhere, bit for bit."""
    torch, capi = dev
    hh, ww = shape
    n = 192
    prm = synth.s1_params(n)
    res = [n, n, n]
    sx, sy = ww / synth.WIDTH, hh / synth.HEIGHT
    cam = dict(width=ww, height=hh, fx=synth.FX * sx, fy=synth.FY * sy, cx=synth.CX * sx, cy=synth.CY * sy)
    k4 = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32)
    vs, trunc = prm["tsdf_voxel_size"], tranc_dist(prm)
    rng = np.random.default_rng(2)
    scaled = torch.empty((hh, ww), dtype=torch.float32, device="cuda")
    dmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    outs = []
    total = np.zeros(3, np.int64)
    for flags in (32, 0):
        v = torch.zeros((n * n, n), dtype=torch.float32, device="cuda"); w = torch.zeros((n * n, n), dtype=torch.int32, device="cuda")
        g = torch.zeros((n * n, n), dtype=torch.float32, device="cuda")
        counts = []
        for k in (0, 3, 6):
            d = synth.s1_frame(k, **cam)
            assert d.shape == (hh, ww)
            d[hh // 3:hh // 3 + 9, ww // 4:ww // 4 + 30] = 0          # a hole
            depth = torch.from_numpy(d.astype(np.int16)).cuda()
            dmax.zero_()
            capi.scale_depth_max(depth, ww * 2, hh, ww, scaled, ww * 4, dmax)
            T = s1_transforms(k, prm)
            ws = torch.zeros(capi.integrate_workspace_bytes(res), dtype=torch.uint8, device="cuda")
            c = torch.zeros(1, dtype=torch.int64, device="cuda")
            capi.integrate_scaled_ex(scaled, ww * 4, hh, ww, k4, 100, res, vs, T["Rv2c"], T["tv2c"], trunc, v, w, g, n * 4, flags | 64, updated=c,
                                     depth_max=dmax, workspace=ws)
            torch.cuda.synchronize()
            counts.append(int(c.item()))
            if flags == 0:
                total += class_counts(ws)
        outs.append(([x.cpu().numpy().view(np.int32) for x in (v, w, g)], counts))
    for x, y in zip(outs[0][0], outs[1][0]):
        assert np.array_equal(x, y)
    assert outs[0][1] == outs[1][1] and outs[0][1][0] > 1000
    assert total[0] > 20 and total[2] > 20, total


def test_brick_classification_adversarial_grazing_surfaces(dev):
    """Surfaces that graze brick faces and tile borders: a staircase of planes whose depths sit within a few voxels of every brick
    boundary along z, a one-pixel-wide pillar and a one-pixel hole inside otherwise free tiles, and the camera rotated so that the
    boxes project onto slanted quadrilaterals.  Classified against exact, bit for bit, at several poses; all three classes taken."""
    torch, capi = dev
    n = 256
    prm = synth.s1_params(n)
    res = [n, n, n]
    Hh, Ww = synth.HEIGHT, synth.WIDTH
    k4, vs, trunc = intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm)
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    # depth staircase: 8 brick planes = 8 * vs metres per brick along z; steps land at brick faces -2 .. +2 voxels
    step = ((xx // 37) + (yy // 29)) % 11
    z_face = (np.floor((2.2 + 0.17 * step) / (8 * vs)) * 8 * vs)
    d = z_face + vs * ((xx // 37) % 5 - 2) + trunc * 1.001 * (((yy // 29) % 3) - 1)
    d = np.clip(np.round(d * 1000), 0, 65535).astype(np.uint16)
    d[100:300:7, 50:250:11] = 900      # one-pixel pillars (nearer)
    d[103:300:7, 53:250:11] = 0        # one-pixel holes
    d[:, 320] = 4900                   # a one-pixel slit (farther)
    depth = torch.from_numpy(d.astype(np.int16)).cuda()
    scaled = torch.empty((Hh, Ww), dtype=torch.float32, device="cuda")
    dmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    capi.scale_depth_max(depth, Ww * 2, Hh, Ww, scaled, Ww * 4, dmax)
    total = np.zeros(3, np.int64)
    for trial in range(6):
        ang = [0.0, 0.0, 0.3, -0.5, 0.8, 1.2][trial]
        ax = np.array([[0, 0, 1.0], [0, 0, 1.0], [0, 1.0, 0], [1.0, 0, 0], [0.6, 0.8, 0], [0.5, 0.5, 0.7071]][trial])
        ax = ax / np.linalg.norm(ax)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        cam = np.array([prm["init_x"], prm["init_y"], prm["init_z"]]) + (rng.uniform(-0.3, 0.3, 3) if trial else 0.0)
        R = np.zeros((3, 3, 2), np.float32); R[..., 0] = Rm.T; R[..., 1] = rng.normal(size=(3, 3)) * 1e-7
        t = np.zeros((3, 2), np.float32); t[:, 0] = -Rm.T @ cam; t[:, 1] = rng.normal(size=3) * 1e-7
        outs = []
        for flags in (32, 0):
            for threshold in (0.0, 0.05):
                v = torch.zeros((n * n, n), dtype=torch.float32, device="cuda"); w = torch.zeros((n * n, n), dtype=torch.int32, device="cuda")
                g = torch.zeros((n * n, n), dtype=torch.float32, device="cuda")
                ws = torch.zeros(capi.integrate_workspace_bytes(res), dtype=torch.uint8, device="cuda")
                counter = torch.zeros(1, dtype=torch.int64, device="cuda")
                for rep in range(2):
                    capi.integrate_scaled_ex(scaled, Ww * 4, Hh, Ww, k4, 100, res, vs, R, t, trunc, v, w, g, n * 4, flags | 64, threshold=threshold,
                                             updated=counter, depth_max=dmax, workspace=ws)
                torch.cuda.synchronize()
                if flags == 0:
                    total += class_counts(ws)
                outs.append(([x.cpu().numpy().view(np.int32) for x in (v, w, g)], int(counter.item())))
        for a, b in ((outs[0], outs[2]), (outs[1], outs[3])):
            for x, y in zip(a[0], b[0]):
                assert np.array_equal(x, y), trial
            assert a[1] == b[1] and a[1] > 1000, trial
    assert total[0] > 20 and total[1] > 0 and total[2] > 100, total


def _one_frame_setup(torch, capi, n, k=3, threshold=0.0):
    prm = synth.s1_params(n, threshold=threshold)
    res = [n, n, n]
    H, W = synth.HEIGHT, synth.WIDTH
    depth = torch.from_numpy(synth.s1_frame(k).astype(np.int16)).cuda()
    scaled = torch.empty((H, W), dtype=torch.float32, device="cuda")
    dmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    tiles = torch.zeros(capi.depth_tiles_bytes(H, W), dtype=torch.uint8, device="cuda")
    capi.scale_depth_tiles(depth, W * 2, H, W, scaled, W * 4, dmax, tiles)
    ws = torch.zeros(capi.integrate_workspace_bytes(res), dtype=torch.uint8, device="cuda")
    T = s1_transforms(k, prm)

    def volume():
        v = torch.empty((n * n, n), dtype=torch.float32, device="cuda"); w = torch.empty((n * n, n), dtype=torch.int32, device="cuda")
        g = torch.empty((n * n, n), dtype=torch.float32, device="cuda")
        capi.init_volume(v, w, g, n * 4, res)
        return v, w, g
    common = lambda vol, R, t: (scaled, W * 4, H, W, intr_of(prm), 100, res, prm["tsdf_voxel_size"], R, t, tranc_dist(prm), vol[0], vol[1], vol[2], n * 4)
    return prm, res, T, scaled, dmax, tiles, ws, volume, common


def test_options_struct_entry_points_read_no_thread_state(dev):
    """xs_integrate_scaled_ex2 / xs_integrate_classify_ex take the depth tiles, the sign map and the events in their options struct and read
    nothing else (ABI 2 has no per-thread setters left): they produce the per-voxel walk's volume bit for bit with the tiles handed over in the
    struct or built by the call itself, classified ahead or not, and classes decided from ANOTHER tile table are not trusted."""
    torch, capi = dev
    n = 128
    prm, res, T, scaled, dmax, tiles, ws, volume, common = _one_frame_setup(torch, capi, n)
    ref = volume()
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    capi.integrate_scaled_ex(*common(ref, T["Rv2c"], T["tv2c"]), 32, updated=cnt, depth_max=dmax, workspace=ws)   # the per-voxel walk everywhere
    torch.cuda.synchronize()
    U = int(cnt.item())
    assert U > 10000
    for own_tiles in (tiles, None):
        vol = volume()
        cnt.zero_()
        capi.integrate_scaled_ex2(*common(vol, T["Rv2c"], T["tv2c"]), capi.integrate_opts(flags=0, depth_tiles=own_tiles), updated=cnt, depth_max=dmax, workspace=ws)
        torch.cuda.synchronize()
        assert int(cnt.item()) == U
        for a, b in zip(ref, vol):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # ... and classified ahead through the struct
    vol = volume()
    cnt.zero_()
    capi.integrate_classify_ex(synth.HEIGHT, synth.WIDTH, intr_of(prm), res, prm["tsdf_voxel_size"], T["Rv2c"], T["tv2c"], tranc_dist(prm), ws,
                               capi.integrate_opts(flags=0, depth_tiles=tiles), slack_scale=2.0, depth_max=dmax)
    capi.integrate_scaled_ex2(*common(vol, T["Rv2c"], T["tv2c"]), capi.integrate_opts(flags=4 | 1, depth_tiles=tiles), updated=cnt, depth_max=dmax, workspace=ws)
    torch.cuda.synchronize()
    assert int(cnt.item()) == U
    for a, b in zip(ref, vol):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the classes a classification left in a workspace are this call's only if they were decided for ITS tile table (and slab, camera,
    # band): classes decided from another frame's table — here a poisoned one, all zeros: every box "sees nothing valid" and would be skipped —
    # followed by LIST_IS_READY with the real table must be decided again, not trusted (round 5 kept workspace, pose and slack only)
    poison = torch.zeros_like(tiles)
    vol = volume()
    cnt.zero_()
    capi.integrate_classify_ex(synth.HEIGHT, synth.WIDTH, intr_of(prm), res, prm["tsdf_voxel_size"], T["Rv2c"], T["tv2c"], tranc_dist(prm), ws,
                               capi.integrate_opts(flags=0, depth_tiles=poison), slack_scale=2.0, depth_max=dmax)
    capi.integrate_scaled_ex2(*common(vol, T["Rv2c"], T["tv2c"]), capi.integrate_opts(flags=4 | 1, depth_tiles=tiles), updated=cnt, depth_max=dmax, workspace=ws)
    torch.cuda.synchronize()
    assert int(cnt.item()) == U
    for a, b in zip(ref, vol):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the entry point without a struct is the same call with an empty one (ABI 2: no per-thread state is left for it to read)
    vol = volume()
    cnt.zero_()
    capi.integrate_scaled(*common(vol, T["Rv2c"], T["tv2c"]), updated=cnt, depth_max=dmax, workspace=ws)
    torch.cuda.synchronize()
    assert int(cnt.item()) == U
    with pytest.raises(capi.XsError):
        bad = capi.integrate_opts()
        bad.struct_bytes = 8
        capi.integrate_scaled_ex2(*common(ref, T["Rv2c"], T["tv2c"]), bad, depth_max=dmax, workspace=ws)


def test_classes_decided_ahead_are_checked_against_the_launch_pose(dev):
    """box classes left by xs_integrate_classify were trusted whenever the caller set LIST_IS_READY.  The library now
    remembers the pose and slack they were padded for and decides the boxes again when the launch's pose lies outside: a caller that
    passes LIST_IS_READY for a pose the LIST covers but the CLASSES do not (xs_integrate_list_covers == 1), without the
    RECLASSIFY_BOXES hint, still gets the plain call's volume bit for bit."""
    torch, capi = dev
    n = 128
    prm, res, T, scaled, dmax, tiles, ws, volume, common = _one_frame_setup(torch, capi, n)
    H, W = synth.HEIGHT, synth.WIDTH
    R, t = T["Rv2c"], T["tv2c"]
    found = None
    for dz in (0.004, 0.006, 0.008, 0.012, 0.016, 0.02, 0.03):     # along the viewing axis: the classes' pad there is a third of a sideways one
        t2 = np.array(t, np.float32).copy(); t2[2, 0] += dz
        if capi.integrate_list_covers(H, W, intr_of(prm), res, prm["tsdf_voxel_size"], R, t, 2.0, R, t2) == 1:
            found = t2
            break
    assert found is not None, "no pose with a covered list and uncovered classes among the candidates"
    ref = volume()
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    capi.integrate_scaled_ex(*common(ref, R, found), 32, updated=cnt, depth_max=dmax, workspace=ws)
    torch.cuda.synchronize()
    U = int(cnt.item())
    for hint in (0, 128):     # without and with XS_INTEGRATE_RECLASSIFY_BOXES
        vol = volume()
        cnt.zero_()
        capi.integrate_classify_ex(H, W, intr_of(prm), res, prm["tsdf_voxel_size"], R, t, tranc_dist(prm), ws, capi.integrate_opts(depth_tiles=tiles),
                                   slack_scale=2.0, depth_max=dmax)
        capi.integrate_scaled_ex2(*common(vol, R, found), capi.integrate_opts(flags=4 | 1 | hint, depth_tiles=tiles), updated=cnt, depth_max=dmax, workspace=ws)
        torch.cuda.synchronize()
        assert int(cnt.item()) == U, hint
        for a, b in zip(ref, vol):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), hint


@pytest.mark.parametrize("threshold", [0.0, 0.02])
def test_boxes_on_the_frustums_side_stream_with_the_in_image_test_alone(dev, threshold):
    """The EDGE class (round 5): a box whose pixel range leaves the image streams its free planes with the reference's in-image test
    (TsdfFusion.cu:123-124) as the only per-voxel decision — a margin test on un-divided coordinates, the exact test within 1/32 px of the
    border.  Twelve views rolled, pitched and yawed by up to 0.6 rad from inside and outside a 160^3 volume (the image border cuts boxes at
    every angle, near the camera and far from it, all four borders), a flat wall far behind everything so that the frustum's sides run
    through free space: volume and count against the per-voxel walk everywhere, bit for bit, classes decided with the launch's own pose
    and decided ahead with the pose slack's pads — and the class counters show the path taken (thousands of planes) in every view."""
    torch, capi = dev
    n = 160
    prm = synth.s1_params(n, threshold=threshold)
    res = [n, n, n]
    H, W = synth.HEIGHT, synth.WIDTH
    rng = np.random.default_rng(0xED6E)
    d = np.full((H, W), 4200, np.uint16)
    d[200:280, 260:380] = 1500          # a nearer patch: a surface band inside the view too
    depth = torch.from_numpy(d.astype(np.int16)).cuda()
    scaled = torch.empty((H, W), dtype=torch.float32, device="cuda")
    dmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    tiles = torch.zeros(capi.depth_tiles_bytes(H, W), dtype=torch.uint8, device="cuda")
    capi.scale_depth_tiles(depth, W * 2, H, W, scaled, W * 4, dmax, tiles)
    ws = torch.zeros(capi.integrate_workspace_bytes(res), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    vs, trunc = prm["tsdf_voxel_size"], tranc_dist(prm)

    def volume():
        v = torch.empty((n * n, n), dtype=torch.float32, device="cuda"); w = torch.empty((n * n, n), dtype=torch.int32, device="cuda")
        g = torch.empty((n * n, n), dtype=torch.float32, device="cuda")
        capi.init_volume(v, w, g, n * 4, res)
        return v, w, g
    seen_edge = 0
    for trial in range(12):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        ang = rng.uniform(0.05, 0.6)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        tv = np.array([3.84, 3.84, 1.0]) + rng.uniform(-1.5, 1.5, 3) * (1.0, 1.0, 0.8)    # camera in the volume frame (7.68 m cube), looking roughly +z
        v2c = np.eye(4); v2c[:3, :3] = Rm.T; v2c[:3, 3] = -Rm.T @ tv
        R = np.zeros((3, 3, 2), np.float32); R[..., 0] = v2c[:3, :3]; R[..., 1] = rng.normal(size=(3, 3)) * 1e-7
        t = np.zeros((3, 2), np.float32); t[:, 0] = v2c[:3, 3]; t[:, 1] = rng.normal(size=3) * 1e-7
        common = lambda vol: (scaled, W * 4, H, W, intr_of(prm), 100, res, vs, R, t, trunc, vol[0], vol[1], vol[2], n * 4)
        ref = volume()
        for rep in range(2):    # two frames: the second updates written voxels (running mean of state that is not zero)
            cnt.zero_()
            capi.integrate_scaled_ex2(*common(ref), capi.integrate_opts(flags=32), threshold=threshold, updated=cnt, depth_max=dmax, workspace=ws)
        torch.cuda.synchronize()
        U = int(cnt.item())
        assert U > 50000, (trial, U)
        for ahead in (False, True):
            vol = volume()
            for rep in range(2):
                cnt.zero_()
                flags = 64
                if ahead:
                    capi.integrate_classify_ex(H, W, intr_of(prm), res, vs, R, t, trunc, ws, capi.integrate_opts(flags=64, depth_tiles=tiles), slack_scale=2.0, depth_max=dmax)
                    flags |= 4 | 1
                capi.integrate_scaled_ex2(*common(vol), capi.integrate_opts(flags=flags, depth_tiles=tiles), threshold=threshold, updated=cnt, depth_max=dmax, workspace=ws)
            torch.cuda.synchronize()
            head = ws[192:220].view(torch.int32).cpu().numpy()
            assert int(cnt.item()) == U, (trial, ahead, int(cnt.item()), U)
            for a, b in zip(ref, vol):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (trial, ahead)
            seen_edge += int(head[6])
            assert int(head[6]) > 500, (trial, ahead, head[:7])     # planes streamed with the in-image test
    assert seen_edge > 50000


@pytest.mark.parametrize("threshold", [0.0, 0.02])
def test_boxes_that_see_invalid_pixels_stream_with_a_validity_test(dev, threshold):
    """The SPECKLE class (round 5): a box whose pixel range holds an invalid pixel (a hole, an out-of-range patch, a speckle) among valid ones
    that all lie far behind it streams its free planes, each voxel gated by the validity of its OWN nearest pixel (found from a
    reciprocal-based projection; the exact projection within 1 / 2048 px of a pixel boundary) and — on the frustum's side — by the in-image
    test.  A noisy wall with 40 holes / out-of-range patches and 0.5 % speckle seen from six rolled / pitched / yawed poses, two frames
    each, nearest-pixel and bilinear depth: volume and count against the per-voxel walk everywhere, bit for bit; the class counters show
    the path taken, and that few boxes are left to walk where round 4 walked nearly all of them."""
    torch, capi = dev
    n = 160
    prm = synth.s1_params(n, threshold=threshold)
    res = [n, n, n]
    H, W = synth.HEIGHT, synth.WIDTH
    rng = np.random.default_rng(0x5BEC)
    base = np.full((H, W), 4200.0) + 2.0 * (rng.random((H, W)) * 2 - 1)
    d = synth.holed(np.clip(np.rint(base), 0, 65535).astype(np.uint16), rng, n_holes=40, speckle=0.005)
    depth = torch.from_numpy(d.astype(np.int16)).cuda()
    scaled = torch.empty((H, W), dtype=torch.float32, device="cuda")
    dmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    tiles = torch.zeros(capi.depth_tiles_bytes(H, W), dtype=torch.uint8, device="cuda")
    capi.scale_depth_tiles(depth, W * 2, H, W, scaled, W * 4, dmax, tiles)
    ws = torch.zeros(capi.integrate_workspace_bytes(res), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    vs, trunc = prm["tsdf_voxel_size"], tranc_dist(prm)

    def volume():
        v = torch.empty((n * n, n), dtype=torch.float32, device="cuda"); w = torch.empty((n * n, n), dtype=torch.int32, device="cuda")
        g = torch.empty((n * n, n), dtype=torch.float32, device="cuda")
        capi.init_volume(v, w, g, n * 4, res)
        return v, w, g
    for trial in range(6):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        ang = rng.uniform(0.02, 0.5)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        tv = np.array([3.84, 3.84, 1.2]) + rng.uniform(-1.0, 1.0, 3) * (1.0, 1.0, 0.8)
        v2c = np.eye(4); v2c[:3, :3] = Rm.T; v2c[:3, 3] = -Rm.T @ tv
        R = np.zeros((3, 3, 2), np.float32); R[..., 0] = v2c[:3, :3]; R[..., 1] = rng.normal(size=(3, 3)) * 1e-7
        t = np.zeros((3, 2), np.float32); t[:, 0] = v2c[:3, 3]; t[:, 1] = rng.normal(size=3) * 1e-7
        common = lambda vol: (scaled, W * 4, H, W, intr_of(prm), 100, res, vs, R, t, trunc, vol[0], vol[1], vol[2], n * 4)
        ref = volume()
        for rep in range(2):
            cnt.zero_()
            capi.integrate_scaled_ex2(*common(ref), capi.integrate_opts(flags=32), threshold=threshold, updated=cnt, depth_max=dmax, workspace=ws)
        torch.cuda.synchronize()
        U = int(cnt.item())
        assert U > 50000, (trial, U)
        for ahead in (False, True):
            vol = volume()
            for rep in range(2):
                cnt.zero_()
                flags = 64
                if ahead:
                    capi.integrate_classify_ex(H, W, intr_of(prm), res, vs, R, t, trunc, ws, capi.integrate_opts(flags=64, depth_tiles=tiles), slack_scale=2.0, depth_max=dmax)
                    flags |= 4 | 1
                capi.integrate_scaled_ex2(*common(vol), capi.integrate_opts(flags=flags, depth_tiles=tiles), threshold=threshold, updated=cnt, depth_max=dmax, workspace=ws)
            torch.cuda.synchronize()
            head = ws[192:224].view(torch.int32).cpu().numpy()
            assert int(cnt.item()) == U, (trial, ahead, int(cnt.item()), U)
            for a, b in zip(ref, vol):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (trial, ahead)
            boxes = int(head[0]) + int(head[1]) + int(head[2])
            assert int(head[7]) > 2000 and int(head[2]) < 0.6 * boxes, (trial, ahead, head[:8])   # (coarse 4.8 cm voxels: the wall's band is a large share of the boxes)
