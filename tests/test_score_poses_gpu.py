"""GPU: the alignment loss of one depth frame at many poses in one pass over the band index (xs_tsdf_score_poses_band, k_band_score_poses)
and the global relocalisation built on it (KinectFusion.score_poses, relocalize_global); DESIGN.md 4.17.  The kernel-level map is
newton_cases.s3_map_and_truth(oracle, 64) uploaded dense: 2 208 band voxels, 34 full chunks and one of 32.  Every sum is asserted within
score_cases.SUM_BOUND = 8 * 2^-24 of its dense counterpart (the six-level pairwise float tree per chunk, everything else in double) and
every count exactly.  Every figure a test asserts on is printed before the assertion."""
import importlib
import threading

import numpy as np
import pytest

import independent_cases as ic
import independent_f64 as ind
import newton_cases as nc
import score_cases as sc
from helpers import intr_of, synth, tranc_dist

W, H = synth.WIDTH, synth.HEIGHT
pytestmark = pytest.mark.gpu
N = 64


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi"), importlib.import_module("x-slam_amd.pipeline")


@pytest.fixture(scope="module")
def be(dev):
    torch, capi, pl = dev
    return ic.GpuBackend(torch, capi, None)


@pytest.fixture(scope="module")
def case(be, oracle):
    """The shared inputs, computed once and left unchanged: the oracle's S3 map at 64^3, the last frame's scaled depth, the 200 poses."""
    prm, gt, ds, truth = nc.s3_map_and_truth(oracle, N)
    poses = sc.kernel_poses(truth)
    Rt = [sc.v2c_f32(m) for m in poses]
    return dict(prm=prm, gt=np.asarray(gt, np.float32), ds=np.asarray(ds, np.float32), truth=truth, poses=poses,
                R=np.stack([r for r, _ in Rt]), t=np.stack([t for _, t in Rt]))


def score_band(be, depth_dev, prm, R, t, idx, ws=None):
    """One launch of xs_tsdf_score_poses_band for the poses R [P, 3, 3], t [P, 3] over a built index: [P, 2] {sum loss, count}."""
    tc, c = be.t, be.c
    P = len(R)
    ws = tc.zeros(c.tsdf_score_poses_workspace_bytes(P), dtype=tc.uint8, device="cuda") if ws is None else ws
    out = tc.full((2 * P,), -1.0, dtype=tc.float64, device="cuda")
    c.tsdf_score_poses_band(depth_dev, W * 4, H, W, intr_of(prm), prm["tsdf_voxel_size"], R, t, tranc_dist(prm), idx, ws, out)
    tc.cuda.synchronize()
    assert int(ws[:256].view(tc.int32).abs().sum().item()) == 0          # every tile's ticket is back at zero
    return out.cpu().numpy().reshape(P, 2)


def dense_losses(be, depth_dev, prm, res, R, t, gt_dev):
    """P launches of the unchanged xs_compute_local_tsdf_loss on the dense map, one per pose: [P, 2]."""
    tc, c = be.t, be.c
    P = len(R)
    ws = tc.zeros(c.tsdf_reduce_workspace_bytes(), dtype=tc.uint8, device="cuda")
    out = tc.full((P, 2), -1.0, dtype=tc.float64, device="cuda")
    for p in range(P):
        c.compute_local_tsdf_loss(depth_dev, W * 4, H, W, intr_of(prm), res, prm["tsdf_voxel_size"], R[p], t[p], tranc_dist(prm), gt_dev, ws, out[p])
    tc.cuda.synchronize()
    return out.cpu().numpy()


def assert_sums_within_bound(got, want, what):
    diff, bound = np.abs(got - want), sc.SUM_BOUND * want
    worst = float((diff / np.where(bound > 0, bound, 1.0)).max())
    print(f"  {what}: |band - dense| / (8 * 2^-24 * dense), worst {worst:.3g}; largest |diff| {float(diff.max()):.3g}")
    assert np.all(diff <= bound), (what, worst)


@pytest.mark.parametrize("res", [(N, N, N), (50, 62, 64), (50, 46, 40)])
def test_one_launch_equals_the_dense_launches(be, case, res):
    """200 poses in one launch against 200 launches of xs_compute_local_tsdf_loss on the dense map the index was built from: every count
    equal, every sum within 8 * 2^-24 of the dense sum.  The poses: the truth, 150 perturbations with full and partial views, the camera
    turned round and one 20 m off (count 0), random ones.  Again with an all-zero depth image: all counts 0 and all sums 0.0.  (50, 62, 64):
    X % 4 != 0, the index is built by the narrow walk and holds the same 2 208 voxels; (50, 46, 40) cuts the band down to 99 voxels, a
    single workgroup with one full chunk and one of 35."""
    tc, c = be.t, be.c
    res = list(res)
    prm = case["prm"]
    gt_dev = be.dev(ic.crop(case["gt"], N, res))
    idx = c.tsdf_band_build(gt_dev, res)
    nvox = int(idx.count)
    print(f"res {res}: {nvox} band voxels = {nvox // 64} chunks + {nvox % 64}")
    assert nvox == (99 if res[2] == 40 else 2208) and nvox % 64 != 0      # (2 208: nine workgroups; both: a partial last chunk)
    depth = be.dev(case["ds"])
    got = score_band(be, depth, prm, case["R"], case["t"], idx)
    want = dense_losses(be, depth, prm, res, case["R"], case["t"], gt_dev)
    counts = want[:, 1]
    print("  dense counts, sorted, every 20th:", np.sort(counts)[::20], " turned / far:", counts[sc.TURNED], counts[sc.FAR])
    assert counts[0] >= 0.8 * counts.max() > 0 and counts[sc.TURNED] == 0 and counts[sc.FAR] == 0
    assert np.sum((counts > 0) & (counts < 0.8 * counts[0])) >= 10          # partial views occur
    assert np.array_equal(got[:, 1], counts), np.flatnonzero(got[:, 1] != counts)
    assert_sums_within_bound(got[:, 0], want[:, 0], "depth frame")
    assert np.all(got[counts == 0, 0] == 0.0)
    empty = tc.zeros((H, W), dtype=tc.float32, device="cuda")
    got0 = score_band(be, empty, prm, case["R"], case["t"], idx)
    want0 = dense_losses(be, empty, prm, res, case["R"], case["t"], gt_dev)
    assert np.all(want0 == 0.0) and np.all(got0 == 0.0)


def test_tile_edges_and_independence(be, case):
    """P = 1, 63, 64, 65, 129 (a partial tile, a full one, one pose into the second, two full and one): every pose's 16 bytes are the same
    in every launch that holds it, the same as a P = 1 launch of that pose alone (whatever lane kept its sums), and the same again on a
    second launch; the workspace sizes and the bound on P."""
    tc, c = be.t, be.c
    prm = case["prm"]
    idx = c.tsdf_band_build(be.dev(case["gt"]), [N, N, N])
    depth = be.dev(case["ds"])
    ws = tc.zeros(c.tsdf_score_poses_workspace_bytes(129), dtype=tc.uint8, device="cuda")
    run = lambda sel: score_band(be, depth, prm, case["R"][sel], case["t"][sel], idx, ws=ws)
    full = run(np.arange(129))
    assert full[0, 1] > 1000 and len({full[p].tobytes() for p in range(129)}) > 100
    for P in (1, 63, 64, 65, 129):
        got = run(np.arange(P))
        assert got.tobytes() == full[:P].tobytes(), P
    assert run(np.arange(129)).tobytes() == full.tobytes()                    # again: the same bits
    for p in (0, 1, 62, 63, 64, 65, 100, 128):
        assert run(np.array([p])).tobytes() == full[p].tobytes(), p
    mixed = np.array([128, 5, 5, 64, 0, 63] + list(range(70, 140)))          # other slots, other neighbours, another P
    ref = score_band(be, depth, prm, case["R"][np.arange(140)], case["t"][np.arange(140)], idx)
    got = run(mixed[:70])
    for slot, p in enumerate(mixed[:70]):
        assert got[slot].tobytes() == ref[p].tobytes(), (slot, p)
    assert c.tsdf_score_poses_workspace_bytes(0) == 0 and c.tsdf_score_poses_workspace_bytes(c.SCORE_MAX_POSES + 1) == 0
    assert c.tsdf_score_poses_workspace_bytes(65) > c.tsdf_score_poses_workspace_bytes(64) == c.tsdf_score_poses_workspace_bytes(1) > 256
    with pytest.raises(c.XsError):
        c.tsdf_score_poses_band(depth, W * 4, H, W, intr_of(prm), prm["tsdf_voxel_size"], case["R"][:1], case["t"][:1], tranc_dist(prm), idx, None,
                                tc.zeros(2, dtype=tc.float64, device="cuda"))


def test_slabs_add_up(be, case):
    """Indices of the planes [0, 32) and [32, 64): per pose the two counts add up to the whole index's exactly, the two sums within
    8 * 2^-24 of it.  This map's band lies in planes 36 .. 49, so the lower index is EMPTY (count 0 yields zeros); [0, 42) and [42, 64)
    cut through it."""
    tc, c = be.t, be.c
    prm = case["prm"]
    gt_dev = be.dev(case["gt"])
    depth = be.dev(case["ds"])
    whole = score_band(be, depth, prm, case["R"], case["t"], c.tsdf_band_build(gt_dev, [N, N, N]))
    assert whole[0, 1] > 1000
    for cut in (32, 42):
        lo_idx = c.tsdf_band_build(gt_dev, [N, N, N], 0, cut)
        hi_idx = c.tsdf_band_build(gt_dev[cut * N * N:], [N, N, N], cut, N)
        print(f"cut at {cut}: band voxels {int(lo_idx.count)} + {int(hi_idx.count)}")
        assert lo_idx.count + hi_idx.count == 2208 and (lo_idx.count > 0) == (cut == 42) and hi_idx.count > 0
        lo = score_band(be, depth, prm, case["R"], case["t"], lo_idx)
        hi = score_band(be, depth, prm, case["R"], case["t"], hi_idx)
        if cut == 32:
            assert np.all(lo == 0.0)
        else:
            assert lo[0, 1] > 0 and hi[0, 1] > 0
        assert np.array_equal(lo[:, 1] + hi[:, 1], whole[:, 1])
        assert_sums_within_bound(lo[:, 0] + hi[:, 0], whole[:, 0], f"two slabs cut at {cut}")


def test_against_the_float64_model(be, case):
    """Sum loss and count of eight poses (the truth and seven perturbations) against independent_f64.tsdf_residual_loss with the margins of
    test_independent_gpu.test_hessian_loss_gradient_and_second_derivative: count within max(2, 1e-4 count), loss within 5e-4."""
    prm = case["prm"]
    idx = be.c.tsdf_band_build(be.dev(case["gt"]), [N, N, N])
    got = score_band(be, be.dev(case["ds"]), prm, case["R"][:8], case["t"][:8], idx)
    g3 = case["gt"].reshape(N, N, N)
    for p in range(8):
        R4 = np.zeros((3, 3, 4), np.float32); R4[..., 0] = case["R"][p]
        t4 = np.zeros((3, 4), np.float32); t4[:, 0] = case["t"][p]
        loss, count, _ = ind.tsdf_residual_loss(0.0, ic.H2, R4, t4, g3, case["ds"], intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm), 0)
        print(f"  pose {p}: count {got[p, 1]} model {count}, loss {got[p, 0]} model {loss}")
        assert abs(got[p, 1] - count) <= max(2, 1e-4 * count)
        assert abs(got[p, 0] - loss) <= 5e-4 * abs(loss)
    assert got[0, 1] > 1000


# ---- orchestrator level ----------------------------------------------------------------------------------------------------------------
def s3_map(torch, pl, n=128, nframes=6, prm=None):
    """test_reloc_batch_gpu.s3_map's setup: scene S3 fused by the pipeline."""
    kf = pl.KinectFusion(prm or synth.s1_params(n))
    dfr = [torch.from_numpy(synth.s3_frame(k).view(np.int16)).cuda() for k in range(nframes + 1)]
    for k in range(nframes):
        assert kf.process_frame(dfr[k]) == 1
    return kf, dfr


def test_score_poses_equals_the_kernel_level_call(dev, be):
    """KinectFusion.score_poses on 70 candidates is bit-equal to xs_tsdf_score_poses_band over an index of volume()'s values with the v2c real
    parts of host_newton_seeded_poses; 4096 + 5 candidates through the chunking give the first 70 the same bits (and the last five theirs);
    after one more process_frame the scores differ: the index follows the volume."""
    torch, capi, pl = dev
    n = 128
    kf, dfr = s3_map(torch, pl, n)
    prm = synth.s1_params(n)
    cands = pl.pose_candidates(kf.camera2volume(), 0.3, 0.3, 70)
    s, cnt = kf.score_poses(dfr[5], cands)
    assert s.shape == (70,) and cnt.shape == (70,) and s.dtype == np.float64 and cnt.max() > 1000
    Rt = [pl.host_newton_seeded_poses(m) for m in cands]
    R = np.stack([r[0, ..., 0] for r, _ in Rt]); t = np.stack([tt[0, :, 0] for _, tt in Rt])
    idx = capi.tsdf_band_build(be.dev(kf.volume()[0]), [n, n, n])
    assert int(idx.count) == kf.relocalization_index_voxels()
    depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    capi.scale_depth(dfr[5], W * 2, H, W, depth, W * 4)
    want = score_band(be, depth, prm, R, t, idx)
    assert s.tobytes() == want[:, 0].tobytes() and cnt.tobytes() == want[:, 1].tobytes()
    many = np.concatenate([cands] * 59)[:4096 + 5]
    s2, c2 = kf.score_poses(dfr[5], many)
    assert s2.shape == (4101,) and s2[:70].tobytes() == s.tobytes() and c2[:70].tobytes() == cnt.tobytes()
    assert s2[4096:].tobytes() == s[4096 % 70:4096 % 70 + 5].tobytes() and c2[4096:].tobytes() == cnt[4096 % 70:4096 % 70 + 5].tobytes()
    assert kf.process_frame(dfr[6]) == 1
    s3, c3 = kf.score_poses(dfr[5], cands)
    print("changed after one more frame:", int((c3 != cnt).sum()), "counts,", int((s3 != s).sum()), "sums of 70")
    assert (c3 != cnt).any() or (s3 != s).any()
    kf.close()


def test_global_relocalisation(dev):
    """Scene S3 at 128^3, six frames fused; truth = the last frame's camera2volume, start 0.883 m and 50.6 degrees off it.  Gauss-Newton from
    the start fails or ends more than 10 cm off; relocalize_global over 2048 Halton candidates around the start (keep 8, 10 iterations) ends
    within 1 cm and 0.5 degrees of the truth, with S >= 0.98 x the truth's own S and above the winning candidate's S before refinement.  The
    margins are wide over the CPU twin's figures (tests/test_score_poses_cpu.py; at 128^3: best candidate 4 973 of 9 640, winner within
    1.9 mm / 0.03 degrees, S after 9 629.5)."""
    torch, capi, pl = dev
    kf, dfr = s3_map(torch, pl, 128)
    truth = kf.camera2volume()[..., 0].astype(np.float64)
    start = sc.global_start(truth)
    ok0, end0, _ = kf.relocalize(dfr[5], sc.as_c2v32(start), iterations=sc.GLOBAL_ITERATIONS)
    far0 = sc.pose_error(end0[..., 0], truth)
    print("Gauss-Newton from the start: ok", ok0, "ends", far0)
    assert not ok0 or far0[0] > 0.10
    s_t, c_t = kf.score_poses(dfr[5], sc.as_c2v32(np.stack([truth, start])))
    S_truth, S_start = sc.S(s_t, c_t)
    cands = pl.pose_candidates(start, sc.GLOBAL_BOX_T, sc.GLOBAL_BOX_R, sc.GLOBAL_CANDIDATES)
    ok, best, rep = kf.relocalize_global(dfr[5], cands, keep=sc.GLOBAL_KEEP, iterations=sc.GLOBAL_ITERATIONS, damping=sc.GLOBAL_DAMPING)
    err = sc.pose_error(best[..., 0], truth)
    print("S at truth", S_truth, "at start", S_start, "report", rep, "error", err)
    assert ok
    assert err[0] <= 0.01 and err[1] <= 0.5
    assert rep["S_after"] >= 0.98 * S_truth
    assert rep["S_after"] > rep["S_before"]
    # the report is what score_poses says of the winner and of its candidate
    s_w, c_w = kf.score_poses(dfr[5], np.stack([best, cands[rep["index"]]]))
    assert rep["sum_loss_after"] == s_w[0] and rep["count_after"] == c_w[0] and rep["S_after"] == c_w[0] - s_w[0] and rep["S_before"] == c_w[1] - s_w[1]
    assert 1 <= rep["refined_ok"] <= sc.GLOBAL_KEEP and rep["index_voxels"] == kf.relocalization_index_voxels() and np.all(best[..., 1] == 0)
    # nothing in view of any candidate: not ok
    lost = cands[:16].copy(); lost[:, :3, 3, 0] += 50.0
    ok_l, best_l, rep_l = kf.relocalize_global(dfr[5], lost, keep=4, iterations=3)
    assert not ok_l and rep_l["index"] == -1 and best_l.tobytes() == lost[0].tobytes()
    kf.close()


def test_sharded_scores_equal_the_single_instance(dev):
    """Two ranks as threads on one GPU: each rank's launch over the index of its owned planes, the 2 x 70 doubles all-reduced, against the
    single instance's score_poses: counts equal, sums within 8 * 2^-24; every rank gets the same bits."""
    torch, capi, pl = dev
    sh = importlib.import_module("x-slam_amd.sharded")
    world, n = 2, 128
    prm = dict(synth.s1_params(n), icp_shard_rows=False)
    single, dfr = s3_map(torch, pl, n, prm=prm)
    cands = pl.pose_candidates(single.camera2volume(), 0.3, 0.3, 70)
    want_s, want_c = single.score_poses(dfr[5], cands)
    lw = sh.LocalWorld(torch, world)
    shards = [sh.ShardedKinectFusion(prm, r, world, collective=lw.collective_for(r)) for r in range(world)]
    gots, errors = [None] * world, []

    def work(r):
        try:
            for d in dfr[:6]:
                assert shards[r].process_frame(d) == 1
            gots[r] = shards[r].score_poses(dfr[5], cands)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            lw.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    assert np.array_equal(shards[0].world2camera(), single.world2camera())      # replicated ICP: the same map in both
    assert want_c.max() > 1000
    for r in range(world):
        assert np.array_equal(gots[r][1], want_c)
        assert_sums_within_bound(gots[r][0], want_s, f"rank {r}")
        assert gots[r][0].tobytes() == gots[0][0].tobytes()
    for s in shards:
        s.close()
    single.close()
