"""GPU: batched relocalisation over the band index (KinectFusion.relocalize_batch, xs_kf_relocalize_batch): every frame's ok flag,
final pose and loss history equal relocalize for that frame alone, bit for bit; the index follows every write of the volume; the
batch, single-frame and terms workspaces do not interfere; shard mode all-reduces the batch's sums."""
import importlib
import threading

import numpy as np
import pytest

from helpers import synth
from test_gauss_newton_gpu import twist_matrix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.pipeline"), importlib.import_module("x-slam_amd.sharded")


def s3_map(torch, pl, n, nframes=6):
    """The setup of test_relocalization_loop_against_an_oracle_twin: scene S3 fused by the pipeline."""
    kf = pl.KinectFusion(synth.s1_params(n))
    dfr = [torch.from_numpy(synth.s3_frame(k).view(np.int16)).cuda() for k in range(8)]
    for k in range(nframes):
        assert kf.process_frame(dfr[k]) == 1
    return kf, dfr


def queries(torch, kf, dfr, count=8, seed=0):
    """count (depth, start) pairs: frames 4 and 5 from perturbed poses, one empty depth image, one pose 20 m off the map."""
    rng = np.random.default_rng(seed)
    c2v = kf.camera2volume()[..., 0].astype(np.float64)
    empty = torch.zeros_like(dfr[0])
    out = []
    for i in range(count):
        xi = rng.normal(size=6) * [0.006, 0.006, 0.006, 0.004, 0.004, 0.004]
        start = twist_matrix(xi) @ c2v
        d = dfr[5 if i % 2 == 0 else 4]
        if i == 2:
            d = empty
        if i == 6:
            start = start.copy(); start[:3, 3] += [20.0, 0.0, 0.0]
        m = np.zeros((4, 4, 2), np.float32); m[..., 0] = start
        out.append((d, m))
    return out


def singles(kf, qs, iterations, damping=1e-3):
    return [kf.relocalize(d, m, iterations=iterations, damping=damping) for d, m in qs]


def assert_same(batch, single, iterations):
    ok, c2v, hist = batch
    assert hist.shape == (len(single), iterations + 1)
    for f, (ok1, c1, h1) in enumerate(single):
        assert ok[f] == ok1, f
        assert c2v[f].tobytes() == c1.tobytes(), f
        assert hist[f].tobytes() == h1.tobytes(), (f, hist[f], h1)


@pytest.mark.parametrize("n", [128, 256])
def test_batch_equals_single_frame_loop(dev, n):
    torch, pl, _ = dev
    kf, dfr = s3_map(torch, pl, n)
    qs = queries(torch, kf, dfr)
    for iterations in (0, 1, 5):
        single = singles(kf, qs, iterations)
        batch = kf.relocalize_batch([d for d, _ in qs], np.stack([m for _, m in qs]), iterations=iterations)
        assert_same(batch, single, iterations)
        if iterations == 5:
            assert not batch[0][2] and not batch[0][6] and batch[0].sum() == 6
            assert all(batch[2][f, -1] < batch[2][f, 0] for f in range(8) if batch[0][f])
    assert kf.relocalization_index_voxels() > 5000
    kf.close()


def test_batch_above_the_launch_bound(dev):
    """More frames than one launch takes (XS_BAND_MAX_FRAMES = 32): chunked, same results."""
    torch, pl, _ = dev
    kf, dfr = s3_map(torch, pl, 128)
    qs = queries(torch, kf, dfr, count=37, seed=4)
    single = singles(kf, qs, 2)
    assert_same(kf.relocalize_batch([d for d, _ in qs], np.stack([m for _, m in qs]), iterations=2), single, 2)
    kf.close()


def test_index_follows_the_volume(dev, tmp_path):
    """The index is rebuilt after an integrate, after load_checkpoint of an earlier checkpoint and after a write through volume_ptr +
    rebuild_sign_map: relocalize_batch equals relocalize on the map as it is then, and the index size changes."""
    torch, pl, sh = dev
    kf, dfr = s3_map(torch, pl, 128, nframes=5)
    ck = str(tmp_path / "five.ckpt")
    kf.save_checkpoint(ck)

    def check():
        qs = queries(torch, kf, dfr, count=4, seed=9)
        single = singles(kf, qs, 3)
        assert_same(kf.relocalize_batch([d for d, _ in qs], np.stack([m for _, m in qs]), iterations=3), single, 3)
        return kf.relocalization_index_voxels()

    n5 = check()
    assert kf.process_frame(dfr[5]) == 1
    n6 = check()
    assert n6 != n5
    assert kf.load_checkpoint(ck)
    assert check() == n5
    p, step = kf.volume_ptr("value")
    n = 128
    vol = torch.as_tensor(sh._DevView(p, step // 4 * n * n, "<f4"), device="cuda").view(n * n, step // 4)
    vol[40 * n:60 * n, :n] = 0.5          # twenty planes turned into band
    torch.cuda.synchronize()
    kf.rebuild_sign_map()
    n_w = check()
    assert n_w != n5
    kf.close()


def test_interleaving_changes_nothing(dev):
    """relocalize, relocalize_batch and gauss_newton_terms on one instance, interleaved: each gives what it gives alone."""
    torch, pl, _ = dev
    kf, dfr = s3_map(torch, pl, 128)
    qs = queries(torch, kf, dfr, count=5, seed=2)
    D, M = [d for d, _ in qs], np.stack([m for _, m in qs])
    alone_single = singles(kf, qs, 4)
    alone_batch = kf.relocalize_batch(D, M, iterations=4)
    alone_terms = kf.gauss_newton_terms(dfr[5], qs[0][1])
    for _ in range(2):
        t = kf.gauss_newton_terms(dfr[5], qs[0][1])
        b = kf.relocalize_batch(D, M, iterations=4)
        s = singles(kf, qs, 4)
        assert t.tobytes() == alone_terms.tobytes()
        assert_same(b, s, 4)
        assert_same(alone_batch, s, 4)
        for (o1, c1, h1), (o2, c2, h2) in zip(s, alone_single):
            assert o1 == o2 and c1.tobytes() == c2.tobytes() and h1.tobytes() == h2.tobytes()
    kf.close()


def test_sharded_batch_equals_sharded_single(dev):
    """Two ranks as threads on one GPU (LocalWorld): relocalize_batch over each rank's owned planes with the F x 29 sums all-reduced equals
    the sharded per-frame relocalize, bit for bit, on every rank."""
    torch, pl, sh = dev
    world, n = 2, 128
    prm = synth.s1_params(n)
    lw = sh.LocalWorld(torch, world)
    shards = [sh.ShardedKinectFusion(prm, r, world, collective=lw.collective_for(r)) for r in range(world)]
    dfr = [torch.from_numpy(synth.s3_frame(k).view(np.int16)).cuda() for k in range(6)]
    results, errors = [None] * world, []
    qs = [None]

    def work(r):
        try:
            for d in dfr:
                assert shards[r].process_frame(d) == 1
            if r == 0:
                qs[0] = queries(torch, shards[0], dfr, count=6, seed=5)
            lw.barrier.wait()
            q = qs[0]
            single = singles(shards[r], q, 3)
            batch = shards[r].relocalize_batch([d for d, _ in q], np.stack([m for _, m in q]), iterations=3)
            results[r] = (single, batch, shards[r].relocalization_index_voxels())
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            lw.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    for r in range(world):
        single, batch, nvox = results[r]
        assert_same(batch, single, 3)
        assert_same(batch, results[0][0], 3)
    assert sum(results[r][2] for r in range(world)) > 0     # (a rank's owned planes may hold no band at all)
    assert sum(results[r][0][f][0] for r in range(world) for f in range(6)) > 0
    for s in shards:
        s.close()
